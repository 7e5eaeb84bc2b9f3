"""The multiplicity trigger of the pad traces on the device (include/attpc_engine.h, "multiplicity trigger") against its
numpy restatement (tests/trigger_reference.py): every field of every record EXACTLY equal -- the stage is integer
arithmetic.  The stage alone on hand-made and random rows (``traces_to_trigger``); the fused paths on their own delivered
traces; chunk and first-event invariance; full against partial readout; the gate of the trace rows; nothing else moves
with the stage on or off; a cloud of lone arrivals; the writers.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (BaselineSettings, PeakSettings, TriggerSettings, clouds_to_trace_rows,
                                              clouds_to_traces, configure_traces,
                                              configure_trigger, traces_to_trigger)
from tests import trigger_reference as ref
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu

NUM_TB, NUM_PADS = _abi.NUM_TB, _abi.NUM_PADS
GROUPS10 = (np.arange(NUM_PADS) * 7 % 10).astype(np.uint8)


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _pedestals(seed=3):
    return np.random.default_rng(seed).integers(200, 401, size=NUM_PADS).astype(np.int16)


def _assert_records(got, want, what=""):
    assert got.dtype == _abi.TRIGGER_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, ref.differing(got, want))


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
def _hand_events(rng):
    """(offsets, pads, y rows above the pedestal) of events with 0, 1, 5, 70, 0, 2 and 3 rows: the edges of the sample
    axis and of the lanes' 8-sample blocks, more rows than waves, an empty event directly behind the heavy one."""
    def row(*runs, level=200):
        y = np.zeros(NUM_TB, dtype=np.int64)
        for lo, hi in runs:
            y[lo:hi + 1] = level
        return y

    events = [
        [],
        [(17, row((100, 100)))],                                  # a run of length 1
        [(0, row((0, 0))),                                        # a hit at sample 0
         (1, row((500, 511))),                                    # a run ending at the array's end
         (2, row((0, 511))),                                      # all 512 samples hit
         (3, row((3, 7), (64, 70))),                              # ends on 7 | 8, starts on 63 | 64
         (10239, row((8, 12), (60, 63)))],                        # starts on 7 | 8, ends on 63 | 64
    ]
    heavy_pads = rng.choice(NUM_PADS, size=70, replace=False)
    _, heavy = ref.pulse_rows(rng, 70, pads=heavy_pads)
    events.append([(int(p), y.astype(np.int64)) for p, y in zip(heavy_pads, heavy)])
    events.append([])
    events.append([(40, row((5, 10), (60, 70))),                  # runs that span lane boundaries
                   (41, row((511, 511)))])                        # a hit at sample 511
    events.append([(50, row((30, 40), level=25)),                 # y == threshold: no hit
                   (51, row((30, 40), level=26)),
                   (52, row((35, 45)))])
    offsets = np.cumsum([0] + [len(e) for e in events])
    pads = np.array([p for e in events for p, _ in e], dtype=np.int32)
    y = np.stack([r for e in events for _, r in e])
    return offsets, pads, y


def test_stage_alone_on_hand_made_rows(ctx):
    rng = np.random.default_rng(5)
    offsets, pads, y = _hand_events(rng)
    assert np.diff(offsets).tolist() == [0, 1, 5, 70, 0, 2, 3]
    groups16 = (np.arange(NUM_PADS) % 16).astype(np.uint8)
    groups16[[2, 41]] = 255  # the all-hit row and the hit at 511 take no part under this map
    ped = _pedestals()
    n_fired = 0
    for pedestals in (None, ped):
        samples = (y + (0 if pedestals is None else pedestals.astype(np.int64)[pads][:, None])).astype(np.int16)
        for groups in (None, groups16):
            for window, mg in ((1, 2), (50, 20), (512, 60)):
                for min_groups in (1, 3):
                    trigger = TriggerSettings(25, window, mg if groups is None else max(1, mg // 4), min_groups, groups)
                    got = traces_to_trigger(offsets, pads, samples, trigger, pedestals, ctx)
                    _assert_records(got, ref.records(offsets, pads, samples, trigger, pedestals),
                                    (pedestals is not None, groups is not None, window, min_groups))
                    n_fired += int(got["fired"].sum())
                    assert got["n_rows"].tolist() == [0, 1, 5, 70, 0, 2, 3]
    assert n_fired > 0
    # the rows of one event alone give its record again (nothing of a neighbour's counters is left)
    trigger = TriggerSettings(25, 50, 5, 3, groups16)
    whole = traces_to_trigger(offsets, pads, samples, trigger, ped, ctx)
    for e in (3, 4, 5):
        lo, hi = offsets[e], offsets[e + 1]
        alone = traces_to_trigger([0, hi - lo], pads[lo:hi], samples[lo:hi], trigger, ped, ctx)
        assert alone.tolist() == whole[e:e + 1].tolist()
    assert traces_to_trigger([0], pads[:0], samples[:0], trigger, ped, ctx).shape == (0,)
    with pytest.raises(ValueError):  # the library's own check, behind the package's
        bad = _abi.TriggerDesc(25, 0, 1, 1, None, 0, 0)
        out = np.empty(1, dtype=_abi.TRIGGER_DTYPE)
        ctx.check(ctx.lib.attpc_trigger_rows(ctx.handle, 1, _abi.iptr(np.array([0, 0]), _abi.C.c_int64), None, None, None, bad,
                                             _abi.iptr(out, _abi.TriggerRecord)), "attpc_trigger_rows")


# ---------------------------------------------------------------- 2. random rows ----
@pytest.mark.parametrize("params", [(25, 1, 3, 1), (25, 50, 40, 2), (60, 512, 150, 1)], ids=["w1", "w50", "w512"])
def test_stage_alone_on_random_rows(ctx, params):
    rng = np.random.default_rng(23)
    ped = _pedestals(9)
    counts = rng.integers(0, 41, size=64)
    counts[[3, 4]] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)])
    pads, samples = ref.pulse_rows(rng, int(offsets[-1]), ped)
    threshold, window, mg, min_groups = params
    trigger = TriggerSettings(threshold, window, mg, min_groups, GROUPS10)
    got = traces_to_trigger(offsets, pads, samples, trigger, ped, ctx)
    _assert_records(got, ref.records(offsets, pads, samples, trigger, ped), params)
    assert 0 < got["fired"].sum() < 64 and got["n_hit_pads"].max() > 10, (got["fired"].sum(), got["peak_group_sum"].tolist())


# ---------------------------------------------------------------- 3 .. 7. the fused paths ----
NOISY = {"noise_sigma": 5.0, "threshold": 20.0, "readout": "partial"}
TRIGGER = TriggerSettings(25, window=50, group_multiplicity=60, min_groups=2, groups=GROUPS10)


def _engine(inp, ctx, trace_kw=NOISY, ped_seed=3, **kw):
    from attpc_engine_amd.engine import Engine

    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)
    eng.configure_traces(inp.config, pedestals=_pedestals(ped_seed), offset=int(np.argmax(get_response(inp.config))), **trace_kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings())
    eng.configure_baseline()
    return eng


@pytest.fixture(scope="module", params=["o16aa", "be10dp"])
def fused(request, ctx):
    """The delivered traces of 32 events, their records from the device and from the restatement (computed once)."""
    inp = Inputs(request.param)
    eng = _engine(inp, ctx)
    eng.configure_trigger(TRIGGER)
    n, seed = 32, 41
    res = eng.run_traces(n, seed=seed, first_event=0)
    want = ref.records(res["offsets"], res["pads"], res["samples"], TRIGGER, _pedestals())
    want.setflags(write=False)
    return inp, n, seed, res, want


def test_fused_records_equal_the_restatement_of_the_delivered_traces(ctx, fused):
    inp, n, seed, res, want = fused
    _assert_records(res["trigger"], want, "run_traces(fetch=True)")
    assert (res["labels"] == -1).any() and want["n_hit_pads"].max() > 20  # noise-only rows are there, and pads hit
    eng = _engine(inp, ctx)
    eng.configure_trigger(TRIGGER)
    resident = eng.run_traces(n, seed=seed, fetch=False)
    _assert_records(resident["trigger"], want, "run_traces(fetch=False)")
    assert resident["trace"] == res["trace"]
    only = eng.run_trigger(n, seed=seed)
    _assert_records(only["trigger"], want, "run_trigger")
    assert "pads" not in only and only["trace"] == res["trace"]
    rows = eng.run_trace_rows(n, seed=seed)
    _assert_records(rows["trigger"], want, "run_trace_rows")
    _assert_records(eng.run_trace_rows(n, seed=seed, fetch=False)["trigger"], want, "run_trace_rows(fetch=False)")
    eng.configure_baseline(BaselineSettings(20.0))
    with_baseline = eng.run_trace_rows(n, seed=seed)
    _assert_records(with_baseline["trigger"], want, "run_trace_rows with the Fourier baseline")
    assert with_baseline["trace_rows"] != rows["trace_rows"]  # (the baseline did change the rows)
    eng.configure_baseline()
    # the host-cloud entry points take the same path
    cloud = eng.run(8, seed=seed, fetch=True)
    tr = clouds_to_traces(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed)
    _assert_records(tr[4]["trigger"], want[:8], "clouds_to_traces")
    _assert_records(clouds_to_trace_rows(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed)[3]["trigger"],
                    want[:8], "clouds_to_trace_rows")
    eng.configure_trigger()


def test_records_do_not_depend_on_chunks_or_the_first_event(ctx, fused):
    inp, n, seed, _, want = fused
    small = _engine(inp, ctx, chunk_events=8)  # 4 chunks
    small.configure_trigger(TRIGGER)
    try:
        _assert_records(small.run_trigger(n, seed=seed)["trigger"], want, "chunk_events 8")
        _assert_records(small.run_trace_rows(n, seed=seed, fetch=False)["trigger"], want, "trace rows, chunk_events 8")
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    eng = _engine(inp, ctx)
    eng.configure_trigger(TRIGGER)
    shifted = eng.run_trigger(n, seed=seed, first_event=10)["trigger"]
    _assert_records(shifted[:n - 10], want[10:], "first_event 10")
    eng.configure_trigger()


def test_full_readout_gives_the_records_of_partial_readout(ctx):
    inp = Inputs("be10dp")
    n, seed = 8, 6
    records = {}
    for readout in ("partial", "full"):
        eng = _engine(inp, ctx, {**NOISY, "readout": readout})
        eng.configure_trigger(TRIGGER)
        records[readout] = eng.run_trigger(n, seed=seed)["trigger"]
        eng.configure_trigger()
    for field in ref.FIELDS:
        if field != "n_rows":
            assert records["full"][field].tolist() == records["partial"][field].tolist(), field
    assert (records["full"]["n_rows"] > records["partial"]["n_rows"]).all() and records["partial"]["n_hit_pads"].max() > 0


def _half_multiplicity(records):
    """A group multiplicity that about half of the events with rows reach in ``records`` (those of a run with one group;
    ``peak_group_sum`` says what every event reaches): the upper part fires, the lower part does not."""
    reach = np.sort(records["peak_group_sum"][records["n_rows"] > 0])
    middle = int(reach[len(reach) // 2])
    return max(1, middle + 1 if middle < reach[-1] else middle)


def _row_checksum(offsets, rows, first_event=0):
    total = 0
    for e in range(len(offsets) - 1):
        for r in rows[offsets[e]:offsets[e + 1]]:
            total += ((first_event + e) << 23) + (int(r[5]) << 9) + int(np.floor(r[6]))
    return total % (1 << 64)


def test_gate(ctx, fused):
    inp, n, seed, _, _ = fused
    eng = _engine(inp, ctx)
    eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
    reach = eng.run_trigger(n, seed=seed)["trigger"]
    mg = _half_multiplicity(reach)
    trigger = TriggerSettings(25, window=50, group_multiplicity=mg)
    eng.configure_trigger(trigger)
    open_ = eng.run_trace_rows(n, seed=seed)
    fired = open_["trigger"]["fired"] != 0
    assert (fired == (reach["peak_group_sum"] >= mg)).all()  # one run gives the efficiency curve over Mg
    assert 0 < fired.sum() < n, (mg, reach["peak_group_sum"].tolist())  # both kinds occur: the test cannot pass vacuously
    eng.configure_trigger(trigger.gated())
    gated = eng.run_trace_rows(n, seed=seed)
    _assert_records(gated["trigger"], open_["trigger"], "gated")
    counts = np.where(fired, np.diff(open_["offsets"]), 0)
    assert np.diff(gated["offsets"]).tolist() == counts.tolist() and (counts[fired] > 0).any()
    keep = np.repeat(fired, np.diff(open_["offsets"]))
    assert (np.diff(open_["offsets"])[~fired] > 0).any()  # the gate did drop rows
    np.testing.assert_array_equal(gated["rows"], open_["rows"][keep])
    np.testing.assert_array_equal(gated["labels"], open_["labels"][keep])
    np.testing.assert_array_equal(gated["event_points"], open_["event_points"])
    assert gated["trace_rows"] == {"n_rows": int(keep.sum()), "row_checksum": _row_checksum(gated["offsets"], gated["rows"])}
    assert open_["trace_rows"]["row_checksum"] == _row_checksum(open_["offsets"], open_["rows"])
    assert gated["stats"]["n_points"] == int(keep.sum())
    assert eng.run_trace_rows(n, seed=seed, fetch=False)["trace_rows"] == gated["trace_rows"]
    # the traces themselves are delivered whatever the gate says
    traces = eng.run_traces(n, seed=seed, fetch=False)
    eng.configure_trigger()
    assert eng.run_traces(n, seed=seed, fetch=False)["trace"] == traces["trace"]


def test_off(ctx, fused):
    inp, n, seed, res, _ = fused
    fresh = _abi.Context(0)
    out = np.empty(1, dtype=_abi.TRIGGER_DTYPE)
    assert fresh.lib.attpc_trigger_last(fresh.handle, 0, 0, _abi.iptr(out, _abi.TriggerRecord)) == _abi.E_NOTCONFIGURED
    fresh.close()
    eng = _engine(inp, ctx)
    eng.configure_trigger()
    off_traces = eng.run_traces(n, seed=seed, fetch=False)
    assert "trigger" not in off_traces
    assert ctx.lib.attpc_trigger_last(ctx.handle, 0, 1, _abi.iptr(out, _abi.TriggerRecord)) == _abi.E_NOTCONFIGURED
    off_rows = eng.run_trace_rows(n, seed=seed, fetch=False)
    assert ctx.lib.attpc_trigger_last(ctx.handle, 0, 1, _abi.iptr(out, _abi.TriggerRecord)) == _abi.E_NOTCONFIGURED
    eng.configure_trigger(TRIGGER)
    on_traces = eng.run_traces(n, seed=seed, fetch=False)
    on_rows = eng.run_trace_rows(n, seed=seed, fetch=False)
    assert on_traces["trace"] == off_traces["trace"] == res["trace"] and on_rows["trace_rows"] == off_rows["trace_rows"]
    assert ctx.lib.attpc_trigger_last(ctx.handle, n, 1, _abi.iptr(out, _abi.TriggerRecord)) == _abi.E_INVALID
    assert ctx.lib.attpc_trigger_last(ctx.handle, n - 1, 1, _abi.iptr(out, _abi.TriggerRecord)) == _abi.OK
    assert out.tolist() == on_rows["trigger"][n - 1:].tolist()
    eng.configure_trigger()


# ---------------------------------------------------------------- 8. physics sanity ----
@pytest.mark.parametrize("n_pads", [1, 7, 40])
def test_lone_arrivals_of_one_bucket_count_their_pads(ctx, n_pads):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    at, r_max = int(np.argmax(resp)), float(resp.max())
    configure_traces(inp.config, ctx, resp, threshold=40.0, offset=at)
    pads = np.arange(n_pads) * 250 + 3
    points = np.column_stack([pads.astype(np.float64), np.full(n_pads, 200.25), np.full(n_pads, 1000.0 / r_max)])
    offsets, labels = np.array([0, n_pads]), np.full(n_pads, 2)
    for mg, fires in ((n_pads, 1), (n_pads + 1, 0)):
        configure_trigger(ctx, TriggerSettings(500, window=1, group_multiplicity=mg))
        rec = clouds_to_traces(offsets, points, labels, ctx)[4]["trigger"][0]
        assert (rec["peak_group_sum"], rec["fired"], rec["n_rows"], rec["n_hit_pads"]) == (n_pads, fires, n_pads, n_pads)
        # (the pulses are equal: all pads cross the level together, a few samples before the peak at 200)
        assert 184 < rec["peak_sample"] <= 200 and rec["sample"] == (rec["peak_sample"] if fires else -1)
    configure_trigger(ctx, None)


# ---------------------------------------------------------------- 9. the writers ----
def test_writers_write_the_fired_events(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd.detector import SpyralWriter, TraceWriter
    from attpc_engine_amd.engine import run_fused
    from tests.test_gpu_peaks import _read_spyral_files
    from tests.test_gpu_traces import _read_trace_files

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n, seed = 24, 17
    kw = {"noise_sigma": 4.0, "pedestals": _pedestals(12), "offset": 7}
    from attpc_engine_amd.engine import Engine

    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings())
    eng.configure_baseline()
    eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
    trigger = TriggerSettings(25, window=50, group_multiplicity=_half_multiplicity(eng.run_trigger(n, seed=seed)["trigger"]))
    eng.configure_trigger(trigger)
    rows = eng.run_trace_rows(n, seed=seed)
    traces = eng.run_traces(n, seed=seed)
    fired = rows["trigger"]["fired"] != 0
    want = [e for e in range(n) if fired[e] and rows["event_points"][e] > 0]
    assert 0 < len(want) < int((rows["event_points"] > 0).sum())
    for name in ("rows", "traces"):
        (tmp_path / name).mkdir()
    run_fused(inp.pipeline, inp.config, SpyralWriter(tmp_path / "rows", inp.config, max_events_per_file=10, peaks=PeakSettings(), **kw),
              n, inp.indices, seed=seed, batch_size=7, context=ctx, trigger=trigger)
    got, _ = _read_spyral_files(tmp_path / "rows")
    assert sorted(got) == want
    for e in want:
        lo, hi = rows["offsets"][e], rows["offsets"][e + 1]
        np.testing.assert_array_equal(got[e][0], rows["rows"][lo:hi])
        np.testing.assert_array_equal(got[e][1], rows["labels"][lo:hi])
    run_fused(inp.pipeline, inp.config, TraceWriter(tmp_path / "traces", inp.config, max_events_per_file=10, **kw), n,
              inp.indices, seed=seed, batch_size=7, context=ctx, trigger=trigger)
    got = _read_trace_files(tmp_path / "traces")
    assert sorted(got) == want
    for e in want:
        lo, hi = traces["offsets"][e], traces["offsets"][e + 1]
        np.testing.assert_array_equal(got[e][0], traces["pads"][lo:hi])
        np.testing.assert_array_equal(got[e][1], traces["samples"][lo:hi])
    configure_trigger(ctx, None)
