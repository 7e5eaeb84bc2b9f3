"""The micromegas gain of the pad traces on the device (include/attpc_engine.h, "micromegas gain of the traces") against
its numpy restatement (tests/gain_reference.py): every gained charge EXACTLY equal -- the contract fixes every rounding
--, and every trace exactly the trace restatements' on the gained cloud.  The stage alone on a hand-made cloud
(``clouds_to_gain``); traces of a host cloud with the label rule on the cloud's own charge; the fused pipeline against
its own delivered cloud, in chunks and split; off is off; the trace rows and the trigger on top.  Needs a real MI355X:
``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (GainSettings, PeakSettings, TriggerSettings, clouds_to_gain, clouds_to_traces,
                                              configure_gain, configure_traces, gaussian_noise_table,
                                              normal_quantile_table, readout_mask)
from tests import gain_reference as ref
from tests.helpers import Inputs
from tests.trace_reference import traces as reference_traces

pytestmark = pytest.mark.gpu

NUM_TB, NUM_PADS = _abi.NUM_TB, _abi.NUM_PADS
Z = normal_quantile_table()
SEED_HI = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _gain_map(seed=2):
    """Pad gains of 0.8 .. 1.2 with dead pads (0) among them, pads 0 and 10239 alive."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.8, 1.2, size=NUM_PADS)
    g[rng.choice(np.arange(1, NUM_PADS - 1), size=300, replace=False)] = 0.0
    return g


def _pedestals(seed=3):
    return np.random.default_rng(seed).integers(200, 401, size=NUM_PADS).astype(np.int16)


def _assert_traces(got, want, what=""):
    """(offsets, pads, samples, labels, sums) of the device and of the restatement: identical."""
    for k, name in enumerate(("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=f"{what} {name}")
    assert got[4] == want[4], (what, got[4], want[4])


def _traces_of(res):
    return res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"]


# ---------------------------------------------------------------- 1. the stage alone ----
CHARGES = (0.0, 1.0, 2.0, 3.0, 5.0, 10.0, 1e3, 1e5, 1e7)


def _hand_cloud():
    """Three events -- 1 100 rows, none, 900 rows -- with a (pad, t) of their own each, over the whole pad plane and
    time axis (the corners pad 0 / 10239 and t 0 / 511 included), every charge of CHARGES on many rows."""
    rng = np.random.default_rng(17)
    events = []
    for n in (1100, 0, 900):
        keys = rng.choice(NUM_PADS * NUM_TB, size=n, replace=False)
        if n:
            keys[:4] = [0, 511, 10239 * NUM_TB, 10239 * NUM_TB + 511]
            keys = np.unique(keys)
        q = np.array(CHARGES)[rng.integers(0, len(CHARGES), size=len(keys))]
        q[:4] = [1.0, 5.0, 1.0, 1e5][:len(q)]
        events.append(np.stack([(keys // NUM_TB).astype(float), keys % NUM_TB + rng.random(len(keys)), q], axis=1)
                      if len(keys) else np.zeros((0, 3)))
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in events])])
    return offsets, np.concatenate(events)


@pytest.mark.parametrize("f", [1.0, 0.3])
def test_stage_alone_equals_the_restatement(ctx, f):
    offsets, points = _hand_cloud()
    assert 1900 < len(points) <= 2000 and offsets[1] == offsets[2]
    pad_gain = _gain_map()
    seed, first = SEED_HI, (1 << 32) + 3
    got = clouds_to_gain(offsets, points, ctx, seed, first, GainSettings(rel_variance=f, pad_gain=pad_gain, stream=6))
    want = ref.Gain(f, Z, pad_gain, stream=6).cloud(offsets, points, seed, first)
    np.testing.assert_array_equal(got, want)
    pads = points[:, 0].astype(int)
    assert (got[pad_gain[pads] == 0.0] == 0.0).all() and (pad_gain[pads] == 0.0).any()
    assert (got[points[:, 2] == 0.0] == 0.0).all() and (got[(points[:, 2] > 0) & (pad_gain[pads] > 0)] > 0).mean() > 0.99
    # another stream and another first event draw other numbers; the gain map alone draws none
    other = clouds_to_gain(offsets, points, ctx, seed, first, GainSettings(rel_variance=f, pad_gain=pad_gain))
    assert (other != got).mean() > 0.5
    np.testing.assert_array_equal(other, ref.Gain(f, Z, pad_gain).cloud(offsets, points, seed, first))
    only_map = clouds_to_gain(offsets, points, ctx, seed, first, GainSettings(pad_gain=pad_gain))
    np.testing.assert_array_equal(only_map, points[:, 2] * pad_gain[pads])
    np.testing.assert_array_equal(clouds_to_gain(offsets, points, ctx, seed, first), points[:, 2])  # off: q'' = q
    # a split call gives the same rows: event i is the global event first_event + i
    tail = clouds_to_gain(offsets[2:] - offsets[2], points[offsets[2]:], ctx, seed, first + 2,
                          GainSettings(rel_variance=f, pad_gain=pad_gain, stream=6))
    np.testing.assert_array_equal(tail, want[offsets[2]:])
    configure_gain(ctx, None)


def test_the_library_validates_descriptor_and_rows(ctx):
    table, gains = np.array(Z), np.ones(NUM_PADS)

    def configure(f, pad_gain=None, quantiles=table, stream=0):
        desc = _abi.TraceGainDesc(f, _abi.dptr(pad_gain), _abi.dptr(quantiles), stream, 0)
        ctx.check(ctx.lib.attpc_trace_configure_gain(ctx.handle, desc), "attpc_trace_configure_gain")

    decreasing, infinite, negative, nan_gain = table.copy(), table.copy(), gains.copy(), gains.copy()
    decreasing[100] = decreasing[99] - 1e-3
    infinite[-1] = np.inf
    negative[5], nan_gain[6] = -0.5, np.nan
    for bad in ({"f": 1.5}, {"f": -0.1}, {"f": np.nan}, {"f": np.inf}, {"f": 0.5, "pad_gain": negative},
                {"f": 0.0, "pad_gain": nan_gain}, {"f": 0.5, "quantiles": decreasing}, {"f": 0.5, "quantiles": infinite},
                {"f": 0.5, "quantiles": None}, {"f": 0.5, "stream": 1 << 30}):
        with pytest.raises(ValueError):
            configure(**bad)
    configure(0.0, quantiles=None)  # f = 0 needs no table
    configure(0.5, gains, stream=(1 << 30) - 1)
    # the calls above went past the package's token: turn the stage off the same way, then the token is right again
    ctx.check(ctx.lib.attpc_trace_configure_gain(ctx.handle, None), "attpc_trace_configure_gain")
    ctx.forget("trace_gain")
    for pts in ([[1.0, 3.2, 5.0], [1.0, 3.7, 6.0]], [[10240.0, 3.0, 5.0]], [[1.5, 3.0, 5.0]], [[1.0, 512.0, 5.0]],
                [[1.0, 3.0, -1.0]], [[1.0, 3.0, np.inf]]):
        with pytest.raises(ValueError):  # the row validation of attpc_traces
            clouds_to_gain(np.array([0, len(pts)]), np.array(pts), ctx)
    assert clouds_to_gain(np.array([0]), np.zeros((0, 3)), ctx).shape == (0,)


# ---------------------------------------------------------------- 2. traces of a host cloud ----
def _box_response():
    resp = np.zeros(NUM_TB)
    resp[:24] = np.concatenate([np.linspace(0.1, 0.5, 12), np.linspace(0.5, 0.05, 12)])
    return resp


def _host_events(gain, first):
    """(seed, offsets, points, labels) of four events (one empty): lone arrivals of every size, pile-up on one pad up to
    saturation, rows at both ends of the time axis and of the pad plane, and in event 0 a pad whose two rows, q = 100
    and 101, swap order under the fluctuation (the seed, high word set, is searched for here on the CPU)."""
    t0 = 100
    seed = next(SEED_HI + k for k in range(200)
                if np.diff(gain.rows(SEED_HI + k, first, [77, 77], [t0, t0 + 150], [100.0, 101.0]))[0] < 0)
    ev0 = [[77, t0 + 0.4, 100.0], [77, t0 + 150.9, 101.0], [0, 0.0, 300.0], [10239, 511.99, 5000.0], [5, 40.5, 1.0],
           [6, 40.5, 90.0], [7, 40.5, 0.0], [8, 10.1, 1e5]]
    ev0 += [[300, 100.0 + 3 * k, 150.0 + k] for k in range(40)]                      # a long pile-up
    ev2 = [[p, 20.0 + (p % 7), 85.0] for p in range(1000, 1060)]                       # around threshold 40 at R = 0.5
    ev2 += [[2000, 200.5, 6000.0], [2000, 205.5, 6000.0]]                              # saturates when summed
    ev3 = [[4000 + k, 500.0 + (k % 12), 200.0] for k in range(30)]                     # the response runs off the end
    events = [ev0, [], ev2, ev3]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in events])])
    points = np.array([r for e in events for r in e], dtype=np.float64)
    labels = np.arange(len(points), dtype=np.int64) % 5
    labels[:2] = [3, 4]
    return seed, offsets, points, labels


@pytest.mark.parametrize("threshold", [-1.0, 40.0])
def test_traces_of_a_host_cloud(ctx, threshold):
    inp = Inputs("o16aa")
    resp, offset = _box_response(), 3
    pad_gain = _gain_map(4)
    pad_gain[[77, 300, 2000]] = [1.0, 1.1, 0.9]
    first = (1 << 32) - 2  # the events cross the low word
    gain = ref.Gain(1.0, Z, pad_gain, stream=1)
    seed, offsets, points, labels = _host_events(gain, first)
    configure_traces(inp.config, ctx, resp, threshold, offset)
    configure_gain(ctx, GainSettings(rel_variance=1.0, pad_gain=pad_gain, stream=1))
    got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
    want = ref.traces_with_gain(offsets, points, labels, gain, seed, first,
                                lambda pts: reference_traces(offsets, pts, labels, resp, threshold, offset, first_event=first))
    _assert_traces(got, want, f"threshold {threshold}")
    # pads and labels against the trace restatement on the ORIGINAL cloud
    plain = reference_traces(offsets, points, labels, resp, -1.0, offset, first_event=first)
    if threshold < 0:
        np.testing.assert_array_equal(got[1], plain[1])
        np.testing.assert_array_equal(got[3], plain[3])
    else:
        assert 0 < got[4]["n_rows"] < plain[4]["n_rows"]
        for e in range(len(offsets) - 1):
            of_pad = dict(zip(plain[1][plain[0][e]:plain[0][e + 1]].tolist(), plain[3][plain[0][e]:plain[0][e + 1]].tolist()))
            assert [of_pad[p] for p in got[1][got[0][e]:got[0][e + 1]].tolist()] == got[3][got[0][e]:got[0][e + 1]].tolist()
    # the swapped pad: the smaller cloud charge carries the larger gained charge, the label stays that of q = 101
    q2 = gain.cloud(offsets, points, seed, first)
    assert q2[0] > q2[1] and points[0, 2] < points[1, 2]
    row = int(np.flatnonzero(got[1][:got[0][1]] == 77)[0])
    assert got[3][row] == labels[1] == 4
    configure_gain(ctx, None)
    configure_traces(inp.config, ctx, None, None, 0)


# ---------------------------------------------------------------- 3. the pipeline ----
N, SEED, FIRST = 64, 29, 5
GAIN = GainSettings(theta=0.0, pad_gain=_gain_map(8), stream=3)
GAIN_REF = ref.Gain(1.0, Z, GAIN.pad_gain, stream=3)


def _engine(inp, ctx, gain=GAIN, **kw):
    from attpc_engine_amd.engine import Engine

    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))))
    eng.configure_gain(gain)
    return eng


@pytest.fixture(scope="module")
def pipeline(ctx):
    """be10dp: the delivered cloud of events FIRST .. FIRST + N - 1 and the restatement (gain, then trace) of it,
    computed once and read-only."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    cloud = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
    resp, thr = get_response(inp.config), float(inp.config.elec_params.adc_threshold)
    offset = int(np.argmax(resp))
    want = ref.traces_with_gain(cloud["offsets"], cloud["points"], cloud["labels"], GAIN_REF, SEED, FIRST,
                                lambda pts: reference_traces(cloud["offsets"], pts, cloud["labels"], resp, thr, offset,
                                                             first_event=FIRST))
    for a in want[:4]:
        a.setflags(write=False)
    return inp, cloud, want


def test_pipeline_equals_gain_then_trace_of_its_own_cloud(ctx, pipeline):
    inp, cloud, want = pipeline
    eng = _engine(inp, ctx)
    res = eng.run_traces(N, seed=SEED, first_event=FIRST)
    _assert_traces(_traces_of(res), want, "run_traces")
    assert want[4]["n_rows"] > 10 * N
    # unchanged: the cloud's statistics, event_points, the kinematics
    np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
    for key in ("n_points", "charge_checksum", "key_checksum", "n_track_samples"):
        assert res["stats"][key] == cloud["stats"][key], key
    np.testing.assert_array_equal(res["p4"], cloud["p4"])
    # ... and the gain does something: the traces differ from those without it
    eng.configure_gain()
    plain = eng.run_traces(N, seed=SEED, first_event=FIRST, fetch=False)["trace"]
    assert plain["sample_checksum"] != want[4]["sample_checksum"]


@pytest.mark.parametrize("chunk_events", [16, 64])
def test_pipeline_does_not_depend_on_chunks(ctx, pipeline, chunk_events):
    inp, _, want = pipeline
    eng = _engine(inp, ctx, chunk_events=chunk_events)
    try:
        _assert_traces(_traces_of(eng.run_traces(N, seed=SEED, first_event=FIRST)), want, f"chunk_events {chunk_events}")
        resident = eng.run_traces(N, seed=SEED, first_event=FIRST, fetch=False)
        assert resident["trace"] == want[4]
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        eng.configure_gain()


def test_pipeline_events_asked_for_alone(ctx, pipeline):
    inp, _, want = pipeline
    eng = _engine(inp, ctx)
    res = eng.run_traces(32, seed=SEED, first_event=FIRST + 32)
    lo = want[0][32]
    np.testing.assert_array_equal(res["offsets"], want[0][32:] - lo)
    np.testing.assert_array_equal(res["pads"], want[1][lo:])
    np.testing.assert_array_equal(res["samples"], want[2][lo:])
    np.testing.assert_array_equal(res["labels"], want[3][lo:])
    eng.configure_gain()


def test_pipeline_with_noise_pedestals_and_partial_readout(ctx, pipeline):
    """The first 8 events of the same ids (the readout restatement draws 512 samples for each of the 10 000 pads of the
    readout set per event: 8 events keep the test at a few seconds; nothing in the gain depends on the number)."""
    from tests.readout_reference import PARTIAL
    from tests.readout_reference import traces as readout_traces
    from tests.trace_noise_reference import Noise

    inp, cloud, _ = pipeline
    n, thr, ped = 8, 20.0, _pedestals()
    resp = get_response(inp.config)
    offset = int(np.argmax(resp))
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, threshold=thr, offset=offset, noise_sigma=5.0, pedestals=ped, readout="partial")
    res = eng.run_traces(n, seed=SEED, first_event=FIRST)
    cdf, min_level = gaussian_noise_table(5.0)
    noise = Noise(cdf, min_level, pedestals=ped)
    offsets = cloud["offsets"][:n + 1]
    points, labels = cloud["points"][:offsets[-1]], cloud["labels"][:offsets[-1]]
    want = ref.traces_with_gain(offsets, points, labels, GAIN_REF, SEED, FIRST,
                                lambda pts: readout_traces(offsets, pts, labels, resp, thr, offset, noise, SEED, FIRST,
                                                           PARTIAL, readout_mask(None).astype(bool)))
    _assert_traces(_traces_of(res), want, "noise, pedestals, partial readout")
    assert (res["labels"] == -1).any() and (res["labels"] >= 0).any()
    small = _engine(inp, ctx, chunk_events=4)  # the same settings across a chunk boundary
    small.configure_traces(inp.config, threshold=thr, offset=offset, noise_sigma=5.0, pedestals=ped, readout="partial")
    try:
        _assert_traces(_traces_of(small.run_traces(n, seed=SEED, first_event=FIRST)), want, "chunk_events 4")
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    eng.configure_gain()
    configure_traces(inp.config, ctx, None, None, 0)


# ---------------------------------------------------------------- 4. off is off ----
def test_off_is_off(ctx):
    inp = Inputs("be10dp")
    n, seed, first = 16, 7, 100
    fresh = _abi.Context(0)  # never saw a gain
    never = _engine(inp, fresh, gain=None).run_traces(n, seed=seed, first_event=first)
    fresh.close()
    eng = _engine(inp, ctx)
    on = eng.run_traces(n, seed=seed, first_event=first)
    assert on["trace"]["sample_checksum"] != never["trace"]["sample_checksum"]
    for what, setting in (("turned off", None), ("f = 0 without a gain map", GainSettings(rel_variance=0.0))):
        eng.configure_gain(GAIN)
        eng.configure_gain(setting)
        off = eng.run_traces(n, seed=seed, first_event=first)
        _assert_traces(_traces_of(off), _traces_of(never), what)
        assert off["stats"]["charge_checksum"] == never["stats"]["charge_checksum"]
    # the host-cloud entry point as well
    cloud = eng.run(4, seed=seed, first_event=first, fetch=True)
    host = clouds_to_traces(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed, first_event=first)
    rows = never["offsets"][4]
    np.testing.assert_array_equal(host[0], never["offsets"][:5])
    for k, key in ((1, "pads"), (2, "samples"), (3, "labels")):
        np.testing.assert_array_equal(host[k], never[key][:rows], err_msg=f"attpc_traces_at, off: {key}")


# ---------------------------------------------------------------- 5. reach: trace rows and the trigger ----
@pytest.mark.parametrize("name", ["o16aa", "be10dp"])
def test_trace_rows_and_trigger_see_the_gained_traces(ctx, name):
    from tests import trigger_reference
    from tests.peaks_reference import Geometry, Peaks, trace_rows

    inp = Inputs(name)
    n, seed, first, ped = 8, 41, 3, _pedestals()
    trigger = TriggerSettings(25, window=50, group_multiplicity=60, min_groups=2,
                              groups=(np.arange(NUM_PADS) * 7 % 10).astype(np.uint8))
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), noise_sigma=5.0, threshold=20.0,
                         pedestals=ped, readout="partial")
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings())
    eng.configure_trigger(trigger)
    try:
        tr = eng.run_traces(n, seed=seed, first_event=first)
        rows = eng.run_trace_rows(n, seed=seed, first_event=first)
        want = trace_rows(tr["offsets"], tr["pads"], tr["samples"], tr["labels"], Peaks(), Geometry.of(inp.config), seed, first, ped)
        np.testing.assert_array_equal(rows["offsets"], want[0])
        np.testing.assert_array_equal(rows["rows"], want[1])
        np.testing.assert_array_equal(rows["labels"], want[2])
        assert rows["trace_rows"] == want[3] and want[3]["n_rows"] > 0
        records = trigger_reference.records(tr["offsets"], tr["pads"], tr["samples"], trigger, ped)
        for got in (tr["trigger"], rows["trigger"], eng.run_trigger(n, seed=seed, first_event=first)["trigger"]):
            assert got.tobytes() == records.tobytes(), trigger_reference.differing(got, records)
        # the gain reached them: without it the same ids give other traces
        eng.configure_gain()
        assert eng.run_traces(n, seed=seed, first_event=first, fetch=False)["trace"] != tr["trace"]
    finally:
        eng.configure_gain()
        eng.configure_trigger()
        configure_traces(inp.config, ctx, None, None, 0)
