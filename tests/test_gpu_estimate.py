"""The track estimates of the trace rows on the device (include/attpc_engine.h, "track estimates of the trace rows")
against their numpy restatement (tests/estimate_reference.py): integer fields equal, f64 fields bit for bit, NaN in the
same places.  The stage alone on hand-made rows at the shapes where the kernel can go wrong (``rows_to_estimates``); the
fused path on its own delivered rows, resident, in chunks, behind a gating trigger, and with nothing else moving;
``simulate_batch_trace_rows(estimates=)``.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import PeakSettings, TriggerSettings, simulate_batch_trace_rows
from tests import estimate_reference as ref
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu

FIELD = 2.85
INDICES8 = [2, 5, 3, 2, 7, 9, 11, 4]  # n_sim = 8: every wave takes two positions; label 2 is given twice


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _settings(radius=25.0, min_points=30):
    return EstimateSettings(radius, min_points, magnetic_field=FIELD), ref.Params(radius, min_points, FIELD)


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
def _track(rng, n_used, backward=False, unused=(), jitter=0.6, **kw):
    """A track of ``n_used`` used rows (outside a 25 mm beam region) in ascending z; ``backward``: it travels towards
    low z (its start, the end nearer the axis, is its last row); ``unused``: (position, count) runs of rows inside the
    beam region put in front of the used row at that position."""
    kw = {"radius_mm": 120.0, "centre_mm": (150.0, 10.0), "turn": 1.4, **kw}
    rows = ref.arc_track(n_used, jitter=jitter, rng=rng, **kw)
    assert (np.hypot(rows[:, 0], rows[:, 1]) > 25.5).all()
    if backward:
        rows[:, :2] = rows[::-1, :2]
    for at, count in sorted(unused, reverse=True):
        inside = np.zeros((count, 8))
        inside[:, 0], inside[:, 1] = rng.uniform(-15.0, 15.0, count), rng.uniform(-15.0, 15.0, count)
        inside[:, 2], inside[:, 4] = rows[min(at, n_used - 1), 2], 77.0
        rows = np.concatenate([rows[:at], inside, rows[at:]])
    return rows


def _interleave(rng, tracks, noise_rows=0):
    """The rows of ``tracks`` [(rows, label)] row by row in turn, with ``noise_rows`` rows of label -1 between them."""
    tracks = list(tracks)
    if noise_rows:
        noise = np.zeros((noise_rows, 8))
        noise[:, :3], noise[:, 4] = rng.uniform(-250.0, 250.0, (noise_rows, 3)), 30.0
        tracks.append((noise, -1))
    order = np.argsort(np.concatenate([np.arange(len(r)) * 1.0 + 0.01 * i for i, (r, _) in enumerate(tracks)]), kind="stable")
    rows = np.concatenate([r for r, _ in tracks])[order]
    labels = np.concatenate([np.full(len(r), label, dtype=np.int64) for r, label in tracks])[order]
    return rows, labels


def _hand_events(rng):
    events = []
    # tile edges of the used rows, and of the segment (m = 64 | 65, 128 | 129), forward and backward
    for sizes in ((63, 64, 65), (127, 128, 129), (255, 256, 257)):
        events.append(_interleave(rng, [(_track(rng, n, backward=bool(i % 2)), label)
                                        for i, (n, label) in enumerate(zip(sizes, (2, 5, 3)))]))
    # a backward track whose segment starts in the last, partial tile of the event (150 rows = 2 tiles + 22)
    events.append((_track(rng, 150, backward=True), np.full(150, 7, dtype=np.int64)))
    # two labels row by row with -1 rows between them, the other positions absent
    events.append(_interleave(rng, [(_track(rng, 90), 9), (_track(rng, 75, backward=True, centre_mm=(-150.0, 30.0), phase=0.2), 11)], 60))
    # unused rows between used ones: single ones, a run across a tile edge, a run of more than a tile
    events.append((_track(rng, 140, unused=[(1, 1), (5, 3), (60, 10), (70, 100), (139, 2)]), np.full(256, 4, dtype=np.int64)))
    events.append((_track(rng, 140, backward=True, unused=[(0, 5), (80, 70), (139, 1)]), np.full(216, 3, dtype=np.int64)))
    events.append((np.zeros((0, 8)), np.zeros(0, dtype=np.int64)))  # no rows
    inside = np.zeros((50, 8))
    inside[:, :2] = rng.uniform(-17.0, 17.0, (50, 2))
    events.append((inside, np.full(50, 2, dtype=np.int64)))  # wholly inside the beam region
    events.append(_interleave(rng, [(_track(rng, 29), 2), (_track(rng, 30), 5)]))  # min_points - 1 and min_points
    i = np.arange(45)
    events.append((ref.spyral_rows(480 + 9 * i, 12 * i, 300 + 21 * i), np.full(45, 9, dtype=np.int64)))  # collinear
    events.append((ref.spyral_rows([700] * 40, [-90] * 40, 50 * np.arange(40)), np.full(40, 5, dtype=np.int64)))  # one point
    bad = _track(rng, 80)
    bad[10, 0], bad[20, 2], bad[30, 4], bad[40, 1] = 321.0, np.nan, 2.0 ** 31, -np.inf
    events.append((bad, np.full(80, 11, dtype=np.int64)))  # rows out of range
    # all eight positions in one event
    events.append(_interleave(rng, [(_track(rng, 40 + 13 * s, backward=bool(s % 2), phase=3.3 + 0.3 * s), label)
                                    for s, label in enumerate((2, 5, 3, 7, 9, 11, 4))], 25))
    return events


def _csr(events):
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in events])])
    return offsets, np.concatenate([r for r, _ in events]), np.concatenate([l for _, l in events])


@pytest.fixture(scope="module")
def hand():
    """The hand-made events in CSR form and their reference records (computed once, read-only)."""
    events = _hand_events(np.random.default_rng(17))
    offsets, rows, labels = _csr(events)
    want = ref.records(offsets, rows, labels, INDICES8, _settings()[1])
    want.setflags(write=False)
    return events, want


def test_stage_alone_on_hand_made_rows(ctx, hand):
    events, want = hand
    settings, _ = _settings()
    got = rows_to_estimates(*_csr(events), INDICES8, settings, ctx)
    ref.assert_same_records(got, want)
    status = want["status"]
    # the cases are there: fits of both directions, every kind of record without one, and the twice-given label
    assert (status == 0).sum() > 15 and {1, -1} <= set(want["direction"][status == 0].tolist())
    for bit in (_abi.EST_EMPTY, _abi.EST_FEW, _abi.EST_RANGE, _abi.EST_NO_CIRCLE, _abi.EST_NO_SLOPE):
        assert (status & bit).any(), bit
    assert (want["status"][:, 3] == _abi.EST_EMPTY).all() and (want["n_rows"][:, 0] > 0).sum() > 4
    assert {64, 65, 128, 129} <= set(want["n_fit"].ravel().tolist()) and want["n_used"][9, 0] == 29 and want["n_fit"][9, 1] == 30
    # 3 events in one call, and one event alone: nothing of a neighbour is left
    ref.assert_same_records(rows_to_estimates(*_csr(events[:3]), INDICES8, settings, ctx), want[:3])
    ref.assert_same_records(rows_to_estimates(*_csr(events[5:6]), INDICES8, settings, ctx), want[5:6])
    assert rows_to_estimates([0], np.zeros((0, 8)), np.zeros(0), INDICES8, settings, ctx).shape == (0, 8)
    # other settings: no beam region, another threshold of points
    other, other_ref = _settings(0.0, 64)
    offsets, rows, labels = _csr(events[:6])
    ref.assert_same_records(rows_to_estimates(offsets, rows, labels, [5, 2], other, ctx), ref.records(offsets, rows, labels, [5, 2], other_ref))


def test_cap_at_2048_rows(ctx):
    rng = np.random.default_rng(3)
    settings, params = _settings()
    long_track = _track(rng, 4200, jitter=1.0, turn=5.5, dz_mm=0.15)
    events = [(long_track, np.full(4200, 2, dtype=np.int64)),
              (_track(rng, 4200, backward=True, jitter=1.0, turn=5.5, dz_mm=0.15), np.full(4200, 5, dtype=np.int64)),
              (long_track[:4096], np.full(4096, 2, dtype=np.int64))]
    offsets, rows, labels = _csr(events)
    want = ref.records(offsets, rows, labels, [2, 5], params)
    assert want["n_fit"][[0, 1, 2], [0, 1, 0]].tolist() == [2048] * 3
    assert [int(s) & _abi.EST_CAPPED for s in want["status"][[0, 1, 2], [0, 1, 0]]] == [_abi.EST_CAPPED, _abi.EST_CAPPED, 0]
    ref.assert_same_records(rows_to_estimates(offsets, rows, labels, [2, 5], settings, ctx), want)


def test_300_events_in_one_call(ctx, hand):
    events, want = hand
    order = np.random.default_rng(8).integers(0, len(events), size=300)
    got = rows_to_estimates(*_csr([events[i] for i in order]), INDICES8, _settings()[0], ctx)
    ref.assert_same_records(got, want[order])


def test_the_library_checks_its_arguments(ctx):
    out = np.empty((1, 1), dtype=_abi.ESTIMATE_DTYPE)
    layout = _abi.EventLayout()
    layout.n_sim = 1
    offsets = np.array([0, 0], dtype=np.int64)

    def call(desc, lay=layout, off=offsets):
        return ctx.lib.attpc_rows_estimate(ctx.handle, 1, _abi.iptr(off, _abi.C.c_int64), None, None, lay, desc,
                                           _abi.iptr(out, _abi.TrackEstimate))

    assert call(_abi.EstimateDesc(25.0, FIELD, 30, 0)) == _abi.OK and out["status"][0, 0] == _abi.EST_EMPTY
    for bad in ((-1.0, FIELD, 30, 0), (np.nan, FIELD, 30, 0), (25.0, np.nan, 30, 0), (25.0, FIELD, 2, 0), (25.0, FIELD, 30, 1)):
        assert call(_abi.EstimateDesc(*bad)) == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_estimates(ctx.handle, _abi.EstimateDesc(*bad)) == _abi.E_INVALID, bad
    wide = _abi.EventLayout()
    wide.n_sim = _abi.MAX_SIM + 1
    assert call(_abi.EstimateDesc(25.0, FIELD, 30, 0), lay=wide) == _abi.E_INVALID
    assert call(_abi.EstimateDesc(25.0, FIELD, 30, 0), off=np.array([3, 1], dtype=np.int64)) == _abi.E_INVALID


# ---------------------------------------------------------------- 2. fused ----
NOISY = {"noise_sigma": 5.0, "threshold": 20.0, "readout": "partial"}
ESTIMATES = EstimateSettings(20.0, 15)
PEAKS = PeakSettings(prominence=10.0, threshold=15.0)  # low enough for noise-only pads to make rows of label -1
N, SEED = 48, 29


def _trace_kw(inp):
    pedestals = np.random.default_rng(3).integers(200, 401, size=_abi.NUM_PADS).astype(np.int16)
    return {**NOISY, "pedestals": pedestals, "offset": int(np.argmax(get_response(inp.config)))}


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine

    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)
    eng.configure_traces(inp.config, **_trace_kw(inp))
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PEAKS)
    eng.configure_baseline()
    eng.configure_trigger()
    return eng


@pytest.fixture(scope="module")
def fused(ctx):
    """The delivered trace rows of 48 events of be10dp with noise and partial readout, the records the device made of
    them, and the restatement's records of the delivered rows (computed once, read-only)."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    res = eng.run_trace_rows(N, seed=SEED)
    params = ref.Params(ESTIMATES.beam_region_radius, ESTIMATES.min_points, inp.config.det_params.bfield)
    want = ref.records(res["offsets"], res["rows"], res["labels"], inp.indices, params)
    want.setflags(write=False)
    eng.configure_estimates()
    return inp, res, want, params


def test_fused_records_equal_the_restatement_of_the_delivered_rows(ctx, fused):
    inp, res, want, _ = fused
    ref.assert_same_records(res["estimates"], want)
    assert (res["labels"] == -1).any() and (want["status"] == 0).sum() >= 4 and (want["direction"] != 0).any()
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
    ref.assert_same_records(resident["estimates"], want)
    assert resident["trace_rows"] == res["trace_rows"] and "rows" not in resident
    only = eng.run_estimates(N, seed=SEED)
    ref.assert_same_records(only["estimates"], want)
    np.testing.assert_array_equal(only["p4"], res["p4"])
    np.testing.assert_array_equal(only["vertex"], res["vertex"])
    assert only["indices"] == list(inp.indices) and only["trace_rows"] == res["trace_rows"] and (only["status"] == res["status"]).all()
    shifted = eng.run_estimates(N, seed=SEED, first_event=10)["estimates"]
    ref.assert_same_records(shifted[:N - 10], want[10:])
    eng.configure_estimates()
    with pytest.raises(RuntimeError):
        eng.run_estimates(N, seed=SEED)


def test_fused_records_do_not_depend_on_chunks(ctx, fused):
    inp, res, want, _ = fused
    small = _engine(inp, ctx, chunk_events=16)  # 3 chunks
    small.configure_estimates(ESTIMATES)
    try:
        ref.assert_same_records(small.run_estimates(N, seed=SEED)["estimates"], want)
        chunked = small.run_trace_rows(N, seed=SEED)
        ref.assert_same_records(chunked["estimates"], want)
        np.testing.assert_array_equal(chunked["rows"], res["rows"])
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        small.configure_estimates()


def test_fused_gate_leaves_empty_records(ctx, fused):
    inp, res, want, params = fused
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
    reach = np.sort(eng.run_trace_rows(N, seed=SEED, fetch=False)["trigger"]["peak_group_sum"])
    middle = int(reach[N // 2])
    mg = max(1, middle + 1 if middle < reach[-1] else middle)  # about half of the events reach it
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=mg, gate=True))
    gated = eng.run_trace_rows(N, seed=SEED)
    fired = gated["trigger"]["fired"] != 0
    assert 0 < fired.sum() < N, reach.tolist()
    ref.assert_same_records(gated["estimates"], ref.records(gated["offsets"], gated["rows"], gated["labels"], inp.indices, params))
    assert (gated["estimates"]["status"][~fired] == _abi.EST_EMPTY).all() and (gated["estimates"]["n_rows"][~fired] == 0).all()
    ref.assert_same_records(gated["estimates"][fired], want[fired])
    eng.configure_trigger()
    eng.configure_estimates()


def test_off_nothing_moves(ctx, fused):
    inp, res, _, _ = fused
    out = np.empty(len(inp.indices), dtype=_abi.ESTIMATE_DTYPE)
    eng = _engine(inp, ctx)
    off = eng.run_trace_rows(N, seed=SEED)
    assert "estimates" not in off
    assert ctx.lib.attpc_estimates_last(ctx.handle, 0, 1, _abi.iptr(out, _abi.TrackEstimate)) == _abi.E_NOTCONFIGURED
    for key in ("rows", "labels", "offsets", "event_points", "p4", "vertex"):
        np.testing.assert_array_equal(off[key], res[key], err_msg=key)
    assert off["trace_rows"] == res["trace_rows"]
    eng.configure_estimates(ESTIMATES)
    on = eng.run_trace_rows(N, seed=SEED, fetch=False)
    assert on["trace_rows"] == off["trace_rows"]
    assert ctx.lib.attpc_estimates_last(ctx.handle, N, 1, _abi.iptr(out, _abi.TrackEstimate)) == _abi.E_INVALID
    assert ctx.lib.attpc_estimates_last(ctx.handle, N - 1, 1, _abi.iptr(out, _abi.TrackEstimate)) == _abi.OK
    ref.assert_same_records(out.reshape(1, -1), on["estimates"][N - 1:])
    eng.configure_estimates()


# ---------------------------------------------------------------- 3. the file-driven entry point ----
def test_simulate_batch_trace_rows_gives_the_fused_records(ctx, fused):
    inp, res, want, _ = fused
    off, rows, labels, raw, stats = simulate_batch_trace_rows(res["p4"], res["vertex"], inp.z, inp.a, inp.config, SEED, inp.indices,
                                                              ctx=ctx, peaks=PEAKS, estimates=ESTIMATES, **_trace_kw(inp))
    np.testing.assert_array_equal(rows, res["rows"])
    np.testing.assert_array_equal(off, res["offsets"])
    ref.assert_same_records(stats["estimates"], want)
    plain = simulate_batch_trace_rows(res["p4"][:4], res["vertex"][:4], inp.z, inp.a, inp.config, SEED, inp.indices, ctx=ctx,
                                      peaks=PEAKS, **_trace_kw(inp))
    assert "estimates" not in plain[4]  # estimates=None turns the stage off again
