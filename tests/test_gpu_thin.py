"""The thinned track points on the device (include/attpc_engine.h, "thinned track points") against their numpy
restatement (tests/thin_reference.py): points, labels, offsets and info equal; the estimates of thinned points bit for
bit as ``assert_same_records`` compares.  The stage alone on hand-made rows at the shapes where the kernel can go wrong
(``rows_to_points``); the fused path on its own delivered rows, resident, in chunks, behind a gating trigger, and with
nothing else moving; ``simulate_batch_trace_rows(estimates=, thinning=)``.  A fused run cannot contain a row that is
out of range, so the dropped rows are tested on the stage alone (``n_dropped``, from which the fused path sets RANGE).
Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from attpc_engine_amd.detector.traces import TriggerSettings, simulate_batch_trace_rows
from tests import estimate_reference as est
from tests import thin_reference as ref
from tests.helpers import Inputs
from tests.test_gpu_estimate import N, PEAKS, SEED, _engine, _trace_kw

pytestmark = pytest.mark.gpu

INDICES8 = [2, 5, 3, 2, 7, 9, 11, 4]  # n_sim = 8: every wave takes two positions; label 2 is given twice
H = 80  # units of a 5 mm step


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
def _runs(rng, runs, step=H):
    """Rows [n, 8] of consecutive runs [(bin, rows)]: z anywhere in the bin, x and y off the quantisation grid,
    integrals with ties of rint and some below 1, amplitudes with some NaN."""
    bins = np.concatenate([np.full(count, b, dtype=np.int64) for b, count in runs])
    n = len(bins)
    rows = np.zeros((n, 8))
    rows[:, 0], rows[:, 1] = rng.uniform(-319.0, 319.0, n), rng.uniform(-319.0, 319.0, n)
    rows[:, 2] = (bins * step + rng.integers(0, step, n)) / 16.0
    rows[:, 3] = np.where(rng.random(n) < 0.1, np.nan, rng.uniform(5.0, 900.0, n))
    rows[:, 4] = np.where(rng.random(n) < 0.15, rng.integers(-40, 2, n), rng.integers(2, 4000, n) + 0.5)
    return rows


def _labelled(rows, label):
    return rows, np.full(len(rows), label, dtype=np.int64)


def _mix(rng, tracks, p_other=0.0):
    """The rows of ``tracks`` [(rows, label)] merged in random order (each track's own order kept), with rows of label
    -1 and 99 (not in the indices) strewn in at the rate ``p_other``."""
    tracks = list(tracks)
    total = sum(len(r) for r, _ in tracks)
    if p_other:
        for label in (-1, 99):
            tracks.append(_labelled(_runs(rng, [(0, max(1, int(p_other * total)))]), label))
    which = rng.permutation(np.concatenate([np.full(len(r), i) for i, (r, _) in enumerate(tracks)]))
    at = [0] * len(tracks)
    rows, labels = [], []
    for i in which:
        rows.append(tracks[i][0][at[i]])
        labels.append(tracks[i][1][at[i]])
        at[i] += 1
    return np.array(rows).reshape(-1, 8), np.array(labels, dtype=np.int64)


def _hand_events(rng):
    events = []
    # a run over lanes 62 .. 65; runs of exactly one aligned tile; a run of 130 rows behind 7
    events.append(_labelled(_runs(rng, [(0, 62), (1, 4), (2, 10)]), 2))
    events.append(_labelled(_runs(rng, [(0, 64), (1, 64), (2, 64)]), 5))
    events.append(_labelled(_runs(rng, [(-3, 7), (-2, 130), (4, 1)]), 3))
    # single-row runs: P = R (two tiles and a partial one)
    events.append(_labelled(_runs(rng, [(b, 1) for b in range(150)]), 7))
    # rows of another label and of -1 inside the runs, whatever lies at the tile edges
    events.append(_mix(rng, [_labelled(_runs(rng, [(b, int(c)) for b, c in enumerate(rng.integers(1, 40, 12))]), 5),
                             _labelled(_runs(rng, [(b, int(c)) for b, c in enumerate(rng.integers(1, 70, 9))]), 3)], 0.3))
    other = _labelled(_runs(rng, [(0, 200)]), 9)
    other[1][[63, 64, 65, 127, 128]] = [-1, 4, -1, 99, -1]  # ... and at the tile edges for certain
    events.append(other)
    # a run that ends on the event's last row in a partial tile
    events.append(_labelled(_runs(rng, [(0, 60), (1, 10)]), 11))
    # negative z and the bin edges
    edges = _runs(rng, [(0, 12)])
    edges[:, 2] = np.array([-161, -160, -81, -80, -79, -1, 0, 1, 79, 80, 81, 160]) / 16.0
    events.append(_labelled(edges, 4))
    # integrals <= 0 only, and all zero; amplitudes all NaN
    low = _runs(rng, [(0, 20), (1, 20), (2, 70)])
    low[:20, 4], low[20:40, 4], low[40:, 3] = 0.0, rng.integers(-500, 1, 20), np.nan
    events.append(_labelled(low, 2))
    # dropped rows: inside a run, at its start, a whole run, at a tile edge
    bad = _runs(rng, [(0, 30), (1, 5), (2, 40), (3, 30)])
    bad[3, 0], bad[30, 2], bad[31, 4], bad[35:75, 1], bad[63, 0], bad[64, 2], bad[104, 4] = 321.0, np.nan, 2.0 ** 31, -320.5, np.inf, 9000.0, -2.0 ** 31
    events.append(_labelled(bad, 5))
    # a bin of 4097 rows and one of 8193 rows, off the tile grid and with other rows between
    events.append(_mix(rng, [_labelled(_runs(rng, [(2, 5), (3, 4097), (4, 3)]), 7)], 0.02))
    events.append(_labelled(_runs(rng, [(1, 37), (4, 8193), (5, 2)]), 9))
    events.append(_labelled(_runs(rng, [(4, 4096), (5, 4096), (5, 1)]), 9))  # 4096 ended by a change of bin, then a split
    # unsorted rows
    events.append(_labelled(_runs(rng, [(int(b), 1) for b in rng.integers(-4, 4, 300)]), 3))
    # all seven labels in one event; no rows; no participating row
    events.append(_mix(rng, [_labelled(_runs(rng, [(b, int(c)) for b, c in enumerate(rng.integers(1, 30, 6 + s))]), label)
                             for s, label in enumerate((2, 5, 3, 7, 9, 11, 4))], 0.1))
    events.append((np.zeros((0, 8)), np.zeros(0, dtype=np.int64)))
    events.append(_labelled(_runs(rng, [(0, 70)]), 99))
    events[-1][1][::3] = -1
    return events


def _csr(events):
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in events])])
    return offsets, np.concatenate([r for r, _ in events]), np.concatenate([l for _, l in events])


@pytest.fixture(scope="module")
def hand():
    """The hand-made events and the reference's points of every one of them (computed once, read-only)."""
    events = _hand_events(np.random.default_rng(23))
    want = ref.thin(*_csr(events), INDICES8, 5.0)
    for array in want:
        array.setflags(write=False)
    return events, want


def _of_events(want, order):
    """The reference's result for the events ``order`` of the hand-made set in one call."""
    off, pts, lab, info = want
    pieces = [(pts[off[i]:off[i + 1]], lab[off[i]:off[i + 1]]) for i in order]
    return (np.concatenate([[0], np.cumsum([len(p) for p, _ in pieces])]), np.concatenate([p for p, _ in pieces]),
            np.concatenate([l for _, l in pieces]), info[list(order)])


def test_stage_alone_on_hand_made_rows(ctx, hand):
    events, want = hand
    got = rows_to_points(*_csr(events), INDICES8, ThinSettings(5.0), ctx)
    ref.assert_same_points(got, want)
    off, pts, lab, info = want
    # the cases are there
    assert info["n_points"][0, 0] == 3 and pts[off[1]:off[2], 5].tolist() == [64, 64, 64] and 130 in pts[off[2]:off[3], 5]
    assert info[3, 4].tolist() == (150, 150, 0, 0) and (info["n_rows"][:, 3] == 0).all()  # P = R; the second position of label 2
    assert info[9, 1]["n_dropped"] == 44 and info["n_dropped"].sum() == 44
    assert info[10, 4]["n_split"] == 2 and info[11, 5]["n_split"] == 3 and info[12, 5]["n_split"] == 2
    assert pts[off[11]:off[12], 5].tolist() == [37, 4096, 4096, 1, 2] and pts[off[11]:off[12], 7].tolist() == [0, 1, 1, 0, 0]
    assert pts[off[12]:off[13], 5].tolist() == [4096, 4096, 1] and pts[off[12]:off[13], 7].tolist() == [0, 1, 0]
    assert (pts[:, 6] < 0).any() and np.isnan(pts[:, 3]).any() and (pts[:, 4] <= 0).any() and (info[14]["n_points"] > 0).sum() == 7
    assert not info[15]["n_rows"].any() and not info[16]["n_rows"].any() and off[15] == off[17]
    # one event alone, three in one call: nothing of a neighbour is left
    for order in ([4], [11], [5, 15, 9]):
        ref.assert_same_points(rows_to_points(*_csr([events[i] for i in order]), INDICES8, ThinSettings(5.0), ctx), _of_events(want, order))
    empty = rows_to_points([0], np.zeros((0, 8)), np.zeros(0), INDICES8, ThinSettings(5.0), ctx)
    assert empty[0].tolist() == [0] and empty[1].shape == (0, 8) and empty[3].shape == (0, 8)
    # other positions: two of them, an absent label
    offsets, rows, labels = _csr(events[:10])
    ref.assert_same_points(rows_to_points(offsets, rows, labels, [5, 17, 2], ThinSettings(5.0), ctx), ref.thin(offsets, rows, labels, [5, 17, 2], 5.0))


@pytest.mark.parametrize("z_step", [1.0 / 16.0, 512.0, 0.7])
def test_smallest_and_largest_step_and_the_bound_case(ctx, hand, z_step):
    events, _ = hand
    rng = np.random.default_rng(41)
    top = _runs(rng, [(0, 4096), (0, 10)])
    top[:, 2], top[:, 4] = 8192.0, 2.0 ** 31 - 1.0  # w = 2^31 - 1, Z = 2^17, 4096 rows: |Sz| at its bound
    bottom = top.copy()
    bottom[:, 2] = -8192.0
    wide = _runs(rng, [(b, 3) for b in range(-16, 16)], step=8192)  # the whole z range
    more = [_labelled(top, 2), _labelled(bottom, 5), _labelled(wide, 3)] + [events[i] for i in (0, 2, 4, 7, 9, 13, 14)]
    offsets, rows, labels = _csr(more)
    want = ref.thin(offsets, rows, labels, INDICES8, z_step)
    ref.assert_same_points(rows_to_points(offsets, rows, labels, INDICES8, ThinSettings(z_step), ctx), want)
    assert want[3]["n_split"][0, 0] == 2 and want[1][0, 4] == 4096.0 * (2.0 ** 31 - 1.0) and want[1][0, 2] == 8192.0
    assert want[1][want[0][1], 2] == -8192.0


def test_300_events_in_one_call(ctx, hand):
    events, want = hand
    order = np.random.default_rng(8).integers(0, len(events), size=300)
    got = rows_to_points(*_csr([events[i] for i in order]), INDICES8, ThinSettings(5.0), ctx)
    ref.assert_same_points(got, _of_events(want, order))


def test_points_are_rows_of_the_estimates(ctx, hand):
    """The composition the fused contract is defined by, on the hand-made rows: device points into the device's
    estimates against the restatements of both."""
    events, want = hand
    settings, params = EstimateSettings(25.0, 3, magnetic_field=2.85), est.Params(25.0, 3, 2.85)
    off, pts, lab, _ = rows_to_points(*_csr(events), INDICES8, ThinSettings(5.0), ctx)
    records = rows_to_estimates(off, pts, lab, INDICES8, settings, ctx)
    est.assert_same_records(records, est.records(want[0], want[1], want[2], INDICES8, params))
    assert (records["status"] == 0).sum() >= 5


def test_the_library_checks_its_arguments_and_the_capacity(ctx, hand):
    events, want = hand
    layout = _abi.EventLayout()
    layout.n_sim = 8
    for s, index in enumerate(INDICES8):
        layout.indices[s] = index
    i64 = _abi.C.c_int64
    offsets, rows, labels = _csr(events[3:4])  # single-row runs: P = R = 150
    R = len(rows)

    def call(desc=_abi.ThinDesc(5.0, 0, 0), lay=layout, off=offsets, capacity=R):
        out = (np.zeros(2, dtype=np.int64), np.full((R, 8), -7.0), np.zeros(R, dtype=np.int64), np.zeros((1, lay.n_sim if lay.n_sim <= 8 else 8), dtype=_abi.THIN_INFO_DTYPE),
               np.full(1, -1, dtype=np.int64))
        rc = ctx.lib.attpc_rows_thin(ctx.handle, 1, _abi.iptr(off, i64), _abi.dptr(rows), _abi.iptr(labels, i64), lay, desc, capacity,
                                     _abi.iptr(out[0], i64), _abi.dptr(out[1]), _abi.iptr(out[2], i64), _abi.iptr(out[3], _abi.ThinInfo),
                                     _abi.iptr(out[4], i64))
        return rc, out

    rc, out = call()
    assert rc == _abi.OK and out[4][0] == R and out[0].tolist() == [0, R]
    np.testing.assert_array_equal(out[1], _of_events(want, [3])[1])
    rc, out = call(capacity=R - 1)
    assert rc == _abi.E_CAPACITY and out[4][0] == R and out[0].tolist() == [0, R] and out[3]["n_points"][0, 4] == R
    np.testing.assert_array_equal(out[1][:R - 1], _of_events(want, [3])[1][:R - 1])
    assert (out[1][R - 1] == -7.0).all()  # nothing behind the capacity was written
    for bad in ((0.0, 0, 0), (0.06, 0, 0), (513.0, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (5.0, 1, 0), (5.0, 0, 1)):
        assert call(_abi.ThinDesc(*bad))[0] == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_thinning(ctx.handle, _abi.ThinDesc(*bad)) == _abi.E_INVALID, bad
    wide = _abi.EventLayout()
    wide.n_sim = _abi.MAX_SIM + 1
    assert call(lay=wide)[0] == _abi.E_INVALID
    assert call(off=np.array([3, 1], dtype=np.int64))[0] == _abi.E_INVALID
    assert call(capacity=-1)[0] == _abi.E_INVALID
    with pytest.raises(TypeError):
        rows_to_points(offsets, rows, labels, INDICES8, 5.0, ctx)


# ---------------------------------------------------------------- 2. fused ----
ESTIMATES = EstimateSettings(20.0, 8)
THINNING = ThinSettings(5.0)


@pytest.fixture(scope="module")
def fused(ctx):
    """The delivered trace rows of 48 events of be10dp with noise and partial readout, the records the device made of
    their thinned points, and the restatement's records (computed once, read-only)."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_thinning(THINNING)
    res = eng.run_trace_rows(N, seed=SEED)
    params = est.Params(ESTIMATES.beam_region_radius, ESTIMATES.min_points, inp.config.det_params.bfield)
    want = ref.fused_records(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING.z_step, params)
    want.setflags(write=False)
    eng.configure_estimates()
    eng.configure_thinning()
    return inp, res, want, params


def _thinned_engine(inp, ctx, **kw):
    eng = _engine(inp, ctx, **kw)
    eng.configure_estimates(ESTIMATES)
    eng.configure_thinning(THINNING)
    return eng


def _off(eng):
    eng.configure_estimates()
    eng.configure_thinning()


def test_fused_records_equal_the_restatement_of_the_delivered_rows(ctx, fused):
    inp, res, want, params = fused
    est.assert_same_records(res["estimates"], want)
    assert res["thinning"] == 5.0 and (res["labels"] == -1).any() and (want["status"] == 0).sum() >= 4
    raw = est.records(res["offsets"], res["rows"], res["labels"], inp.indices, params)
    assert (want["n_rows"] <= raw["n_rows"]).all() and (want["n_rows"] < raw["n_rows"]).any()  # points, not rows
    eng = _thinned_engine(inp, ctx)
    resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
    est.assert_same_records(resident["estimates"], want)
    assert resident["trace_rows"] == res["trace_rows"] and resident["thinning"] == 5.0 and "rows" not in resident
    only = eng.run_estimates(N, seed=SEED)
    est.assert_same_records(only["estimates"], want)
    assert only["thinning"] == 5.0 and only["trace_rows"] == res["trace_rows"]
    np.testing.assert_array_equal(only["p4"], res["p4"])
    # the composition of the two stages alone on the delivered rows gives the fused records
    points = rows_to_points(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING, ctx)
    assert not points[3]["n_dropped"].any()
    alone = rows_to_estimates(*points[:3], inp.indices, ESTIMATES, ctx, config=inp.config)
    est.assert_same_records(alone, want)
    _off(eng)


def test_fused_records_do_not_depend_on_chunks(ctx, fused):
    inp, res, want, _ = fused
    small = _thinned_engine(inp, ctx, chunk_events=16)  # 3 chunks
    try:
        est.assert_same_records(small.run_estimates(N, seed=SEED)["estimates"], want)
        chunked = small.run_trace_rows(N, seed=SEED)
        est.assert_same_records(chunked["estimates"], want)
        np.testing.assert_array_equal(chunked["rows"], res["rows"])
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        _off(small)


def test_fused_gate_leaves_empty_records(ctx, fused):
    inp, res, want, params = fused
    eng = _thinned_engine(inp, ctx)
    eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
    reach = np.sort(eng.run_trace_rows(N, seed=SEED, fetch=False)["trigger"]["peak_group_sum"])
    middle = int(reach[N // 2])
    mg = max(1, middle + 1 if middle < reach[-1] else middle)  # about half of the events reach it
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=mg, gate=True))
    gated = eng.run_trace_rows(N, seed=SEED)
    fired = gated["trigger"]["fired"] != 0
    assert 0 < fired.sum() < N, reach.tolist()
    est.assert_same_records(gated["estimates"], ref.fused_records(gated["offsets"], gated["rows"], gated["labels"], inp.indices, 5.0, params))
    assert (gated["estimates"]["status"][~fired] == _abi.EST_EMPTY).all() and (gated["estimates"]["n_rows"][~fired] == 0).all()
    est.assert_same_records(gated["estimates"][fired], want[fired])
    eng.configure_trigger()
    _off(eng)


def test_thinning_moves_nothing_else_and_is_inert_alone(ctx, fused):
    inp, res, want, params = fused
    out = np.empty(len(inp.indices), dtype=_abi.ESTIMATE_DTYPE)
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    plain = eng.run_trace_rows(N, seed=SEED)  # the estimates without thinning: the raw rows' records, nothing else differs
    assert "thinning" not in plain
    est.assert_same_records(plain["estimates"], est.records(res["offsets"], res["rows"], res["labels"], inp.indices, params))
    for key in ("rows", "labels", "offsets", "event_points", "p4", "vertex"):
        np.testing.assert_array_equal(plain[key], res[key], err_msg=key)
    assert plain["trace_rows"] == res["trace_rows"]
    eng.configure_estimates()
    eng.configure_thinning(THINNING)  # thinning without the estimates
    alone = eng.run_trace_rows(N, seed=SEED)
    assert "estimates" not in alone and "thinning" not in alone and alone["trace_rows"] == res["trace_rows"]
    assert ctx.lib.attpc_estimates_last(ctx.handle, 0, 1, _abi.iptr(out, _abi.TrackEstimate)) == _abi.E_NOTCONFIGURED
    np.testing.assert_array_equal(alone["rows"], res["rows"])
    eng.configure_thinning()


# ---------------------------------------------------------------- 3. the file-driven entry point ----
def test_simulate_batch_trace_rows_gives_the_fused_records(ctx, fused):
    inp, res, want, params = fused
    kw = dict(ctx=ctx, peaks=PEAKS, **_trace_kw(inp))
    off, rows, labels, raw, stats = simulate_batch_trace_rows(res["p4"], res["vertex"], inp.z, inp.a, inp.config, SEED, inp.indices,
                                                              estimates=ESTIMATES, thinning=THINNING, **kw)
    np.testing.assert_array_equal(rows, res["rows"])
    np.testing.assert_array_equal(off, res["offsets"])
    est.assert_same_records(stats["estimates"], want)
    assert stats["thinning"] == 5.0
    plain = simulate_batch_trace_rows(res["p4"][:8], res["vertex"][:8], inp.z, inp.a, inp.config, SEED, inp.indices, estimates=ESTIMATES, **kw)
    assert "thinning" not in plain[4]  # thinning=None turns the stage off again: the raw rows' records
    est.assert_same_records(plain[4]["estimates"], est.records(off[:9], rows, labels, inp.indices, params))
    simulate_batch_trace_rows(res["p4"][:2], res["vertex"][:2], inp.z, inp.a, inp.config, SEED, inp.indices, **kw)  # (both off again)
