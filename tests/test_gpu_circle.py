"""The geometric circle fit on the device (include/attpc_engine.h, "geometric circle fit") against its numpy
restatement (tests/circle_reference.py): integer fields equal, f64 fields bit for bit, NaN in the same places -- the
device is never measured against a tolerance.  The stage alone on hand-made rows at the shapes where the kernel can go
wrong (``rows_to_estimates(circle=)``); the thinned points through the stage alone against the fused records; the fused
path on its own delivered rows, in chunks and behind a gating trigger; and with the stage off nothing moves.  Needs a
real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from attpc_engine_amd.detector.traces import TriggerSettings, simulate_batch_trace_rows
from tests import circle_reference as ref
from tests import estimate_reference as est
from tests import thin_reference as thin
from tests.helpers import Inputs
from tests.test_gpu_estimate import INDICES8, PEAKS, _csr, _engine, _interleave, _trace_kw, _track

pytestmark = pytest.mark.gpu

FIELD = 2.85
CIRCLE = CircleFitSettings()
CIRCLE_REF = ref.Settings()


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _settings(radius=25.0, min_points=3):
    return EstimateSettings(radius, min_points, magnetic_field=FIELD), est.Params(radius, min_points, FIELD)


# ---------------------------------------------------------------- 6. the stage alone, hand-made rows ----
SHORT_ARC = dict(radius_mm=300.0, centre_mm=(330.0, 20.0), turn=0.7)  # the segment, its first half, spans 20 degrees


def _hand_events(rng):
    """With min_points = 3 the segment has m = (n_used + 1) div 2 rows: m = 3, 63, 64, 65 and 129."""
    events = []
    events.append(_interleave(rng, [(_track(rng, 5, jitter=0.0), 2), (_track(rng, 125, **SHORT_ARC), 5), (_track(rng, 127), 3)]))
    events.append(_interleave(rng, [(_track(rng, 129, backward=True), 7), (_track(rng, 257, **SHORT_ARC), 9)], 40))
    # rows of the beam region between used rows: single ones, a run across a tile edge, a run of more than a tile
    events.append((_track(rng, 140, unused=[(1, 1), (5, 3), (60, 10), (70, 100), (139, 2)], **SHORT_ARC), np.full(256, 4, dtype=np.int64)))
    events.append((_track(rng, 140, backward=True, unused=[(0, 5), (80, 70), (139, 1)]), np.full(216, 3, dtype=np.int64)))
    i = np.arange(45)
    events.append((est.spyral_rows(480 + 9 * i, 12 * i, 300 + 21 * i), np.full(45, 9, dtype=np.int64)))  # collinear
    events.append((np.zeros((0, 8)), np.zeros(0, dtype=np.int64)))  # no rows
    # all eight positions in one event: waves take positions s and s + 4; label 2 is given twice
    events.append(_interleave(rng, [(_track(rng, 40 + 13 * s, backward=bool(s % 2), phase=3.3 + 0.3 * s), label)
                                    for s, label in enumerate((2, 5, 3, 7, 9, 11, 4))], 25))
    return events


@pytest.fixture(scope="module")
def hand():
    """The hand-made events and their reference records (computed once, read-only)."""
    events = _hand_events(np.random.default_rng(24))
    assert max(len(r) for r, _ in events) <= 2100
    want = ref.records(*_csr(events), INDICES8, _settings()[1], CIRCLE_REF)
    want.setflags(write=False)
    return events, want


def test_stage_alone_on_hand_made_rows(ctx, hand):
    events, want = hand
    settings, params = _settings()
    got = rows_to_estimates(*_csr(events), INDICES8, settings, ctx, circle=CIRCLE)
    est.assert_same_records(got, want)
    # the cases are there
    status, fitted = want["status"], want["reserved"] > 0
    assert {3, 63, 64, 65, 129} <= set(want["n_fit"][fitted].tolist()) and {1, -1} <= set(want["direction"][fitted].tolist())
    assert fitted.sum() >= 14 and (want["reserved"][fitted] >= 2).all() and not (status[fitted] & _abi.EST_NO_CIRCLE).any()
    assert status[4, 5] & _abi.EST_NO_CIRCLE and want["reserved"][4, 5] == 0 and (status[5] == _abi.EST_EMPTY).all()
    assert (status[:, 3] == _abi.EST_EMPTY).all() and (want["reserved"][~fitted] == 0).all()
    assert fitted[6, [0, 1, 2, 4, 5, 6, 7]].all()  # both positions of every wave
    # the refinement moved the circles, and nothing that does not depend on the circle
    plain = est.records(*_csr(events), INDICES8, params)
    assert (got["radius"][fitted] != plain["radius"][fitted]).mean() > 0.9
    for name in ("n_rows", "n_used", "n_fit", "direction", "charge", "arc"):
        np.testing.assert_array_equal(got[name], plain[name], err_msg=name)
    for name in ("slope", "x_mean", "y_mean", "dedx"):
        np.testing.assert_array_equal(got[name].view(np.int64), plain[name].view(np.int64), err_msg=name)
    # one event alone, and the stage off through the same call path: the records of attpc_rows_estimate
    est.assert_same_records(rows_to_estimates(*_csr(events[2:3]), INDICES8, settings, ctx, circle=CIRCLE), want[2:3])
    est.assert_same_records(rows_to_estimates(*_csr(events), INDICES8, settings, ctx), plain)
    assert rows_to_estimates([0], np.zeros((0, 8)), np.zeros(0), INDICES8, settings, ctx, circle=CIRCLE).shape == (0, 8)


def test_two_evaluations_and_a_loose_tolerance(ctx, hand):
    events, want = hand
    settings, params = _settings()
    offsets, rows, labels = _csr(events)
    two = rows_to_estimates(offsets, rows, labels, INDICES8, settings, ctx, circle=CircleFitSettings(max_evaluations=2))
    want_two = ref.records(offsets, rows, labels, INDICES8, params, ref.Settings(max_evaluations=2))
    est.assert_same_records(two, want_two)
    ran = want_two["reserved"] > 0
    assert (want_two["reserved"][ran] == 2).all() and (want_two["status"][ran] & _abi.EST_NOT_CONVERGED).mean() > 0.5
    assert not (want["status"] & _abi.EST_NOT_CONVERGED).any()  # with the defaults every one of them converges
    loose = rows_to_estimates(offsets, rows, labels, INDICES8, settings, ctx, circle=CircleFitSettings(64, 50.0))
    est.assert_same_records(loose, ref.records(offsets, rows, labels, INDICES8, params, ref.Settings(64, 50.0)))


def test_a_segment_of_2048_rows(ctx):
    """min_points = 2048 and 2100 used rows: m = 2048, every word of the wave's LDS, 32 terms in every lane."""
    rng = np.random.default_rng(5)
    settings, params = _settings(25.0, 2048)
    forward = _track(rng, 2100, jitter=1.0, turn=4.0, dz_mm=0.3)
    events = [(forward, np.full(2100, 2, dtype=np.int64)),
              (_track(rng, 2100, backward=True, jitter=1.0, turn=1.2, dz_mm=0.3, radius_mm=160.0, centre_mm=(190.0, 10.0)),
               np.full(2100, 5, dtype=np.int64))]
    offsets, rows, labels = _csr(events)
    want = ref.records(offsets, rows, labels, [2, 5], params, CIRCLE_REF)
    assert want["n_fit"][[0, 1], [0, 1]].tolist() == [est.EST_MAX_FIT] * 2 and (want["reserved"][[0, 1], [0, 1]] >= 2).all()
    assert not (want["status"] & _abi.EST_CAPPED).any()
    est.assert_same_records(rows_to_estimates(offsets, rows, labels, [2, 5], settings, ctx, circle=CIRCLE), want)


def test_300_events_in_one_call(ctx, hand):
    events, want = hand
    order = np.random.default_rng(8).integers(0, len(events), size=300)
    got = rows_to_estimates(*_csr([events[i] for i in order]), INDICES8, _settings()[0], ctx, circle=CIRCLE)
    est.assert_same_records(got, want[order])


def test_the_library_checks_its_arguments(ctx):
    out = np.empty((1, 1), dtype=_abi.ESTIMATE_DTYPE)
    layout = _abi.EventLayout()
    layout.n_sim = 1
    offsets = np.array([0, 0], dtype=np.int64)
    good = _abi.EstimateDesc(25.0, FIELD, 30, 0)

    def call(circle, desc=good):
        return ctx.lib.attpc_rows_estimate_circle(ctx.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, layout, desc, circle,
                                                  _abi.iptr(out, _abi.TrackEstimate))

    assert call(_abi.CircleDesc(2.0 ** -7, 32, 0)) == _abi.OK and out["status"][0, 0] == _abi.EST_EMPTY and out["reserved"][0, 0] == 0
    assert call(None) == _abi.E_INVALID and call(_abi.CircleDesc(1.0, 32, 0), _abi.EstimateDesc(25.0, FIELD, 2, 0)) == _abi.E_INVALID
    for bad in ((0.0, 32, 0), (-1.0, 32, 0), (np.nan, 32, 0), (np.inf, 32, 0), (1.0, 1, 0), (1.0, 65, 0), (1.0, 32, 1)):
        assert call(_abi.CircleDesc(*bad)) == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_circle(ctx.handle, _abi.CircleDesc(*bad)) == _abi.E_INVALID, bad


# ---------------------------------------------------------------- 7. and 8. fused ----
ESTIMATES = EstimateSettings(20.0, 15)
THINNED_ESTIMATES = EstimateSettings(20.0, 8)
THINNING = ThinSettings(5.0)
N, N_THINNED, SEED = 48, 200, 29


def _params(inp, estimates):
    return est.Params(estimates.beam_region_radius, estimates.min_points, inp.config.det_params.bfield)


def _off(eng):
    eng.configure_estimates()
    eng.configure_thinning()
    eng.configure_circle_fit()


def _thinned_want(res, inp, params):
    """The fused records with thinning and the circle fit both on: this contract on the event's point rows, RANGE
    OR-ed in where thinning dropped a row of the label."""
    point_offsets, points, point_labels, info = thin.thin(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING.z_step)
    records = ref.records(point_offsets, points, point_labels, inp.indices, params, CIRCLE_REF)
    records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    return records


@pytest.fixture(scope="module")
def fused(ctx):
    """48 events of be10dp with noise and partial readout, the estimates and the circle fit on: the delivered rows, the
    device's records and the restatement's records of the delivered rows (computed once, read-only)."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_circle_fit(CIRCLE)
    res = eng.run_trace_rows(N, seed=SEED)
    want = ref.records(res["offsets"], res["rows"], res["labels"], inp.indices, _params(inp, ESTIMATES), CIRCLE_REF)
    want.setflags(write=False)
    _off(eng)
    return inp, res, want


@pytest.fixture(scope="module")
def fused_thinned(ctx):
    """200 events with thinning on as well: the records are those of the thinned points."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    eng.configure_estimates(THINNED_ESTIMATES)
    eng.configure_thinning(THINNING)
    eng.configure_circle_fit(CIRCLE)
    res = eng.run_trace_rows(N_THINNED, seed=SEED)
    want = _thinned_want(res, inp, _params(inp, THINNED_ESTIMATES))
    want.setflags(write=False)
    _off(eng)
    return inp, res, want


def test_points_through_the_stage_alone_equal_the_fused_records(ctx, fused_thinned):
    inp, res, want = fused_thinned
    assert res["circle"] == "geometric" and res["thinning"] == 5.0
    points = rows_to_points(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING, ctx)
    assert not points[3]["n_dropped"].any()
    alone = rows_to_estimates(*points[:3], inp.indices, THINNED_ESTIMATES, ctx, config=inp.config, circle=CIRCLE)
    est.assert_same_records(alone, res["estimates"])


def test_fused_records_equal_the_restatement_of_the_delivered_rows(ctx, fused, fused_thinned):
    inp, res, want = fused
    est.assert_same_records(res["estimates"], want)
    ran = want["reserved"] > 0
    assert res["circle"] == "geometric" and "thinning" not in res and ran.sum() >= 4 and (want["reserved"][~ran] == 0).all()
    inp, res_thinned, want_thinned = fused_thinned
    est.assert_same_records(res_thinned["estimates"], want_thinned)
    assert (want_thinned["reserved"] > 0).sum() >= 40
    # resident, and the estimates alone
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_circle_fit(CIRCLE)
    resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
    est.assert_same_records(resident["estimates"], want)
    assert resident["trace_rows"] == res["trace_rows"] and resident["circle"] == "geometric" and "rows" not in resident
    shifted = eng.run_estimates(N, seed=SEED, first_event=10)
    est.assert_same_records(shifted["estimates"][:N - 10], want[10:])
    assert shifted["circle"] == "geometric"
    _off(eng)
    # the file-driven entry point
    stats = simulate_batch_trace_rows(res["p4"], res["vertex"], inp.z, inp.a, inp.config, SEED, inp.indices, ctx=ctx, peaks=PEAKS,
                                      estimates=ESTIMATES, circle=CIRCLE, **_trace_kw(inp))[4]
    est.assert_same_records(stats["estimates"], want)
    assert stats["circle"] == "geometric"


def test_fused_records_do_not_depend_on_chunks(ctx, fused, fused_thinned):
    inp, res, want = fused
    _, res_thinned, want_thinned = fused_thinned
    small = _engine(inp, ctx, chunk_events=16)  # 3 chunks of the 48 events, 13 of the 200
    small.configure_estimates(ESTIMATES)
    small.configure_circle_fit(CIRCLE)
    try:
        chunked = small.run_trace_rows(N, seed=SEED)
        est.assert_same_records(chunked["estimates"], want)
        np.testing.assert_array_equal(chunked["rows"], res["rows"])
        small.configure_estimates(THINNED_ESTIMATES)
        small.configure_thinning(THINNING)
        est.assert_same_records(small.run_estimates(N_THINNED, seed=SEED)["estimates"], want_thinned)
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        _off(small)


def test_fused_gate_leaves_empty_records(ctx, fused):
    inp, res, want = fused
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_circle_fit(CIRCLE)
    eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
    reach = np.sort(eng.run_trace_rows(N, seed=SEED, fetch=False)["trigger"]["peak_group_sum"])
    middle = int(reach[N // 2])
    mg = max(1, middle + 1 if middle < reach[-1] else middle)  # about half of the events reach it
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=mg, gate=True))
    gated = eng.run_trace_rows(N, seed=SEED)
    fired = gated["trigger"]["fired"] != 0
    assert 0 < fired.sum() < N, reach.tolist()
    empty = gated["estimates"][~fired]
    assert (empty["status"] == _abi.EST_EMPTY).all() and (empty["n_rows"] == 0).all() and (empty["reserved"] == 0).all()
    est.assert_same_records(gated["estimates"][fired], want[fired])
    eng.configure_trigger()
    _off(eng)


# ---------------------------------------------------------------- 9. off, nothing moves ----
def test_off_nothing_moves(ctx, fused):
    inp, res, _ = fused
    fresh = _abi.Context(0)  # a context that never saw the stage
    never = _engine(inp, fresh)
    never.configure_estimates(ESTIMATES)
    base = never.run_trace_rows(N, seed=SEED)
    assert "circle" not in base
    eng = _engine(inp, ctx)
    eng.configure_estimates(ESTIMATES)
    eng.configure_circle_fit(CIRCLE)
    eng.configure_circle_fit()  # on, then off again
    assert ctx.lib.attpc_trace_configure_circle(ctx.handle, None) == _abi.OK
    off = eng.run_trace_rows(N, seed=SEED)
    assert "circle" not in off
    for key in ("rows", "labels", "offsets", "event_points", "p4", "vertex"):
        np.testing.assert_array_equal(off[key], base[key], err_msg=key)
        np.testing.assert_array_equal(res[key], base[key], err_msg=key)  # nor does the stage on move them
    assert off["trace_rows"] == base["trace_rows"] == res["trace_rows"]
    assert off["estimates"].tobytes() == base["estimates"].tobytes() and (off["estimates"]["reserved"] == 0).all()
    est.assert_same_records(base["estimates"], est.records(base["offsets"], base["rows"], base["labels"], inp.indices, _params(inp, ESTIMATES)))
    # alone, without the estimates, the stage is inert
    eng.configure_estimates()
    eng.configure_circle_fit(CIRCLE)
    alone = eng.run_trace_rows(N, seed=SEED, fetch=False)
    assert "estimates" not in alone and "circle" not in alone and alone["trace_rows"] == base["trace_rows"]
    _off(eng)
