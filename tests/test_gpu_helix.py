"""The helix slope on the device (include/attpc_engine.h, "helix slope") against its numpy restatement
(tests/helix_reference.py): integer fields equal, f64 fields bit for bit, NaN in the same places -- the device is never
measured against a tolerance.  The stage alone on hand-made rows at the shapes where the kernel can go wrong
(``rows_to_estimates(helix=)``), behind the Kasa circle and behind the geometric circle fit, with every regressor; the
same on thinned points; the fused path on its own delivered rows, in one call, two calls and chunks, at event ids past
2^32; and with the stage off nothing moves.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from tests import circle_reference as circ
from tests import estimate_reference as est
from tests import helix_cases as cases
from tests import helix_reference as ref
from tests import thin_reference as thin
from tests.helix_cases import INDICES8
from tests.helpers import Inputs
from tests.test_gpu_estimate import _engine

pytestmark = pytest.mark.gpu

FIELD = 2.85
CIRCLE = CircleFitSettings()
CIRCLE_REF = circ.Settings()
SETTINGS = EstimateSettings(25.0, 3, magnetic_field=FIELD)
PARAMS = est.Params(25.0, 3, FIELD)
REGRESSORS = ("auto", "z_on_path", "path_on_z")


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
@pytest.fixture(scope="module")
def hand():
    """The hand-made events, and per circle (off, on) what the restatement made of them in front of the stage's
    settings (computed once, read-only)."""
    events = cases.hand_events(np.random.default_rng(26))
    assert max(len(r) for r, _ in events.values()) <= 4200
    offsets, rows, labels = cases.csr(events)
    return events, {refined: ref.prepared(offsets, rows, labels, INDICES8, PARAMS, CIRCLE_REF if refined else None) for refined in (False, True)}


@pytest.mark.parametrize("refined", [False, True], ids=["kasa", "circle fit"])
def test_stage_alone_on_hand_made_rows(ctx, hand, refined):
    events, prepared = hand
    names = list(events)
    circle = CIRCLE if refined else None
    for regressor, name in enumerate(REGRESSORS):
        want = ref.records_from(prepared[refined], ref.Settings(regressor), FIELD)
        got = rows_to_estimates(*cases.csr(events), INDICES8, SETTINGS, ctx, circle=circle, helix=HelixSlopeSettings(name))
        est.assert_same_records(got, want)
        # the cases are there
        status = want["status"]
        ran = (want["n_fit"] > 0) & (status & _abi.EST_NO_HELIX == 0)
        assert {3, 63, 64, 65, 129, 2048} <= set(want["n_fit"][ran].tolist()) and {1, -1} <= set(want["direction"][ran].tolist())
        assert (want["slope"][ran] < 0).any() and (want["slope"][ran] > 0).any() and ran.sum() >= 15
        assert status[names.index("capped"), 6] & _abi.EST_CAPPED and ran[names.index("capped"), 6]
        assert status[names.index("collinear"), 5] & _abi.EST_NO_CIRCLE and status[names.index("collinear"), 5] & _abi.EST_NO_HELIX
        assert status[names.index("turn cap"), 7] & _abi.EST_NO_HELIX and want["n_fit"][names.index("turn cap"), 7] == 2048
        assert status[names.index("centre, flat"), 0] & _abi.EST_NO_HELIX
        assert bool(status[names.index("centre, flat"), 1] & _abi.EST_NO_HELIX) == (regressor == 2)
        assert (status[names.index("empty")] == _abi.EST_EMPTY).all() and (status[:, 3] == _abi.EST_EMPTY).all()
        assert ran[names.index("eight"), [0, 1, 2, 4, 5, 6, 7]].all()  # both positions of every wave
        assert (want["reserved"][ran] >= 2).all() if refined else (want["reserved"] == 0).all()
    # the wraps fall where they were put: between ranks 63 | 64 and 64 | 65
    for s, at in ((4, 64), (5, 65)):
        _, seg, (a, b, _) = prepared[False][names.index("wraps")][s]
        phi, _ = ref.phi_q(seg[:, 0] - seg[0, 0], seg[:, 1] - seg[0, 1], a, b)
        assert (np.flatnonzero(np.abs(np.diff(phi)) > ref.HALF_TURN) + 1).tolist() == [at]
    # nothing moves but slope, vz, brho and the status
    off = rows_to_estimates(*cases.csr(events), INDICES8, SETTINGS, ctx, circle=circle)
    est.assert_same_records(off, (circ.records(*cases.csr(events), INDICES8, PARAMS, CIRCLE_REF) if refined
                                  else est.records(*cases.csr(events), INDICES8, PARAMS)))
    assert not (off["status"] & _abi.EST_NO_HELIX).any()
    for field in est.INT_FIELDS + est.F64_FIELDS:
        if field not in ("slope", "vz", "brho", "status"):
            assert got[field].tobytes() == off[field].tobytes(), field
    stopped = (got["status"] & _abi.EST_NO_HELIX) != 0
    assert got[stopped].tobytes() == _with_bit(off[stopped]).tobytes()  # NO_HELIX: the stage-off record plus the bit
    assert (got["slope"][ran] != off["slope"][ran]).mean() > 0.9
    # one event alone, and no event at all
    i = names.index("wraps")
    est.assert_same_records(rows_to_estimates(*cases.csr([events["wraps"]]), INDICES8, SETTINGS, ctx, circle=circle,
                                              helix=HelixSlopeSettings("path_on_z")), want[i:i + 1])
    assert rows_to_estimates([0], np.zeros((0, 8)), np.zeros(0), INDICES8, SETTINGS, ctx, circle=circle, helix=HelixSlopeSettings()).shape == (0, 8)


def _with_bit(records):
    records = records.copy()
    records["status"] |= _abi.EST_NO_HELIX
    return records


def test_300_events_in_one_call(ctx, hand):
    events, prepared = hand
    want = ref.records_from(prepared[True], ref.Settings(), FIELD)
    small = [name for name in events if name not in ("capped", "turn cap")]
    order = np.random.default_rng(8).integers(0, len(small), size=300)
    index = [list(events).index(small[i]) for i in order]
    got = rows_to_estimates(*cases.csr([events[small[i]] for i in order]), INDICES8, SETTINGS, ctx, circle=CIRCLE, helix=HelixSlopeSettings())
    est.assert_same_records(got, want[index])


def test_the_library_checks_its_arguments(ctx):
    out = np.empty((1, 1), dtype=_abi.ESTIMATE_DTYPE)
    layout = _abi.EventLayout()
    layout.n_sim = 1
    offsets = np.array([0, 0], dtype=np.int64)
    good = _abi.EstimateDesc(25.0, FIELD, 30, 0)

    def call(helix, circle=None, desc=good):
        return ctx.lib.attpc_rows_estimate_helix(ctx.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, layout, desc, circle, helix,
                                                 _abi.iptr(out, _abi.TrackEstimate))

    assert call(_abi.HelixDesc(0, 0)) == _abi.OK and out["status"][0, 0] == _abi.EST_EMPTY
    assert call(_abi.HelixDesc(2, 0), _abi.CircleDesc(2.0 ** -7, 32, 0)) == _abi.OK and out["status"][0, 0] == _abi.EST_EMPTY
    assert call(None) == _abi.E_INVALID and call(_abi.HelixDesc(0, 0), None, _abi.EstimateDesc(25.0, FIELD, 2, 0)) == _abi.E_INVALID
    assert call(_abi.HelixDesc(0, 0), _abi.CircleDesc(0.0, 32, 0)) == _abi.E_INVALID
    for bad in ((3, 0), (-1, 0), (0, 1), (1, -1)):
        assert call(_abi.HelixDesc(*bad)) == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_helix(ctx.handle, _abi.HelixDesc(*bad)) == _abi.E_INVALID, bad
    assert ctx.lib.attpc_trace_configure_helix(ctx.handle, None) == _abi.OK


# ---------------------------------------------------------------- 2. the same on thinned points ----
THINNING = ThinSettings(5.0)


@pytest.mark.parametrize("refined", [False, True], ids=["kasa", "circle fit"])
def test_thinned_points_through_the_stage(ctx, hand, refined):
    events, _ = hand
    events = {name: ev for name, ev in events.items() if name not in ("capped", "turn cap")}  # (at 5 mm they thin to a few points)
    offsets, rows, labels = cases.csr(events)
    point_offsets, points, point_labels, info = thin.thin(offsets, rows, labels, INDICES8, THINNING.z_step)
    got_points = rows_to_points(offsets, rows, labels, INDICES8, THINNING, ctx)
    np.testing.assert_array_equal(got_points[0], point_offsets)
    assert got_points[1].tobytes() == np.ascontiguousarray(points).tobytes()
    want = ref.records(point_offsets, points, point_labels, INDICES8, PARAMS, ref.Settings(), CIRCLE_REF if refined else None)
    got = rows_to_estimates(*got_points[:3], INDICES8, SETTINGS, ctx, circle=CIRCLE if refined else None, helix=HelixSlopeSettings())
    est.assert_same_records(got, want)
    ran = (want["n_fit"] > 0) & (want["status"] & _abi.EST_NO_HELIX == 0)
    assert ran.sum() >= 8 and {1, -1} <= set(want["direction"][ran].tolist())


# ---------------------------------------------------------------- 3. fused ----
ESTIMATES = EstimateSettings(20.0, 10)
HELIX = HelixSlopeSettings()
N, SEED = 64, 29
FAR_SEED, FAR_FIRST = (0xDEADBEEF << 32) | 5, (1 << 32) + 3  # a seed whose high word is set, event ids past 2^32


def _off(eng):
    eng.configure_estimates()
    eng.configure_thinning()
    eng.configure_circle_fit()
    eng.configure_helix_slope()


def _on(eng, refined, thinned=True):
    eng.configure_estimates(ESTIMATES)
    eng.configure_thinning(THINNING if thinned else None)
    eng.configure_circle_fit(CIRCLE if refined else None)
    eng.configure_helix_slope(HELIX)


def _want(res, inp, refined, thinned=True):
    """The fused records: this contract on the event's point rows (the delivered rows without thinning), RANGE OR-ed in
    where thinning dropped a row of the label."""
    params = est.Params(ESTIMATES.beam_region_radius, ESTIMATES.min_points, inp.config.det_params.bfield)
    if not thinned:
        return ref.records(res["offsets"], res["rows"], res["labels"], inp.indices, params, ref.Settings(), CIRCLE_REF if refined else None)
    point_offsets, points, point_labels, info = thin.thin(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING.z_step)
    records = ref.records(point_offsets, points, point_labels, inp.indices, params, ref.Settings(), CIRCLE_REF if refined else None)
    records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    return records


@pytest.fixture(scope="module")
def fused(ctx):
    """64 events of be10dp with noise and partial readout; estimates, thinning at 5 mm and the helix slope on, the circle
    fit off and on: refined -> (the call's result, the restatement's records of the delivered rows), read-only."""
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    out = {}
    for refined in (False, True):
        _on(eng, refined)
        res = eng.run_trace_rows(N, seed=SEED)
        want = _want(res, inp, refined)
        want.setflags(write=False)
        out[refined] = (res, want)
    _off(eng)
    return inp, out


def test_fused_records_equal_the_restatement_of_the_delivered_rows(ctx, fused):
    inp, runs = fused
    eng = _engine(inp, ctx)
    for refined, (res, want) in runs.items():
        est.assert_same_records(res["estimates"], want)
        ran = (want["n_fit"] > 0) & (want["status"] & _abi.EST_NO_HELIX == 0)
        assert res["slope"] == "helix" and res["thinning"] == 5.0 and ("circle" in res) == refined and ran.sum() >= 20
        _on(eng, refined)
        resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
        est.assert_same_records(resident["estimates"], want)
        assert resident["slope"] == "helix" and resident["trace_rows"] == res["trace_rows"] and "rows" not in resident
        alone = eng.run_estimates(N, seed=SEED)
        est.assert_same_records(alone["estimates"], want)
        assert alone["slope"] == "helix"
    # without thinning: the raw rows through the same pass
    _on(eng, False, thinned=False)
    raw = eng.run_trace_rows(N, seed=SEED)
    est.assert_same_records(raw["estimates"], _want(raw, inp, False, thinned=False))
    assert raw["slope"] == "helix" and "thinning" not in raw
    _off(eng)


def test_fused_records_do_not_depend_on_calls_or_chunks(ctx, fused):
    inp, runs = fused
    res, want = runs[True]
    eng = _engine(inp, ctx)
    _on(eng, True)
    first, second = eng.run_estimates(24, seed=SEED), eng.run_estimates(N - 24, seed=SEED, first_event=24)
    est.assert_same_records(np.concatenate([first["estimates"], second["estimates"]]), want)
    small = _engine(inp, ctx, chunk_events=5)  # 13 chunks of the 64 events
    try:
        _on(small, True)
        chunked = small.run_trace_rows(N, seed=SEED)
        est.assert_same_records(chunked["estimates"], want)
        np.testing.assert_array_equal(chunked["rows"], res["rows"])
        _on(small, False)
        est.assert_same_records(small.run_estimates(N, seed=SEED)["estimates"], runs[False][1])
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        _off(small)


def test_fused_at_event_ids_past_2_32(ctx, fused):
    inp, _ = fused
    eng = _engine(inp, ctx)
    _on(eng, True)
    far = eng.run_trace_rows(16, seed=FAR_SEED, first_event=FAR_FIRST)
    want = _want(far, inp, True)
    est.assert_same_records(far["estimates"], want)
    assert ((want["n_fit"] > 0) & (want["status"] & _abi.EST_NO_HELIX == 0)).sum() >= 4
    halves = [eng.run_estimates(8, seed=FAR_SEED, first_event=FAR_FIRST + 8 * i)["estimates"] for i in range(2)]
    est.assert_same_records(np.concatenate(halves), want)
    near = eng.run_estimates(16, seed=FAR_SEED & 0xFFFFFFFF, first_event=FAR_FIRST & 0xFFFFFFFF)["estimates"]
    assert near.tobytes() != far["estimates"].tobytes()  # the high words count
    _off(eng)


# ---------------------------------------------------------------- 4. off, nothing moves ----
def test_off_nothing_moves(ctx, fused):
    inp, runs = fused
    res = runs[True][0]
    fresh = _abi.Context(0)  # a context that never saw the stage
    never = _engine(inp, fresh)
    never.configure_estimates(ESTIMATES)
    never.configure_thinning(THINNING)
    never.configure_circle_fit(CIRCLE)
    base = never.run_trace_rows(N, seed=SEED)
    assert "slope" not in base
    eng = _engine(inp, ctx)
    _on(eng, True)
    eng.configure_helix_slope()  # on, then off again
    assert ctx.lib.attpc_trace_configure_helix(ctx.handle, None) == _abi.OK
    off = eng.run_trace_rows(N, seed=SEED)
    assert "slope" not in off
    for key in ("rows", "labels", "offsets", "event_points", "p4", "vertex"):
        np.testing.assert_array_equal(off[key], base[key], err_msg=key)
        np.testing.assert_array_equal(res[key], base[key], err_msg=key)  # nor does the stage on move them
    assert off["trace_rows"] == base["trace_rows"] == res["trace_rows"]
    assert off["estimates"].tobytes() == base["estimates"].tobytes() and not (off["estimates"]["status"] & _abi.EST_NO_HELIX).any()
    # ... and they are the records of the contract without this stage
    params = est.Params(ESTIMATES.beam_region_radius, ESTIMATES.min_points, inp.config.det_params.bfield)
    point_offsets, points, point_labels, info = thin.thin(base["offsets"], base["rows"], base["labels"], inp.indices, THINNING.z_step)
    parent = circ.records(point_offsets, points, point_labels, inp.indices, params, CIRCLE_REF)
    parent["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    est.assert_same_records(base["estimates"], parent)
    # alone, without the estimates, the stage is inert
    _off(eng)
    eng.configure_helix_slope(HELIX)
    alone = eng.run_trace_rows(N, seed=SEED, fetch=False)
    assert "estimates" not in alone and "slope" not in alone and alone["trace_rows"] == base["trace_rows"]
    _off(eng)
