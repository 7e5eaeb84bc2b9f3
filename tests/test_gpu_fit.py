"""The track fit on the device (include/attpc_engine.h, "track fit") against its numpy restatement
(tests/fit_reference.py): integer fields equal, f64 fields bit for bit, NaN in the same places -- the device is never
measured against a tolerance.  The stage alone on the hand-made cases (tests/fit_cases.py) with given starts and with
the start from the estimates, through more workgroups than the launch has; the same on thinned points; the fused path
on its own delivered rows, in one call, two calls and chunks, at event ids past 2^32, with the rows fetched or left on
the device, and through ``simulate_batch_trace_rows(fit=)``; and with the stage off nothing moves.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.fit import TrackFitSettings, rows_to_fit
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from tests import estimate_reference as est
from tests import fit_cases as cases
from tests import fit_reference as ref
from tests import thin_reference as thin
from tests.fit_cases import INDICES8
from tests.helpers import Inputs
from tests.test_gpu_estimate import PEAKS, _engine, _trace_kw

pytestmark = pytest.mark.gpu

FIELD = 2.85
ESTIMATE = EstimateSettings(cases.BEAM_REGION, cases.MIN_POINTS, magnetic_field=FIELD)
PARAMS = est.Params(cases.BEAM_REGION, cases.MIN_POINTS, FIELD)
FIT = TrackFitSettings(**cases.SETTINGS)
FIT_REF = ref.Settings(**cases.SETTINGS)


@pytest.fixture(scope="module")
def ctx():
    """A context with the detector of be10dp configured: its tables, masses, charges, fields and length are the model."""
    ctx = _abi.Context(0)
    _engine(Inputs("be10dp"), ctx)
    return ctx


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
@pytest.fixture(scope="module")
def hand():
    """The hand-made events, their estimate records, and what the restatement makes of them from the special starts
    and from the estimates (computed once, read-only)."""
    model = cases.model()
    events = cases.hand_cases(model)
    csr = cases.csr(events)
    estimates = est.records(*csr, INDICES8, PARAMS)
    start = cases.special_starts(events)
    want = {given: ref.records(*csr, INDICES8, model, estimates, FIT_REF, cases.BEAM_REGION, start=start if given else None)
            for given in (True, False)}
    for records in want.values():
        records.setflags(write=False)
    return events, csr, estimates, start, want


@pytest.mark.parametrize("given", [True, False], ids=["start=", "start from the estimates"])
def test_stage_alone_on_hand_made_rows(ctx, hand, given):
    events, csr, estimates, start, want = hand
    names = list(events)
    est.assert_same_records(rows_to_estimates(*csr, INDICES8, ESTIMATE, ctx), estimates)  # what the fit starts from
    got = rows_to_fit(*csr, cases.layout(), estimates, ctx, FIT, start if given else None, estimate_settings=ESTIMATE)
    ref.assert_same_records(got, want[given])
    # the cases are there
    w, e8 = want[given], names.index("eight")
    status = w["status"]
    assert w["n_points"][e8].tolist() == [3, 7, 8, 9, 63, 64, 65, 129] and (w["evaluations"][e8] >= 1).sum() >= 7
    assert status[names.index("capped"), 6] & _abi.FIT_CAPPED and w["n_points"][names.index("capped"), 6] == 2048
    assert status[e8, 2] & _abi.FIT_STEP_CAP and status[names.index("same z"), 1] == _abi.FIT_FEW
    assert status[names.index("same z"), 3] & _abi.FIT_NOT_CONVERGED and (status[names.index("empty")] == _abi.FIT_EMPTY).all()
    assert status[names.index("single"), 4] & (_abi.FIT_EMPTY | _abi.FIT_FEW | _abi.FIT_NO_START) == 0
    assert {_abi.FIT_END_STOPPED, _abi.FIT_END_LEFT, _abi.FIT_END_STEP_CAP} <= set(w["end"][w["evaluations"] > 0].tolist())
    assert status[names.index("collinear"), 5] == _abi.FIT_NO_START
    if given:
        assert status[e8, 0] == _abi.FIT_NO_START and status[e8, 7] & _abi.FIT_SINGULAR and w["n_inside"][e8, 4] < 63
    # one event alone, and no event at all
    i = names.index("single")
    alone = rows_to_fit(*cases.csr([events["single"]]), cases.layout(), estimates[i:i + 1], ctx, FIT,
                        start[i:i + 1] if given else None, estimate_settings=ESTIMATE)
    ref.assert_same_records(alone, w[i:i + 1])
    none = rows_to_fit([0], np.zeros((0, 8)), np.zeros(0), cases.layout(), np.zeros((0, 8), dtype=_abi.ESTIMATE_DTYPE), ctx, FIT)
    assert none.shape == (0, 8)


def test_a_label_given_twice_and_a_position_without_species(ctx, hand):
    events, csr, _, _, _ = hand
    lay = cases.layout(cases.INDICES_TWICE, without=(4,))
    estimates = est.records(*csr, cases.INDICES_TWICE, PARAMS)
    want = ref.records(*csr, cases.INDICES_TWICE, ref.Model(Inputs("be10dp").det, lay), estimates, FIT_REF, cases.BEAM_REGION)
    got = rows_to_fit(*csr, lay, estimates, ctx, FIT, estimate_settings=ESTIMATE)
    ref.assert_same_records(got, want)
    e8 = list(events).index("eight")
    assert want["status"][e8, 3] == _abi.FIT_EMPTY and want["status"][e8, 7] == _abi.FIT_NO_START and want["evaluations"][e8, 0] >= 2


def test_more_groups_of_tracks_than_workgroups(ctx, hand):
    """1 100 events of eight positions are 1 100 groups of eight tracks for 1 024 workgroups: the last 76 groups are a
    workgroup's second."""
    events, _, estimates, start, want = hand
    names = list(events)
    small = [names.index(n) for n in ("single", "empty", "same z")]
    order = np.concatenate([np.random.default_rng(30).choice(small, size=1090), [names.index("eight")] * 4, small[:1] * 6])
    assert len(order) == 1100
    got = rows_to_fit(*cases.csr([events[names[i]] for i in order]), cases.layout(), estimates[order], ctx, FIT, start[order],
                      estimate_settings=ESTIMATE)
    ref.assert_same_records(got, want[True][order])


def test_the_library_checks_its_arguments(ctx):
    out = np.empty((1, 1), dtype=_abi.FIT_DTYPE)
    estimates = np.zeros((1, 1), dtype=_abi.ESTIMATE_DTYPE)
    estimates["status"] = _abi.EST_EMPTY
    lay = cases.layout([2], [0])
    offsets = np.array([0, 0], dtype=np.int64)
    good_e, good_f = _abi.EstimateDesc(25.0, FIELD, 30, 0), FIT.desc()

    def call(c, fit=good_f, estimate=good_e, records=estimates):
        return c.lib.attpc_rows_fit(c.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, lay, estimate,
                                    None if records is None else _abi.iptr(records, _abi.TrackEstimate), None, fit,
                                    _abi.iptr(out, _abi.TrackFit))

    assert call(ctx) == _abi.OK and out["status"][0, 0] == _abi.FIT_EMPTY and np.isnan(out["f"][0, 0])
    assert call(ctx, fit=None) == _abi.E_INVALID and call(ctx, estimate=None) == _abi.E_INVALID and call(ctx, records=None) == _abi.E_INVALID
    assert call(ctx, estimate=_abi.EstimateDesc(25.0, FIELD, 2, 0)) == _abi.E_INVALID
    nan = float("nan")
    for bad in ((0.0, 1e-4, 1e-4, 100, 8), (nan, 1e-4, 1e-4, 100, 8), (1e-10, nan, 1e-4, 100, 8), (1e-10, 1e-4, float("inf"), 100, 8),
                (1e-10, 1e-4, 1e-4, 0, 8), (1e-10, 1e-4, 1e-4, 10001, 8), (1e-10, 1e-4, 1e-4, 100, 1), (1e-10, 1e-4, 1e-4, 100, 33)):
        assert call(ctx, fit=_abi.FitDesc(*bad)) == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_fit(ctx.handle, _abi.FitDesc(*bad)) == _abi.E_INVALID, bad
    assert ctx.lib.attpc_trace_configure_fit(ctx.handle, None) == _abi.OK
    assert ctx.lib.attpc_fits_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED
    assert call(_abi.Context(0)) == _abi.E_NOTCONFIGURED  # no detector: no model


# ---------------------------------------------------------------- 2. the same on thinned points ----
THINNING = ThinSettings(5.0)


def test_thinned_points_through_the_stage(ctx, hand):
    events, _, _, _, _ = hand
    events = {name: ev for name, ev in events.items() if name != "capped"}  # (at 5 mm it thins to a few points)
    offsets, rows, labels = cases.csr(events)
    point_offsets, points, point_labels, _ = thin.thin(offsets, rows, labels, INDICES8, THINNING.z_step)
    got_points = rows_to_points(offsets, rows, labels, INDICES8, THINNING, ctx)
    assert got_points[1].tobytes() == np.ascontiguousarray(points).tobytes()
    estimates = est.records(point_offsets, points, point_labels, INDICES8, PARAMS)
    want = ref.records(point_offsets, points, point_labels, INDICES8, cases.model(), estimates, FIT_REF, cases.BEAM_REGION)
    got = rows_to_fit(*got_points[:3], cases.layout(), rows_to_estimates(*got_points[:3], INDICES8, ESTIMATE, ctx), ctx, FIT,
                      estimate_settings=ESTIMATE)
    ref.assert_same_records(got, want)
    assert (want["evaluations"] >= 2).sum() >= 5 and (want["g"][want["evaluations"] >= 2][:, 2] < 0).any()


# ---------------------------------------------------------------- 3. fused ----
ESTIMATES = EstimateSettings(20.0, 10)
CIRCLE, HELIX = CircleFitSettings(), HelixSlopeSettings()
FUSED = dict(time_step=2e-9, max_steps=600, max_evaluations=6, tolerance_momentum=1e-3, tolerance_position=1e-3)
N, SEED = 32, 30
FAR_SEED, FAR_FIRST = (0xDEADBEEF << 32) | 5, (1 << 32) + 3  # a seed whose high word is set, event ids past 2^32


def _off(eng):
    eng.configure_estimates()
    eng.configure_thinning()
    eng.configure_circle_fit()
    eng.configure_helix_slope()
    eng.configure_track_fit()


def _on(eng, fit=True):
    eng.configure_estimates(ESTIMATES)
    eng.configure_thinning(THINNING)
    eng.configure_circle_fit(CIRCLE)
    eng.configure_helix_slope(HELIX)
    eng.configure_track_fit(TrackFitSettings(**FUSED) if fit else None)


def _want(res, inp):
    """The fused records: this contract on the thinned points of the delivered rows, started from the delivered estimate
    records (which tests/test_gpu_helix.py holds to their own contract)."""
    point_offsets, points, point_labels, _ = thin.thin(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING.z_step)
    return ref.records(point_offsets, points, point_labels, inp.indices, ref.Model(inp.det, inp.layout), res["estimates"],
                       ref.Settings(**FUSED), ESTIMATES.beam_region_radius)


@pytest.fixture(scope="module")
def fused():
    """32 events of be10dp with noise and partial readout; estimates, thinning at 5 mm, circle fit, helix slope and the
    track fit on: (the call's result, the restatement's records), read-only."""
    ctx = _abi.Context(0)
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    _on(eng)
    res = eng.run_trace_rows(N, seed=SEED)
    want = _want(res, inp)
    want.setflags(write=False)
    _off(eng)
    return ctx, inp, res, want


def test_fused_records_equal_the_restatement_of_the_delivered_rows(fused):
    ctx, inp, res, want = fused
    ref.assert_same_records(res["fits"], want)
    ran = want["evaluations"] >= 2
    assert ran.sum() >= 10 and ran[:, 0].any() and ran[:, 1].any() and res["fits"].shape == res["estimates"].shape == (N, 2)
    eng = _engine(inp, ctx)
    _on(eng)
    resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
    ref.assert_same_records(resident["fits"], want)
    assert resident["trace_rows"] == res["trace_rows"] and "rows" not in resident
    assert resident["estimates"].tobytes() == res["estimates"].tobytes()
    alone = eng.run_estimates(N, seed=SEED)
    ref.assert_same_records(alone["fits"], want)
    _off(eng)


def test_fused_records_do_not_depend_on_calls_or_chunks(fused):
    ctx, inp, res, want = fused
    eng = _engine(inp, ctx)
    _on(eng)
    first, second = eng.run_estimates(12, seed=SEED), eng.run_estimates(N - 12, seed=SEED, first_event=12)
    ref.assert_same_records(np.concatenate([first["fits"], second["fits"]]), want)
    small = _engine(inp, ctx, chunk_events=5)  # 7 chunks of the 32 events
    try:
        _on(small)
        chunked = small.run_trace_rows(N, seed=SEED)
        ref.assert_same_records(chunked["fits"], want)
        np.testing.assert_array_equal(chunked["rows"], res["rows"])
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        _off(small)


def test_fused_at_event_ids_past_2_32(fused):
    ctx, inp, _, _ = fused
    eng = _engine(inp, ctx)
    _on(eng)
    far = eng.run_trace_rows(12, seed=FAR_SEED, first_event=FAR_FIRST)
    want = _want(far, inp)
    ref.assert_same_records(far["fits"], want)
    assert (want["evaluations"] >= 2).sum() >= 2
    halves = [eng.run_estimates(6, seed=FAR_SEED, first_event=FAR_FIRST + 6 * i)["fits"] for i in range(2)]
    ref.assert_same_records(np.concatenate(halves), want)
    _off(eng)


def test_simulate_batch_trace_rows_gives_the_fused_records(fused):
    from attpc_engine_amd.detector.traces import simulate_batch_trace_rows

    ctx, inp, res, want = fused
    kw = dict(ctx=ctx, peaks=PEAKS, estimates=ESTIMATES, thinning=THINNING, circle=CIRCLE, helix=HELIX, **_trace_kw(inp))
    off, rows, labels, raw, stats = simulate_batch_trace_rows(res["p4"], res["vertex"], inp.z, inp.a, inp.config, SEED, inp.indices,
                                                              fit=TrackFitSettings(**FUSED), **kw)
    np.testing.assert_array_equal(rows, res["rows"])
    ref.assert_same_records(stats["fits"], want)
    assert stats["estimates"].tobytes() == res["estimates"].tobytes()
    plain = simulate_batch_trace_rows(res["p4"][:4], res["vertex"][:4], inp.z, inp.a, inp.config, SEED, inp.indices, **kw)[4]
    assert "fits" not in plain and "estimates" in plain  # fit=None turns the stage off again
    simulate_batch_trace_rows(res["p4"][:2], res["vertex"][:2], inp.z, inp.a, inp.config, SEED, inp.indices, ctx=ctx, peaks=PEAKS,
                              **_trace_kw(inp))  # (everything off again)


# ---------------------------------------------------------------- 4. off, nothing moves ----
def test_off_nothing_moves(fused):
    ctx, inp, res, _ = fused
    fresh = _abi.Context(0)  # a context that never saw the stage
    never = _engine(inp, fresh)
    _on(never, fit=False)
    base = never.run_trace_rows(N, seed=SEED)
    assert "fits" not in base
    eng = _engine(inp, ctx)
    _on(eng)
    eng.configure_track_fit()  # on, then off again
    off = eng.run_trace_rows(N, seed=SEED)
    assert "fits" not in off and ctx.lib.attpc_fits_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED
    for key in ("rows", "labels", "offsets", "event_points", "p4", "vertex"):
        np.testing.assert_array_equal(off[key], base[key], err_msg=key)
        np.testing.assert_array_equal(res[key], base[key], err_msg=key)  # nor does the stage on move them
    assert off["trace_rows"] == base["trace_rows"] == res["trace_rows"]
    assert off["estimates"].tobytes() == base["estimates"].tobytes() == res["estimates"].tobytes()
    # alone, without the estimates, the stage is inert
    _off(eng)
    eng.configure_track_fit(TrackFitSettings(**FUSED))
    alone = eng.run_trace_rows(N, seed=SEED, fetch=False)
    assert "estimates" not in alone and "fits" not in alone and alone["trace_rows"] == base["trace_rows"]
    _off(eng)
