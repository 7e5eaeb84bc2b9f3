"""The drift correction on the device (``undistort_kernel``, csrc/undistort.hip) against its restatement
(tests/undistort_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The arithmetic of one row is written down operation by operation and the order of an event's rows is a total one
(include/attpc_engine.h, "drift correction"), so every comparison here is bit for bit: the tolerance is zero by
construction, not by measurement.  M is the named map of tests/distortion_cases.py."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.correction import CorrectionSettings, rows_to_correction
from attpc_engine_amd.detector.distortion import DistortionMap
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from tests import distortion_cases as dc
from tests import distortion_reference as dref
from tests import undistort_cases as uc
from tests import undistort_reference as uref
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu

C = _abi.C
ESTIMATES, THINNING, CIRCLE, HELIX = EstimateSettings(min_points=10), ThinSettings(10.0), CircleFitSettings(), HelixSlopeSettings()
SEED, FIRST = 17, (1 << 32) - 10


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.close()


def _assert_same(got, want, what=""):
    rows, labels, order, info = got
    assert info == want[3], (what, info, want[3])
    differ = np.flatnonzero((rows.view(np.uint64) != want[0].view(np.uint64)).any(axis=1))
    assert differ.size == 0, (what, differ[:10], rows[differ[:3]], want[0][differ[:3]])
    assert np.array_equal(labels, want[1]) and np.array_equal(order, want[2]), what


# 1 ------------------------------------------------------------------------------------------ the stage alone ----
@pytest.fixture(scope="module")
def cases():
    offsets, rows, labels, names = uc.stage_cases()
    want = uref.undistort(uc.settings(), offsets, rows, labels)
    for a in (offsets, rows, labels, *want[:3]):
        a.setflags(write=False)
    return offsets, rows, labels, names, want


def test_stage_alone_equals_the_restatement(ctx, cases):
    offsets, rows, labels, names, want = cases
    good = CorrectionSettings(dc.named_map())
    _assert_same(rows_to_correction(offsets, rows, labels, good, dc.drift(), ctx), want, "the case set")
    assert want[3]["n_skipped"] == 27 and want[3]["n_moved"] > 1000 and want[3]["n_unconverged"] == 0
    # every event on its own, and a window of the array (offsets[0] > 0: the rows in front belong to no event)
    for e in range(0, len(names), 2):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        one = np.array([0, hi - lo], dtype=np.int64)
        _assert_same(rows_to_correction(one, rows[lo:hi], labels[lo:hi], good, dc.drift(), ctx),
                     uref.undistort(uc.settings(), one, rows[lo:hi], labels[lo:hi]), names[e])
    window = offsets[9:]
    _assert_same(rows_to_correction(window, rows, labels, good, dc.drift(), ctx), uref.undistort(uc.settings(), window, rows, labels), "window")
    assert rows_to_correction([0], np.zeros((0, 8)), [], good, dc.drift(), ctx)[3] == dict.fromkeys(uref.COUNTS, 0)
    # other settings: one iteration, 64, zero tolerances (three steps leave 1e-6 m: unconverged)
    for changes in ({"iterations": 1}, {"iterations": 64}, {"iterations": 3, "tolerance_xy": 0.0, "tolerance_tb": 0.0}):
        got = rows_to_correction(offsets, rows, labels, CorrectionSettings(dc.named_map(), **changes), dc.drift(), ctx)
        _assert_same(got, uref.undistort(uc.settings(**changes), offsets, rows, labels), changes)
    assert got[3]["n_unconverged"] > 1000


def test_stage_alone_with_other_maps(ctx, cases):
    offsets, rows, labels, _, _ = cases
    m = dc.named_map()
    # no time table: nothing moves and z comes back bit for bit; a map that shifts nothing sorts by column 6
    flat = DistortionMap(m.radial, m.azimuthal, None, rho_max=dc.RHO_MAX, length=dc.LENGTH)
    sorted_rows = uc.rows_of(uc.apparent_points(700, 4))  # (in descending time, as the trace rows come)
    two = np.array([0, 300, 700], dtype=np.int64)
    got = rows_to_correction(two, sorted_rows, np.arange(700), CorrectionSettings(flat), dc.drift(), ctx)
    _assert_same(got, uref.undistort(uc.settings(dc.reference_map(flat)), two, sorted_rows, np.arange(700)), "no time table")
    assert got[3]["n_moved"] == 0 and dref.same_bits(got[0][:, 2], sorted_rows[:, 2])
    zero = DistortionMap(np.zeros((2, 2)), rho_max=dc.RHO_MAX, length=dc.LENGTH)
    got = rows_to_correction(offsets, rows, labels, CorrectionSettings(zero), dc.drift(), ctx)
    _assert_same(got, uref.undistort(uc.settings(dc.reference_map(zero)), offsets, rows, labels), "zero map")
    finite = np.isfinite(rows[got[2]][:, [0, 1, 6]]).all(axis=1)
    assert dref.same_bits(got[0][finite][:, 2], rows[got[2]][finite][:, 2])
    # a map steep enough to diverge: finite rows, and the count says so
    steep = uc.steep_map()
    named = DistortionMap(steep.radial, rho_max=0.6, length=dc.LENGTH)
    pts = uc.rows_of(uc.apparent_points(500, 3, rho_limit=0.25))
    one = np.array([0, 500], dtype=np.int64)
    got = rows_to_correction(one, pts, np.arange(500), CorrectionSettings(named), dc.drift(), ctx)
    _assert_same(got, uref.undistort(uc.settings(steep), one, pts, np.arange(500)), "steep")
    assert np.isfinite(got[0]).all() and got[3]["n_unconverged"] > 400
    # what the library refuses
    info = _abi.UndistortInfo()
    good = CorrectionSettings(m)
    out = np.empty_like(pts)
    i64 = C.c_int64
    for field, value in uc.bad_settings():
        desc = good.desc(dc.drift())
        setattr(desc, field, value)
        args = (ctx.handle, 1, _abi.iptr(one, i64), _abi.dptr(pts), None, desc, _abi.dptr(out), None, None, C.byref(info))
        assert ctx.lib.attpc_rows_undistort(*args) == _abi.E_INVALID, (field, value)
        assert ctx.lib.attpc_trace_configure_correction(ctx.handle, desc) == _abi.E_INVALID, (field, value)
    assert ctx.lib.attpc_rows_undistort(ctx.handle, 1, _abi.iptr(one, i64), _abi.dptr(pts), None, None, _abi.dptr(out), None, None,
                                        C.byref(info)) == _abi.E_INVALID
    # without labels and without order
    ctx.check(ctx.lib.attpc_rows_undistort(ctx.handle, 1, _abi.iptr(one, i64), _abi.dptr(pts), None, good.desc(dc.drift()),
                                           _abi.dptr(out), None, None, C.byref(info)), "attpc_rows_undistort")
    want = uref.undistort(uc.settings(), one, pts, np.arange(500))
    assert dref.same_bits(out, want[0]) and info.as_dict() == want[3]


# 2 ------------------------------------------------------------------------------------------ in the run ----
def _reference_settings(named, config) -> uref.Settings:
    return uref.Settings(dc.reference_map(named, config), int(config.elec_params.windows_edge),
                         int(config.elec_params.micromegas_edge), float(config.det_params.length))


def _stages(eng, on: bool):
    eng.configure_thinning(THINNING if on else None)
    eng.configure_circle_fit(CIRCLE if on else None)
    eng.configure_helix_slope(HELIX if on else None)


def _device_estimates(res, inp, ctx, staged: bool):
    """``rows_to_estimates`` of the delivered rows; ``staged``: through the thinning, with the circle fit and the helix."""
    if not staged:
        return rows_to_estimates(res["offsets"], res["rows"], res["labels"], inp.indices, ESTIMATES, ctx, config=inp.config)
    point_offsets, points, point_labels, info = rows_to_points(res["offsets"], res["rows"], res["labels"], inp.indices, THINNING, ctx)
    records = rows_to_estimates(point_offsets, points, point_labels, inp.indices, ESTIMATES, ctx, config=inp.config,
                                circle=CIRCLE, helix=HELIX)
    records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    return records


@pytest.fixture(scope="module", params=[("be10dp", 8), ("o16aa", 24)], ids=["be10dp", "o16aa"])
def run(request, ctx):
    """One workload with the distortion M on: the rows without the correction, the restatement of their correction with
    M, and the run with the correction on -- plain estimates and staged ones.  Read-only."""
    from attpc_engine_amd.engine import Engine
    name, n = request.param
    inp = Inputs(name)
    named = dc.named_map()
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_distortion(named)
    eng.configure_estimates(ESTIMATES)
    eng.configure_correction()
    _stages(eng, False)
    off = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    want = uref.undistort(_reference_settings(named, inp.config), off["offsets"], off["rows"], off["labels"])
    correction = CorrectionSettings(named)
    eng.configure_correction(correction)
    on = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    _stages(eng, True)
    staged = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    _stages(eng, False)
    eng.configure_correction()
    return inp, n, eng, correction, off, want, on, staged


def test_run_delivers_the_corrected_rows(run):
    inp, n, eng, correction, off, want, on, staged = run
    print("events", n, "rows", len(off["rows"]), "counts", on["correction"])
    assert "correction" not in off and len(off["rows"]) > 200
    for res in (on, staged):
        assert np.array_equal(res["offsets"], off["offsets"]) and np.array_equal(res["event_points"], off["event_points"])
        assert res["trace_rows"] == off["trace_rows"]  # n_rows and the row checksum: (event, pad, sample) terms
        _assert_same((res["rows"], res["labels"], want[2], res["correction"]), want)
    assert want[3]["n_moved"] > 50 and want[3]["n_skipped"] == 0 and want[3]["n_rows"] == len(off["rows"])
    for lo, hi in zip(on["offsets"][:-1], on["offsets"][1:]):
        assert np.all(np.diff(on["rows"][lo:hi, 2]) >= 0.0)
    assert any((np.diff(uref.undistort(_reference_settings(dc.named_map(), inp.config), off["offsets"], off["rows"], off["labels"],
                                       "no_resort")[0][lo:hi, 2]) < 0.0).any() for lo, hi in zip(on["offsets"][:-1], on["offsets"][1:]))


def test_run_estimates_are_those_of_the_delivered_rows(run, ctx):
    inp, n, eng, correction, off, want, on, staged = run
    assert on["estimates"].tobytes() == _device_estimates(on, inp, ctx, False).tobytes()
    assert staged["estimates"].tobytes() == _device_estimates(staged, inp, ctx, True).tobytes()
    assert on["estimates"].tobytes() != off["estimates"].tobytes()
    assert (on["estimates"]["n_fit"] > 0).sum() >= 4


def test_resident_runs_and_chunks_give_the_same(run, ctx):
    inp, n, eng, correction, off, want, on, staged = run
    eng.configure_distortion(dc.named_map())
    eng.configure_estimates(ESTIMATES)
    eng.configure_correction(correction)
    try:
        for res, stages in ((on, False), (staged, True)):
            _stages(eng, stages)
            resident = eng.run_trace_rows(n, seed=SEED, first_event=FIRST, fetch=False)
            alone = eng.run_estimates(n, seed=SEED, first_event=FIRST)
            for other in (resident, alone):
                assert other["estimates"].tobytes() == res["estimates"].tobytes()
                assert other["correction"] == res["correction"] and other["trace_rows"] == res["trace_rows"]
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 5 if n > 8 else 3), "attpc_set_chunk_events")
            try:
                chunked = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
                chunked_resident = eng.run_estimates(n, seed=SEED, first_event=FIRST)
            finally:
                ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
            assert dref.same_bits(chunked["rows"], res["rows"]) and np.array_equal(chunked["labels"], res["labels"])
            for other in (chunked, chunked_resident):
                assert other["estimates"].tobytes() == res["estimates"].tobytes()
                assert other["correction"] == res["correction"] and other["trace_rows"] == res["trace_rows"]
        # two calls: the counts add, the rows follow one another
        _stages(eng, False)
        half = n // 2
        parts = [eng.run_trace_rows(half, seed=SEED, first_event=FIRST + lo) for lo in (0, half)]
        assert dref.same_bits(np.concatenate([p["rows"] for p in parts]), on["rows"])
        assert {k: parts[0]["correction"][k] + parts[1]["correction"][k] for k in uref.COUNTS} == on["correction"]
        # a call whose capacity was too small is repeated: every event still counts once
        small = eng.run_trace_rows(n, seed=SEED, first_event=FIRST, capacity_per_event=1)
        assert dref.same_bits(small["rows"], on["rows"]) and small["correction"] == on["correction"]
    finally:
        _stages(eng, False)
        eng.configure_correction()


def test_null_and_zero_maps_equal_the_unconfigured_run(run, ctx):
    inp, n, eng, correction, off, want, on, staged = run
    eng.configure_distortion(dc.named_map())
    eng.configure_estimates(ESTIMATES)
    _stages(eng, False)
    info = _abi.UndistortInfo()
    for settings in (None, CorrectionSettings(DistortionMap(np.zeros((3, 3)))), "desc of zeros"):
        eng.configure_correction(correction)
        assert "correction" in eng.run_trace_rows(2, seed=SEED, first_event=FIRST)
        if settings == "desc of zeros":  # through the C ABI: a desc whose tables are all zero turns the stage off
            desc = CorrectionSettings(DistortionMap(np.zeros((3, 3)))).desc(inp.config)
            ctx.forget("correction")
            ctx.check(ctx.lib.attpc_trace_configure_correction(ctx.handle, desc), "attpc_trace_configure_correction")
        else:
            eng.configure_correction(settings)
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
        assert "correction" not in res
        assert ctx.lib.attpc_correction_last(ctx.handle, C.byref(info)) == _abi.E_NOTCONFIGURED
        for key in ("offsets", "rows", "labels", "event_points", "estimates", "p4", "vertex", "status"):
            assert res[key].tobytes() == off[key].tobytes(), key
        assert res["trace_rows"] == off["trace_rows"] and res["stats"]["key_checksum"] == off["stats"]["key_checksum"]


def test_host_clouds_take_the_stage(run, ctx):
    """``attpc_trace_rows_at`` on the clouds of a few events: its rows with the correction on are the restatement's of
    its rows with the correction off."""
    from attpc_engine_amd.detector.traces import clouds_to_trace_rows, configure_trace_rows
    inp, n, eng, correction, off, want, on, staged = run
    cloud = eng.run(4, seed=SEED, first_event=FIRST, fetch=True)
    configure_trace_rows(inp.config, ctx)
    ctx.forget("correction")
    configure_trace_rows(inp.config, ctx, correction=CorrectionSettings(DistortionMap(np.zeros((2, 2)))))
    plain = clouds_to_trace_rows(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=SEED, first_event=FIRST)
    configure_trace_rows(inp.config, ctx, correction=correction)
    try:
        fixed = clouds_to_trace_rows(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=SEED, first_event=FIRST)
        counts = ctx.correction_last()
    finally:
        eng.configure_correction()
    expect = uref.undistort(_reference_settings(dc.named_map(), inp.config), plain[0], plain[1], plain[2])
    assert len(plain[1]) > 50 and np.array_equal(fixed[0], plain[0]) and fixed[3]["row_checksum"] == plain[3]["row_checksum"]
    _assert_same((fixed[1], fixed[2], expect[2], counts), expect)
