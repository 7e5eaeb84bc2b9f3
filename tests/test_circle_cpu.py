"""Geometric circle fit, host side (no GPU): the header's declarations against their ctypes mirrors, the Python settings
and the library's exports; the validation of the settings in Python and in the library's own check
(csrc/circle_host.hpp, compiled alone); that C++ -- the code the kernel runs -- against the numpy restatement
(tests/circle_reference.py) bit for bit; the restatement against scipy's Levenberg-Marquardt; what the fit is for, on
short noisy arcs; the same C++ under the address and undefined-behaviour sanitizers, as a program of its own; and the
Python run layer through the recording stand-in library of tests/test_run_layer_cpu.py."""
import ctypes as C
import math
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from tests import circle_reference as ref
from tests import estimate_reference as est

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_trace_configure_circle", "attpc_rows_estimate_circle")
SOURCE = ROOT / "tests" / "native" / "circle_check.cpp"
COMPILE = ["g++", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}",
           f"-I{ROOT / 'include'}"]
CASE = np.dtype([("a", "<f8"), ("b", "<f8"), ("R", "<f8"), ("tolerance", "<f8"), ("max_evaluations", "<i4"), ("m", "<i4")])
FIT = np.dtype([("a", "<f8"), ("b", "<f8"), ("R", "<f8"), ("evaluations", "<i4"), ("converged", "<i4")])
RECORD_CASE = np.dtype([("k", "<i8", 19), ("field", "<f8"), ("tolerance", "<f8"), ("max_evaluations", "<i4"), ("pad", "<i4")])
DESC = np.dtype([("tolerance", "<f8"), ("max_evaluations", "<i4"), ("reserved", "<i4")])


def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


# ---------------------------------------------------------------- header, layout, symbols ----
def test_header_abi_and_python_agree():
    import __graft_entry__ as entry
    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import STATUS_BITS

    header = (ROOT / "include" / "attpc_engine.h").read_text()
    assert "geometric circle fit" in header
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.CIRCLE_SYMBOLS == ENTRY_POINTS and "circle" in _abi.CONFIGURE_SLOTS
    assert "circle_host.hpp" in (ROOT / "__graft_entry__.py").read_text()  # a change of it rebuilds the library
    fields = _abi.CircleDesc._fields_
    args = ", ".join(["sizeof(attpc_circle_desc)"] + [f"offsetof(attpc_circle_desc, {f})" for f, _ in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n'
           f' printf("{" ".join(["%zu"] * (1 + len(fields)))}\\n", {args});\n'
           ' printf("%d %d %d %d %zu\\n", ATTPC_EST_NOT_CONVERGED, ATTPC_CIRCLE_MIN_EVALUATIONS, ATTPC_CIRCLE_MAX_EVALUATIONS,'
           ' ATTPC_ABI_VERSION, sizeof(attpc_track_estimate));\n return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    assert [int(v) for v in out[0].split()] == [C.sizeof(_abi.CircleDesc)] + [getattr(_abi.CircleDesc, f).offset for f, _ in fields]
    assert DESC.itemsize == C.sizeof(_abi.CircleDesc) == 16
    assert [int(v) for v in out[1].split()] == [_abi.EST_NOT_CONVERGED, _abi.CIRCLE_MIN_EVALUATIONS, _abi.CIRCLE_MAX_EVALUATIONS,
                                                _abi.ABI_VERSION, _abi.ESTIMATE_DTYPE.itemsize] == [128, 2, 64, 3, 128]
    assert STATUS_BITS["NOT_CONVERGED"] == 128 and len(set(STATUS_BITS.values())) == len(STATUS_BITS) == 8
    # the defaults: header text, _abi, the settings class, the restatement
    assert re.search(r"tolerance in units, finite and > 0 \(default 2\^-7\); max_evaluations in 2 \.\. 64 \(default\s+\*?\s*32\)", header)
    plain, d = CircleFitSettings(), CircleFitSettings().desc()
    assert (plain.max_evaluations, plain.tolerance) == (32, 2.0 ** -7) == (_abi.CIRCLE_DEFAULT_EVALUATIONS, _abi.CIRCLE_DEFAULT_TOLERANCE)
    assert (d.tolerance, d.max_evaluations, d.reserved) == (2.0 ** -7, 32, 0)
    assert (ref.Settings().max_evaluations, ref.Settings().tolerance) == (32, 2.0 ** -7) and ref.LAMBDA0 == 2.0 ** -10
    entry.build()
    lib = _abi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and re.search(rf" T {name}$", nm, re.M), name


@pytest.mark.parametrize("kw", [{"max_evaluations": 1}, {"max_evaluations": 65}, {"max_evaluations": 0}, {"max_evaluations": 8.0},
                                {"max_evaluations": True}, {"tolerance": 0.0}, {"tolerance": -1.0}, {"tolerance": float("nan")},
                                {"tolerance": float("inf")}, {"tolerance": "1"}])
def test_settings_refuse(kw):
    from attpc_engine_amd.detector.circle import CircleFitSettings

    with pytest.raises(ValueError):
        CircleFitSettings(**kw)


def test_settings_token_and_types():
    from attpc_engine_amd.detector.circle import CircleFitSettings, configure_circle
    from attpc_engine_amd.detector.traces import TraceChain
    from tests.test_run_layer_cpu import RecordingContext

    assert CircleFitSettings(2, 1.0).token() == (1.0, 2) != CircleFitSettings(64, 1.0).token()
    assert CircleFitSettings(np.int32(16), np.float32(0.5)).token() == (0.5, 16)
    config = workloads.o16aa()[1]
    with pytest.raises(TypeError):
        TraceChain(config, circle={"max_evaluations": 3})
    with pytest.raises(TypeError):
        TraceChain(config).replace(circle=32)
    with pytest.raises(TypeError):
        configure_circle(RecordingContext(), (32, 1.0))


# ---------------------------------------------------------------- the host-side C++ of the stage, compiled alone ----
def _runner(tmp, exe):
    def run(mode, heads: np.ndarray, points, out_dtype):
        """``heads``: one record per case; ``points``: per case (u, v), or None (no points behind a head)."""
        blob = b""
        for i, head in enumerate(heads):
            blob += head.tobytes()
            if points is not None:
                blob += np.ascontiguousarray(np.stack(points[i], axis=1), dtype="<i4").tobytes()
        (tmp / "in.bin").write_bytes(blob)
        subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], check=True)
        return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=out_dtype)

    return run


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("circle_check")
    exe = tmp / "circle_check"
    subprocess.run(COMPILE + ["-O2", "-o", str(exe), str(SOURCE)], check=True)
    return _runner(tmp, exe)


DESC_CASES = [((2.0 ** -7, 32, 0), 0), ((1e-300, 2, 0), 0), ((1e300, 64, 0), 0), ((0.0, 32, 0), 1), ((-1.0, 32, 0), 1),
              ((np.nan, 32, 0), 1), ((np.inf, 32, 0), 1), ((1.0, 1, 0), 1), ((1.0, 65, 0), 1), ((1.0, -3, 0), 1), ((1.0, 32, 1), 1),
              ((1.0, 32, -1), 1)]


def test_the_library_refuses_what_is_out_of_range(native):
    got = native("desc", np.array([c for c, _ in DESC_CASES], dtype=DESC), None, np.uint8)
    assert got.tolist() == [bad for _, bad in DESC_CASES]


def point_sets():
    """name -> (u, v, start or None = the Kasa circle, Settings): the cases of the fit, fixed."""
    rng = np.random.default_rng(24)
    sets = {}
    for m in (3, 63, 64, 65, 129, 2048):  # lane-partition edges and the cap
        u, v = ref.arc_points(m, arc_deg=25.0 if m > 3 else 8.0, jitter=6.0 if m > 3 else 0.0, rng=rng)
        sets[f"m{m}"] = (u, v, None, ref.Settings())
    sets["full circle"] = (*ref.arc_points(80, radius=1500.0, arc_deg=355.0, jitter=5.0, rng=rng), None, ref.Settings())
    sets["arc 20 deg"] = (*ref.arc_points(25, arc_deg=20.0, jitter=9.6, rng=rng), None, ref.Settings())
    u, v = ref.arc_points(40, arc_deg=30.0, jitter=4.0, rng=rng)
    sets["point at the trial centre"] = (u, v, (float(u[7]), float(v[7]), 900.0), ref.Settings())  # r == 0 at evaluation 1
    sets["two evaluations"] = (*ref.arc_points(25, arc_deg=20.0, jitter=9.6, rng=rng), None, ref.Settings(max_evaluations=2))
    # a small circle about a spot beside the arc: the first, nearly undamped step overshoots and is rejected
    u, v = ref.arc_points(30, arc_deg=15.0, jitter=8.0, rng=np.random.default_rng(7))
    sets["rejected first step"] = (u, v, (float(u[3]) + 3.0, float(v[3]) - 3.0, 200.0), ref.Settings())
    return sets


@pytest.fixture(scope="module")
def fits():
    """name -> (u, v, start, settings, the restatement's (a, b, R, evaluations, converged, F), its trace)."""
    out = {}
    for name, (u, v, start, settings) in point_sets().items():
        start = ref.kasa_start(u, v) if start is None else start
        trace = []
        out[name] = (u, v, start, settings, ref.fit(u, v, start, settings, trace), trace)
    return out


def test_the_cases_are_what_they_claim(fits):
    for name, (u, v, start, settings, (a, b, R, evaluations, converged, F), trace) in fits.items():
        assert 1 <= evaluations <= settings.max_evaluations and len(trace) == evaluations - 1, name
        assert converged == (name != "two evaluations"), name
        assert np.abs(u).max() <= 10240 and np.abs(v).max() <= 10240, name
    assert fits["two evaluations"][4][3] == 2
    assert fits["rejected first step"][5][0][0] is False and fits["rejected first step"][4][4]
    assert len(fits["m2048"][0]) == est.EST_MAX_FIT
    u, v, start, *_ = fits["point at the trial centre"]
    assert np.any((u == start[0]) & (v == start[1]))


def test_native_fit_and_evaluation_equal_the_restatement(native, fits):
    names = list(fits)
    heads = np.zeros(len(names), dtype=CASE)
    for head, name in zip(heads, names):
        u, v, start, settings, *_ = fits[name]
        head["a"], head["b"], head["R"] = start
        head["tolerance"], head["max_evaluations"], head["m"] = settings.tolerance, settings.max_evaluations, len(u)
    points = [fits[name][:2] for name in names]
    sums = native("eval", heads, points, np.dtype([(s, "<f8") for s in ref.SUMS]))
    got = native("fit", heads, points, FIT)
    for name, k, g in zip(names, sums, got):
        u, v, start, settings, (a, b, R, evaluations, converged, _), _ = fits[name]
        want = ref.evaluate(np.asarray(u), np.asarray(v), *start)
        for s in ref.SUMS:
            assert same_bits(k[s], want[s]), (name, s)
        assert (g["evaluations"], bool(g["converged"])) == (evaluations, converged), name
        assert same_bits(g["a"], a) and same_bits(g["b"], b) and same_bits(g["R"], R), name


def track_rows(u, v, X0=900, Y0=-400):
    """Spyral rows whose fit segment is exactly the points (u, v) + (X0, Y0): with min_points = m and no beam region the
    segment is the first m = max((n + 1) div 2, m) of n = m rows, direction +1 as long as the first point is nearest the
    axis; z rises by 3 mm a row."""
    X, Y = np.asarray(u) + X0, np.asarray(v) + Y0
    return est.spyral_rows(X, Y, 48 * np.arange(len(X)))


def test_native_records_equal_the_restatement(native, fits, monkeypatch):
    """Step 6 with the stage on -- Kasa, refinement, everything behind the circle -- through the C++ the kernel runs."""
    i = np.arange(40)
    tracks = {name: (track_rows(u, v), settings) for name, (u, v, start, settings, *_) in fits.items()
              if name not in ("point at the trial centre", "rejected first step")}  # (their start is not the Kasa circle)
    tracks["collinear"] = (est.spyral_rows(480 + 3 * i, 4 * i, 7 * i), ref.Settings())
    tracks["a point"] = (est.spyral_rows([500] * 40, [20] * 40, 5 * i), ref.Settings())  # NO_CIRCLE and NO_SLOPE
    captured = []
    closed = est.closed_form
    monkeypatch.setattr(est, "closed_form", lambda m, X0, Y0, Z0, k, arc, field: captured.append((m, X0, Y0, Z0, dict(k), arc, field))
                        or closed(m, X0, Y0, Z0, k, arc, field))
    names = ("u", "v", "uu", "uv", "vv", "uuu", "uvv", "vvv", "vuu", "S", "w", "SS", "Sw", "I")
    heads, points, want = np.zeros(len(tracks), dtype=RECORD_CASE), [], []
    for head, (name, (rows, settings)) in zip(heads, tracks.items()):
        params = est.Params(0.0, len(rows), 2.85)
        del captured[:]
        want.append(ref.track_record(rows, params, settings))
        m, X0, Y0, Z0, k, arc, field = captured[0]
        seg = ref.segment(rows, params)
        assert m == len(seg) == len(rows), name
        head["k"], head["field"] = [m, X0, Y0, Z0] + [k[n] for n in names] + [arc], field
        head["tolerance"], head["max_evaluations"] = settings.tolerance, settings.max_evaluations
        points.append((seg[:, 0] - seg[0, 0], seg[:, 1] - seg[0, 1]))
    got = native("record", heads, points, _abi.ESTIMATE_DTYPE)
    both = native("halves", heads, None, np.dtype([("whole", _abi.ESTIMATE_DTYPE), ("halves", _abi.ESTIMATE_DTYPE)]))
    assert both["whole"].tobytes() == both["halves"].tobytes() and len(both) == len(tracks)  # step 6 in one piece and in two
    assert {0, _abi.EST_NO_CIRCLE, _abi.EST_NO_CIRCLE | _abi.EST_NO_SLOPE} <= set(both["whole"]["status"].tolist())
    for name, g, w in zip(tracks, got, want):
        assert g["status"] == w["status"] and g["reserved"] == w["reserved"] and g["charge"] == w["charge"] and g["arc"] == w["arc"], name
        for f in est.F64_FIELDS:
            assert same_bits(g[f], w[f]), (name, f)
    by_name = dict(zip(tracks, want))
    for name in ("collinear", "a point"):  # NO_CIRCLE: untouched, the record of the stage off
        plain = est.track_record(tracks[name][0], est.Params(0.0, 40, 2.85))
        assert by_name[name]["status"] & _abi.EST_NO_CIRCLE and by_name[name]["reserved"] == 0
        assert all(same_bits(by_name[name][f], plain[f]) for f in est.F64_FIELDS) and by_name[name]["status"] == plain["status"]
    two = by_name["two evaluations"]
    assert two["status"] & _abi.EST_NOT_CONVERGED and two["reserved"] == 2
    assert all(not w["status"] & _abi.EST_NOT_CONVERGED and w["reserved"] >= 2 for n, w in by_name.items()
               if n not in ("two evaluations", "collinear", "a point"))
    # the fields that do not depend on the circle are those of the stage off
    plain = est.track_record(tracks["arc 20 deg"][0], est.Params(0.0, 25, 2.85))
    moved = by_name["arc 20 deg"]
    assert all(same_bits(moved[f], plain[f]) for f in ("slope", "x_mean", "y_mean", "dedx")) and moved["radius"] != plain["radius"]


# ---------------------------------------------------------------- the restatement against an independent optimiser ----
# Observed here (scipy 1.15.3, MINPACK lmdif through least_squares(method="lm"), xtol = ftol = gtol = 1e-15), over the
# converged cases of point_sets(): the largest F_ref / F_scipy - 1 was 4.2e-14 ("point at the trial centre"; the others
# between -6e-16 and 2.8e-14: the level of the two orders of summation) and the largest |dR| / R 2.6e-8 ("m63"; "arc 20
# deg" 1.3e-8): the restatement stops at a step of 2^-7 units on a radius near 4800, scipy at machine precision.
# Neither bound can be derived; each is the observed value times 4, for other scipy builds.
EXCESS_BOUND = 4 * 4.2e-14
RADIUS_BOUND = 4 * 2.6e-8


def test_the_restatement_against_scipy(fits):
    from scipy import optimize
    worst_excess, worst_radius = 0.0, 0.0
    for name, (u, v, start, settings, (a, b, R, evaluations, converged, F), _) in fits.items():
        if not converged:
            continue
        uf, vf = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        res = optimize.least_squares(lambda p: np.hypot(uf - p[0], vf - p[1]) - p[2], np.array(start), method="lm",
                                     xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
        f_scipy = float(np.sum(res.fun ** 2))
        radius = abs(R - res.x[2]) / res.x[2]
        if len(u) == 3:  # three points lie on their circle: the minimum is 0 and a ratio to it says nothing; both
            # objectives are then rounding alone, a few ulp of r (|g| <= 4 eps R) in each of the three residuals
            assert max(F, f_scipy) <= 3.0 * (4.0 * np.finfo(np.float64).eps * R) ** 2, (name, F, f_scipy)
            excess = 0.0
        else:
            excess = F / f_scipy - 1.0
        print(f"{name}: F_ref / F_scipy - 1 = {excess:.3e}, |dR| / R = {radius:.3e}, evaluations {evaluations}, scipy nfev {res.nfev}")
        worst_excess, worst_radius = max(worst_excess, excess), max(worst_radius, radius)
    print(f"worst: excess {worst_excess:.3e} (bound {EXCESS_BOUND:.3e}), radius {worst_radius:.3e} (bound {RADIUS_BOUND:.3e})")
    assert worst_excess <= EXCESS_BOUND and worst_radius <= RADIUS_BOUND


# ---------------------------------------------------------------- what the fit is for ----
def test_the_geometric_fit_removes_the_bias_of_short_noisy_arcs():
    """400 arcs of 25 points over 20 degrees of a 300 mm circle, 0.6 mm jitter, coordinates quantised to 1/16 mm."""
    rng = np.random.default_rng(2024)
    R_true, ratios_kasa, ratios_geometric, unconverged, evaluations = 300.0 * 16.0, [], [], 0, []
    for _ in range(400):
        centre = rng.uniform(-500.0, 500.0, 2)
        u, v = ref.arc_points(25, radius=R_true, centre=centre, start=rng.uniform(0.0, 2.0 * np.pi), arc_deg=20.0, jitter=0.6 * 16.0,
                              rng=rng)
        start = ref.kasa_start(u, v)
        assert start is not None
        a, b, R, n, converged, _ = ref.fit(u, v, start, ref.Settings())
        ratios_kasa.append(start[2] / R_true)
        ratios_geometric.append(R / R_true)
        unconverged += not converged
        evaluations.append(n)
    print(f"median R / R_true: Kasa {np.median(ratios_kasa):.4f}, geometric {np.median(ratios_geometric):.4f}; "
          f"evaluations median {int(np.median(evaluations))} max {max(evaluations)}; NOT_CONVERGED {unconverged} of 400")
    assert 0.97 <= np.median(ratios_geometric) <= 1.03
    assert np.median(ratios_kasa) < 0.92
    assert unconverged <= 8  # 2 % of 400


# ---------------------------------------------------------------- the same C++ under the sanitizers, a program of its own ----
def test_the_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path, fits):
    exe = tmp_path / "circle_check_san"
    subprocess.run(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(SOURCE)],
                   check=True)
    run = _runner(tmp_path, exe)
    names = list(fits)
    heads = np.zeros(len(names), dtype=CASE)
    for head, name in zip(heads, names):
        u, v, start, settings, *_ = fits[name]
        head["a"], head["b"], head["R"] = start
        head["tolerance"], head["max_evaluations"], head["m"] = settings.tolerance, settings.max_evaluations, len(u)
    got = run("fit", heads, [fits[name][:2] for name in names], FIT)
    assert got["evaluations"].tolist() == [fits[name][4][3] for name in names]
    assert run("desc", np.array([c for c, _ in DESC_CASES], dtype=DESC), None, np.uint8).tolist() == [bad for _, bad in DESC_CASES]


# ---------------------------------------------------------------- the Python run layer, the library replaced ----
def test_run_layer_configures_and_reports():
    from attpc_engine_amd.detector.circle import CircleFitSettings, circle_result, configure_circle
    from attpc_engine_amd.detector.estimate import EstimateSettings
    from attpc_engine_amd.detector.traces import TraceChain, configure_trace_rows
    from attpc_engine_amd.engine import Engine
    from tests.test_run_layer_cpu import RecordingContext

    pipeline, config, indices = workloads.o16aa()
    ctx = RecordingContext()
    TraceChain(config).configure(ctx, rows=True)
    assert "trace_configure_circle" not in ctx.lib.names() and ctx._tokens["circle"] is None  # off: never called
    settings = CircleFitSettings(12, 0.25)
    TraceChain(config).replace(circle=settings).configure(ctx, rows=True)
    assert ctx.lib.stage_descs()[-1] == ("configure_circle", {"tolerance": 0.25, "max_evaluations": 12, "reserved": 0})
    assert circle_result(ctx) == {}  # alone it is inert
    n_calls = len(ctx.lib.calls)
    configure_circle(ctx, CircleFitSettings(12, 0.25))
    assert len(ctx.lib.calls) == n_calls  # the same content: no call
    TraceChain(config).configure(ctx, rows=True, keep=("estimates",))
    assert ctx._tokens["circle"] == settings.token()  # kept with the estimates
    TraceChain(config).replace(estimates=EstimateSettings(), circle=settings).configure(ctx, rows=True)
    assert circle_result(ctx) == {"circle": "geometric"}
    configure_trace_rows(config, ctx)  # None leaves what the ctx holds ...
    assert ctx._tokens["circle"] == settings.token()
    configure_trace_rows(config, ctx, circle=CircleFitSettings())  # ... a value is configured
    assert ctx._tokens["circle"] == CircleFitSettings().token()
    TraceChain(config).configure(ctx, rows=True)
    assert ctx._tokens["circle"] is None and ctx.lib.stage_descs()[-1] == ("configure_circle", None)
    engine = Engine(pipeline, config, indices, context=RecordingContext())
    engine.configure_estimates(EstimateSettings())
    engine.configure_circle_fit(max_evaluations=16)
    assert engine.ctx.lib.stage_descs()[-1] == ("configure_circle", {"tolerance": 2.0 ** -7, "max_evaluations": 16, "reserved": 0})
    res = engine.run_trace_rows(4, fetch=False)
    assert res["circle"] == "geometric" and "thinning" not in res
    engine.configure_circle_fit()
    assert "circle" not in engine.run_trace_rows(4, fetch=False)
    with pytest.raises(TypeError):
        engine.configure_circle_fit(CircleFitSettings(), tolerance=1.0)
