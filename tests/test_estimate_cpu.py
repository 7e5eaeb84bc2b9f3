"""Track estimates of the trace rows, host side (no GPU): the header's declarations and record layout against their
ctypes and numpy mirrors and the library's exports; the validation of the settings in Python and in the library's own
check (csrc/estimate_host.hpp, compiled alone); the numpy restatement (tests/estimate_reference.py) against analytic
truth on inputs that are exact in units; its bookkeeping; the C++ closed form, quantisation and step length -- the code
the kernel runs -- against the restatement bit for bit; and the Python run layer through the recording stand-in library
of tests/test_run_layer_cpu.py."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from tests import estimate_reference as ref

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_trace_configure_estimates", "attpc_estimates_last", "attpc_rows_estimate")
PYTHAGOREAN = [(16, 63), (25, 60), (33, 56), (39, 52)]  # a^2 + b^2 = 65^2


# ---------------------------------------------------------------- header, layout, symbols ----
def test_header_abi_and_library_agree():
    import __graft_entry__ as entry

    header = (ROOT / "include" / "attpc_engine.h").read_text()
    assert "track estimates of the trace rows" in header
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.ESTIMATE_SYMBOLS == ENTRY_POINTS and "estimates" in _abi.CONFIGURE_SLOTS
    assert "estimate.hip" in entry.HIP_SOURCES and "estimate.hip" in (ROOT / "tools" / "build_variant.sh").read_text()
    structs = {"attpc_track_estimate": _abi.TrackEstimate, "attpc_estimate_desc": _abi.EstimateDesc}
    lines = []
    for name, ctype in structs.items():
        args = ", ".join([f"sizeof({name})"] + [f"offsetof({name}, {field})" for field, _ in ctype._fields_])
        lines.append(f' printf("{" ".join(["%zu"] * (1 + len(ctype._fields_)))}\\n", {args});')
    bits = ("EMPTY", "FEW", "RANGE", "CAPPED", "NO_CIRCLE", "ON_AXIS", "NO_SLOPE", "MAX_FIT")
    lines.append(f' printf("{" ".join(["%d"] * (len(bits) + 1))}\\n", {", ".join("ATTPC_EST_" + b for b in bits)}, ATTPC_ABI_VERSION);')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n' + "\n".join(lines) + "\n return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (name, ctype) in zip(out, structs.items()):
        assert [int(v) for v in line.split()] == [C.sizeof(ctype)] + [getattr(ctype, f).offset for f, _ in ctype._fields_], name
    dtype = _abi.ESTIMATE_DTYPE
    assert dtype.itemsize == 128 == C.sizeof(_abi.TrackEstimate) and dtype.names == tuple(f for f, _ in _abi.TrackEstimate._fields_)
    assert [dtype.fields[f][1] for f in dtype.names] == [getattr(_abi.TrackEstimate, f).offset for f in dtype.names]
    assert dtype.names == ref.INT_FIELDS + ref.F64_FIELDS and all(dtype[f] == np.float64 for f in ref.F64_FIELDS)
    assert [int(v) for v in out[2].split()] == [_abi.EST_EMPTY, _abi.EST_FEW, _abi.EST_RANGE, _abi.EST_CAPPED, _abi.EST_NO_CIRCLE,
                                                _abi.EST_ON_AXIS, _abi.EST_NO_SLOPE, _abi.EST_MAX_FIT, 3] == [1, 2, 4, 8, 16, 32, 64, 2048, 3]
    assert "#define ATTPC_ABI_VERSION 3" in header and _abi.ABI_VERSION == 3
    entry.build()
    lib = _abi.load_library()
    assert lib.attpc_version() == 3
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and re.search(rf" T {name}$", nm, re.M), name


# ---------------------------------------------------------------- the host-side C++ of the stage, compiled alone ----
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("estimate_check")
    exe = tmp / "estimate_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}",
                    f"-I{ROOT / 'include'}", "-o", str(exe), str(ROOT / "tests" / "native" / "estimate_check.cpp")], check=True)

    def run(mode, data: np.ndarray, out_dtype):
        (tmp / "in.bin").write_bytes(np.ascontiguousarray(data).tobytes())
        subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], check=True)
        return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=out_dtype)

    return run


# ---------------------------------------------------------------- settings ----
@pytest.mark.parametrize("kw", [{"beam_region_radius": -1.0}, {"beam_region_radius": float("nan")},
                                {"beam_region_radius": float("inf")}, {"min_points": 2}, {"min_points": 0}, {"min_points": 30.0},
                                {"min_points": True}, {"magnetic_field": float("nan")}])
def test_settings_refuse(kw):
    from attpc_engine_amd.detector.estimate import EstimateSettings

    with pytest.raises(ValueError):
        EstimateSettings(**kw)


def test_settings_defaults_token_and_desc():
    from attpc_engine_amd.detector.estimate import EstimateSettings

    plain = EstimateSettings()
    assert (plain.beam_region_radius, plain.min_points, plain.magnetic_field) == (25.0, 30, None)
    with pytest.raises(ValueError):
        plain.token()  # no field yet
    with pytest.raises(ValueError):
        plain.for_field(float("nan"))
    bound = plain.for_field(2.85)
    d = bound.desc()
    assert (d.beam_region_radius, d.magnetic_field, d.min_points, d.reserved) == (25.0, 2.85, 30, 0)
    assert bound.token() == EstimateSettings(25.0, 30, magnetic_field=2.85).token() != EstimateSettings(20.0).for_field(2.85).token()
    assert EstimateSettings(magnetic_field=3.0).for_field(2.85).magnetic_field == 3.0 and EstimateSettings(0.0, 3).min_points == 3


def test_the_library_refuses_what_is_out_of_range(native):
    desc = np.dtype([("beam_region_radius", "<f8"), ("magnetic_field", "<f8"), ("min_points", "<i4"), ("reserved", "<i4")])
    cases = [((25.0, 2.85, 30, 0), 0), ((0.0, 0.0, 3, 0), 0), ((25.0, -3.0, 30, 0), 0), ((-1e-9, 2.85, 30, 0), 1),
             ((np.nan, 2.85, 30, 0), 1), ((np.inf, 2.85, 30, 0), 1), ((25.0, np.nan, 30, 0), 1), ((25.0, 2.85, 2, 0), 1),
             ((25.0, 2.85, -5, 0), 1), ((25.0, 2.85, 30, 1), 1), ((25.0, 2.85, 30, -1), 1)]
    assert desc.itemsize == C.sizeof(_abi.EstimateDesc)
    got = native("desc", np.array([c for c, _ in cases], dtype=desc), np.uint8)
    assert got.tolist() == [bad for _, bad in cases]


# ---------------------------------------------------------------- the restatement against analytic truth ----
def _circle_points(k, centre):
    """Points in units on the circle of radius 65 k about ``centre`` (integers), by angle over 3/4 of a turn from the
    point nearest the origin's side: the Pythagorean points and their transposes, all signs."""
    pts = set()
    for a, b in PYTHAGOREAN + [(b, a) for a, b in PYTHAGOREAN] + [(0, 65), (65, 0)]:
        pts |= {(sa * a, sb * b) for sa in (1, -1) for sb in (1, -1)}
    pts = sorted(pts, key=lambda p: np.arctan2(p[1], p[0]) % (2 * np.pi))
    start = next(i for i, p in enumerate(pts) if p == (-65, 0))
    pts = (pts[start:] + pts[:start])[:int(0.75 * len(pts))]
    return np.array([(centre[0] + k * x, centre[1] + k * y) for x, y in pts], dtype=np.int64)


@pytest.mark.parametrize("k,centre", [(16, (1600, 320)), (31, (2500, -700)), (7, (-900, 450))])
def test_reference_recovers_an_exact_circle(k, centre):
    xy = _circle_points(k, centre)
    n = len(xy)
    assert n >= 26 and np.all((xy[:, 0] - centre[0]) ** 2 + (xy[:, 1] - centre[1]) ** 2 == (65 * k) ** 2)
    rows = ref.spyral_rows(xy[:, 0], xy[:, 1], 1000 + 40 * np.arange(n))
    # every row used, the whole track in the segment: more than half a turn
    rec = ref.track_record(rows, ref.Params(beam_region_radius=0.0, min_points=n, magnetic_field=3.0))
    outward = 1 if xy[0] @ xy[0] <= xy[-1] @ xy[-1] else -1
    assert (rec["n_rows"], rec["n_used"], rec["n_fit"], rec["status"], rec["direction"]) == (n, n, n, 0, outward)
    # the sums are exact integers below 2^53; what is left is the closed form's few dozen roundings on numbers of
    # order one, far below 1e-9 mm
    assert abs(rec["cx"] - centre[0] / 16.0) < 1e-9 and abs(rec["cy"] - centre[1] / 16.0) < 1e-9
    assert abs(rec["radius"] - 65 * k / 16.0) < 1e-9
    c = np.hypot(centre[0], centre[1]) / 16.0
    assert abs(rec["vx"] - centre[0] / 16.0 * (1 - 65 * k / 16.0 / c)) < 1e-9
    theta = np.arctan2(1.0, rec["slope"])
    assert abs(rec["brho"] - 3.0 * 65 * k / 16.0 * 1e-3 / np.sin(theta)) < 1e-12 and rec["charge"] == 100 * n


@pytest.mark.parametrize("k", [1, 5, 16])
def test_reference_on_an_exact_line(k):
    n = 41
    i = np.arange(n)
    rows = ref.spyral_rows(480 + 3 * k * i, 4 * k * i, 2000 + 7 * k * i)  # starts at 30 mm, outside the beam region
    back = ref.spyral_rows(480 + 3 * k * i[::-1], 4 * k * i[::-1], 2000 + 7 * k * i)  # the same track travelling backward in z
    for track, direction, slope in ((rows, 1, 1.4), (back, -1, -1.4)):
        rec = ref.track_record(track, ref.Params())
        m = max((n + 1) // 2, 30)
        assert (rec["n_used"], rec["n_fit"], rec["direction"]) == (n, m, direction)
        assert rec["status"] == _abi.EST_NO_CIRCLE and rec["slope"] == slope and rec["arc"] == 5 * k * (m - 1)
        assert all(np.isnan(rec[f]) for f in ("cx", "cy", "radius", "vx", "vy", "vz", "brho"))
        assert rec["x_mean"] == (480 + 3 * k * (m - 1) / 2) / 16.0 and rec["dedx"] == 100.0 * m / (5 * k * (m - 1) / 16.0)


# ---------------------------------------------------------------- bookkeeping of the restatement ----
def test_duplicate_index_other_labels_and_few_points():
    track = ref.arc_track(70)
    rows = np.concatenate([track, ref.arc_track(12, phase=2.0)])
    labels = np.concatenate([np.where(np.arange(70) % 7 == 3, -1, 2), np.full(12, 5)])
    got = ref.records([0, 0, len(rows)], rows, labels, [2, 5, 2, 9], ref.Params())
    assert got.shape == (2, 4) and got[0]["status"].tolist() == [_abi.EST_EMPTY] * 4
    first, few, twice, absent = got[1]
    assert first["n_rows"] == 60 and first["status"] == 0 and first["n_fit"] == max((first["n_used"] + 1) // 2, 30)
    alone = ref.track_record(track[np.arange(70) % 7 != 3], ref.Params())
    assert all(first[f] == alone[f] for f in ref.INT_FIELDS + ref.F64_FIELDS)  # label -1 takes no part
    assert (few["n_rows"], few["status"], few["n_fit"], few["direction"], few["charge"], few["arc"]) == (12, _abi.EST_FEW, 0, 0, 0, 0)
    for rec in (few, twice, absent):
        assert all(np.isnan(rec[f]) for f in ref.F64_FIELDS)
    assert (twice["n_rows"], twice["status"]) == (0, _abi.EST_EMPTY) == (absent["n_rows"], absent["status"])
    # min_points exactly, and one short
    assert ref.track_record(track, ref.Params(0.0, 70))["status"] == 0
    assert ref.track_record(track, ref.Params(0.0, 71))["status"] == _abi.EST_FEW


def test_cap_and_range():
    long_track = ref.arc_track(4200, dz_mm=0.2, turn=2.5)
    rec = ref.track_record(long_track, ref.Params(0.0))
    assert (rec["n_used"], rec["n_fit"]) == (4200, 2048) and rec["status"] & _abi.EST_CAPPED
    assert not ref.track_record(long_track[:4096], ref.Params(0.0))["status"] & _abi.EST_CAPPED  # m = 2048 on its own
    track = ref.arc_track(80)
    plain = ref.track_record(track, ref.Params())
    for column, value in ((0, 321.0), (2, np.nan), (1, -320.5), (4, 2.0 ** 31), (2, np.inf)):
        bad = track.copy()
        bad[40, column] = value
        rec = ref.track_record(bad, ref.Params())
        assert rec["status"] == _abi.EST_RANGE and (rec["n_rows"], rec["n_used"]) == (80, plain["n_used"] - 1)
    edge = track.copy()
    edge[40, 0], edge[41, 2], edge[42, 4] = 320.0, -8192.0, -(2.0 ** 31 - 0.75)
    assert ref.track_record(edge, ref.Params())["status"] == 0  # the limits themselves are in range
    # the beam region is an integer comparison in units
    ring = ref.spyral_rows([400] * 40, [0] * 40, np.arange(40))
    assert ref.track_record(ring, ref.Params(25.0, 30))["n_used"] == 40 and ref.track_record(ring, ref.Params(25.04, 30))["n_used"] == 0


# ---------------------------------------------------------------- the kernel's own C++ against the restatement ----
def test_native_closed_form_quantisation_and_steps_equal_the_restatement(native, monkeypatch):
    rng = np.random.default_rng(5)
    tracks = [ref.arc_track(n, jitter=j, rng=rng, **kw) for n, j, kw in [
        (64, 0.0, {}), (200, 0.8, dict(radius_mm=90.0, centre_mm=(-60.0, 70.0), turn=2.0)),
        (60, 0.3, dict(radius_mm=300.0, centre_mm=(290.0, 40.0), turn=0.3)),
        (4300, 1.5, dict(radius_mm=120.0, centre_mm=(100.0, -90.0), turn=5.0, dz_mm=0.2)),
        (3400, 0.5, dict(radius_mm=120.0, centre_mm=(100.0, -90.0), turn=5.0)),  # z leaves the range
        (90, 0.0, dict(radius_mm=60.0, centre_mm=(60.0, 0.0), turn=3.0))]]
    i = np.arange(40)
    tracks += [ref.spyral_rows(480 + 3 * i, 4 * i, 7 * i), ref.spyral_rows([500] * 40, [20] * 40, 5 * i),  # a line, a point
               ref.spyral_rows(*(np.array(v) for v in zip(*[(65 * a, 65 * b, 9 * n) for n, (a, b) in enumerate(
                   [(x, y) for x, y in [(16, 63), (25, 60), (33, 56), (39, 52), (52, 39), (56, 33), (60, 25), (63, 16)]] * 4)])))]
    captured = []
    closed = ref.closed_form
    monkeypatch.setattr(ref, "closed_form", lambda m, X0, Y0, Z0, k, arc, field: captured.append((m, X0, Y0, Z0, dict(k), arc, field))
                        or closed(m, X0, Y0, Z0, k, arc, field))
    want = [ref.track_record(t, ref.Params(10.0, 30, 2.85)) for t in tracks]
    assert len(captured) == len(tracks) and {w["status"] for w in want} >= {0, _abi.EST_NO_CIRCLE, _abi.EST_CAPPED, _abi.EST_RANGE}
    assert any(w["status"] & _abi.EST_NO_SLOPE for w in want)
    names = ("u", "v", "uu", "uv", "vv", "uuu", "uvv", "vvv", "vuu", "S", "w", "SS", "Sw", "I")
    sums = np.dtype([("k", "<i8", 19), ("field", "<f8")])
    data = np.zeros(len(captured), dtype=sums)
    for d, (m, X0, Y0, Z0, k, arc, field) in zip(data, captured):
        d["k"], d["field"] = [m, X0, Y0, Z0] + [k[n] for n in names] + [arc], field
    got = native("closed", data, _abi.ESTIMATE_DTYPE)
    for g, w in zip(got, want):
        assert g["status"] == w["status"] & ~(_abi.EST_CAPPED | _abi.EST_RANGE) and g["charge"] == w["charge"] and g["arc"] == w["arc"]
        for f in ref.F64_FIELDS:
            assert (np.isnan(g[f]) and np.isnan(w[f])) or np.float64(g[f]).tobytes() == np.float64(w[f]).tobytes(), f
    # quantisation: ties, limits, non-finite
    values = np.array([[0.03125, -0.03125, 0.09375, 0.5], [1.5 / 16, 2.5 / 16, -3.5 / 16, 1.5], [320.0, -320.0, 8192.0, 2.0 ** 31 - 0.75],
                       [320.0000001, 0.0, 0.0, 0.0], [0.0, 0.0, -8192.001, 0.0], [0.0, 0.0, 0.0, -(2.0 ** 31)],
                       [np.nan, 0.0, 0.0, 0.0], [0.0, np.inf, 0.0, 0.0], [17.03, -250.77, 512.49, 1234.5]])
    out = native("rows", values, np.dtype([("ok", "<i4"), ("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("I", "<i8")]))
    assert out["ok"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 1]
    good = out["ok"] == 1
    np.testing.assert_array_equal(np.stack([out[c][good] for c in "XYZ"], axis=1), np.rint(16.0 * values[good, :3]).astype(np.int64))
    np.testing.assert_array_equal(out["I"][good], np.rint(values[good, 3]).astype(np.int64))
    assert out[0].tolist()[1:] == (0, 0, 2, 0) and out[1].tolist()[1:] == (2, 2, -4, 2)  # half to even
    steps = rng.integers(-10240, 10241, size=(5000, 2)).astype(np.int32)
    steps[:4] = [[0, 0], [3, 4], [10240, -10240], [1, 1]]
    import math

    d = native("steps", steps, np.int32)
    assert d.tolist() == [int(np.rint(math.sqrt(float(int(x) * int(x) + int(y) * int(y))))) for x, y in steps]


# ---------------------------------------------------------------- the Python run layer, the library replaced ----
def test_run_layer_configures_and_collects():
    from attpc_engine_amd.detector.estimate import EstimateSettings, azimuthal, configure_estimates, polar, truth_tracks
    from attpc_engine_amd.detector.traces import TraceChain
    from tests.test_run_layer_cpu import RecordingContext

    config = workloads.o16aa()[1]
    ctx = RecordingContext()
    TraceChain(config).configure(ctx, rows=True)
    assert "trace_configure_estimates" not in ctx.lib.names() and ctx._tokens["estimates"] is None  # off: never called
    settings = EstimateSettings(20.0, 12)
    TraceChain(config).replace(estimates=settings).configure(ctx, rows=True)
    want = {"beam_region_radius": 20.0, "magnetic_field": float(config.det_params.bfield), "min_points": 12, "reserved": 0}
    assert ctx.lib.stage_descs()[-1] == ("configure_estimates", want)
    assert ctx._tokens["estimates"] == settings.for_field(config.det_params.bfield).token()
    n_calls = len(ctx.lib.calls)
    configure_estimates(ctx, settings, config)
    assert len(ctx.lib.calls) == n_calls  # the same content: no call
    TraceChain(config).configure(ctx, rows=True, keep=("estimates",))
    assert ctx._tokens["estimates"] is not None
    TraceChain(config).configure(ctx, rows=True)
    assert ctx._tokens["estimates"] is None and ctx.lib.stage_descs()[-1] == ("configure_estimates", None)
    with pytest.raises(TypeError):
        TraceChain(config, estimates={"min_points": 3})
    # the trigonometry and the truth
    est = np.zeros(4, dtype=_abi.ESTIMATE_DTYPE)
    est["slope"] = [0.0, 1.0, -1.0, np.nan]
    est["x_mean"], est["y_mean"] = [1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, -1.0]
    np.testing.assert_allclose(polar(est)[:3], [np.pi / 2, np.pi / 4, 3 * np.pi / 4], rtol=0, atol=1e-15)
    assert np.isnan(polar(est)[3])
    np.testing.assert_allclose(azimuthal(est), [0.0, np.pi / 2, np.pi, 3 * np.pi / 2], rtol=0, atol=1e-15)
    p4 = np.zeros((1, 3, 4))
    p4[0, 1, :3], p4[0, 2, :3] = (0.0, 299.792458, 299.792458), (-100.0, 0.0, 0.0)
    truth = truth_tracks(p4, [1, 2, 0], [0, 2, 1])
    np.testing.assert_allclose(truth["brho"][0, :2], [np.sqrt(2.0) / 2.0, 100.0 / 299.792458], rtol=1e-15)
    np.testing.assert_allclose(truth["polar"][0, :2], [np.pi / 4, np.pi / 2], rtol=0, atol=1e-15)
    np.testing.assert_allclose(truth["azimuthal"][0, :2], [np.pi / 2, np.pi], rtol=0, atol=1e-15)
    assert truth["brho"].shape == (1, 3) and not np.isfinite(truth["brho"][0, 2])  # Z = 0
