"""The track fit without a GPU (include/attpc_engine.h, "track fit"): header, struct layout, symbols and settings; the
restatement's integrator (tests/fit_reference.py) against the oracle's trajectory and its stopping-power look-up against
tests/dedx_reference.py; the recovery of known parameters from perturbed starts on the hand-made cases
(tests/fit_cases.py); the host C++ (csrc/fit_host.hpp through tests/native/fit_check.cpp) against the restatement bit
for bit, also under the address and undefined-behaviour sanitizers, as a program of its own; and the restatement's
mutants, every one of which must fail one of these checks."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import dedx_reference
from tests import estimate_reference as est
from tests import fit_cases as cases
from tests import fit_reference as ref
from tests.fit_cases import INDICES8
from tests.helpers import Inputs

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_trace_configure_fit", "attpc_fits_last", "attpc_rows_fit")
SOURCE = ROOT / "tests" / "native" / "fit_check.cpp"
COMPILE = ["g++", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}",
           f"-I{ROOT / 'include'}"]
DESC = np.dtype([("time_step", "<f8"), ("tolerance_momentum", "<f8"), ("tolerance_position", "<f8"), ("max_steps", "<i4"),
                 ("max_evaluations", "<i4")])
CASE = np.dtype([("mass", "<f8"), ("bfield", "<f8"), ("efield", "<f8"), ("density", "<f8"), ("length", "<f8"), ("desc", DESC),
                 ("estimate", _abi.ESTIMATE_DTYPE), ("start", "<f8", (6,)), ("Z", "<i4"), ("use_start", "<i4"), ("n", "<i4"),
                 ("capped", "<i4")])
PARAMS = est.Params(cases.BEAM_REGION, cases.MIN_POINTS, 2.85)
SETTINGS = ref.Settings(**cases.SETTINGS)
RECOVERY_SCALE = 0.3  # of fit_cases.starts: 0.15 % of every momentum component and 0.09 mm of the vertex (see test_recovery)


# ---------------------------------------------------------------- 1. header, layout, symbols, settings ----
def test_header_abi_and_python_agree():
    import __graft_entry__ as entry
    from attpc_engine_amd import detector
    from attpc_engine_amd.detector import fit

    header = (ROOT / "include" / "attpc_engine.h").read_text()
    assert "---- track fit" in header
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.FIT_SYMBOLS == ENTRY_POINTS and "fit" in _abi.CONFIGURE_SLOTS
    graft = (ROOT / "__graft_entry__.py").read_text()
    assert '"fit.hip"' in graft and "fit_host.hpp" in graft  # built, and a change of the header rebuilds the library
    record = [("status", "status"), ("evaluations", "evaluations"), ("n_points", "n_points"), ("n_inside", "n_inside"),
              ("steps", "steps"), ("end", "end"), ("f", "f"), ("lambda", "lambda"), ("g", "g"), ("vertex", "vertex"), ("ke", "ke"),
              ("brho", "brho"), ("path", "path"), ("reserved", "reserved")]
    desc = [f for f, _ in _abi.FitDesc._fields_]
    args = ", ".join(["sizeof(attpc_track_fit)"] + [f"offsetof(attpc_track_fit, {c})" for c, _ in record]
                     + ["sizeof(attpc_fit_desc)"] + [f"offsetof(attpc_fit_desc, {f})" for f in desc])
    consts = ("ATTPC_FIT_EMPTY, ATTPC_FIT_FEW, ATTPC_FIT_CAPPED, ATTPC_FIT_NO_START, ATTPC_FIT_SINGULAR, ATTPC_FIT_STEP_CAP,"
              " ATTPC_FIT_NOT_CONVERGED, ATTPC_FIT_END_STOPPED, ATTPC_FIT_END_LEFT, ATTPC_FIT_END_STEP_CAP, ATTPC_FIT_END_NOT_FINITE,"
              " ATTPC_FIT_MAX_POINTS, ATTPC_FIT_MAX_STEPS, ATTPC_FIT_MIN_EVALUATIONS, ATTPC_FIT_MAX_EVALUATIONS, ATTPC_ABI_VERSION")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n'
           f' printf("{" ".join(["%zu"] * (2 + len(record) + len(desc)))}\\n", {args});\n'
           f' printf("{" ".join(["%d"] * 16)}\\n", {consts});\n return 0; }}\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    sizes = [int(v) for v in out[0].split()]
    assert sizes[0] == 128 == _abi.FIT_DTYPE.itemsize == C.sizeof(_abi.TrackFit)
    assert sizes[1:1 + len(record)] == [_abi.FIT_DTYPE.fields[name][1] for _, name in record] == \
        [0, 4, 8, 12, 16, 20, 24, 32, 40, 64, 88, 96, 104, 112]
    assert sizes[1 + len(record)] == 32 == C.sizeof(_abi.FitDesc) == DESC.itemsize
    assert sizes[2 + len(record):] == [getattr(_abi.FitDesc, f).offset for f in desc] == [DESC.fields[f][1] for f in desc]
    assert [int(v) for v in out[1].split()] == [
        _abi.FIT_EMPTY, _abi.FIT_FEW, _abi.FIT_CAPPED, _abi.FIT_NO_START, _abi.FIT_SINGULAR, _abi.FIT_STEP_CAP, _abi.FIT_NOT_CONVERGED,
        _abi.FIT_END_STOPPED, _abi.FIT_END_LEFT, _abi.FIT_END_STEP_CAP, _abi.FIT_END_NOT_FINITE, _abi.FIT_MAX_POINTS,
        _abi.FIT_MAX_STEPS, _abi.FIT_MIN_EVALUATIONS, _abi.FIT_MAX_EVALUATIONS, _abi.ABI_VERSION] == \
        [1, 2, 8, 16, 32, 64, 128, 1, 2, 3, 4, 2048, 10000, 2, 32, 3]
    assert fit.STATUS_BITS == {"EMPTY": 1, "FEW": 2, "CAPPED": 8, "NO_START": 16, "SINGULAR": 32, "STEP_CAP": 64, "NOT_CONVERGED": 128}
    assert fit.FIT_DTYPE is _abi.FIT_DTYPE
    for name in ("TrackFitSettings", "configure_track_fit", "rows_to_fit"):
        assert name in detector.__all__ and getattr(detector, name) is getattr(fit, name)
    # the restatement's constants are the header's and the shared code's
    shared = (ROOT / "attpc_engine_amd" / "csrc" / "fit_host.hpp").read_text()
    assert "#pragma clang fp contract(off)" in shared and not re.search(r"\b(rsqrt|sin|cos|tan|atan2?|exp|log|pow|fma)\s*\(", shared)
    assert (ref.LAMBDA0, ref.LAMBDA_ACCEPT, ref.LAMBDA_REJECT, ref.DELTA_MOMENTUM) == (2.0 ** -10, 0.04, 10.0, 2.0 ** -16)
    assert "FIT_DELTA_MOMENTUM = 1.52587890625e-05" in shared and float("1.52587890625e-05") == 2.0 ** -16
    entry.build()
    lib = _abi.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and re.search(rf" T {name}$", nm, re.M), name


GOOD = dict(time_step=1e-10, max_steps=10000, max_evaluations=12, tolerance_momentum=1e-4, tolerance_position=1e-4)
BAD = [dict(time_step=0.0), dict(time_step=-1e-10), dict(time_step=float("nan")), dict(time_step=float("inf")),
       dict(tolerance_momentum=0.0), dict(tolerance_momentum=float("nan")), dict(tolerance_position=float("inf")),
       dict(tolerance_position=-1.0), dict(max_steps=0), dict(max_steps=10001), dict(max_evaluations=1), dict(max_evaluations=33)]


def test_settings():
    from attpc_engine_amd.detector.fit import TrackFitSettings, _checked
    from attpc_engine_amd.detector.traces import TraceChain

    s = TrackFitSettings()
    assert s.token() == (1e-10, 1e-4, 1e-4, 10000, 12) and (s.slot, s.call) == ("fit", "attpc_trace_configure_fit")
    d = s.desc()
    assert (d.time_step, d.tolerance_momentum, d.tolerance_position, d.max_steps, d.max_evaluations) == s.token()
    assert TrackFitSettings(max_evaluations=2, max_steps=1).token()[3:] == (1, 2)
    for bad in BAD + [dict(max_steps=1.5), dict(max_evaluations=True), dict(max_steps="7")]:
        with pytest.raises(ValueError):
            TrackFitSettings(**{**GOOD, **bad})
    with pytest.raises(TypeError):
        _checked(12)
    inp = Inputs("be10dp")
    chain = TraceChain(inp.config, fit=s)
    assert chain.fit is s and chain.replace(fit=None).fit is None
    with pytest.raises(TypeError):
        chain.replace(fit=3)


# ---------------------------------------------------------------- the native program ----
def _run(exe, tmp, mode, blob, dtype):
    (tmp / "in.bin").write_bytes(blob)
    subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], check=True)
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=dtype)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fit_check")
    exe = tmp / "fit_check"
    subprocess.run(COMPILE + ["-O2", "-o", str(exe), str(SOURCE)], check=True)
    return lambda mode, blob, dtype: _run(exe, tmp, mode, blob, dtype)


def test_the_library_refuses_what_is_out_of_range(native):
    descs = np.zeros(1 + len(BAD), dtype=DESC)
    for i, change in enumerate([{}] + BAD):
        for name, value in {**GOOD, **change}.items():
            descs[i][name] = value
    assert native("desc", descs.tobytes(), np.uint8).tolist() == [0] + [1] * len(BAD)


# ---------------------------------------------------------------- 2. the integrator and the look-up ----
@pytest.fixture(scope="module")
def detector():
    inp = Inputs("be10dp")
    return inp, cases.model()


def _energies():
    rng = np.random.default_rng(30)
    edges = np.array([0.0, -1.0, np.nan, np.inf, 2.0 ** -30, np.nextafter(2.0 ** -30, 0), 2.0 ** 14, np.nextafter(2.0 ** 14, 0), 2.0 ** 15,
                      1.0, np.nextafter(1.0, 0), 1.03125, np.nextafter(1.03125, 0), 5e-324, 1e-6])
    return np.concatenate([edges, 2.0 ** rng.uniform(-31.0, 14.5, 4000)])


def test_the_lookup_is_the_reference_lookup_bit_for_bit(detector, native):
    _, model = detector
    ke = _energies()
    for sp in model.species:
        want = dedx_reference.lookup(sp.table, ke)
        got = ref.dedx(sp.table[None, :], ke[None, :])[0]
        assert got.tobytes() == want.tobytes()
        assert native("dedx", sp.table.tobytes() + ke.tobytes(), np.float64).tobytes() == want.tobytes()


ORACLE_TRACKS = [(0, 3.0, 0.6, 0.3), (0, 3.0, 2.4, 4.0), (0, 20.0, 1.2, 5.0), (1, 15.0, 0.8, 2.0), (1, 5.0, 1.9, 0.1), (0, 0.3, 1.0, 0.7)]


def oracle_difference(detector, mutant=None):
    """The largest distance in m between the restatement's samples at time_step 1e-10 and the oracle's, over the samples
    both have (the oracle leaves the terminal sample out), and the fewest samples compared."""
    from oracle import pyoracle

    inp, model = detector
    worst, fewest = 0.0, 1 << 30
    grid = ref.Settings(time_step=1e-10, max_steps=10000)
    for species, kinetic, polar, azimuth in ORACLE_TRACKS:
        sp = model.species[species]
        vertex = [0.002, -0.001, 0.4]
        g = cases.momentum(sp, kinetic, polar, azimuth)
        want = pyoracle.trajectory(inp.det_raw, species, vertex, np.array(g) * float(sp.mass))
        got, _ = ref.trajectory(sp, g + vertex, 1.0, grid, mutant)
        n = min(len(got), len(want))
        worst = max(worst, float(np.abs(got[:n, :3] - want[:n, :3]).max()))
        fewest = min(fewest, n)
    return worst, fewest


def test_integrator_against_the_oracle(detector):
    worst, fewest = oracle_difference(detector)
    assert fewest >= 50 and worst <= 1e-9, (worst, fewest)  # both are RK4 on this grid: only the rounding differs


# ---------------------------------------------------------------- 3. recovery, and the native program ----
@pytest.fixture(scope="module")
def hand(detector):
    _, model = detector
    events = cases.hand_cases(model)
    offsets, rows, labels = cases.csr(events)
    estimates = est.records(offsets, rows, labels, INDICES8, PARAMS)
    return events, (offsets, rows, labels), estimates


def restated(hand, model, start, mutant=None, settings=SETTINGS):
    _, csr, estimates = hand
    return ref.records(*csr, INDICES8, model, estimates, settings, cases.BEAM_REGION, start=start, mutant=mutant)


def recovery_failures(hand, model, mutant=None):
    """The regular tracks (those whose true track the settings can follow: no step cap, no shared z) whose fit from the
    perturbed start does not converge or ends above f at the truth."""
    events, (offsets, rows, labels), _ = hand
    got = restated(hand, model, cases.starts(events, scale=RECOVERY_SCALE), mutant)
    truths, names, bad, n = cases.truths(events), list(events), [], 0
    for e, name in enumerate(names):
        for case, label in events[name]:
            s = INDICES8.index(label)
            if name in ("same z", "collinear") or case.steps > SETTINGS.max_steps:
                continue
            mine = labels[offsets[e]:offsets[e + 1]] == label
            points, _ = ref.used_points(rows[offsets[e]:offsets[e + 1]][mine], cases.BEAM_REGION)
            f_truth = ref.objective([model.position[s]], [points], truths[e, s], model.length, SETTINGS)[0]
            n += 1
            rec = got[e, s]
            if rec["status"] & ~_abi.FIT_CAPPED or not rec["f"] <= f_truth:
                bad.append((name, s, int(rec["status"]), float(rec["f"]), float(f_truth)))
    return bad, n, got


def test_recovery(hand, detector):
    """A minimum cannot lie above the value at the truth: no tolerance.  The perturbation is 0.15 % of every momentum
    component and 0.09 mm of the vertex, in a fixed sign pattern: with max_evaluations = 8 and tolerances of 1e-3 every
    regular track converges from there; from 0.5 % and 0.3 mm the 129-point track stops 0.2 % above f(truth) with
    these tolerances, and with tolerances of 2e-4 three tracks need more than 8 evaluations."""
    _, model = detector
    bad, n, got = recovery_failures(hand, model)
    assert not bad and n == 9, bad
    events = hand[0]
    names = list(events)
    # the cases are there
    status, e8 = got["status"], names.index("eight")
    assert got["n_points"][e8].tolist() == [3, 7, 8, 9, 63, 64, 65, 129] and (got["evaluations"][e8] >= 2).all()
    assert status[names.index("capped"), 6] == _abi.FIT_CAPPED and got["n_points"][names.index("capped"), 6] == 2048
    assert status[e8, 2] & _abi.FIT_STEP_CAP and got["end"][e8, 2] == _abi.FIT_END_STEP_CAP and got["steps"][e8, 2] == SETTINGS.max_steps
    assert status[names.index("same z"), 3] & _abi.FIT_NOT_CONVERGED and got["evaluations"][names.index("same z"), 3] == SETTINGS.max_evaluations
    assert status[names.index("same z"), 1] == _abi.FIT_FEW and (status[names.index("empty")] == _abi.FIT_EMPTY).all()
    assert (status[names.index("single"), [0, 1, 2, 3, 5, 6, 7]] == _abi.FIT_EMPTY).all() and status[names.index("single"), 4] == 0
    assert {_abi.FIT_END_STOPPED, _abi.FIT_END_LEFT, _abi.FIT_END_STEP_CAP} <= set(got["end"][got["evaluations"] > 0].tolist())
    assert (got["g"][e8, :, 2] > 0).any() and (got["g"][e8, :, 2] < 0).any()  # forward and backward
    assert (got["n_inside"][e8] < got["n_points"][e8]).any()  # points beyond the end of the final trial


def native_cases(hand, model, start, settings=SETTINGS):
    events, (offsets, rows, labels), estimates = hand
    blob = b""
    inp = Inputs("be10dp")
    for e in range(len(offsets) - 1):
        for s, label in enumerate(INDICES8):
            sp = model.position[s]
            mine = labels[offsets[e]:offsets[e + 1]] == label
            points, n_used = ref.used_points(rows[offsets[e]:offsets[e + 1]][mine], cases.BEAM_REGION)
            head = np.zeros((), dtype=CASE)
            head["mass"], head["Z"] = (float(sp.mass), int(sp.charge)) if sp is not None else (1.0, 0)
            head["bfield"], head["efield"], head["density"], head["length"] = inp.det.bfield, inp.det.efield, inp.det.density, model.length
            for name in DESC.names:
                head["desc"][name] = getattr(settings, name)
            head["estimate"] = estimates[e, s]
            head["use_start"] = start is not None
            head["start"] = start[e, s] if start is not None else 0.0
            head["n"], head["capped"] = len(points), n_used > _abi.FIT_MAX_POINTS
            table = sp.table if sp is not None else np.zeros(_abi.DEDX_NODES)
            blob += head.tobytes() + table.tobytes() + np.ascontiguousarray(points).tobytes()
    return blob


def native_mismatch(native, hand, model, mutant=None):
    """Does the native program differ from the (mutant) restatement on the cases, from given starts or from the
    estimates?"""
    events = hand[0]
    for start in (cases.special_starts(events), None):
        want = restated(hand, model, start, mutant)
        got = native("fit", native_cases(hand, model, start), _abi.FIT_DTYPE).reshape(want.shape)
        try:
            ref.assert_same_records(got, want)
        except AssertionError:
            return True
    return False


def test_native_records_equal_the_restatement(native, hand, detector):
    _, model = detector
    events = hand[0]
    start = cases.special_starts(events)
    want = restated(hand, model, start)
    got = native("fit", native_cases(hand, model, start), _abi.FIT_DTYPE).reshape(want.shape)
    ref.assert_same_records(got, want)
    e = list(events).index("eight")
    assert want["status"][e, 0] == _abi.FIT_NO_START and np.isnan(want["f"][e, 0]) and want["n_points"][e, 0] == 3
    assert want["n_inside"][e, 4] < want["n_points"][e, 4] and want["evaluations"][e, 4] >= 2
    assert want["status"][e, 7] & _abi.FIT_SINGULAR and want["evaluations"][e, 7] == 1
    # from the estimates
    want = restated(hand, model, None)
    got = native("fit", native_cases(hand, model, None), _abi.FIT_DTYPE).reshape(want.shape)
    ref.assert_same_records(got, want)
    assert (want["evaluations"] >= 2).sum() >= 6 and want["status"][list(events).index("collinear"), 5] == _abi.FIT_NO_START
    # a label given twice and a position without a species: the second layout
    twice = ref.Model(Inputs("be10dp").det, cases.layout(cases.INDICES_TWICE, without=(4,)))
    offsets, rows, labels = hand[1]
    estimates = est.records(offsets, rows, labels, cases.INDICES_TWICE, PARAMS)
    records = ref.records(offsets, rows, labels, cases.INDICES_TWICE, twice, estimates, SETTINGS, cases.BEAM_REGION)
    assert records["status"][e, 3] == _abi.FIT_EMPTY and records["status"][e, 7] == _abi.FIT_NO_START and records["n_points"][e, 7] == 129


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_mutants_fail(native, hand, detector, mutant):
    _, model = detector
    failed = []
    if mutant in ("b_sign", "no_dedx"):
        worst, _ = oracle_difference(detector, mutant)
        failed += ["oracle"] if worst > 1e-9 else []
    if recovery_failures(hand, model, mutant)[0]:
        failed.append("recovery")
    if native_mismatch(native, hand, model, mutant):
        failed.append("native")
    assert failed, mutant
    if mutant in ("b_sign", "no_dedx"):
        assert "oracle" in failed and "native" in failed


# ---------------------------------------------------------------- the same C++ under the sanitizers, a program of its own ----
def test_the_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path, hand, detector):
    _, model = detector
    exe = tmp_path / "fit_check_san"
    subprocess.run(COMPILE + ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", str(exe),
                              str(SOURCE)], check=True)
    run = lambda mode, blob, dtype: _run(exe, tmp_path, mode, blob, dtype)  # noqa: E731
    assert not native_mismatch(run, hand, model)
    ke = _energies()
    table = model.species[0].table
    assert run("dedx", table.tobytes() + ke.tobytes(), np.float64).tobytes() == dedx_reference.lookup(table, ke).tobytes()
