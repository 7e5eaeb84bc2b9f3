"""The drift correction without a GPU (include/attpc_engine.h, "drift correction"): csrc/undistort_host.hpp, compiled
alone for the host, equals tests/undistort_reference.py bit for bit on the case set and runs clean under the sanitizers;
the mutants of the restatement fail that comparison; the correction closes the loop of the forward map and agrees with
``DistortionMap.undistort_rows``; a steep map does not converge and says so; the checks of the settings; and the way
``correction=`` reaches the library."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector import correction as cmod
from attpc_engine_amd.detector.correction import CorrectionSettings, configure_correction, rows_to_correction
from attpc_engine_amd.detector.distortion import DistortionMap
from tests import distortion_cases as dc
from tests import distortion_reference as dref
from tests import undistort_cases as uc
from tests import undistort_reference as uref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ("attpc_trace_configure_correction", "attpc_correction_last", "attpc_rows_undistort"):
        assert re.search(rf"ATTPC_API int32_t {name}\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS and name in _abi.UNDISTORT_SYMBOLS
    assert "correction" in _abi.CONFIGURE_SLOTS
    fields = re.search(r"typedef struct attpc_undistort_desc \{([^}]*)\} attpc_undistort_desc;", header).group(1)
    names = re.findall(r"^\s*(?:double|int32_t|attpc_distort_desc) (\w+);", fields, re.M)
    assert names == [name for name, _ in _abi.UndistortDesc._fields_]
    assert C.sizeof(_abi.UndistortDesc) == 96 and _abi.UndistortDesc.tolerance_xy.offset == 80
    fields = re.search(r"typedef struct attpc_undistort_info \{([^}]*)\} attpc_undistort_info;", header).group(1)
    assert re.findall(r"^\s*int64_t (\w+);", fields, re.M) == list(uref.COUNTS) == list(cmod.COUNTS)
    assert [name for name, _ in _abi.UndistortInfo._fields_] == list(uref.COUNTS)
    shared = (CSRC / "undistort_host.hpp").read_text()
    assert "fp contract(off)" in shared and "fma" not in shared
    assert int(re.search(r"UNDISTORT_MAX_ITERATIONS = (\d+);", shared).group(1)) == cmod.MAX_ITERATIONS == 64
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"undistort.hip"' in entry and '"undistort_host.hpp"' in entry


# ------------------------------------------------------------------------------------------ bit for bit on the host ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "undistort_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _settings_words(s: uref.Settings, **changes) -> np.ndarray:
    m = s.map
    given = [m.radial, m.azimuthal, m.time]
    head = {"windows_edge": s.windows_edge, "micromegas_edge": s.micromegas_edge, "length": s.length,
            "iterations": s.iterations, "tolerance_xy": s.tolerance_xy, "tolerance_tb": s.tolerance_tb}
    head.update(changes)
    words = [*head.values(), m.rho_step, m.tau_step, m.tb_origin, *m.shape, *(0.0 if t is None else 1.0 for t in given)]
    return np.concatenate([np.array(words, dtype=np.float64), *(np.ravel(t) for t in given if t is not None)])


def _run(exe: Path, tmp: Path, mode: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _native(exe, tmp, s: uref.Settings, offsets, rows, labels):
    """The stand-alone program on a CSR array -> (rows, labels, order, counts) as the restatement gives them."""
    body = np.concatenate([rows, labels.astype(np.float64)[:, None]], axis=1).ravel()
    out = _run(exe, tmp, "rows", np.concatenate([_settings_words(s), [len(offsets) - 1], offsets.astype(np.float64), body]))
    table = out[:-4].reshape(-1, 10)
    info = dict(zip(uref.COUNTS, (int(v) for v in out[-4:])))
    return np.ascontiguousarray(table[:, :8]), table[:, 8].astype(np.int64), table[:, 9].astype(np.int64), info


def _same(got, want) -> bool:
    return (dref.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            and got[3] == want[3])


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("undistort")
    exe = tmp / "undistort_check"
    _build(exe, ["-O2"])
    return exe, tmp


@pytest.fixture(scope="module")
def cases():
    offsets, rows, labels, names = uc.stage_cases()
    return offsets, rows, labels, names, uref.undistort(uc.settings(), offsets, rows, labels)


def test_case_set_holds_what_it_names(cases):
    offsets, rows, labels, names, (out, out_labels, order, info) = cases
    sizes = dict(zip(names, np.diff(offsets)))
    assert [n for n in names[::2]][:7] == [f"{n} rows" for n in uc.SIZES] and set(names[1::2]) == {"empty"}
    assert info["n_rows"] == len(rows) and info["n_unconverged"] == 0
    # skipped: the 6 non-finite edge records; 13 rows made non-finite, and 3 whose NaN payload fell in column 6; 5 all-NaN rows
    assert info["n_skipped"] == 6 + 13 + 3 + 5 and info["n_moved"] > 1000
    t_of = {}
    for e, name in enumerate(names):
        lo, hi = offsets[e], offsets[e + 1]
        ev = out[lo:hi]
        good = np.isfinite(ev[:, 0]) & np.isfinite(ev[:, 1]) & np.isfinite(ev[:, 6])
        # corrected rows first, in ascending z; the skipped ones behind them, in input order
        assert not good[int(good.sum()):].any(), name
        z = ev[good, 2]
        assert np.all(np.diff(z) >= 0.0), name
        assert np.all(np.diff(order[lo:hi][~good]) > 0), name
        t_of[name] = dc.WIN_EDGE - z / 1000.0 / dc.LENGTH * (dc.WIN_EDGE - dc.MM_EDGE)
        assert sorted(order[lo:hi]) == list(range(lo, hi)), name
    assert sizes["one t"] == 130 and np.array_equal(order[offsets[names.index("one t")]:][:130] - offsets[names.index("one t")], np.arange(130))
    assert t_of["all below 0"].max() < 0.0 and t_of["all above 511"].min() > 511.0
    assert t_of["across 0 and 512"].min() < 0.0 and t_of["across 0 and 512"].max() > 512.0
    np.testing.assert_array_equal(out_labels, labels[order])
    assert dref.same_bits(out[:, 3:], rows[order][:, 3:])  # columns 3 .. 7 keep their bits, NaN payloads included
    assert np.isnan(rows[:, 3:]).sum() >= 12 + 25  # (12 of the 18 payloads are NaNs, the others infinities)


def test_host_rows_equal_the_reference_bit_for_bit(native, cases):
    exe, tmp = native
    offsets, rows, labels, _, want = cases
    got = _native(exe, tmp, uc.settings(), offsets, rows, labels)
    assert got[3] == want[3], (got[3], want[3])
    assert _same(got, want), np.flatnonzero((got[0].view(np.uint64) != want[0].view(np.uint64)).any(axis=1))[:10]
    for changes in ({"iterations": 1}, {"iterations": 64}, {"iterations": 3, "tolerance_xy": 0.0, "tolerance_tb": 0.0}):
        s = uc.settings(**changes)
        assert _same(_native(exe, tmp, s, offsets, rows, labels), uref.undistort(s, offsets, rows, labels)), changes
    few = uref.undistort(uc.settings(iterations=3, tolerance_xy=0.0, tolerance_tb=0.0), offsets, rows, labels)[3]
    assert few["n_unconverged"] > 1000  # (three steps leave 1e-6 m: above a zero tolerance)
    # the tables a map leaves out are zeros
    m = dc.reference_map()
    part = dref.Map(m.rho_step, m.tau_step, m.tb_origin, None, m.azimuthal, None)
    assert _same(_native(exe, tmp, uc.settings(part), offsets, rows, labels), uref.undistort(uc.settings(part), offsets, rows, labels))


def test_sanitized_build_runs_clean(tmp_path, cases):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    exe = tmp_path / "undistort_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    offsets, rows, labels, _, want = cases
    assert _same(_native(exe, tmp_path, uc.settings(), offsets, rows, labels), want)
    for field, value in uc.bad_settings():
        assert _run(exe, tmp_path, "desc", _settings_words(uc.settings(), **{field: value})).tolist() == [1.0], (field, value)


@pytest.mark.parametrize("mutant", uref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(native, cases, mutant):
    exe, tmp = native
    offsets, rows, labels, _, want = cases
    got = _native(exe, tmp, uc.settings(), offsets, rows, labels)
    assert _same(got, want)
    wrong = uref.undistort(uc.settings(), offsets, rows, labels, mutant)
    differ = (got[0].view(np.uint64) != wrong[0].view(np.uint64)).any(axis=1) | (got[2] != wrong[2])
    print(mutant, "rows that differ:", int(differ.sum()), "counts", wrong[3])
    assert differ.any(), mutant


def test_host_desc_checks(native):
    exe, tmp = native
    s = uc.settings()
    assert _run(exe, tmp, "desc", _settings_words(s)).tolist() == [0.0]
    assert _run(exe, tmp, "desc", _settings_words(s, iterations=1, tolerance_xy=0.0, tolerance_tb=0.0)).tolist() == [0.0]
    assert _run(exe, tmp, "desc", _settings_words(s, iterations=64, windows_edge=dc.MM_EDGE + 1)).tolist() == [0.0]
    for field, value in uc.bad_settings():
        assert _run(exe, tmp, "desc", _settings_words(s, **{field: value})).tolist() == [1.0], (field, value)
    bad_map = dref.Map(0.0, s.map.tau_step, s.map.tb_origin, s.map.radial, None, None)  # the map's own rules hold too
    assert _run(exe, tmp, "desc", _settings_words(uc.settings(bad_map))).tolist() == [1.0]


# ------------------------------------------------------------------------------------------ what the stage is for ----
def test_correction_closes_the_loop_of_the_forward_map():
    """Points uniform in rho < 0.28 m and tb in 10 .. 560, moved by M and corrected with M at 12 iterations, come back
    to within 1e-9 m and 1e-6 time buckets (measured in numpy on 2e5 points: 1.3e-15 m, 4.5e-13 tb; last step 1.6e-14 m
    and 3.1e-12 tb, so nothing is unconverged at the default tolerances)."""
    truth = dc.random_records(20000, seed=5)
    seen = dref.shift_records(dc.reference_map(), truth)
    s = uc.settings()
    x, y, t, (dx, dy, dt) = uref.correct_points(s, seen[:, 0], seen[:, 1], seen[:, 2])
    err_xy = max(np.abs(x - truth[:, 0]).max(), np.abs(y - truth[:, 1]).max())
    err_tb = np.abs(t - truth[:, 2]).max()
    step_xy, step_tb = max(np.abs(dx).max(), np.abs(dy).max()), np.abs(dt).max()
    print(f"closure: {err_xy:.3g} m, {err_tb:.3g} tb; last step {step_xy:.3g} m, {step_tb:.3g} tb")
    assert err_xy <= 1e-9 and err_tb <= 1e-6
    rows = uc.rows_of(seen[:, :3])
    offsets = np.array([0, 7000, 7000, len(rows)], dtype=np.int64)
    out, _, order, info = uref.undistort(s, offsets, rows, np.zeros(len(rows), dtype=np.int64))
    assert info["n_unconverged"] == 0 and info["n_skipped"] == 0 and info["n_rows"] == len(rows)
    assert np.abs(out[:, :2] / 1000.0 - truth[order, :2]).max() <= 1e-9
    want_z = (dc.WIN_EDGE - truth[order, 2]) / (dc.WIN_EDGE - dc.MM_EDGE) * dc.LENGTH * 1000.0
    assert np.abs(out[:, 2] - want_z).max() <= 1e-6 * 1000.0 * dc.LENGTH / (dc.WIN_EDGE - dc.MM_EDGE) + 1e-9


def test_rows_sorted_by_apparent_time_need_the_resort():
    """3 000 random rows in descending apparent time: after the correction a third of the adjacent pairs are inverted
    (the issue's count: 1 112 of 2 999), and the stage's output has none."""
    rows = uc.rows_of(uc.apparent_points(3000, 1))
    offsets = np.array([0, 3000], dtype=np.int64)
    labels = np.zeros(3000, dtype=np.int64)
    unsorted = uref.undistort(uc.settings(), offsets, rows, labels, "no_resort")[0]
    inverted = int((np.diff(unsorted[:, 2]) < 0.0).sum())
    out, _, _, info = uref.undistort(uc.settings(), offsets, rows, labels)
    print("inverted adjacent pairs without the re-sort:", inverted, "of 2999; rows moved:", info["n_moved"])
    assert inverted > 500 and not (np.diff(out[:, 2]) < 0.0).any() and info["n_moved"] > 1000


def test_agreement_with_undistort_rows():
    """``DistortionMap.undistort_rows`` takes the time from z, the stage from column 6: x, y and z agree to 1e-6 mm."""
    rows = uc.rows_of(uc.apparent_points(5000, 2))
    offsets = np.array([0, 5000], dtype=np.int64)
    out, _, order, _ = uref.undistort(uc.settings(), offsets, rows, np.zeros(5000, dtype=np.int64))
    host = dc.named_map().undistort_rows(rows, dc.drift(), iterations=12)[order]
    gap = np.abs(out[:, :3] - host[:, :3]).max()
    print("largest |stage - undistort_rows| over x, y, z:", gap, "mm")
    assert gap <= 1e-6
    assert dref.same_bits(out[:, 3:], host[:, 3:])


def test_a_steep_map_diverges_and_says_so(native):
    exe, tmp = native
    s = uc.settings(uc.steep_map())
    rows = uc.rows_of(uc.apparent_points(500, 3, rho_limit=0.25))
    offsets = np.array([0, 500], dtype=np.int64)
    labels = np.arange(500, dtype=np.int64)
    want = uref.undistort(s, offsets, rows, labels)
    assert np.isfinite(want[0]).all() and want[3]["n_unconverged"] > 400 and want[3]["n_skipped"] == 0
    assert _same(_native(exe, tmp, s, offsets, rows, labels), want)


def test_a_map_without_a_time_table_moves_no_row(native):
    exe, tmp = native
    m = dc.reference_map()
    flat = dref.Map(m.rho_step, m.tau_step, m.tb_origin, m.radial, m.azimuthal, np.zeros(m.shape))
    rows = uc.rows_of(uc.apparent_points(700, 4))
    offsets = np.array([0, 300, 700], dtype=np.int64)
    labels = np.arange(700, dtype=np.int64)
    want = uref.undistort(uc.settings(flat), offsets, rows, labels)
    assert want[3]["n_moved"] == 0 and np.array_equal(want[2], np.arange(700))
    assert dref.same_bits(want[0][:, 2], rows[:, 2])  # z comes back bit for bit: the rows' own expression
    assert not dref.same_bits(want[0][:, :2], rows[:, :2])
    assert _same(_native(exe, tmp, uc.settings(flat), offsets, rows, labels), want)


# ------------------------------------------------------------------------------------------ the Python layer ----
def test_argument_checks():
    m = dc.named_map()
    for bad in (0, 65, True, False, 12.0, "12", None, -1):
        with pytest.raises(ValueError):
            CorrectionSettings(m, iterations=bad)
    for field in ("tolerance_xy", "tolerance_tb"):
        for bad in (float("nan"), float("inf"), -1e-9, "1", True, None):
            with pytest.raises(ValueError):
                CorrectionSettings(m, **{field: bad})
    for bad in ("a map", None, m.radial, dc.reference_map()):
        with pytest.raises(TypeError):
            CorrectionSettings(bad)
    good = CorrectionSettings(m)
    assert (good.iterations, good.tolerance_xy, good.tolerance_tb) == (12, 1e-6, 1e-3) and good.on
    assert CorrectionSettings(m, iterations=1, tolerance_xy=0, tolerance_tb=0).iterations == 1
    assert CorrectionSettings(m, iterations=np.int64(64)).iterations == 64
    with pytest.raises(ValueError):
        good.token(None)  # a missing config
    with pytest.raises(ValueError):
        good.desc(None)
    with pytest.raises(ValueError):
        good.desc(dc.drift(micromegas_edge=560, windows_edge=560))
    with pytest.raises(TypeError):
        configure_correction(None, "settings", dc.drift())
    with pytest.raises(TypeError):
        rows_to_correction([0], np.zeros((0, 8)), [], m, dc.drift())
    with pytest.raises(ValueError):
        rows_to_correction([0, 1], np.zeros((1, 8)), [0], good, None)
    off = CorrectionSettings(DistortionMap(np.zeros((3, 3))))
    assert off.on is False and off.token(dc.drift()) is None
    desc = good.desc(dc.drift())
    assert (desc.windows_edge, desc.micromegas_edge, desc.length, desc.iterations) == (560, 10, 1.0, 12)
    assert (desc.tolerance_xy, desc.tolerance_tb, desc.map.n_rho, desc.map.n_tau, desc.map.tb_origin) == (1e-6, 1e-3, 33, 41, 10.0)
    assert good.token(dc.drift()) != good.token(dc.drift(length=0.5)) != CorrectionSettings(m, iterations=11).token(dc.drift(length=0.5))


def _correction_calls(lib):
    return [desc for name, desc in lib.configure_descs if name == "attpc_trace_configure_correction"]


def test_correction_reaches_the_library(tmp_path, monkeypatch):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.detector.simulator import plan_delivery
    from attpc_engine_amd.detector.traces import PeakSettings, TraceChain, configure_trace_rows
    from attpc_engine_amd.detector.thinning import ThinSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings
    from attpc_engine_amd.engine import Engine
    from tests.test_run_layer_cpu import PlainWriter, RecordingContext

    pipeline, config, indices = workloads.o16aa()
    good = CorrectionSettings(dc.named_map(), iterations=7)
    with pytest.raises(TypeError):
        TraceChain(config, correction="settings")
    with pytest.raises(TypeError):
        TraceChain(config).replace(correction=dc.named_map())
    chain = TraceChain(config, estimates=EstimateSettings(), thinning=ThinSettings(10.0), correction=good)
    ctx = RecordingContext()
    chain.configure(ctx, rows=True)
    calls = _correction_calls(ctx.lib)
    assert len(calls) == 1 and calls[0]["iterations"] == 7 and calls[0]["windows_edge"] == config.elec_params.windows_edge
    names = ctx.lib.names()
    assert names.index("trace_configure_correction") < names.index("trace_configure_thinning")
    chain.configure(ctx, rows=True)                           # the same settings again: the token skips the call
    chain.replace(correction=None).configure(ctx, rows=True)  # off
    assert [c if c is None else c["iterations"] for c in _correction_calls(ctx.lib)] == [7, None]
    fresh = RecordingContext()
    TraceChain(config, correction=good).configure(fresh)      # traces, not rows: the stage is not touched
    assert _correction_calls(fresh.lib) == []
    configure_trace_rows(config, fresh, correction=good)
    configure_trace_rows(config, fresh)                       # None leaves what the ctx holds
    assert len(_correction_calls(fresh.lib)) == 1
    engine = Engine(pipeline, config, indices, context=fresh)
    engine.configure_correction()
    engine.configure_correction(map=dc.named_map(), iterations=3)
    engine.configure_correction(good)
    assert [c if c is None else c["iterations"] for c in _correction_calls(fresh.lib)] == [7, None, 3, 7]
    with pytest.raises(TypeError):
        engine.configure_correction(good, iterations=3)
    # the writers: only trace rows take it
    writer = SpyralWriter(tmp_path, config, peaks=PeakSettings(), correction=good)
    assert writer.chain.correction is good and plan_delivery(writer, config)[2].correction is good
    other = CorrectionSettings(dc.named_map(), iterations=5)
    assert plan_delivery(writer, config, correction=other)[2].correction is other
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, correction=good)
    with pytest.raises(ValueError):
        plan_delivery(SpyralWriter(tmp_path, config), config, correction=good)
    with pytest.raises(ValueError):
        plan_delivery(PlainWriter(tmp_path), config, correction=good)
