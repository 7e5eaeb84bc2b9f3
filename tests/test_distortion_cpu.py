"""The drift distortion without a GPU (include/attpc_engine.h, "drift distortion"): csrc/distort_host.hpp, compiled
alone for the host, equals tests/distortion_reference.py bit for bit and runs clean under the sanitizers; the mutants of
the restatement fail that comparison; the closed form of ``linear_radial_field``; the fixed-point inverse on Spyral
rows; the checks of a map; and the way ``distortion=`` reaches the library from every run function."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector import distortion as dmod
from attpc_engine_amd.detector.distortion import DistortionMap, configure_distortion
from tests import distortion_cases as dc
from tests import distortion_reference as dref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ("attpc_det_configure_distortion", "attpc_samples_distort"):
        assert re.search(rf"ATTPC_API int32_t {name}\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS and name in _abi.DISTORT_SYMBOLS
    assert "distortion" in _abi.CONFIGURE_SLOTS
    fields = re.search(r"typedef struct attpc_distort_desc \{([^}]*)\} attpc_distort_desc;", header).group(1)
    names = [n for line in re.findall(r"^\s*(?:double|int32_t|const double\*) ([\w, ]+);", fields, re.M) for n in line.split(", ")]
    assert names == [name for name, _ in _abi.DistortDesc._fields_]
    assert C.sizeof(_abi.DistortDesc) == 56 and _abi.DistortDesc.radial.offset == 32
    shared = (CSRC / "distort_host.hpp").read_text()
    assert "fp contract(off)" in shared
    for name, value in (("DISTORT_MAX_NODES", dmod.MAX_NODES), ("DISTORT_MAX_SHIFT", dmod.MAX_SHIFT), ("DISTORT_MAX_TIME", dmod.MAX_TIME)):
        assert float(re.search(rf"{name} = ([0-9.]+);", shared).group(1)) == value


# ------------------------------------------------------------------------------------------ bit for bit on the host ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "distort_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _map_words(m: dref.Map, n_rho=None, n_tau=None, tables=True) -> np.ndarray:
    shape = m.shape
    given = [t for t in (m.radial, m.azimuthal, m.time)] if tables else [None] * 3
    head = [m.rho_step, m.tau_step, m.tb_origin, shape[0] if n_rho is None else n_rho, shape[1] if n_tau is None else n_tau,
            *(0.0 if t is None else 1.0 for t in given)]
    return np.concatenate([np.array(head, dtype=np.float64), *(np.ravel(t) for t in given if t is not None)])


def _run(exe: Path, tmp: Path, mode: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _native_shift(exe, tmp, m: dref.Map, records: np.ndarray) -> np.ndarray:
    return _run(exe, tmp, "shift", np.concatenate([_map_words(m), records.ravel()])).reshape(-1, 4)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("distort")
    exe = tmp / "distort_check"
    _build(exe, ["-O2"])
    return exe, tmp


@pytest.fixture(scope="module")
def records():
    return dc.random_records(), dc.edge_records()


def test_edge_set_holds_the_edges(records):
    _, edge = records
    m = dc.reference_map()
    with np.errstate(all="ignore"):
        rho = np.sqrt(edge[:, 0] ** 2 + edge[:, 1] ** 2)
        a, b = rho / m.rho_step, (edge[:, 2] - m.tb_origin) / m.tau_step
    assert (rho == 0.0).sum() >= 12 and np.signbit(edge[rho == 0.0, 0]).any() and np.signbit(edge[rho == 0.0, 1]).any()
    assert ((a == np.floor(a)) & (a > 0) & (a < dc.N_RHO - 1)).sum() >= 10 and (a == dc.N_RHO - 1).any()
    assert (a > dc.N_RHO - 1).sum() >= 40 and (b < 0).sum() >= 40 and (b > dc.N_D - 1).sum() >= 40
    assert ((b == np.floor(b)) & (b >= 0) & (b <= dc.N_D - 1)).sum() >= 5
    assert np.isnan(edge[:, :3]).any(axis=1).sum() == 3 and np.isinf(edge[:, :3]).any(axis=1).sum() == 3
    assert np.isnan(edge[:, 3]).sum() == 2


def test_host_shift_equals_the_reference_bit_for_bit(native, records):
    exe, tmp = native
    m = dc.reference_map()
    for what, data in zip(("random", "edges"), records):
        want = dref.shift_records(m, data)
        got = _native_shift(exe, tmp, m, data)
        assert dref.same_bits(got, want), (what, np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[:10])
        assert dref.same_bits(got[:, 3], data[:, 3])  # q' = q
        moved = (got[:, :3].view(np.uint64) != data[:, :3].view(np.uint64)).any(axis=1)
        assert moved.sum() > 0.9 * len(data) if what == "random" else moved.sum() > 100
    random, edge = records
    shifted = dref.shift_records(m, random)
    plane = np.hypot(shifted[:, 0] - random[:, 0], shifted[:, 1] - random[:, 1]).max()
    late = np.abs(shifted[:, 2] - random[:, 2]).max()
    print(f"M on 20 000 records inside rho < 0.28 m: largest shift {plane * 1e3:.2f} mm, {late:.2f} time buckets")
    assert 0.015 < plane < 0.0224 and 3.0 < late < 4.0
    # a record that is not finite keeps its bits; the tables a map leaves out are zeros
    bad = ~np.isfinite(edge[:, :3]).all(axis=1)
    assert dref.same_bits(dref.shift_records(m, edge)[bad], edge[bad])
    for keep in range(3):
        tables = [t if k == keep else None for k, t in enumerate((m.radial, m.azimuthal, m.time))]
        part = dref.Map(m.rho_step, m.tau_step, m.tb_origin, *tables)
        zeros = dref.Map(m.rho_step, m.tau_step, m.tb_origin, *(np.zeros(m.shape) if t is None else t for t in tables))
        got = _native_shift(exe, tmp, part, edge)
        assert dref.same_bits(got, dref.shift_records(part, edge)) and dref.same_bits(got, dref.shift_records(zeros, edge))


def test_sanitized_build_runs_clean(tmp_path, records):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    exe = tmp_path / "distort_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    m = dc.reference_map()
    for data in (records[0][:2000], records[1]):
        assert dref.same_bits(_native_shift(exe, tmp_path, m, data), dref.shift_records(m, data))
    for _, words in _desc_cases(m):
        _run(exe, tmp_path, "desc", words)


@pytest.mark.parametrize("mutant", dref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(native, records, mutant):
    exe, tmp = native
    m = dc.reference_map()
    data = np.concatenate(records)
    got = _native_shift(exe, tmp, m, data)
    assert dref.same_bits(got, dref.shift_records(m, data))
    wrong = dref.shift_records(m, data, mutant)
    differ = (got.view(np.uint64) != wrong.view(np.uint64)).any(axis=1)
    print(mutant, "records that differ:", int(differ.sum()))
    assert differ.any(), mutant


# ------------------------------------------------------------------------------------------ the checks of a desc ----
def _desc_cases(m: dref.Map):
    """(what, the native check's input words) of every bad desc of tests/distortion_cases.py."""
    out = []
    for what, value in dc.bad_descs():
        bad = dref.Map(m.rho_step, m.tau_step, m.tb_origin, m.radial.copy(), m.azimuthal.copy(), m.time.copy())
        if what in ("rho_step", "tau_step", "tb_origin"):
            setattr(bad, what, value)
            out.append(((what, value), _map_words(bad)))
        elif what in ("n_rho", "n_tau"):
            out.append(((what, value), _map_words(bad, **{what: value}, tables=False)))
        else:
            getattr(bad, what)[5, 7] = value
            out.append(((what, value), _map_words(bad)))
    return out


def test_host_desc_checks(native):
    exe, tmp = native
    m = dc.reference_map()
    assert _run(exe, tmp, "desc", _map_words(m)).tolist() == [0.0, 0.0]
    assert _run(exe, tmp, "desc", _map_words(m, tables=False)).tolist() == [0.0, 1.0]  # every table NULL: off
    zeros = dref.Map(m.rho_step, m.tau_step, m.tb_origin, np.zeros(m.shape), None, np.zeros(m.shape))
    assert _run(exe, tmp, "desc", _map_words(zeros)).tolist() == [0.0, 1.0]          # every value zero: off
    edge = dref.Map(m.rho_step, m.tau_step, m.tb_origin, np.full((2, 2), 1.0), np.full((2, 2), -1.0), np.full((2, 2), -1024.0))
    assert _run(exe, tmp, "desc", _map_words(edge)).tolist() == [0.0, 0.0]           # the caps themselves are allowed
    big = dref.Map(m.rho_step, m.tau_step, m.tb_origin, None, None, np.full((256, 256), 0.5))
    assert _run(exe, tmp, "desc", _map_words(big)).tolist() == [0.0, 0.0]
    for what, words in _desc_cases(m):
        assert _run(exe, tmp, "desc", words).tolist() == [1.0, 0.0], what


def test_every_bad_map_is_a_value_error():
    m = dc.named_map()
    tables = {"radial": m.radial, "azimuthal": m.azimuthal, "time": m.time}
    for what, value in dc.bad_descs():
        if what in tables:
            bad = {k: v.copy() for k, v in tables.items()}
            bad[what][5, 7] = value
            with pytest.raises(ValueError):
                DistortionMap(**bad)
        elif what in ("n_rho", "n_tau"):
            shape = (max(value, 0), 3) if what == "n_rho" else (3, max(value, 0))
            with pytest.raises(ValueError):
                DistortionMap(np.zeros(shape))
            with pytest.raises(ValueError):
                DistortionMap.from_function(lambda r, d: (r * d, r * d, r * d), **{"n_rho" if what == "n_rho" else "n_d": value})
    for kw in ({"rho_max": 0.0}, {"rho_max": float("nan")}, {"rho_max": float("inf")}, {"length": 0.0}, {"length": -1.0},
               {"length": float("nan")}, {"rho_max": "1"}):
        with pytest.raises(ValueError):
            DistortionMap(m.radial, **kw)
    for args in ((), (np.zeros(5),), (np.zeros((3, 3)), np.zeros((3, 4))), (np.zeros((3, 3, 3)),), ([["a", "b"], ["c", "d"]],)):
        with pytest.raises(ValueError):
            DistortionMap(*args)
    with pytest.raises(ValueError):
        DistortionMap.linear_radial_field(float("nan"), 2.0)
    with pytest.raises(ValueError):
        m.steps(dc.drift(micromegas_edge=560, windows_edge=560))  # no drift: tau_step would be 0
    with pytest.raises(ValueError):
        m.undistort_rows(np.zeros((4, 8)), dc.drift(), iterations=-1)
    with pytest.raises(TypeError):
        configure_distortion(None, "a map")
    assert DistortionMap(np.zeros((3, 3))).on is False and m.on is True


def test_desc_of_two_configs():
    m = dc.named_map()
    for config, want in ((dc.drift(), (0.292 / 32, 550.0 / 40, 10.0)),
                         (dc.drift(length=1.0, micromegas_edge=60, windows_edge=396), (0.292 / 32, 336.0 / 40, 60.0))):
        desc = m.desc(config)
        assert (desc.rho_step, desc.tau_step, desc.tb_origin, desc.n_rho, desc.n_tau) == (*want, 33, 41)
        assert m.steps(config) == want
        ref = dc.reference_map(m, config)
        assert (ref.rho_step, ref.tau_step, ref.tb_origin) == want
        np.testing.assert_array_equal(np.ctypeslib.as_array(desc.radial, (33, 41)), m.radial)
        np.testing.assert_array_equal(np.ctypeslib.as_array(desc.time, (33, 41)), m.time)
    # a map without a length of its own takes the config's: its last node is the window, whatever the length
    free = DistortionMap(m.radial, m.azimuthal, m.time)
    assert free.steps(dc.drift(length=0.5, micromegas_edge=60, windows_edge=396)) == (0.292 / 32, 336.0 / 40, 60.0)
    # a map made for 1 m in a chamber of 0.5 m: its nodes keep their distances, twice the chamber's drift
    assert m.steps(dc.drift(length=0.5, micromegas_edge=60, windows_edge=396)) == (0.292 / 32, 336.0 * 2.0 / 40, 60.0)
    assert m.token(dc.drift()) != m.token(dc.drift(micromegas_edge=60)) and DistortionMap(np.zeros((2, 2))).token(dc.drift()) is None


# ------------------------------------------------------------------------------------------ the physics' closed form ----
def test_linear_radial_field_is_reproduced_by_the_interpolation(records):
    """dr = eps_max (rho / rho_max) d / (1 + (omega tau)^2) is bilinear in (rho, d): the interpolation of its node
    values gives it back to rounding (measured in numpy: 4e-18 m)."""
    field = DistortionMap.linear_radial_field(0.05, 2.0, dc.N_RHO, dc.N_D, dc.RHO_MAX, dc.LENGTH)
    assert not field.time.any() and np.array_equal(field.azimuthal, 2.0 * field.radial)
    data = records[0]
    m = dc.reference_map(field)
    radial_only = dref.Map(m.rho_step, m.tau_step, m.tb_origin, field.radial, None, None)
    shifted = dref.shift_records(radial_only, data)
    rho = np.hypot(data[:, 0], data[:, 1])
    dr = np.hypot(shifted[:, 0], shifted[:, 1]) - rho
    d = (data[:, 2] - dc.MM_EDGE) / (dc.WIN_EDGE - dc.MM_EDGE) * dc.LENGTH
    closed = 0.05 * rho / dc.RHO_MAX * d / (1.0 + 4.0)
    # (|x'| - |x| carries the rounding of two hypots of 0.28 m, 1e-16 m; the table value itself is compared below)
    i, fr = dmod._cell(rho / m.rho_step, dc.N_RHO)
    j, fs = dmod._cell((data[:, 2] - m.tb_origin) / m.tau_step, dc.N_D)
    table_value = dmod._bilinear(field.radial, i, j, fr, fs)
    print("largest |dr - closed form|:", np.abs(table_value - closed).max(), "m; through the shifted points:", np.abs(dr - closed).max())
    assert np.abs(table_value - closed).max() < 1e-15
    assert np.abs(dr - closed).max() < 1e-15
    # the package's forward map is the restatement's
    got = dc.named_map().shift(data[:, 0], data[:, 1], data[:, 2], dc.drift())
    want = dref.shift_records(dc.reference_map(), data)
    for k in range(3):
        assert dref.same_bits(got[k], want[:, k])


# ------------------------------------------------------------------------------------------ the inverse ----
def _rows_of(points, config):
    """Spyral rows [P, 8] of (x m, y m, tb): x, y in mm, z through the writer's relation, the other columns marked."""
    mm, win = config.elec_params.micromegas_edge, config.elec_params.windows_edge
    rows = np.empty((len(points), 8))
    rows[:, 0], rows[:, 1] = points[:, 0] * 1000.0, points[:, 1] * 1000.0
    rows[:, 2] = (win - points[:, 2]) / (win - mm) * config.det_params.length * 1000.0  # writer.py:103-105
    rows[:, 3:] = np.arange(5.0) + 100.0
    return rows


def _points_of(rows, config):
    mm, win = config.elec_params.micromegas_edge, config.elec_params.windows_edge
    tb = win - rows[:, 2] / (config.det_params.length * 1000.0) * (win - mm)
    return np.stack([rows[:, 0] / 1000.0, rows[:, 1] / 1000.0, tb], axis=1)


def test_undistort_rows_inverts_the_map(records):
    config, m, ref = dc.drift(), dc.named_map(), dc.reference_map()
    truth = records[0]
    seen = dref.shift_records(ref, truth)
    rows = _rows_of(seen, config)
    observed = _points_of(rows, config)
    worst = []
    for k in range(9):
        estimate = _points_of(m.undistort_rows(rows, config, iterations=k), config)
        forward = dref.shift_records(ref, np.column_stack([estimate, truth[:, 3]]))[:, :3]
        gap = np.abs(forward - observed)
        worst.append((gap[:, :2].max(), gap[:, 2].max()))
    print("discrepancy per iteration (m, time buckets):", worst)
    for (xy0, tb0), (xy1, tb1) in zip(worst[:-1], worst[1:]):
        assert xy1 * 5.0 <= xy0 and tb1 * 5.0 <= tb0, worst
    back = m.undistort_rows(rows, config)  # 12 iterations
    got = _points_of(back, config)
    err_xy, err_tb = np.abs(got[:, :2] - truth[:, :2]).max(), np.abs(got[:, 2] - truth[:, 2]).max()
    print(f"after 12 iterations: {err_xy:.3g} m, {err_tb:.3g} time buckets")
    assert err_xy <= 1e-12 and err_tb <= 1e-9
    np.testing.assert_array_equal(back[:, 3:], rows[:, 3:])
    assert back is not rows and np.array_equal(rows, _rows_of(seen, config))  # the input is left alone


# ------------------------------------------------------------------------------------------ plumbing ----
def _distortion_calls(lib):
    return [desc for name, desc in lib.configure_descs if name == "attpc_det_configure_distortion"]


def test_distortion_reaches_run_batch_from_every_run_function(tmp_path, monkeypatch):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.detector import simulator as sim
    from attpc_engine_amd.detector.maps import simulate_batch_maps
    from attpc_engine_amd.detector.selection import Selection, simulate_batch_selected
    from attpc_engine_amd.detector.summary import simulate_batch_summary
    from attpc_engine_amd.detector.traces import simulate_batch_trace_rows, simulate_batch_traces
    from attpc_engine_amd.engine import Engine, run_fused
    from tests.test_run_layer_cpu import PlainWriter, RecordingContext, _kinematics, _kinematics_file

    import sys
    import warnings
    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    workload = workloads.o16aa()
    pipeline, config, indices = workload
    m = dc.named_map()
    want = {"rho_step": 0.292 / 32, "tau_step": 550.0 / 40, "tb_origin": 10.0, "n_rho": 33, "n_tau": 41}
    momenta, vertices, z, a = _kinematics(workload, 4)
    args = (momenta, vertices, z, a, config, 3, indices)

    # every file-driven run function hands the keyword to run_batch, with the call's own config
    seen = []
    real = sim.run_batch

    def spy(call, *a_, **kw):
        seen.append((call, kw.get("distortion")))
        return real(call, *a_, **kw)

    monkeypatch.setattr(sim, "run_batch", spy)
    ctx = RecordingContext()
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    functions = {
        "attpc_det_run": lambda **kw: sim.simulate_batch(*args, ctx=ctx, **kw),
        "attpc_det_run_spyral": lambda **kw: sim.simulate_batch_spyral(*args, ctx=ctx, **kw),
        "attpc_det_run_traces": lambda **kw: simulate_batch_traces(*args, ctx=ctx, **kw),
        "attpc_det_run_trace_rows": lambda **kw: simulate_batch_trace_rows(*args, ctx=ctx, **kw),
    }
    for call, function in functions.items():
        seen.clear()
        ctx.lib.configure_descs.clear()
        function(distortion=m)
        assert seen == [(call, m)], (call, seen)
        function(distortion=m)      # the same map again: the token skips the upload
        function()                  # without the keyword: off for that call
        assert _distortion_calls(ctx.lib) == [want, None], (call, _distortion_calls(ctx.lib))
    seen.clear()
    ctx.lib.configure_descs.clear()
    sim.simulate(momenta[0], vertices[0], z, a, config, np.random.default_rng(1), indices, distortion=m)
    assert seen == [("attpc_det_run", m)] and _distortion_calls(ctx.lib) == [want]
    path = _kinematics_file(workload, tmp_path, 6)
    seen.clear()
    sim.run_simulation(config, path, PlainWriter(tmp_path), indices, batch_size=4, seed=5, distortion=m)
    assert seen == [("attpc_det_run", m)] * 2
    seen.clear()
    (tmp_path / "spyral").mkdir()
    sim.run_simulation(config, path, SpyralWriter(tmp_path / "spyral", config), indices, batch_size=4, seed=5, distortion=m)
    assert seen == [("attpc_det_run_spyral", m)] * 2
    sim.run_simulation(config, path, PlainWriter(tmp_path), indices, batch_size=4, seed=5)
    assert seen[-1] == ("attpc_det_run", None) and _distortion_calls(ctx.lib)[-1] is None
    monkeypatch.setattr(sim, "run_batch", real)

    # the summary, selected and maps forms configure the same stage
    for function, extra in ((simulate_batch_summary, {}), (simulate_batch_selected, {"selection": Selection(n_kept=(1, None))}),
                            (simulate_batch_maps, {})):
        fresh = RecordingContext()
        try:
            function(*args, ctx=fresh, distortion=m, **extra)
        except Exception:  # (the stand-in library fills none of these modes' outputs; the configure calls come first)
            pass
        assert _distortion_calls(fresh.lib) == [want], function.__name__

    # the engine: configure_distortion with a map or its keywords, off with neither; run_fused hands it on
    fresh = RecordingContext()
    engine = Engine(pipeline, config, indices, context=fresh)
    assert _distortion_calls(fresh.lib) == []
    engine.configure_distortion(m)
    engine.configure_distortion(radial=m.radial, azimuthal=m.azimuthal, time=m.time, length=1.0)
    engine.configure_distortion()
    assert _distortion_calls(fresh.lib) == [want, None]
    with pytest.raises(TypeError):
        engine.configure_distortion(m, radial=m.radial)
    Engine(pipeline, config, indices, context=fresh).configure_distortion(m)
    Engine(pipeline, config, indices, context=fresh)  # a new engine starts with the stage off
    assert _distortion_calls(fresh.lib) == [want, None, want, None]
    fused = RecordingContext()
    (tmp_path / "fused").mkdir()
    run_fused(pipeline, config, SpyralWriter(tmp_path / "fused", config), 6, indices, seed=8, batch_size=4, context=fused,
              distortion=m)
    assert _distortion_calls(fused.lib) == [want]
    names = fused.lib.names()
    assert names.index("det_configure_distortion") < names.index("sim_run_spyral")
