"""The particle identification without a GPU (include/attpc_engine.h, "particle identification"): the contract's names
everywhere; the case set holds what it names; the restatement (tests/pid_reference.py) and its mutants, each of which
the exact comparison catches; csrc/pid_host.hpp, compiled alone for the host, plain and under the sanitizers (a
stand-alone program with its own main), equal to the restatement exactly; the checks of the gates; ``Gate.from_band``;
``by_position``; the argument checks of the Python layer."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd import detector
from attpc_engine_amd.detector import pid as pmod
from attpc_engine_amd.detector.pid import Gate, PidSettings, by_position
from tests import pid_cases as pc
from tests import pid_reference as pref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"
ENTRY_POINTS = ("attpc_trace_configure_pid", "attpc_pid_last", "attpc_estimates_pid", "attpc_rows_fit_pid")
NAN, INF = float("nan"), float("inf")


def _flat(text: str) -> str:
    return text.replace("\n * ", " ").replace("\n// ", " ").replace("\n", " ")


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.PID_SYMBOLS == ENTRY_POINTS and "pid" in _abi.CONFIGURE_SLOTS
    assert int(re.search(r"#define ATTPC_ABI_VERSION (\d+)", header).group(1)) == 3  # additions only
    for struct, cls in (("attpc_pid_desc", _abi.PidDesc), ("attpc_pid_record", _abi.PidRecord)):
        fields = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header).group(1)
        names = [n.strip() for line in re.findall(r"^\s*(?:double|int32_t) ([\w, \[\]]+);", fields, re.M)
                 for n in re.sub(r"\[\w+\]", "", line).split(",")]
        assert names == [name for name, _ in cls._fields_], (struct, names)
    assert (C.sizeof(_abi.PidDesc), C.sizeof(_abi.PidRecord)) == (4136, 16)
    assert _abi.PidDesc.vertices.offset == 40 and _abi.PID_DTYPE.descr == pref.PID_DTYPE.descr
    for name, value in (("ATTPC_PID_ANY", _abi.PID_ANY), ("ATTPC_PID_OWN", _abi.PID_OWN), ("ATTPC_PID_MAX_VERTICES", _abi.PID_MAX_VERTICES),
                        ("ATTPC_PID_NO_ESTIMATE", _abi.PID_NO_ESTIMATE), ("ATTPC_PID_NONE", _abi.PID_NONE),
                        ("ATTPC_PID_TAKEN", _abi.PID_TAKEN), ("ATTPC_PID_AMBIGUOUS", _abi.PID_AMBIGUOUS),
                        ("ATTPC_FIT_NO_PID", _abi.FIT_NO_PID)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert (pref.ANY, pref.OWN, pref.MAX_VERTICES, pref.FIT_NO_PID) == (_abi.PID_ANY, _abi.PID_OWN, _abi.PID_MAX_VERTICES, 256)
    assert pmod.STATUS_BITS == {"NO_ESTIMATE": pref.NO_ESTIMATE, "NONE": pref.NONE, "TAKEN": pref.TAKEN, "AMBIGUOUS": pref.AMBIGUOUS}
    assert pmod.STATUS_BITS == {"NO_ESTIMATE": 1, "NONE": 2, "TAKEN": 4, "AMBIGUOUS": 8}
    from attpc_engine_amd.detector import fit

    assert not _abi.FIT_NO_PID & sum(fit.STATUS_BITS.values())  # a new bit of the fit's status
    shared = (CSRC / "pid_host.hpp").read_text()
    kernel = (CSRC / "pid.hip").read_text()
    fit_kernel = (CSRC / "fit.hip").read_text()
    assert "asm" not in kernel and "float" not in kernel and "pid_inside(" in kernel and "pid_assign_slot(" in kernel and "__ballot" in kernel
    assert "fp contract(off)" in shared and "pid_edge(" in shared and "/" not in shared.split("pid_edge(double x")[1].split("}")[0]
    assert "template <bool PID>" in fit_kernel and "ATTPC_FIT_NO_PID" in fit_kernel and "fit_kernel<false>" in fit_kernel
    assert "pid_kernel" in (CSRC / "pid.hip").read_text() and "launch_pid" in (CSRC / "tracks_args.hpp").read_text()
    for text in (header, (ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        flat = _flat(text)
        assert "particle identification" in flat.lower() and "(y0 > y) != (y1 > y)" in flat, text[:60]
        assert "lowest" in flat.lower() and "NO_PID" in flat
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"pid.hip"' in entry and '"pid_host.hpp"' in entry
    for name in ("Gate", "PidSettings", "configure_pid", "pid_last", "estimates_to_pid", "by_position"):
        assert hasattr(detector, name) and name in detector.__all__, name
    assert "attpc_estimates_pid" in (ROOT / "INTEGRATION.md").read_text()
    assert "r33_pid" in (ROOT / "profiles" / "README.md").read_text()
    for text in ((ROOT / "README.md").read_text(), pmod.__doc__):
        assert "run_fused" in _flat(text) and "clustering=" in _flat(text)  # who does not take pid=


# ------------------------------------------------------------------------------------------ the cases, the restatement ----
def test_case_set_holds_what_it_names():
    pc.check_cases()


def test_restatement_on_every_case():
    """What must hold of any result, on every case."""
    for name, records in pc.reference().items():
        case = pc.cases()[name]
        assert records.shape == case.estimates.shape
        position, held, status = records["position"], records["held"], records["status"]
        assert np.all((position >= -1) & (position < case.n_sim)) and np.all(held >> case.n_sim == 0), name
        assigned = position >= 0
        assert np.all((held[assigned] >> position[assigned]) & 1 == 1), name  # a slot is assigned a position that holds it
        assert not (status[assigned] & ~pref.AMBIGUOUS).any(), name
        assert np.all((status[~assigned] & (pref.NO_ESTIMATE | pref.NONE | pref.TAKEN)) != 0), name
        for e in range(min(len(records), 200)):  # no position twice in an event
            got = position[e][position[e] >= 0]
            assert len(set(got.tolist())) == len(got), (name, e)
        if case.mode == pref.OWN:
            assert np.all(position[assigned] == np.nonzero(assigned)[1]), name
        gated = [p for p in range(case.n_sim) if case.gates[p] is not None]
        assert not (held & ~sum(1 << p for p in gated)).any(), name
        assert np.all(records["species"] == -1), name
        with_species = pref.records(case.estimates, case.gates, case.mode, species=pc.species_of(case))
        table = np.array(pc.species_of(case) + [-1])
        assert np.array_equal(with_species["species"], table[position]) and np.array_equal(with_species["position"], position), name


@pytest.mark.parametrize("mutant", pref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(mutant):
    caught = [name for name, case in pc.cases().items()
              if not pref.same(pref.records(case.estimates, case.gates, case.mode, mutant=mutant), pc.reference()[name])]
    print(mutant, "differs on", caught)
    assert caught, mutant


def test_gate_contains_is_the_restatement():
    for name, vertices in pc.GATES.items():
        case = pc.cases()["many, n_sim 8"]
        x, y = case.estimates["brho"], case.estimates["dedx"]
        assert np.array_equal(Gate(vertices).contains(x, y), pref.inside(vertices, x, y) & pref.testable(x, y)), name


# ------------------------------------------------------------------------------------------ the host code alone ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "pid_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _head(gates, mode, species, reserved=0, n_vertices=None) -> np.ndarray:
    counts = [0 if g is None else len(g) for g in gates] if n_vertices is None else n_vertices
    vertices = np.zeros((8, 32, 2))
    for p, gate in enumerate(gates):
        if gate is not None:
            vertices[p, :len(gate)] = gate
    return np.concatenate([[mode, reserved], counts, vertices.ravel(), list(species) + [-1] * (8 - len(species))]).astype(np.float64)


def _run(exe: Path, tmp: Path, what: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), what, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _native(exe, tmp, case: pc.Case, species) -> np.ndarray:
    points = np.stack([case.estimates["brho"], case.estimates["dedx"]], axis=-1).ravel()
    out = _run(exe, tmp, "records", np.concatenate([_head(case.gates, case.mode, species), [case.n_sim, len(case.estimates)], points]))
    table = out.reshape(len(case.estimates), case.n_sim, 4).astype(np.int64)
    records = np.zeros(table.shape[:2], dtype=pref.PID_DTYPE)
    for k, name in enumerate(pref.PID_DTYPE.names):
        records[name] = table[..., k]
    return records


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pid")
    exe = tmp / "pid_check"
    _build(exe, ["-O2"])
    return exe, tmp


def test_host_form_equals_the_restatement(native):
    exe, tmp = native
    for name, case in pc.cases().items():
        species = pc.species_of(case)
        assert pref.same(_native(exe, tmp, case, species), pref.records(case.estimates, case.gates, case.mode, species=species)), name
        assert pref.same(_native(exe, tmp, case, [-1] * case.n_sim), pc.reference()[name]), name


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone executable."""
    exe = tmp_path / "pid_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for name in ("triangle", "band", "hbox", "wide", "overlap", "overlap, own", "alphas", "no events", "one event", "many, n_sim 8"):
        case = pc.cases()[name]
        assert pref.same(_native(exe, tmp_path, case, [-1] * case.n_sim), pc.reference()[name]), name
    for change in BAD_DESCS:
        assert _run(exe, tmp_path, "desc", _desc_words(**change)).tolist() == [1.0], change


# ------------------------------------------------------------------------------------------ the gates' checks ----
def _desc_words(gates=None, mode=pref.ANY, reserved=0, n_vertices=None, vertex=None) -> np.ndarray:
    gates = list(pc.cases()["alphas"].gates if gates is None else gates)
    if vertex is not None:
        p, v, c, value = vertex
        gates[p] = np.array(gates[p], dtype=np.float64)
        gates[p][v, c] = value
    return _head(gates, mode, [-1] * 8, reserved, n_vertices)


BAD_DESCS = [{"mode": 2}, {"mode": -1}, {"reserved": 1}, {"n_vertices": [1, 0, 0, 0, 0, 0, 0, 0]}, {"n_vertices": [4, 2, 5, 0, 0, 0, 0, 0]},
             {"n_vertices": [4, 5, 5, 0, 0, 0, 0, 33]}, {"n_vertices": [-3, 5, 5, 0, 0, 0, 0, 0]},
             {"vertex": (0, 1, 0, NAN)}, {"vertex": (2, 4, 1, NAN)}, {"vertex": (1, 0, 1, INF)}, {"vertex": (1, 2, 0, -INF)}]
GOOD_DESCS = [{}, {"mode": pref.OWN}, {"gates": [None] * 8}, {"gates": [pc.GATES["band"]] * 8}, {"vertex": (0, 1, 0, -1e300)},
              {"n_vertices": [3, 5, 5, 0, 0, 0, 0, 0]}]


def test_host_desc_checks(native):
    exe, tmp = native
    for change in GOOD_DESCS:
        assert _run(exe, tmp, "desc", _desc_words(**change)).tolist() == [0.0], change
    for change in BAD_DESCS:
        assert _run(exe, tmp, "desc", _desc_words(**change)).tolist() == [1.0], change
    assert pref.desc_error(pc.cases()["alphas"].gates, pref.ANY) is None
    assert pref.desc_error(pc.cases()["alphas"].gates, 2) and pref.desc_error([np.zeros((2, 2))] + [None] * 7, pref.ANY)
    assert pref.desc_error([np.full((3, 2), NAN)] + [None] * 7, pref.ANY) and pref.desc_error([np.zeros((33, 2))] + [None] * 7, pref.ANY)
    # a NaN behind n_vertices is not read
    gates = list(pc.cases()["alphas"].gates)
    words = _head(gates, pref.ANY, [-1] * 8)
    words[2 + 8 + 2 * 4] = NAN  # vertex 4 of position 0, which has four
    assert _run(exe, tmp, "desc", words).tolist() == [0.0]


# ------------------------------------------------------------------------------------------ the Python layer ----
def _banana(rng, n):
    brho = rng.uniform(0.3, 1.5, size=n)
    dedx = 40.0 / brho ** 2 * np.exp(rng.normal(0.0, 0.15, size=n))
    return brho, dedx


def test_gate_from_band():
    rng = np.random.default_rng(8)
    brho, dedx = _banana(rng, 20000)
    for bins, coverage in ((12, (0.02, 0.98)), (15, (0.1, 0.9)), (1, (0.0, 1.0)), (4, (0.25, 0.75))):
        gate = Gate.from_band(brho, dedx, bins=bins, coverage=coverage)
        assert 3 <= len(gate) <= _abi.PID_MAX_VERTICES and len(gate) == 2 * bins + 2
        share = gate.contains(brho, dedx).mean()
        # every point between its bin's quantiles is inside, and the outer vertices at a bin edge add at most the
        # neighbouring bin's tails: no less than the stated share, and for the banana not the whole sample either
        print(bins, coverage, len(gate), share)
        assert share >= coverage[1] - coverage[0] - 2.0 / (len(brho) / bins), (bins, coverage, share)
        if coverage != (0.0, 1.0):
            assert share < 1.0, (bins, coverage, share)
    # another species' band is outside it
    other = Gate.from_band(brho, dedx * 6.0)
    gate = Gate.from_band(brho, dedx)
    assert other.contains(brho, dedx).mean() < 0.01 and gate.contains(brho, dedx * 6.0).mean() < 0.01
    # NaN, infinite and non-positive records are ignored
    dirty_x = np.concatenate([brho, [NAN, 1.0, INF, 0.0, -1.0, 1.0]])
    dirty_y = np.concatenate([dedx, [50.0, NAN, 50.0, 50.0, 50.0, -2.0]])
    assert np.array_equal(Gate.from_band(dirty_x, dirty_y).vertices, gate.vertices)
    assert PidSettings([gate, other]).desc().n_vertices[0] == 26
    for bad in (0, 16, 2.0, True, "12"):
        with pytest.raises(ValueError):
            Gate.from_band(brho, dedx, bins=bad)
    for bad in ((0.5, 0.5), (0.9, 0.1), (-0.1, 0.9), (0.1, 1.1)):
        with pytest.raises(ValueError):
            Gate.from_band(brho, dedx, coverage=bad)
    with pytest.raises(ValueError):
        Gate.from_band(brho[:10], dedx[:10])
    with pytest.raises(ValueError):
        Gate.from_band(brho, dedx[:-1])


def test_by_position_round_trip():
    case = pc.cases()["many, n_sim 8"]
    pid = pc.reference()["many, n_sim 8"]
    out, slot_of = by_position(case.estimates, pid)
    n, n_sim = pid.shape
    assert out.shape == slot_of.shape == (n, n_sim) and out.dtype == case.estimates.dtype
    events, slots = np.nonzero(pid["position"] >= 0)
    assert np.array_equal(slot_of[events, pid["position"][events, slots]], slots)
    assert (slot_of >= 0).sum() == len(events)
    assert out[events, pid["position"][events, slots]].tobytes() == case.estimates[events, slots].tobytes()
    empty = out[slot_of < 0]
    assert np.all(empty["status"] == _abi.EST_EMPTY) and np.all(np.isnan(empty["brho"])) and np.all(empty["n_rows"] == 0)
    # and back: the slot a position was taken from holds the record again
    back = np.zeros_like(case.estimates)
    e, p = np.nonzero(slot_of >= 0)
    back[e, slot_of[e, p]] = out[e, p]
    assert back[events, slots].tobytes() == case.estimates[events, slots].tobytes()
    fits = np.zeros((n, n_sim), dtype=_abi.FIT_DTYPE)
    fits["ke"] = np.arange(n * n_sim).reshape(n, n_sim)
    moved, _ = by_position(fits, pid)
    assert np.array_equal(moved["ke"][events, pid["position"][events, slots]], fits["ke"][events, slots])
    assert np.all(moved["status"][slot_of < 0] == _abi.FIT_EMPTY)
    with pytest.raises(ValueError):
        by_position(fits[:, :3], pid)


def test_argument_checks():
    square = [(0, 0), (1, 0), (1, 1), (0, 1)]
    for bad in ([(0, 0), (1, 1)], [(0, 0)] * 33, [(0, 0, 0)] * 4, [(0, 0), (1, NAN), (1, 1)], [(0, 0), (INF, 0), (1, 1)], "gate", 3.0,
                [("a", "b")] * 3):
        with pytest.raises(ValueError):
            Gate(bad)
    assert len(Gate(square)) == 4 and len(Gate(np.zeros((32, 2)))) == 32
    assert Gate.rectangle((0.0, 2.0), (1.0, 3.0)).vertices.tolist() == [[0, 1], [2, 1], [2, 3], [0, 3]]
    for bad in ("both", 0, None, "ANY"):
        with pytest.raises(ValueError):
            PidSettings([square], mode=bad)
    with pytest.raises(ValueError):
        PidSettings([square] * 9)
    for bad in ({8: square}, {-1: square}, {"0": square}, {True: square}):
        with pytest.raises(ValueError):
            PidSettings(bad)
    with pytest.raises(ValueError):
        PidSettings([[(0, 0), (1, 1)]])
    for bad in ("gates", None, 5):
        with pytest.raises(TypeError):
            PidSettings(bad)
    settings = PidSettings({2: square, 0: Gate(pc.GATES["band"])}, mode="own")
    desc = settings.desc()
    assert list(desc.n_vertices) == [32, 0, 4, 0, 0, 0, 0, 0] and (desc.mode, desc.reserved) == (_abi.PID_OWN, 0)
    vertices = np.ctypeslib.as_array(desc.vertices)
    assert vertices.shape == (8, 32, 2) and np.array_equal(vertices[0], pc.GATES["band"]) and vertices[2, :4].tolist() == [list(map(float, v)) for v in square]
    assert not vertices[1].any() and not vertices[2, 4:].any()
    assert settings.token() == PidSettings([Gate(pc.GATES["band"]), None, square], "own").token() != PidSettings([square], "own").token()
    assert PidSettings([square]).token() != PidSettings([square], "own").token()
    with pytest.raises(TypeError):
        pmod.configure_pid(None, "gates")
    with pytest.raises(TypeError):
        pmod.estimates_to_pid(np.zeros((1, 1), dtype=_abi.ESTIMATE_DTYPE), [square])
    from attpc_engine_amd.detector.traces import TraceChain, _checked_pid

    with pytest.raises(TypeError):
        _checked_pid([square])
    assert _checked_pid(None) is None and _checked_pid(settings) is settings
    import inspect

    from attpc_engine_amd.detector import fit, traces
    from attpc_engine_amd.engine import Engine

    assert "pid" in inspect.signature(fit.rows_to_fit).parameters and "pid" in inspect.signature(TraceChain.__init__).parameters
    assert "pid" in inspect.signature(traces.configure_trace_rows).parameters and "pid" in inspect.signature(traces.simulate_batch_trace_rows).parameters
    assert list(inspect.signature(Engine.configure_pid).parameters) == ["self", "gates", "mode"]
