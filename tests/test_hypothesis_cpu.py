"""The fit hypotheses without a GPU (include/attpc_engine.h, "fit hypotheses"): the contract's names everywhere; the
walk cases with hand-written f tables, which hold what they name; the restatement (tests/hypothesis_reference.py) and
its mutants, each of which the exact comparison catches; csrc/hypothesis_host.hpp, compiled alone for the host, plain
and under the sanitizers (a stand-alone program with its own main), equal to the restatement exactly; the physics the
stage rests on, on the hand-made tracks of tests/fit_cases.py; ``by_position`` on these records; the settings' checks."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd import detector
from attpc_engine_amd.detector import hypothesis as hmod
from attpc_engine_amd.detector import traces
from attpc_engine_amd.detector.hypothesis import HypothesisSettings
from attpc_engine_amd.detector.pid import by_position
from tests import fit_cases
from tests import fit_reference as fref
from tests import hypothesis_cases as hc
from tests import hypothesis_reference as href

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"
ENTRY_POINTS = ("attpc_trace_configure_hypotheses", "attpc_hypotheses_last", "attpc_hypothesis_fits_last",
                "attpc_rows_fit_hypotheses")


def _flat(text: str) -> str:
    return text.replace("\n * ", " ").replace("\n// ", " ").replace("\n", " ")


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.HYPOTHESIS_SYMBOLS == ENTRY_POINTS == tuple(_abi.SYMBOL_GROUPS["hypotheses"]) and "hypotheses" in _abi.CONFIGURE_SLOTS
    assert int(re.search(r"#define ATTPC_ABI_VERSION (\d+)", header).group(1)) == 3 == _abi.ABI_VERSION  # additions only
    assert "---- fit hypotheses (opt-in" in header
    for struct, cls in (("attpc_hypothesis_desc", _abi.HypothesisDesc), ("attpc_fit_hypothesis", _abi.FitHypothesis)):
        fields = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header).group(1)
        names = [n.strip() for line in re.findall(r"^\s*(?:double|int32_t) ([\w, \[\]]+);", fields, re.M)
                 for n in re.sub(r"\[\w+\]", "", line).split(",")]
        assert names == [name for name, _ in cls._fields_], (struct, names)
    assert (C.sizeof(_abi.HypothesisDesc), C.sizeof(_abi.FitHypothesis)) == (8, 96)
    assert _abi.HYPOTHESIS_DTYPE.itemsize == 96 and _abi.FitHypothesis.f.offset == 24 and _abi.FitHypothesis.f_next.offset == 88
    assert _abi.HYPOTHESIS_DTYPE.descr == href.HYPOTHESIS_DTYPE.descr and hmod.HYPOTHESIS_DTYPE is _abi.HYPOTHESIS_DTYPE
    for name, value in (("ATTPC_HYP_NO_CANDIDATE", _abi.HYP_NO_CANDIDATE), ("ATTPC_HYP_NO_FIT", _abi.HYP_NO_FIT),
                        ("ATTPC_HYP_TAKEN", _abi.HYP_TAKEN), ("ATTPC_HYP_DISPLACED", _abi.HYP_DISPLACED)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert hmod.STATUS_BITS == {"NO_CANDIDATE": 1, "NO_FIT": 2, "TAKEN": 4, "DISPLACED": 8}
    assert hmod.STATUS_BITS == {"NO_CANDIDATE": href.NO_CANDIDATE, "NO_FIT": href.NO_FIT, "TAKEN": href.TAKEN, "DISPLACED": href.DISPLACED}
    # not a row of the trace-row chain: engine-level, like the reaction reconstruction
    assert not any(stage.field in ("hypotheses", "hypothesis") or stage.settings is HypothesisSettings for stage in traces.STAGES)
    import inspect

    from attpc_engine_amd.engine import Engine

    for function in (traces.configure_trace_rows, traces.simulate_batch_trace_rows, traces.TraceChain.__init__):
        assert "hypotheses" not in inspect.signature(function).parameters
    assert list(inspect.signature(Engine.configure_fit_hypotheses).parameters) == ["self", "settings", "parameters"]
    shared = (CSRC / "hypothesis_host.hpp").read_text()
    kernel = (CSRC / "hypothesis.hip").read_text()
    fit_kernel = (CSRC / "fit.hip").read_text()
    assert "hypothesis_selection_kernel" in kernel and "hypothesis_event(" in kernel and "asm" not in kernel and "float" not in kernel
    walk = shared.split("ATTPC_HYP_HD void hypothesis_event(")[1].split("// A batch on the host")[0]
    assert not re.search(r"\bf\w*\s*[-+*/]\s|[-+*/]\s*r\.f", walk)  # comparisons and copies only: no arithmetic on f
    assert "fit_kernel<false, true>" in fit_kernel and "hypothesis_tried(" in fit_kernel and "fp contract(off)" in fit_kernel
    assert "launch_fit_hypotheses" in (CSRC / "tracks_args.hpp").read_text()
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"hypothesis.hip"' in entry and '"hypothesis_host.hpp"' in entry
    for name in ("HypothesisSettings", "configure_fit_hypotheses", "hypotheses_last", "rows_to_fit_hypotheses", "HYPOTHESIS_DTYPE"):
        assert hasattr(detector, name) and name in detector.__all__, name
    for text in (header, (ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        flat = _flat(text).lower()
        assert "fit hypotheses" in flat and "lowest" in flat and "displaced" in flat, text[:60]
    assert "4.4s" in (ROOT / "DESIGN.md").read_text()
    assert "r36_fit_hypotheses" in (ROOT / "profiles" / "README.md").read_text()
    assert (ROOT / "tools" / "hypothesis_rate.py").exists() and (ROOT / "profiles" / "r36_fit_hypotheses.md").exists()


# ------------------------------------------------------------------------------------------ the walk, by hand ----
def test_walk_cases_hold_what_they_name():
    hc.check_walk_cases()
    assert set(hc.walk_cases()) >= {"two slots prefer one position", "three slots for two fitted positions",
                                    "an exact tie between two species", "a NaN f", "tried == 0",
                                    "a pid mask that leaves one candidate"}


def _walked(case, mutant=None):
    layout, _, fits, estimates, pid = hc.walk_arrays(case)
    tried = href.tried(layout, 1, case.candidates, pid, mutant)
    return href.walk(fits, tried, layout, estimates, mutant)


@pytest.mark.parametrize("mutant", href.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(mutant):
    caught = []
    for name, case in hc.walk_cases().items():
        want, want_fits = _walked(case)
        got, got_fits = _walked(case, mutant)
        if not href.same(got, want) or got_fits.tobytes() != want_fits.tobytes():
            caught.append(name)
    print(mutant, "differs on", caught)
    assert caught, mutant


def test_layout_of_the_hypotheses():
    for species, first, of_position in (([0, 1, 1, 0, 0, 1, 0, 1], [0, 1], [0, 1, 1, 0, 0, 1, 0, 1]), ([5, 5, 3], [0, 2], [0, 0, 1]),
                                        ([-1, 4, -1, 4], [1], [-1, 0, -1, 0]), ([-1, -1], [], [-1, -1]), ([7], [0], [0]),
                                        ([3, 2, 1, 0, 3, 2, 1, 0], [0, 1, 2, 3], [0, 1, 2, 3, 0, 1, 2, 3]),
                                        (list(range(8)), list(range(8)), list(range(8)))):
        layout = href.Layout(species)
        assert (layout.first, layout.of_position, layout.n) == (first, of_position, len(first)), species
    assert href.Layout(fit_cases.SPECIES8).hypothesis_species() == [0, 1]


# ------------------------------------------------------------------------------------------ the host code alone ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "hypothesis_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _run(exe: Path, tmp: Path, what: str, data) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), what, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _head(candidates, reserved, has_pid, species, n_events):
    return [candidates, reserved, float(has_pid), len(species), n_events] + list(species) + [-1] * (8 - len(species))


def _native(exe, tmp, layout, candidates, pid, fits, estimates):
    """The stand-alone program on fit records [n, n_sim, H] -> (records, and status, n_points, f, tag of the chosen fits)."""
    n, n_sim, n_hyp = fits.shape
    held = np.zeros((n, n_sim)) if pid is None else pid["held"]
    slots = np.stack([held, estimates["n_used"]], axis=-1).ravel()
    tags = np.arange(fits.size, dtype=np.float64).reshape(fits.shape)
    pairs = np.stack([fits["status"], fits["f"], tags], axis=-1).ravel()
    out = _run(exe, tmp, "records", np.concatenate([_head(candidates, 0, pid is not None, layout.species, n), slots, pairs]))
    table = out.reshape(n, n_sim, 19)
    records = np.zeros((n, n_sim), dtype=href.HYPOTHESIS_DTYPE)
    for k, name in enumerate(("position", "species", "tried", "fitted", "status", "reserved")):
        records[name] = table[..., k]
    records["f"], records["f_next"] = table[..., 6:14], table[..., 14]
    return records, table[..., 15:]


def _check_native(exe, tmp, layout, candidates, pid, fits, estimates, name):
    want, want_fits = href.walk(fits, href.tried(layout, len(fits), candidates, pid), layout, estimates)
    got, chosen = _native(exe, tmp, layout, candidates, pid, fits, estimates)
    assert href.same(got, want), (name, got, want)
    tags = np.arange(fits.size).reshape(fits.shape)
    for e, k in np.ndindex(*want.shape):
        position = want["position"][e, k]
        if position >= 0:
            assert chosen[e, k, 3] == tags[e, k, layout.of_position[position]], (name, e, k)
            assert chosen[e, k, 0] == want_fits["status"][e, k] and href.same_f64(chosen[e, k, 2], want_fits["f"][e, k]), (name, e, k)
        else:
            assert chosen[e, k, 0] == href.FIT_NO_PID and chosen[e, k, 1] == want_fits["n_points"][e, k] and np.isnan(chosen[e, k, 2]), (name, e, k)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hypothesis")
    exe = tmp / "hypothesis_check"
    _build(exe, ["-O2"])
    return exe, tmp


def _random_tables(rng, n, species):
    """Fit records [n, n_sim, H] with f on a coarse grid (ties), NaN, infinities and every status that matters."""
    layout = href.Layout(species)
    n_sim = len(species)
    fits = np.zeros((n, n_sim, layout.n), dtype=_abi.FIT_DTYPE)
    f = rng.integers(1, 6, size=fits.shape) / 2.0
    kind = rng.integers(0, 12, size=fits.shape)
    f[kind == 0], f[kind == 1] = np.nan, np.inf
    fits["f"] = f
    fits["status"] = np.where(kind == 2, _abi.FIT_NO_START, np.where(kind == 3, _abi.FIT_FEW, np.where(kind == 4, _abi.FIT_NOT_CONVERGED, 0)))
    estimates = np.zeros((n, n_sim), dtype=_abi.ESTIMATE_DTYPE)
    estimates["n_used"] = rng.integers(0, 3000, size=(n, n_sim))
    pid = np.zeros((n, n_sim), dtype=_abi.PID_DTYPE)
    pid["held"] = rng.integers(0, 256, size=(n, n_sim))
    return layout, fits, estimates, pid


def test_host_form_equals_the_restatement(native, pinned):
    exe, tmp = native
    for name, case in hc.walk_cases().items():
        layout, _, fits, estimates, pid = hc.walk_arrays(case)
        _check_native(exe, tmp, layout, case.candidates, pid, fits, estimates, name)
    rng = np.random.default_rng(36)
    for species in ([0, 1, 1, 0, 0, 1, 0, 1], [4, 4, 2], [-1, 3], [1], [0, 1, 2, 3, 4, 5, 6, 7], [-1, -1, -1]):
        layout, fits, estimates, pid = _random_tables(rng, 300, species)
        for candidates, with_pid in ((href.ALL, False), (href.ALL, True), (0b1011, True), (0b100, False)):
            _check_native(exe, tmp, layout, candidates, pid if with_pid else None, fits, estimates, (species, candidates, with_pid))
    layout, estimates, fits, _, _ = pinned  # and on real fit records
    _check_native(exe, tmp, layout, href.ALL, None, fits, estimates, "hand-made tracks")
    # the layout the host makes
    for species in ([0, 1, 1, 0, 0, 1, 0, 1], [5, 5, 3], [-1, 4, -1, 4], [-1, -1], [7]):
        layout = href.Layout(species)
        out = _run(exe, tmp, "layout", _head(0b1101, 0, False, species, 0)).astype(np.int64)
        assert out[0] == layout.n and out[1] == 0b1101 & layout.with_species, species
        assert out[2:2 + layout.n].tolist() == layout.first and (out[2 + layout.n:10] == -1).all()
        assert out[18:18 + len(species)].tolist() == layout.of_position
        assert out[10:10 + layout.n].tolist() == [sum(1 << p for p, h in enumerate(layout.of_position) if h == i) for i in range(layout.n)]


BAD_DESCS = [(0, 0), (1 << 8, 0), (0x1FF, 0), (-1, 0), (3, 1), (3, -1)]
GOOD_DESCS = [(1, 0), (0xFF, 0), (0x80, 0), (0b1010, 0)]


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone executable."""
    exe = tmp_path / "hypothesis_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for name, case in hc.walk_cases().items():
        layout, _, fits, estimates, pid = hc.walk_arrays(case)
        _check_native(exe, tmp_path, layout, case.candidates, pid, fits, estimates, name)
    rng = np.random.default_rng(37)
    for species in ([0, 1, 2, 3, 4, 5, 6, 7], [0, 0, 0, 0, 0, 0, 0, 0], [-1, 2, 2], []):
        layout, fits, estimates, pid = _random_tables(rng, 50, species)
        _check_native(exe, tmp_path, layout, href.ALL, pid, fits, estimates, species)
        _check_native(exe, tmp_path, layout, 0x80, None, fits, estimates, species)
    for desc in BAD_DESCS:
        assert _run(exe, tmp_path, "desc", _head(*desc, False, [0], 0)).tolist() == [1.0], desc


def test_host_desc_checks(native):
    exe, tmp = native
    for desc in GOOD_DESCS:
        assert _run(exe, tmp, "desc", _head(*desc, False, [0], 0)).tolist() == [0.0] and href.desc_error(*desc) is None, desc
    for desc in BAD_DESCS:
        assert _run(exe, tmp, "desc", _head(*desc, False, [0], 0)).tolist() == [1.0] and href.desc_error(*desc), desc


# ------------------------------------------------------------------------------------------ the physics pin ----
@pytest.fixture(scope="module")
def pinned():
    """The events "eight" and "single" of tests/fit_cases.py with ``fit_cases.SETTINGS``, every slot fitted as the proton
    and as the 11Be: (layout, estimates, fits [2, 8, 2], records, chosen fits), read-only."""
    model, events, _, _, _, layout = hc.hand()
    csr = fit_cases.csr({name: events[name] for name in ("eight", "single")})
    from tests import estimate_reference as est

    estimates = est.records(*csr, fit_cases.INDICES8, hc.PARAMS)
    tried = href.tried(layout, 2)
    fits = href.all_fits(*csr, fit_cases.INDICES8, model, estimates, fref.Settings(**fit_cases.SETTINGS), fit_cases.BEAM_REGION,
                         layout, tried)
    records, chosen = href.walk(fits, tried, layout, estimates)
    for array in (estimates, fits, records, chosen):
        array.setflags(write=False)
    return layout, estimates, fits, records, chosen


def test_every_hand_made_track_takes_a_position_of_its_true_species(pinned):
    layout, estimates, fits, records, chosen = pinned
    assert layout.n == 2 and layout.hypothesis_species() == [0, 1] and fits.shape == (2, 8, 2)
    species = np.array(fit_cases.SPECIES8)
    # "eight": the identity assignment, no slot displaced
    assert records["position"][0].tolist() == list(range(8)) and not (records["status"][0] & href.DISPLACED).any()
    assert records["species"][0].tolist() == fit_cases.SPECIES8 and (records["status"][0] == 0).all()
    assert (records["tried"] == 0xFF).all() and (records["fitted"][0] == 0xFF).all()
    # "single": the one track (label 7, position 4, a proton) takes a proton position, the empty slots none
    with_points = ~((estimates["status"] & (_abi.EST_EMPTY | _abi.EST_FEW)) != 0)
    assert with_points[1].tolist() == [False] * 4 + [True] + [False] * 3
    assert species[records["position"][1, 4]] == 0 and records["position"][1, 4] == 0  # (the lowest free proton position)
    empty = ~with_points[1]
    assert (records["position"][1][empty] == -1).all() and (records["status"][1][empty] == href.NO_FIT).all()
    assert (chosen["status"][1][empty] == href.FIT_NO_PID).all()
    # the ratio of the two f at every track: the true species is the lower one
    f = fits["f"]
    for e, k in zip(*np.nonzero(with_points)):
        true = species[k] if e == 0 else 0
        ratio = f[e, k, 1 - true] / f[e, k, true]
        print(e, k, "f true", f[e, k, true], "f other", f[e, k, 1 - true], "ratio", ratio)
        assert ratio > 1.0, (e, k, ratio)
        assert href.same_f64(records["f_next"][e, k], f[e, k, 1 - true])
        assert chosen[e, k].tobytes() == fits[e, k, true].tobytes()


def test_by_position_takes_hypothesis_records(pinned):
    """``detector.pid.by_position`` reads ``position`` of its second argument: these records serve as they are."""
    _, _, _, records, chosen = pinned
    moved, slot_of = by_position(chosen, records)
    assert slot_of[0].tolist() == list(range(8)) and slot_of[1].tolist() == [4] + [-1] * 7
    assert moved[0].tobytes() == chosen[0].tobytes() and moved[1, 0].tobytes() == chosen[1, 4].tobytes()
    assert (moved["status"][1, 1:] == _abi.FIT_EMPTY).all()
    as_pid = np.zeros(records.shape, dtype=_abi.PID_DTYPE)
    as_pid["position"] = records["position"]
    again, slots_again = by_position(chosen, as_pid)
    assert again.tobytes() == moved.tobytes() and np.array_equal(slots_again, slot_of)  # what it does for pid records


# ------------------------------------------------------------------------------------------ the settings ----
def test_settings_checks():
    assert HypothesisSettings().candidates == 0xFF and HypothesisSettings(None).token() == (0xFF,)
    assert HypothesisSettings([0, 2]).candidates == 5 and HypothesisSettings(0b110).candidates == 6 and HypothesisSettings((7,)).candidates == 0x80
    desc = HypothesisSettings([1]).desc()
    assert (desc.candidates, desc.reserved) == (2, 0)
    for bad in (0, 1 << _abi.MAX_SIM, 0x1FF, -1, [], [8], [-1], [0, _abi.MAX_SIM], [1.0], [True]):
        with pytest.raises(ValueError):
            HypothesisSettings(bad)
    for bad in ("01", 1.0, True, b"\x01", object()):
        with pytest.raises(TypeError):
            HypothesisSettings(bad)
    with pytest.raises(TypeError):
        hmod.configure_fit_hypotheses(None, 3)
    with pytest.raises(TypeError):
        hmod.rows_to_fit_hypotheses([0], np.zeros((0, 8)), np.zeros(0), fit_cases.layout(), np.zeros((0, 8), dtype=_abi.ESTIMATE_DTYPE),
                                    None, detector.TrackFitSettings(), 0xFF)
    with pytest.raises(TypeError):
        hmod.rows_to_fit_hypotheses([0], np.zeros((0, 8)), np.zeros(0), fit_cases.layout(), np.zeros((0, 8), dtype=_abi.ESTIMATE_DTYPE),
                                    None, None, HypothesisSettings())
    assert HypothesisSettings.slot == "hypotheses" and HypothesisSettings.call in ENTRY_POINTS
