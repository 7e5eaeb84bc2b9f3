"""The reaction reconstruction without a GPU (include/attpc_engine.h, "reaction reconstruction"): the contract's names
everywhere; the numpy restatement (tests/reaction_reference.py) against exact arithmetic (tests/golden/reaction_exact.npz,
written by tests/reaction_exact_reference.py with mpmath) within bounds whose constants were measured against it; the
bins at their edges; closure on four-vectors this stage did not make; the mutants of the restatement, each of which the
exact comparison catches; csrc/reaction_host.hpp, compiled alone for the host, plain and under the sanitizers (a
stand-alone program with its own main), equal to the restatement byte for byte; the checks of the settings.

Measured against mpmath on the 4 320 cases of the fixture (be10dp and o16aa, row 2 and row 3, no target / 2 nodes /
2 049 nodes), in units of the scales the fixture carries (tests/reaction_exact_reference.py derives them):
    beam energy   max |dT_b| / (2^-53 beam_energy)  = 0.95
    Ex            max |dEx|  / (2^-53 E^2 / m_r)    = 1.762
    theta_cm      max |dth|  / S_th                 = 1.431
asserted at 4 times these, as tests/kin_exact_check.py does."""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd import detector
from attpc_engine_amd.detector import reaction as rmod
from attpc_engine_amd.detector.reaction import ReactionSettings, ReactionSpectra
from tests import reaction_cases as rc
from tests import reaction_reference as pref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"
ENTRY_POINTS = ("attpc_reaction_configure", "attpc_reaction_last", "attpc_reaction_spectra_last", "attpc_reaction_records")
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53
K_BEAM, K_EX, K_THETA = 4 * 0.95, 4 * 1.762, 4 * 1.431  # 4 x measured (the module's docstring)


def _flat(text: str) -> str:
    return text.replace("\n * ", " ").replace("\n// ", " ").replace("\n", " ")


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.REACTION_SYMBOLS == ENTRY_POINTS and "reaction" in _abi.CONFIGURE_SLOTS
    assert tuple(_abi.SYMBOL_GROUPS["reaction"]) == ENTRY_POINTS
    assert int(re.search(r"#define ATTPC_ABI_VERSION (\d+)", header).group(1)) == 3  # additions only
    for struct, cls in (("attpc_reaction_desc", _abi.ReactionDesc), ("attpc_reaction_record", _abi.ReactionRecord)):
        fields = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header).group(1)
        names = [n.strip() for line in re.findall(r"^\s*(?:const double\*|double|int32_t|int64_t) ([\w, \[\]]+);", fields, re.M)
                 for n in re.sub(r"\[\w+\]", "", line).split(",")]
        assert names == [name for name, _ in cls._fields_], (struct, names)
    assert (C.sizeof(_abi.ReactionDesc), C.sizeof(_abi.ReactionRecord), rmod.REACTION_DTYPE.itemsize) == (136, 64, 64)
    for name, value in (("ATTPC_REACTION_FROM_FIT", _abi.REACTION_FROM_FIT), ("ATTPC_REACTION_FROM_ESTIMATE", _abi.REACTION_FROM_ESTIMATE),
                        ("ATTPC_REACTION_NO_TRACK", _abi.REACTION_NO_TRACK), ("ATTPC_REACTION_OUTSIDE_TARGET", _abi.REACTION_OUTSIDE_TARGET),
                        ("ATTPC_REACTION_UNPHYSICAL", _abi.REACTION_UNPHYSICAL), ("ATTPC_REACTION_NO_TRUTH", _abi.REACTION_NO_TRUTH),
                        ("ATTPC_REACTION_MAX_EX", _abi.REACTION_MAX_EX), ("ATTPC_REACTION_MAX_THETA", _abi.REACTION_MAX_THETA),
                        ("ATTPC_REACTION_MAX_ELOSS", _abi.REACTION_MAX_ELOSS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert rmod.STATUS_BITS == {"NO_TRACK": pref.NO_TRACK, "OUTSIDE_TARGET": pref.OUTSIDE_TARGET, "UNPHYSICAL": pref.UNPHYSICAL,
                                "NO_TRUTH": pref.NO_TRUTH} == {"NO_TRACK": 1, "OUTSIDE_TARGET": 2, "UNPHYSICAL": 4, "NO_TRUTH": 8}
    assert (pref.FROM_FIT, pref.FROM_ESTIMATE) == (_abi.REACTION_FROM_FIT, _abi.REACTION_FROM_ESTIMATE) and rmod.PI == pref.PI
    shared = (CSRC / "reaction_host.hpp").read_text()
    kernel = (CSRC / "reaction.hip").read_text()
    assert "asm" not in kernel and "float" not in kernel and "reaction_event(" in kernel and "atomicAdd" in kernel
    assert shared.count("fp contract(off)") >= 4 and "helix_atan2w(" in shared and "atan2(" not in shared and "fma" not in shared
    for text in (header, (ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        flat = _flat(text)
        assert "reaction reconstruction" in flat.lower() and "theta_cm" in flat and "NO_TRUTH" in flat, text[:60]
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"reaction.hip"' in entry and '"reaction_host.hpp"' in entry
    for name in ("ReactionSettings", "ReactionSpectra", "configure_reaction", "reaction_last", "records_to_reaction"):
        assert hasattr(detector, name) and name in detector.__all__, name
    assert "attpc_reaction_records" in (ROOT / "INTEGRATION.md").read_text()
    assert "r35_reaction" in (ROOT / "profiles" / "README.md").read_text()
    for out_of_scope in ("run_fused", "run_simulation", "simulate_batch_trace_rows"):
        assert out_of_scope in _flat((ROOT / "README.md").read_text()).lower().split("reaction reconstruction")[1][:6000]
    from attpc_engine_amd.detector.traces import STAGES

    assert not any("reaction" in str(stage).lower() for stage in STAGES)  # not a row of the chain
    from attpc_engine_amd.engine import Engine

    assert all(hasattr(Engine, name) for name in ("configure_reaction", "run_spectra"))


# ------------------------------------------------------------------------------------------ against exact arithmetic ----
def _groups():
    z = rc.fixture()
    for reaction in z["reactions"]:
        for target in z["targets"]:
            for row in (2, 3):
                yield str(reaction), str(target), row, z[f"{reaction}_{target}_row{row}"]


def test_fixture_covers_what_the_issue_names():
    z = rc.fixture()
    assert list(z["reactions"]) == ["be10dp", "o16aa"] and list(z["targets"]) == ["none", "two", "long"]
    assert len(z["be10dp_two_eloss"]) == 2 and len(z["o16aa_long_eloss"]) == 2049
    assert list(z["columns"]) == ["z", "px", "py", "pz", "beam_ke", "ex", "theta_cm", "scale_ex", "scale_theta", "ex_thrown",
                                  "polar_thrown"]
    n = 0
    for reaction, target, row, c in _groups():
        n += len(c)
        assert {0.0, 1.0} <= set(c[:, 0]) and c[:, 0].min() < 0.0 and c[:, 0].max() > 1.0 and np.any((c[:, 0] > 0) & (c[:, 0] < 1))
        assert {0.0, pref.PI} <= set(c[:, 10]) and np.any(c[:, 9] == 0.0) and c[:, 9].max() > 10.0
        on_axis = np.isin(c[:, 10], (0.0, pref.PI))
        assert np.all(c[on_axis, 1] == 0.0) and np.all(c[on_axis, 2] == 0.0) and np.all(c[~on_axis, 1] != 0.0)
        if row == 2:  # the ejectile's own angle and the residual's excitation come back
            assert np.allclose(c[:, 6], c[:, 10], atol=1e-6) and np.allclose(c[:, 5], c[:, 9], atol=1e-6)
    assert n == 4320


def test_restatement_against_exact_arithmetic():
    z = rc.fixture()
    worst = {"beam": 0.0, "ex": 0.0, "theta": 0.0}
    for reaction, target, row, c in _groups():
        s = rc.base_settings(reaction, target, observed_row=row)
        beam = float(z[f"{reaction}_beam"])
        t_b = pref.beam_ke(s, c[:, 0])
        ex, theta, m2 = pref.value(s, t_b, c[:, 1], c[:, 2], c[:, 3])
        assert not np.isnan(ex).any() and np.all(m2 > 0), (reaction, target, row)
        k_beam = np.max(np.abs(t_b - c[:, 4])) / (U * beam)
        k_ex, k_theta = np.max(np.abs(ex - c[:, 5]) / c[:, 7]), np.max(np.abs(theta - c[:, 6]) / c[:, 8])
        print(f"{reaction} {target} row {row}: K_beam {k_beam:.3f} K_ex {k_ex:.3f} K_theta {k_theta:.3f}")
        worst = {"beam": max(worst["beam"], k_beam), "ex": max(worst["ex"], k_ex), "theta": max(worst["theta"], k_theta)}
        assert k_beam <= K_BEAM and k_ex <= K_EX and k_theta <= K_THETA, (reaction, target, row, k_beam, k_ex, k_theta)
        if target == "none":
            assert np.all(t_b == beam)
        # theta_cm exactly 0 and exactly PI where nothing is transverse
        forward, backward = c[:, 10] == (pref.PI if row == 3 else 0.0), c[:, 10] == (0.0 if row == 3 else pref.PI)
        assert np.all(theta[c[:, 10] == 0.0] == 0.0) and np.all(theta[c[:, 10] == pref.PI] == pref.PI), (forward.sum(), backward.sum())
    print("worst", worst)
    # the scale of Ex is the cancellation in M2: 2^-53 E^2 / m_r
    for reaction, target, row, c in _groups():
        m = rc.fixture()[f"{reaction}_masses"]
        e = c[:, 4] + m[1] + m[0]
        assert np.allclose(c[:, 7], U * e * e / m[5 - row], rtol=1e-12)


def test_bins_at_their_edges():
    for lo, hi, n in ((-2.0, 14.0, 64), (0.0, pref.PI, 36), (0.0, pref.PI, 180), (-1.0, 3.0, 256), (0.1, 0.7, 7), (5.0, 6.0, 1)):
        inv = float(n) / (hi - lo)
        below_hi = math.nextafter(hi, -INF)
        assert pref.bins([lo, below_hi, hi, NAN, math.nextafter(lo, -INF), INF, -INF], lo, hi, inv, n).tolist() == [0, n - 1, -1, -1, -1, -1, -1]
        edges = [lo + k / inv for k in range(1, n)]
        got = pref.bins(edges, lo, hi, inv, n)
        want = [min(int(math.floor((v - lo) * inv)), n - 1) for v in edges]  # the rule in plain Python floats
        assert got.tolist() == want, (lo, hi, n)
        assert np.all((got >= 0) & (got < n)) and np.all(np.abs(got - np.arange(1, n)) <= 1)
        if (lo, hi) == (-2.0, 14.0) or (lo, hi, n) == (-1.0, 3.0, 256):  # dyadic widths: every edge opens its own bin
            assert got.tolist() == list(range(1, n))
        # the double below an edge: v - lo may round up to the edge, so it is of the bin below or of the edge's own --
        # whichever the rule in plain Python floats says
        just_below = [math.nextafter(v, -INF) for v in edges]
        got = pref.bins(just_below, lo, hi, inv, n)
        assert got.tolist() == [min(int(math.floor((v - lo) * inv)), n - 1) for v in just_below]
        assert np.all((got == np.arange(0, n - 1)) | (got == np.arange(1, n)))
    # a product that rounds up to n stays in the last bin
    lo, hi, n = 0.0, pref.PI, 180
    v = math.nextafter(hi, -INF)
    assert pref.bins([v], lo, hi, float(n) / hi, n).tolist() == [n - 1]


def test_closure_on_vectors_this_stage_did_not_make():
    """The reference-generated four-vectors of tests/golden/kinematics.npz: the Ex made from row 2 is the invariant
    mass of row 3 less the residual's mass, within the bound of Ex."""
    kin = np.load(rc.GOLDEN / "kinematics.npz")
    checked = 0
    for key in ("be10dp_inverse", "o16aa_a12c", "c12dp"):
        masses, beam, p4, status = kin[f"{key}_masses"][:4], kin[f"{key}_beam"], kin[f"{key}_p4"], kin[f"{key}_status"]
        ok = status == 0
        s = pref.Settings(masses, 1, float(beam[0]))
        ex, theta, _ = pref.value(s, beam[ok], p4[ok, 2, 0], p4[ok, 2, 1], p4[ok, 2, 2])
        r = p4[ok, 3]
        want = np.sqrt(r[:, 3] ** 2 - (r[:, 0] ** 2 + r[:, 1] ** 2 + r[:, 2] ** 2)) - masses[3]
        e = beam[ok] + masses[1] + masses[0]
        bound = K_EX * U * e * e / masses[3]  # (measured: 1.32, 1.40 and 2.33 of the scale on the three sets)
        print(key, int(ok.sum()), float(np.max(np.abs(ex - want) / (U * e * e / masses[3]))))
        assert np.all(np.abs(ex - want) <= bound), key
        assert np.allclose(want, kin[f"{key}_ex"][ok, 0], atol=1e-6) and np.all((theta >= 0) & (theta <= pref.PI))
        # and observed from the other side: row 3 gives the ejectile's excitation (none) and the same angle
        s3 = pref.Settings(masses, 1, float(beam[0]), observed_row=3)
        quiet = ok & (np.abs(kin[f"{key}_ex"][:, 0]) < 1e-12)
        if quiet.any():
            ex3, theta3, _ = pref.value(s3, beam[quiet], p4[quiet, 3, 0], p4[quiet, 3, 1], p4[quiet, 3, 2])
            th2 = pref.value(s, beam[quiet], p4[quiet, 2, 0], p4[quiet, 2, 1], p4[quiet, 2, 2])[1]
            assert np.all(np.abs(ex3) < 1e-6) and np.allclose(theta3, th2, atol=1e-7)
        checked += int(ok.sum())
    assert checked > 300


# ------------------------------------------------------------------------------------------ the cases and the mutants ----
def _cases():
    cases = {"fit": rc.make(130, 8), "estimate, twice, row 3": rc.make(65, 8, pref.FROM_ESTIMATE, "twice", observed_row=3),
             "o16aa, no target": rc.make(64, 2, reaction="o16aa", target="none", track=1), "edges": rc.edge_case()}
    for i, variant in enumerate(rc.edge_variants(rc.edge_case())):
        cases[f"edges {i}"] = variant
    return cases


def test_restatement_on_every_case():
    """What must hold of any result."""
    seen = 0
    for name, case in _cases().items():
        rec, cells = rc.reference(case)
        s = case.settings
        seen |= int(np.bitwise_or.reduce(rec["status"]))
        plane = s.n_ex * s.n_theta
        truth, both, reco, resp, outside = (cells[:plane], cells[plane:2 * plane], cells[2 * plane:3 * plane],
                                            cells[3 * plane:3 * plane + s.n_ex ** 2], cells[-3:])
        has_truth, good = (rec["status"] & pref.NO_TRUTH) == 0, rec["status"] == 0
        assert truth.sum() + outside[0] == has_truth.sum() and reco.sum() + outside[1] == good.sum() == resp.sum() + outside[2], name
        assert np.all(both <= truth) and both.sum() <= good.sum(), name
        assert np.all(np.isnan(rec["ex"]) == ((rec["status"] & (pref.NO_TRACK | pref.UNPHYSICAL)) != 0)), name
        assert np.all(np.isnan(rec["truth_ex"]) == ~has_truth) and np.all(rec["reserved"] == 0.0), name
        assert np.all(np.isnan(rec["beam_ke"]) == ((rec["status"] & pref.NO_TRACK) != 0)), name
        assert np.all((rec["slot"] >= -1) & (rec["slot"] < (case.fits if case.fits is not None else case.estimates).shape[1])), name
    assert seen == 15  # every status bit


@pytest.mark.parametrize("mutant", pref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(mutant):
    caught = []
    for name, case in _cases().items():
        rec, cells = rc.reference(case)
        mrec, mcells = rc.reference(case, mutant)
        if not (pref.same(rec, mrec) and np.array_equal(cells, mcells)):
            caught.append(name)
    print(mutant, "differs on", caught)
    assert caught, mutant
    if mutant in ("classical beam momentum", "no energy loss", "sign of pz", "masses swapped"):
        # ... and the exact fixture catches the arithmetic ones far outside the bound
        z = rc.fixture()
        c = z["be10dp_long_row2"]
        s = rc.base_settings("be10dp", "long")
        ex = pref.value(s, pref.beam_ke(s, c[:, 0], mutant), c[:, 1], c[:, 2], c[:, 3], mutant)[0]
        with np.errstate(invalid="ignore"):
            assert not np.all(np.abs(ex - c[:, 5]) <= K_EX * c[:, 7]), mutant


def _hand_counted():
    """Four records whose cells are counted by hand: 4 Ex bins of 2 MeV over 0 .. 8, 2 theta_cm bins of pi / 2.
    The cells: truth [4][2] at 0, truth_reconstructed at 8, reconstructed at 16, ex_response [truth 4][reconstructed 4]
    at 24, outside at 40."""
    s = pref.Settings([1.0, 1.0, 1.0, 1.0], 1, 1.0, ex_lo=0.0, ex_hi=8.0, n_ex=4, n_theta=2)
    rec = np.zeros(4, dtype=pref.REACTION_DTYPE)
    #                 status         Ex   theta   truth Ex, theta
    rows = [(0,             5.0, 2.0,    1.0, 0.5),   # bins: reconstructed (2, 1), truth (0, 0) -> response [0][2]
            (pref.NO_TRACK, NAN, NAN,    3.0, 2.0),   # thrown, not reconstructed: truth (1, 1) alone
            (0,             8.0, 0.5,    1.0, 0.5),   # Ex at hi: outside for reconstructed and response, truth (0, 0)
            (0,             3.4, 0.5,    7.9, 3.0)]   # 3.4 / 2 = 1.7: bin 1 by floor (2 by rounding); truth (3, 1)
    for i, (status, ex, theta, truth_ex, truth_theta) in enumerate(rows):
        rec[i]["status"], rec[i]["ex"], rec[i]["theta_cm"] = status, ex, theta
        rec[i]["truth_ex"], rec[i]["truth_theta_cm"] = truth_ex, truth_theta
    want = np.zeros(s.n_cells, dtype=np.uint64)
    assert s.n_cells == 43
    want[0 * 2 + 0] = 2               # truth (0, 0): records 0 and 2
    want[1 * 2 + 1] = 1               # truth (1, 1): record 1
    want[3 * 2 + 1] = 1               # truth (3, 1): record 3
    want[8 + 0 * 2 + 0] = 2           # truth_reconstructed (0, 0): records 0 and 2 (status 0; binned at the TRUTH)
    want[8 + 3 * 2 + 1] = 1           # ... and (3, 1): record 3
    want[16 + 2 * 2 + 1] = 1          # reconstructed (2, 1): record 0
    want[16 + 1 * 2 + 0] = 1          # reconstructed (1, 0): record 3
    want[24 + 0 * 4 + 2] = 1          # ex_response [truth 0][reconstructed 2]: record 0
    want[24 + 3 * 4 + 1] = 1          # ex_response [truth 3][reconstructed 1]: record 3
    want[40 + 1] = 1                  # outside of reconstructed: record 2
    want[40 + 2] = 1                  # outside of ex_response: record 2
    return s, rec, want


def test_cells_counted_by_hand():
    """The layout and the orientation of the spectra against an expectation written down cell by cell, not against the
    restatement itself; each of the four mutants that are not arithmetic fails it."""
    s, rec, want = _hand_counted()
    assert pref.cells(s, rec).tolist() == want.tolist()
    for mutant in ("round for floor", "hi inclusive", "truth of the reconstructed only", "response transposed"):
        assert pref.cells(s, rec, mutant).tolist() != want.tolist(), mutant
    spectra = ReactionSpectra(ReactionSettings([1.0] * 4, 1, 1.0, ex_range=(0.0, 8.0), ex_bins=4, theta_bins=2), want)
    assert spectra.ex_response[0, 2] == 1 and spectra.ex_response[2, 0] == 0 and spectra.ex_response[3, 1] == 1  # [truth][reconstructed]
    assert spectra.truth[0, 0] == 2 and spectra.truth_reconstructed[0, 0] == 2 and spectra.reconstructed[2, 1] == 1
    assert spectra.outside.tolist() == [0, 1, 1] and spectra.efficiency()[1, 1] == 0.0 and spectra.efficiency()[0, 0] == 1.0


# ------------------------------------------------------------------------------------------ the host code alone ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "reaction_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _head(s: pref.Settings, **change) -> np.ndarray:
    eloss = [] if s.eloss is None else list(s.eloss)
    words = {"masses": list(s.masses[:4]), "beam_energy": s.beam_energy, "z_min": s.z_min, "z_max": s.z_max, "ex_lo": s.ex_lo,
             "ex_hi": s.ex_hi, "ex_inv_width": s.ex_inv_width, "theta_inv_width": s.theta_inv_width, "eloss_len": len(eloss),
             "has_target": int(s.eloss is not None), "charge": s.charge, "track": s.track, "observed_row": s.observed_row,
             "source": s.source, "n_ex": s.n_ex, "n_theta": s.n_theta, "reserved": 0}
    eloss = change.pop("eloss", eloss)
    words.update(change)
    flat = words.pop("masses") + list(words.values())
    return np.array(flat + list(eloss), dtype=np.float64)


def _run(exe: Path, tmp: Path, what: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), what, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _native(exe, tmp, case: rc.Case):
    s = case.settings
    src = case.fits if case.fits is not None else case.estimates
    n, n_sim = src.shape
    if case.fits is not None:
        slots = np.concatenate([src["status"][..., None].astype(np.float64), src["g"], src["vertex"][..., 2:3]], axis=-1)
    else:
        slots = np.stack([src["status"].astype(np.float64), src["brho"], src["slope"], src["vz"], np.zeros((n, n_sim))], axis=-1)
    parts = [slots.reshape(n, -1)]
    if case.pid is not None:
        parts.append(case.pid["position"].astype(np.float64))
    parts += [case.p4.reshape(n, -1), case.vertex, case.status[:, None].astype(np.float64)]
    words = np.concatenate([_head(s), [n_sim, case.p4.shape[1], n, float(case.pid is not None)], np.concatenate(parts, axis=1).ravel()])
    out = _run(exe, tmp, "records", words)
    table, cells = out[:8 * n].reshape(n, 8), out[8 * n:]
    rec = np.zeros(n, dtype=pref.REACTION_DTYPE)
    rec["status"], rec["slot"] = table[:, 0].astype(np.int32), table[:, 1].astype(np.int32)
    for k, name in enumerate(("beam_ke", "ex", "theta_cm", "truth_beam_ke", "truth_ex", "truth_theta_cm")):
        rec[name] = table[:, 2 + k]
    return rec, cells.astype(np.uint64)


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reaction")
    exe = tmp / "reaction_check"
    _build(exe, ["-O2"])
    return exe, tmp


def _all_cases():
    yield from _cases().items()
    for n in (1, 65):
        for n_sim in (1, 8):
            for mode in rc.PID_MODES:
                for source in (pref.FROM_FIT, pref.FROM_ESTIMATE):
                    yield f"{n} x {n_sim}, pid {mode}, source {source}", rc.make(n, n_sim, source, mode)
    yield "one cell", rc.make(130, 8, cells="one", flags=False)
    yield "own cells", rc.make(130, 8, cells="own", flags=False)
    yield "estimate edges", rc.edge_case(pref.FROM_ESTIMATE)


def test_host_form_equals_the_restatement(native):
    exe, tmp = native
    for name, case in _all_cases():
        rec, cells = _native(exe, tmp, case)
        want, want_cells = rc.reference(case)
        assert pref.same(rec, want), (name, np.nonzero(rec != want)[0][:5])
        assert np.array_equal(cells, want_cells), name
    for lo, hi, n in ((-2.0, 14.0, 64), (0.0, pref.PI, 180), (0.1, 0.7, 7)):
        inv = float(n) / (hi - lo)
        values = np.array([lo, math.nextafter(hi, -INF), hi, NAN, -INF, INF] + [lo + k / inv for k in range(n + 1)])
        got = _run(exe, tmp, "bins", np.concatenate([_head(rc.base_settings()), [n, lo, hi, inv, len(values)], values]))
        assert got.astype(np.int64).tolist() == pref.bins(values, lo, hi, inv, n).tolist()


def test_spectra_of_one_cell_and_of_own_cells():
    one = rc.make(130, 8, cells="one", flags=False)
    rec, cells = rc.reference(one)
    spectra = ReactionSpectra(rc.to_settings(one.settings), cells)
    assert np.all(rec["status"] == 0) and spectra.truth.max() == spectra.reconstructed.max() == spectra.ex_response.max() == 130
    assert not spectra.outside.any() and np.count_nonzero(spectra.cells) == 4
    own = rc.make(130, 8, cells="own", flags=False)
    rec, cells = rc.reference(own)
    spectra = ReactionSpectra(rc.to_settings(own.settings), cells)
    assert np.all(rec["status"] == 0) and spectra.truth.max() == 1 and spectra.truth.sum() == 130 == np.count_nonzero(spectra.reconstructed)
    assert np.array_equal(spectra.truth, spectra.reconstructed) and np.array_equal(spectra.truth, spectra.truth_reconstructed)
    eff = spectra.efficiency()
    assert np.all(eff[spectra.truth > 0] == 1.0) and np.all(np.isnan(eff[spectra.truth == 0]))


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone executable."""
    exe = tmp_path / "reaction_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for name, case in _all_cases():
        rec, cells = _native(exe, tmp_path, case)
        want, want_cells = rc.reference(case)
        assert pref.same(rec, want) and np.array_equal(cells, want_cells), name
    # vertices far outside the table, and values no int holds
    wild = rc.make(16, 1, flags=False)
    wild.fits["vertex"][:, 0, 2] = [1e300, -1e300, 1e12, -1e12, 3e9, -3e9, 2147483.648e3, 0.0, 1000.0, 999.9999999999999, INF, -INF,
                                     NAN, 1e-300, -1e-300, 5e-324]
    wild.vertex[:, 2] = wild.fits["vertex"][:, 0, 2] / 1000.0
    rec, cells = _native(exe, tmp_path, wild)
    want, want_cells = rc.reference(wild)
    assert pref.same(rec, want) and np.array_equal(cells, want_cells)
    for change in BAD_DESCS:
        assert _run(exe, tmp_path, "desc", _head(rc.base_settings(), **change)).tolist() == [1.0], change


# ------------------------------------------------------------------------------------------ the settings' checks ----
BAD_DESCS = [{"masses": [0.0, 1.0, 1.0, 1.0]}, {"masses": [1.0, 1.0, NAN, 1.0]}, {"masses": [1.0, INF, 1.0, 1.0]}, {"beam_energy": 0.0},
             {"beam_energy": NAN}, {"has_target": 2}, {"z_max": 0.0}, {"z_min": NAN}, {"eloss_len": 1}, {"eloss_len": 65537},
             {"eloss": [0.0, NAN], "eloss_len": 2}, {"has_target": 0}, {"charge": 0}, {"track": 8}, {"track": -1}, {"observed_row": 1},
             {"observed_row": 4}, {"source": 2}, {"n_ex": 0}, {"n_ex": 257}, {"n_theta": 181}, {"n_theta": 0}, {"ex_hi": -2.0},
             {"ex_lo": NAN}, {"ex_inv_width": 4.000000000000001}, {"ex_inv_width": NAN}, {"theta_inv_width": 11.0}, {"reserved": 1}]
GOOD_DESCS = [{}, {"observed_row": 3}, {"source": 1}, {"track": 7}, {"has_target": 0, "eloss_len": 0, "eloss": []},
              {"n_ex": 256, "ex_inv_width": 16.0}, {"n_theta": 180, "theta_inv_width": 180.0 / pref.PI}]


def test_host_desc_checks(native):
    exe, tmp = native
    for change in GOOD_DESCS:
        assert _run(exe, tmp, "desc", _head(rc.base_settings(), **change)).tolist() == [0.0], change
    for change in BAD_DESCS:
        assert _run(exe, tmp, "desc", _head(rc.base_settings(), **change)).tolist() == [1.0], change


def test_settings_and_spectra():
    masses = rc.fixture()["be10dp_masses"]
    good = dict(masses=masses, charge=1, beam_energy=93.0, target=(0.0, 1.0, np.linspace(0.0, 20.0, 33)))
    s = ReactionSettings(**good)
    d = s.desc()
    assert (d.n_ex, d.n_theta, d.track, d.observed_row, d.source, d.has_target, d.eloss_len, d.reserved) == (64, 36, 0, 2, 0, 1, 33, 0)
    assert d.ex_inv_width == 4.0 and d.theta_inv_width == 36.0 / pref.PI and s.n_cells == 3 * 64 * 36 + 64 * 64 + 3
    assert np.ctypeslib.as_array(d.eloss, shape=(33,)).tolist() == s.eloss.tolist() and list(d.masses) == list(masses)
    assert pref.Settings.of(s).ex_inv_width == s.ex_inv_width and pref.Settings.of(s).n_cells == s.n_cells
    no_target = ReactionSettings(masses, 1, 93.0)
    assert (no_target.desc().has_target, no_target.desc().eloss_len) == (0, 0) and not no_target.desc().eloss
    assert s.token() == ReactionSettings(**good).token() != no_target.token()
    assert s.token() != ReactionSettings(**{**good, "target": (0.0, 1.0, np.linspace(0.0, 20.5, 33))}).token()
    for change in ({"masses": masses[:3]}, {"masses": [1.0, 1.0, -1.0, 1.0]}, {"masses": [1.0, 1.0, NAN, 1.0]}, {"charge": 0}, {"charge": 1.0},
                   {"charge": True}, {"beam_energy": 0.0}, {"beam_energy": INF}, {"beam_energy": "93"}, {"target": (1.0, 0.0, [0.0, 1.0])},
                   {"target": (0.0, 1.0, [0.0])}, {"target": (0.0, 1.0, [0.0, NAN])}, {"target": (0.0, 1.0, np.zeros(65537))},
                   {"track": 8}, {"track": -1}, {"track": 0.0}, {"observed_row": 1}, {"observed_row": 4}, {"observed_row": True},
                   {"source": "truth"}, {"source": 0}, {"ex_range": (1.0, 1.0)}, {"ex_range": (0.0, NAN)}, {"ex_bins": 0}, {"ex_bins": 257},
                   {"theta_bins": 181}, {"theta_bins": 0}, {"theta_bins": 36.0}):
        with pytest.raises(ValueError):
            ReactionSettings(**{**good, **change})
    s.check_indices([2, 3])
    ReactionSettings(**{**good, "track": 1, "observed_row": 3}).check_indices([2, 3])
    for bad_indices in ([3, 2], [4, 5], []):
        with pytest.raises(ValueError):
            s.check_indices(bad_indices)
    with pytest.raises(TypeError):
        rmod.configure_reaction(None, "settings")
    with pytest.raises(TypeError):
        rmod.records_to_reaction("settings", np.zeros((1, 4, 4)), np.zeros((1, 3)))
    with pytest.raises(ValueError):
        rmod.records_to_reaction(s, np.zeros((1, 4, 4)), np.zeros((1, 3)), estimates=np.zeros((1, 1), dtype=_abi.ESTIMATE_DTYPE))
    for bad in (dict(p4=np.zeros((1, 3, 4))), dict(p4=np.zeros((2, 4, 4))), dict(vertex=np.zeros((1, 2))), dict(status=np.zeros(2)),
                dict(pid=np.zeros((1, 2), dtype=_abi.PID_DTYPE)), dict(fits=np.zeros((1, 9), dtype=_abi.FIT_DTYPE)),
                dict(settings=ReactionSettings(**{**good, "track": 3}))):
        kw = {"settings": s, "p4": np.zeros((1, 4, 4)), "vertex": np.zeros((1, 3)), "fits": np.zeros((1, 1), dtype=_abi.FIT_DTYPE), **bad}
        with pytest.raises(ValueError):
            rmod.records_to_reaction(**kw)
    spectra = ReactionSpectra(s)
    assert spectra.truth.shape == spectra.reconstructed.shape == spectra.truth_reconstructed.shape == (64, 36)
    assert spectra.ex_response.shape == (64, 64) and spectra.outside.shape == (3,) and spectra.cells.dtype == np.uint64
    assert spectra.ex_edges[0] == -2.0 and spectra.ex_edges[-1] == 14.0 and len(spectra.ex_edges) == 65
    assert spectra.theta_edges[0] == 0.0 and abs(spectra.theta_edges[-1] - pref.PI) < 1e-15 and len(spectra.theta_edges) == 37
    a, b = ReactionSpectra(s, np.arange(s.n_cells)), ReactionSpectra(s, np.ones(s.n_cells))
    assert np.array_equal((a + b).cells, np.arange(s.n_cells) + 1) and (a + b) == (b + a) and a != b
    assert (a + b).truth.base is not None and np.array_equal((a + b).outside, a.outside + 1)
    with pytest.raises(ValueError):
        a + ReactionSpectra(no_target)
    with pytest.raises(ValueError):
        ReactionSpectra(s, np.zeros(5))
    assert np.isnan(ReactionSpectra(s).efficiency()).all()


def test_from_pipeline_takes_what_the_kinematics_upload():
    from tests.helpers import Inputs

    for name in ("be10dp", "o16aa"):
        inp = Inputs(name)
        kin = inp.kin
        for track, row in enumerate(inp.indices):
            if row not in (2, 3):
                with pytest.raises(ValueError):
                    ReactionSettings.from_pipeline(inp.pipeline, track=track, indices=inp.indices)
                continue
            s = ReactionSettings.from_pipeline(inp.pipeline, track=track, indices=inp.indices, source="estimate", ex_bins=32)
            assert s.masses == tuple(kin.masses[i] for i in range(4)) and s.beam_energy == kin.beam_energy
            assert (s.observed_row, s.charge, s.track, s.source, s.ex_bins) == (row, int(inp.z[row]), track, "estimate", 32)
            assert bool(kin.has_target) == (s.eloss is not None)
            if kin.has_target:
                assert (s.z_min, s.z_max) == (kin.z_min, kin.z_max)
                assert s.eloss.tolist() == np.ctypeslib.as_array(kin.eloss, shape=(kin.eloss_len,)).tolist()
