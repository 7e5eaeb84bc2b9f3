"""The exact kinematics reference (tests/kin_exact_reference.py, mpmath) checked against itself, the committed
fixture against its generator, the CPU oracle against the fixture, and the comparison against wrong formulas.
No GPU."""
import numpy as np
import pytest
from mpmath import mp, mpf

from attpc_engine_amd import _abi, nuclear_map
from oracle import pyoracle as orc
from tests import kin_exact_check as chk
from tests import kin_exact_reference as ref


@pytest.fixture(scope="module")
def fx(golden_dir):
    return chk.load(golden_dir)


@pytest.fixture(scope="module")
def regenerated():
    return ref.build_fixture()


# ------------------------------------------------------------------ the fixture ----------------
def test_fixture_regenerates_exactly(fx, regenerated, golden_dir):
    assert sorted(fx) == sorted(regenerated)
    for key, val in regenerated.items():
        assert fx[key].dtype == val.dtype and fx[key].shape == val.shape, key
        assert fx[key].tobytes() == np.ascontiguousarray(val).tobytes(), key  # NaN payloads and signed zeros included
    largest = max(p.stat().st_size for p in golden_dir.glob("*.npz") if p.name != "kin_exact.npz")
    assert (golden_dir / "kin_exact.npz").stat().st_size <= largest


def test_fixture_case_counts(fx):
    classes = [str(c) for c in fx["classes"]]
    names = [str(n) for n in fx["chains"]] + [str(n) for n in fx["decay_sets"]]
    counts = {c: sum(int((fx[f"{n}_class"] == i).sum()) for n in names) for i, c in enumerate(classes)}
    assert counts == chk.EXPECTED_CASES
    sizes = [len(fx[f"{n}_class"]) for n in names]
    assert max(sizes) <= 600 and any(s > 256 and s % 256 for s in sizes)
    assert len(fx["mg24_chain8_class"]) <= 40
    assert (fx["mg24_chain8_status"] == 0).sum() >= 8  # the eight-step chain at full depth
    for n in names:  # every hair set straddles the exact threshold (not 32 : 32, the f64 sum m1 + m2 is itself rounded)
        hair = fx[f"{n}_class"] == classes.index("hair")
        if hair.any():
            q = fx[f"{n}_q"][hair, 0]
            assert hair.sum() == 64 and (q > 0).sum() >= 24 and (q <= 0).sum() >= 24 and (np.diff(q) < 0).all(), n


# ------------------------------------------------------------------ the reference against itself ----
def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), mpf(1))


SELF_CHECK_STEPS = [  # (parent momentum, parent mass, m_a, m_b, th, ph)
    ((0.0, 0.0, 385.5), 14904.665, 3727.379, 11174.86, 1.0, 2.0),
    ((0.0, 0.0, 0.0), 14904.665, 3727.379, 11174.86, 0.3, -1.0),
    ((212.3, -97.1, 1106.9), 14917.2, 3727.379, 11174.86 + 4.44, 2.2, 5.5),
    ((-31.0, 64.0, 5.0), 8400.0, 938.272, 7456.89, 3.1, 0.1),
    ((212.3, -97.1, 1106.9), 14902.239 + 1e-7, 3727.379, 11174.86, 1.0, 2.0),  # 1e-7 MeV above the threshold
    ((0.0, 0.0, 23000.0), 24200.0, 938.272, 23252.0, 0.7, 4.0),  # the long chain's energies
]


@pytest.mark.parametrize("case", range(len(SELF_CHECK_STEPS)))
def test_reference_invariants(case):
    momentum, m_parent, m_a, m_b, th, ph = SELF_CHECK_STEPS[case]
    with mp.workdps(ref.DPS):
        tol = mpf(10) ** -40
        parent = [mpf(v) for v in momentum]
        parent.append(mp.sqrt(mpf(m_parent) ** 2 + sum(v ** 2 for v in parent)))
        m_a, m_b, th, ph = mpf(m_a), mpf(m_b), mpf(th), mpf(ph)
        a, b, e_a, p_star, _ = ref.exact_step(parent, m_a, m_b, th, ph)
        m_parent = ref.mass(parent)
        assert _rel(ref.mass(a), m_a) < tol and _rel(ref.mass(b), m_b) < tol            # mass shells
        assert all(_rel(a[i] + b[i], parent[i]) < tol for i in range(4))                # a + b = P
        dot = a[3] * parent[3] - sum(a[i] * parent[i] for i in range(3))
        assert _rel(dot / m_parent, e_a) < tol                                           # energy of a in P's rest frame
        if parent[0] == 0 and parent[1] == 0:
            gam, beta = parent[3] / m_parent, parent[2] / parent[3]
            assert _rel(a[2], gam * (p_star * mp.cos(th) + beta * e_a)) < tol            # textbook boost along z
            turn = (mp.atan2(a[1], a[0]) - ph) / (2 * mp.pi)
            assert abs(turn - mp.nint(turn)) < tol                                       # azimuth, mod 2 pi


def test_reference_lise_known_answer():
    """12C(d,p) at 16 MeV, 20 degrees in the centre of mass: 18.391 MeV (the reference's tests/test_kinematics.py)."""
    nm = nuclear_map
    masses = [nm.get_data(6, 12).mass, nm.get_data(1, 2).mass, nm.get_data(1, 1).mass, nm.get_data(6, 13).mass]
    out = ref.exact_chain(masses, 16.0, [0.0], [np.deg2rad(20.0)], [0.0])
    assert out["status"] == 0
    with mp.workdps(ref.DPS):
        ke = out["rows"][2][3] - mpf(float(masses[2]))
        assert mp.nint(ke * 1000) == 18391


# ------------------------------------------------------------------ the oracle against the fixture ----
def _kin_desc(masses):
    desc = _abi.KinDesc()
    desc.n_steps = 1 + (len(masses) - 4) // 2
    for i, m in enumerate(masses):
        desc.masses[i] = m
    return desc


def _oracle_chain(fx, name):
    return orc.kin_calculate(_kin_desc(fx[f"{name}_masses"]), fx[f"{name}_beam"], fx[f"{name}_ex"], fx[f"{name}_th"],
                             fx[f"{name}_ph"])


def _oracle_decays(fx, name):
    L = orc.lib()
    m1, m2 = (float(v) for v in fx[f"{name}_m"])
    parents, ex, th, ph = (np.ascontiguousarray(fx[f"{name}_{k}"]) for k in ("parent", "ex", "th", "ph"))
    p4 = np.full((len(ex), 2, 4), np.nan)
    status = np.ones(len(ex), dtype=np.int32)
    for i in range(len(ex)):
        parent = parents[i].copy()
        if L.orc_decay_allowed(orc.d(parent), m1, m2, ex[i]):
            out = np.empty((2, 4))
            L.orc_decay_calculate(orc.d(parent), m1, m2, th[i], ph[i], ex[i], orc.d(out))
            p4[i], status[i] = out, 0
    return p4, status


def test_oracle_against_exact(fx):
    """Decided cases: status equal and rows within 4 K S_row, bulk and angle also within 1e-9 MeV; hair cases: status 0
    means finite rows within the bound (before two_body clamped e_a^2 - m^2 at 0, o16_a12c held a status-0 case with
    NaN rows and this test failed on it)."""
    tally = chk.Tally()
    for name in fx["chains"]:
        chk.compare(fx, str(name), *_oracle_chain(fx, str(name)), chk.K_ORACLE, tally)
    for name in fx["decay_sets"]:
        chk.compare(fx, str(name), *_oracle_decays(fx, str(name)), chk.K_ORACLE, tally)
    tally.assert_complete()
    print(f"\noracle vs exact: largest error / S_row {tally.worst[0]:.4f} at {tally.worst[1]}; "
          f"largest bulk / angle error {tally.worst_plain[0]:.3e} MeV at {tally.worst_plain[1]}")


# ------------------------------------------------------------------ the comparison catches a wrong formula ----
def _boost(p, bx, by, bz, mutation):
    gam = 1.0 / np.sqrt(1.0 - (bx * bx + by * by + bz * bz))
    bgam = gam / (1.0 + gam) if mutation == "bgam" else gam * gam / (1.0 + gam)
    if mutation == "z_only":
        bx = by = 0.0
    x = (1.0 + bgam * bx * bx) * p[0] + bgam * bx * by * p[1] + bgam * bx * bz * p[2] + gam * bx * p[3]
    y = bgam * bx * by * p[0] + (1.0 + bgam * by * by) * p[1] + bgam * by * bz * p[2] + gam * by * p[3]
    z = bgam * bx * bz * p[0] + bgam * by * bz * p[1] + (1.0 + bgam * bz * bz) * p[2] + gam * bz * p[3]
    return np.array([x, y, z, gam * (bx * p[0] + by * p[1] + bz * p[2]) + gam * p[3]])


def _two_body(parent, m_out, m_other, ex, polar, azim, mutation=None):
    """kinematics.hip's two_body in numpy f64, with one deliberate mistake if ``mutation`` names it."""
    bx, by, bz = parent[:3] / parent[3]
    ecm = _boost(parent, -bx, -by, -bz, mutation)[3]
    mo = m_other if mutation == "no_ex" else m_other + ex
    e_a = (m_out * m_out - mo * mo + ecm * ecm) / (2.0 * ecm)
    d = e_a * e_a - m_out * m_out
    p_a = np.sqrt(0.0 if d < 0.0 else d)
    if mutation == "azimuth_sign":
        azim = -azim
    cm = np.array([p_a * np.sin(polar) * np.cos(azim), p_a * np.sin(polar) * np.sin(azim), p_a * np.cos(polar), e_a])
    back = -1.0 if mutation == "boost_back_minus_beta" else 1.0
    a = _boost(cm, back * bx, back * by, back * bz, mutation)
    return a, parent - a


def _inv_mass(p):
    m2 = p[3] * p[3] - (p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    return np.sqrt(m2) if m2 >= 0.0 else -np.sqrt(-m2)


def _numpy_chain(fx, name, mutation):
    m = fx[f"{name}_masses"]
    n_steps = 1 + (len(m) - 4) // 2
    beam, ex, th, ph = (fx[f"{name}_{k}"] for k in ("beam", "ex", "th", "ph"))
    p4 = np.full((len(beam), len(m), 4), np.nan)
    status = np.zeros(len(beam), dtype=np.int32)
    for i, t in enumerate(beam):
        pz = np.sqrt(t * (t + 2.0 * m[1]))
        s = m[0] + t + m[1]
        if not (m[2] + m[3] + ex[i, 0]) < np.sqrt(s * s - pz * pz):
            status[i] = 1
            continue
        if t < -(m[0] + m[1] - (m[2] + m[3] + ex[i, 0])) * (m[2] + m[3]) / (m[2] + m[3] - m[1]):
            status[i] = -1
            continue
        p4[i, 0], p4[i, 1] = [0.0, 0.0, 0.0, m[0]], [0.0, 0.0, pz, t + m[1]]
        p4[i, 2], p4[i, 3] = _two_body(p4[i, 0] + p4[i, 1], m[2], m[3], ex[i, 0], th[i, 0], ph[i, 0], mutation)
        for k in range(1, n_steps):
            prev, m1, m2 = p4[i, 3 + 2 * (k - 1)], m[4 + 2 * (k - 1)], m[5 + 2 * (k - 1)]
            if not (_inv_mass(prev) - (m1 + m2 + ex[i, k])) > 0.0:
                status[i] = k + 1
                break
            p4[i, 4 + 2 * (k - 1)], p4[i, 5 + 2 * (k - 1)] = _two_body(prev, m1, m2, ex[i, k], th[i, k], ph[i, k], mutation)
    return p4, status


def _numpy_decays(fx, name, mutation):
    m1, m2 = fx[f"{name}_m"]
    parents, ex, th, ph = (fx[f"{name}_{k}"] for k in ("parent", "ex", "th", "ph"))
    p4 = np.full((len(ex), 2, 4), np.nan)
    status = np.ones(len(ex), dtype=np.int32)
    for i in range(len(ex)):
        if (_inv_mass(parents[i]) - (m1 + m2 + ex[i])) > 0.0:
            p4[i, 0], p4[i, 1] = _two_body(parents[i], m1, m2, ex[i], th[i], ph[i], mutation)
            status[i] = 0
    return p4, status


def _restatement_passes(fx, mutation, chains=None, decay_sets=None):
    tally = chk.Tally()
    try:
        with np.errstate(invalid="ignore"):
            for name in fx["chains"] if chains is None else chains:
                chk.compare(fx, str(name), *_numpy_chain(fx, str(name), mutation), chk.K_ORACLE, tally)
            for name in fx["decay_sets"] if decay_sets is None else decay_sets:
                chk.compare(fx, str(name), *_numpy_decays(fx, str(name), mutation), chk.K_ORACLE, tally)
    except AssertionError:
        return False
    return True


def test_restatement_passes_as_written(fx):
    assert _restatement_passes(fx, None)


@pytest.mark.parametrize("mutation", ["azimuth_sign", "no_ex", "boost_back_minus_beta", "bgam", "z_only"])
def test_comparison_catches_a_wrong_formula(fx, mutation):
    assert not _restatement_passes(fx, mutation)


def test_only_the_decays_see_a_boost_along_z_alone(fx):
    """A boost that drops the parent's x and y is right for every reaction (the beam flies along z): the one-step
    chains pass, and it is the decays of parents off the z axis, chained and explicit, that catch it."""
    assert _restatement_passes(fx, "z_only", chains=["c12dp", "be10dp_inverse"], decay_sets=[])
    assert not _restatement_passes(fx, "z_only", chains=["o16aa_a12c"], decay_sets=[])
    assert not _restatement_passes(fx, "z_only", chains=[], decay_sets=["o16_a12c"])
