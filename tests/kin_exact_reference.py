"""Exact two-body kinematics (mpmath, 60 digits) and the cases of ``tests/golden/kin_exact.npz``.

The reference of the kinematics kernels that shares no formula with them.  A step is solved from invariants and
carried to the lab by the rotation-free boost written with the parent's direction n, gamma = E / M and
beta gamma = |p| / M -- no velocity, no 1 / sqrt(1 - beta^2), no boost matrix:

    M     = sqrt(P.P)                         E*_a = (M^2 + m_a^2 - m_b^2) / 2M          p* = sqrt(E*_a^2 - m_a^2)
    q     = p* (sin th cos ph, sin th sin ph, cos th)
    a_vec = q + [(gamma - 1)(q.n) + beta gamma E*_a] n                  a_t = gamma E*_a + beta gamma (q.n)
    b     = P - a                             (a parent at rest: a = (q, E*_a))

Every f64 input is taken as exact: the masses, the beam energy, the angles (f64(pi) is not pi), the excitations and
the parent rows given to the decay entry; m_b = m_other + ex is the exact sum.

``python tests/kin_exact_reference.py`` writes the fixture; ``tests/kin_exact_check.py`` (numpy only) reads it."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

GOLDEN = Path(__file__).resolve().parent / "golden"
DPS = 60
CLASSES = ("bulk", "angle", "energy", "threshold", "hair")
U = mpf(2) ** -53


def exact(fn):
    """Run ``fn`` at 60 digits whatever precision the caller works at."""
    @functools.wraps(fn)
    def run(*args, **kw):
        with mp.workdps(DPS):
            return fn(*args, **kw)
    return run


def _x(v) -> mpf:
    return mpf(float(v))  # an f64 is a dyadic rational: exact in mpf


def mass(p):
    return mp.sqrt(p[3] ** 2 - (p[0] ** 2 + p[1] ** 2 + p[2] ** 2))


@exact
def exact_step(parent, m_a, m_b, th, ph, at_threshold: bool = False):
    """-> (a, b, E*_a, p*, conditioning).  ``conditioning`` = max(1, E*_a / p*, E*_b / p*): what the rounding of the
    parent's mass is multiplied by on its way into p*.  ``at_threshold``: a step that is exactly forbidden
    (E*_a^2 < m_a^2) gives the rows of p* = 0 -- both products at the parent's velocity -- and the conditioning of the
    mirrored p* = sqrt(m_a^2 - E*_a^2); without it such a step is an error."""
    px, py, pz, e = parent
    p2 = px ** 2 + py ** 2 + pz ** 2
    m2 = e ** 2 - p2
    m = mp.sqrt(m2)
    e_a = (m2 + m_a ** 2 - m_b ** 2) / (2 * m)
    d = e_a ** 2 - m_a ** 2
    if d < 0 and not at_threshold:
        raise ValueError("forbidden step")
    p_star = mp.sqrt(d) if d > 0 else mpf(0)
    p_cond = mp.sqrt(abs(d))
    cond = max(mpf(1), e_a / p_cond, (m - e_a) / p_cond) if p_cond > 0 else mp.inf
    q = [p_star * mp.sin(th) * mp.cos(ph), p_star * mp.sin(th) * mp.sin(ph), p_star * mp.cos(th)]
    if p2 == 0:
        a = q + [e_a]
    else:
        p = mp.sqrt(p2)
        n = [px / p, py / p, pz / p]
        gam, bg = e / m, p / m
        qn = q[0] * n[0] + q[1] * n[1] + q[2] * n[2]
        k = (gam - 1) * qn + bg * e_a
        a = [q[i] + k * n[i] for i in range(3)] + [gam * e_a + bg * qn]
    b = [parent[i] - a[i] for i in range(4)]
    return a, b, e_a, p_star, cond


def band(e_parent, m_parent):
    """Width of the excitations whose allowed / forbidden decision f64 cannot make: four roundings of at most
    2^-53 E^2 in m^2, divided by 2M, doubled."""
    return 8 * U * e_parent ** 2 / m_parent


@exact
def exact_chain(masses, beam, ex, th, ph, at_threshold: bool = False):
    """The deterministic map of ``kin_calculate_kernel`` in exact arithmetic -> dict with
    ``rows``   [R][4] mpf, None from the first forbidden step on (all rows if the reaction is forbidden);
    ``q``      per step M_parent - (m1 + m2 + ex) (step 0: E_cm - (m2 + m3 + ex)), None past a forbidden step;
    ``scale``  per row S_row = sum over the steps up to the row's own of 2^-53 E_parent(lab) conditioning(step);
               rows 0 and 1 are inputs of step 0 and take 2^-53 E_parent alone;
    ``status`` 0, 1 (reaction forbidden), -1 (allowed, below the non-relativistic threshold of
               reaction.py:136-143) or s + 1 for the first forbidden decay s;
    ``bands``  per step the f64 decision band of that step (None past a forbidden step)."""
    m = [_x(v) for v in masses]
    n_steps = 1 + (len(m) - 4) // 2
    ex, th, ph = ([_x(v) for v in np.atleast_1d(arr)] for arr in (ex, th, ph))
    t = _x(beam)
    n_rows = len(m)
    out = {"rows": [None] * n_rows, "q": [None] * n_steps, "scale": [None] * n_rows, "status": 0,
           "bands": [None] * n_steps}
    target = [mpf(0), mpf(0), mpf(0), m[0]]
    proj = [mpf(0), mpf(0), mp.sqrt(t * (t + 2 * m[1])), t + m[1]]
    parent = [target[i] + proj[i] for i in range(4)]
    out["q"][0] = mass(parent) - (m[2] + m[3] + ex[0])
    out["bands"][0] = band(parent[3], mass(parent))
    hair0 = at_threshold and abs(out["q"][0]) < 64 * out["bands"][0]
    if not out["q"][0] > 0:
        out["status"] = 1
        if not hair0:
            return out
    q_nr = m[0] + m[1] - (m[2] + m[3] + ex[0])
    if out["status"] == 0 and t < -q_nr * (m[2] + m[3]) / (m[2] + m[3] - m[1]):
        out["status"] = -1
        return out
    a, b, _, _, cond = exact_step(parent, m[2], m[3] + ex[0], th[0], ph[0], at_threshold=hair0)
    total = U * parent[3] * cond
    out["rows"][:4] = [target, proj, a, b]
    out["scale"][:4] = [U * parent[3], U * parent[3], total, total]
    if out["status"]:
        return out
    for s in range(1, n_steps):
        m1, m2 = m[4 + 2 * (s - 1)], m[5 + 2 * (s - 1)]
        parent = b
        out["q"][s] = mass(parent) - (m1 + m2 + ex[s])
        out["bands"][s] = band(parent[3], mass(parent))
        if not out["q"][s] > 0:
            out["status"] = s + 1
            return out
        a, b, _, _, cond = exact_step(parent, m1, m2 + ex[s], th[s], ph[s])
        total = total + U * parent[3] * cond
        out["rows"][4 + 2 * (s - 1): 6 + 2 * (s - 1)] = [a, b]
        out["scale"][4 + 2 * (s - 1): 6 + 2 * (s - 1)] = [total, total]
    return out


@exact
def exact_decay(parent, m1, m2, ex, th, ph, at_threshold: bool = False):
    """``decay_calculate_kernel`` for one explicit f64 parent row -> dict like ``exact_chain`` (rows [2][4])."""
    parent = [_x(v) for v in parent]
    m1, m2, ex, th, ph = _x(m1), _x(m2), _x(ex), _x(th), _x(ph)
    q = mass(parent) - (m1 + m2 + ex)
    bd = band(parent[3], mass(parent))
    out = {"rows": [None, None], "q": [q], "scale": [None, None], "status": 0 if q > 0 else 1, "bands": [bd]}
    hair = at_threshold and abs(q) < 64 * bd
    if out["status"] and not hair:
        return out
    a, b, _, _, cond = exact_step(parent, m1, m2 + ex, th, ph, at_threshold=hair)
    out["rows"] = [a, b]
    out["scale"] = [U * parent[3] * cond] * 2
    return out


# ------------------------------------------------------------------------------------------------- cases ----
F64_PI = float(np.pi)
POLAR_EDGES = (0.0, 1e-8, F64_PI / 2, F64_PI - 1e-8, F64_PI)
AZIMUTH_EDGES = (0.0, F64_PI, 2 * F64_PI, -1.0, 7.0)
CHAINS = ("c12dp", "o16aa_a12c", "b10_3he_chain", "be10dp_inverse", "mg24_chain8")
# projectile mass number and the beam energy (MeV) the golden cases of a chain are drawn around
PROJECTILE_A = {"c12dp": 2, "o16aa_a12c": 4, "b10_3he_chain": 3, "be10dp_inverse": 10, "mg24_chain8": 24}
NOMINAL_BEAM = {"c12dp": 16.0, "o16aa_a12c": 160.0, "b10_3he_chain": 24.0, "be10dp_inverse": 90.0, "mg24_chain8": 800.0}
MG24_NOMINAL_EX = (86.0, 76.0, 65.0, 51.0, 24.0, 20.0, 10.0, 0.0)
# every golden case of the chain whose launch is the one past 256 lanes, a part of the others (file size, run time)
BULK_STRIDE = {"c12dp": 1, "o16aa_a12c": 3, "b10_3he_chain": 3, "be10dp_inverse": 3, "mg24_chain8": 4}
MEV_PER_NUCLEON = (0.5, 2.0, 10.0, 30.0, 100.0)
CHAINED_Q = (1.0, 1e-2, 1e-4, 1e-6)          # a chained step decays the device's own parent: stop at 1e-6 MeV
EXPLICIT_Q = tuple(10.0 ** -k for k in range(10))  # all inputs explicit: on down to 16 bands (added per case)
HAIR_N = 64


def _f(v) -> float:
    return float(v)  # mpf -> nearest f64


@exact
def _ex_at(m_parent, m1, m2, q):
    """The f64 excitation that leaves ``q`` of the exact parent mass: f64(M - m1 - m2 - q)."""
    return _f(m_parent - _x(m1) - _x(m2) - q)


@exact
def _hair_excitations(m_parent, m1, m2):
    """64 excitations for which the f64 sum (m1 + m2) + ex, as the device forms it, takes 64 consecutive f64 values:
    32 at or below the exact parent mass and 32 above."""
    m12 = float(m1) + float(m2)
    top = _f(m_parent)
    if _x(top) > m_parent:
        top = float(np.nextafter(top, 0.0))
    sums = [top]
    for _ in range(HAIR_N // 2 - 1):
        sums.insert(0, float(np.nextafter(sums[0], 0.0)))
    for _ in range(HAIR_N // 2):
        sums.append(float(np.nextafter(sums[-1], np.inf)))
    exs = [_f(_x(s) - _x(m12)) for s in sums]
    assert [m12 + e for e in exs] == sums
    return exs


class _ChainCases:
    def __init__(self, name, masses):
        self.name, self.masses = name, np.asarray(masses, dtype=np.float64)
        self.n_steps = 1 + (len(masses) - 4) // 2
        self.beam, self.ex, self.th, self.ph, self.cls = [], [], [], [], []

    def add(self, cls, beam, ex, th, ph):
        ex, th, ph = (np.broadcast_to(np.asarray(v, dtype=np.float64), (self.n_steps,)).copy() for v in (ex, th, ph))
        for store, value in ((self.beam, float(beam)), (self.ex, ex), (self.th, th), (self.ph, ph), (self.cls, CLASSES.index(cls))):
            store.append(value)

    @exact
    def cm_energy(self, beam):
        m, t = [_x(v) for v in self.masses], _x(beam)
        return mp.sqrt((m[0] + t + m[1]) ** 2 - t * (t + 2 * m[1]))


class _DecayCases:
    def __init__(self, name, m1, m2):
        self.name, self.m = name, np.array([m1, m2], dtype=np.float64)
        self.parent, self.ex, self.th, self.ph, self.cls = [], [], [], [], []

    def add(self, cls, parent, ex, th, ph):
        for store, value in ((self.parent, np.asarray(parent, dtype=np.float64)), (self.ex, float(ex)), (self.th, float(th)),
                             (self.ph, float(ph)), (self.cls, CLASSES.index(cls))):
            store.append(value)


def _row(masses, beam, ex, th, ph, row):
    """An exact row of a chain, rounded to f64: an explicit parent for the decay entry."""
    return np.array([_f(v) for v in exact_chain(masses, beam, ex, th, ph)["rows"][row]])


@exact
def build_cases():
    """-> ([chain case sets], [decay case sets]); a pure function of ``kinematics.npz`` (masses and bulk inputs)."""
    g = np.load(GOLDEN / "kinematics.npz")
    chains = {}
    for name in CHAINS:
        c = chains[name] = _ChainCases(name, g[f"{name}_masses"])
        nominal_ex = MG24_NOMINAL_EX if name == "mg24_chain8" else (0.0,) * c.n_steps
        e0 = NOMINAL_BEAM[name]
        # bulk: the golden inputs themselves
        for i in range(0, len(g[f"{name}_beam"]), BULK_STRIDE[name]):
            c.add("bulk", g[f"{name}_beam"][i], g[f"{name}_ex"][i], g[f"{name}_th"][i], g[f"{name}_ph"][i])
        # energy: 0.5 .. 100 MeV per nucleon, excitation 0 (nominal cascade for the long chain) and -0.5 below it
        for per_nucleon in MEV_PER_NUCLEON:
            for shift in (0.0, -0.5):
                c.add("energy", per_nucleon * PROJECTILE_A[name], np.array(nominal_ex) + shift, 1.0, 2.0)
        # threshold, decided: the reaction step
        e_cm = c.cm_energy(e0)
        m_sum = c.masses[2], c.masses[3]
        q_list = list(EXPLICIT_Q if c.n_steps == 1 else CHAINED_Q)
        if c.n_steps == 1:
            q_list.append(16 * band(_x(c.masses[0]) + _x(e0) + _x(c.masses[1]), e_cm))
        if name == "mg24_chain8":
            q_list = q_list[::3]
        for q in q_list:
            for sign in (1, -1):
                ex = np.array(nominal_ex, dtype=np.float64)
                ex[0] = _ex_at(e_cm, *m_sum, sign * mpf(q))
                c.add("threshold", e0, ex, 1.0, 2.0)
        # threshold, decided: decay steps of the chains (the parent's mass is exactly m_residual + ex of the step before)
        first_ex = {"o16aa_a12c": 9.585, "b10_3he_chain": 4.0}.get(name, nominal_ex[0])
        for s in range(1, c.n_steps):
            if name == "mg24_chain8" and s not in (1, 4, 7):
                continue
            for q in (CHAINED_Q[::3] if name == "mg24_chain8" else CHAINED_Q):
                for sign in (1, -1):
                    ex = np.array(nominal_ex, dtype=np.float64)
                    ex[0] = first_ex
                    if name == "b10_3he_chain":
                        ex[1] = 1.0  # 9B*(4.0) -> a + 5Li*(1.0): 1.3 MeV to spare, and 5Li* -> a + p is open
                    m_parent = _x(c.masses[3 if s == 1 else 5 + 2 * (s - 2)]) + _x(ex[s - 1])
                    ex[s] = _ex_at(m_parent, c.masses[4 + 2 * (s - 1)], c.masses[5 + 2 * (s - 1)], sign * mpf(q))
                    c.add("threshold", e0, ex, [0.3] + [1.0] * (c.n_steps - 1), [0.5] + [2.0] * (c.n_steps - 1))
    # angles: the reaction of a one-step chain, and both steps of the two-step chain (parent of the decay well off z)
    for th in POLAR_EDGES:
        for ph in AZIMUTH_EDGES:
            chains["c12dp"].add("angle", 16.0, 0.0, th, ph)
            chains["o16aa_a12c"].add("angle", 160.0, [9.585, 0.0], [th, 1.0], [ph, 2.0])
            chains["o16aa_a12c"].add("angle", 160.0, [9.585, 0.0], [2.0, th], [0.5, ph])
    # hair: the reaction step of two chains, excitation by excitation through the exact threshold
    for name in ("c12dp", "be10dp_inverse"):
        c = chains[name]
        for ex in _hair_excitations(c.cm_energy(NOMINAL_BEAM[name]), c.masses[2], c.masses[3]):
            c.add("hair", NOMINAL_BEAM[name], ex, 1.0, 2.0)

    # ---- explicit parents for the decay entry: exact rows of the chains, rounded to f64 ----
    o16, b10, mg = (chains[k].masses for k in ("o16aa_a12c", "b10_3he_chain", "mg24_chain8"))
    sets = [
        # 16O*(9.585) -> a + 12C off the z axis: the parent on which the oracle returned NaN rows with status 0
        (_DecayCases("o16_a12c", o16[4], o16[5]), _row(o16, 160.0, [9.585, 0.0], [0.3, 1.0], [0.5, 2.0], 3)),
        (_DecayCases("b9_a5li", b10[4], b10[5]), _row(b10, 24.0, [4.0, 1.0, 0.0], [2.0, 1.0, 1.0], [0.5, 2.0, 2.0], 3)),
        (_DecayCases("li5_ap", b10[6], b10[7]), _row(b10, 24.0, [4.0, 1.0, 0.0], [2.0, 1.0, 1.0], [0.5, 2.0, 4.0], 5)),
        (_DecayCases("al26_p25mg", mg[4], mg[5]), _row(mg, 800.0, MG24_NOMINAL_EX, [2.5] + [1.0] * 7, [0.5] + [2.0] * 7, 3)),
    ]
    for dset, parent in sets:
        p = [_x(v) for v in parent]
        m_parent = mass(p)
        for q in list(EXPLICIT_Q) + [16 * band(p[3], m_parent)]:
            for sign in (1, -1):
                dset.add("threshold", parent, _ex_at(m_parent, *dset.m, sign * mpf(q)), 1.0, 2.0)
        for ex in _hair_excitations(m_parent, *dset.m):
            dset.add("hair", parent, ex, 1.0, 2.0)
    off_axis = _row(o16, 160.0, [9.585, 0.0], [2.0, 1.0], [0.5, 2.0], 3)
    at_rest = np.array([0.0, 0.0, 0.0, off_axis[3]])
    for th in POLAR_EDGES:
        for ph in AZIMUTH_EDGES:
            sets[0][0].add("angle", off_axis, 0.0, th, ph)
    for th, ph in ((0.0, 0.0), (1.0, 2.0), (F64_PI, -1.0)):
        sets[0][0].add("angle", at_rest, 0.0, th, ph)  # a parent at rest: no boost at all
    return list(chains.values()), [d for d, _ in sets]


def _pack(results, n_rows, n_steps):
    n = len(results)
    p4 = np.full((n, n_rows, 4), np.nan)
    scale = np.full((n, n_rows), np.nan)
    q = np.full((n, n_steps), np.nan)
    bands = np.full((n, n_steps), np.nan)
    status = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(results):
        status[i] = r["status"]
        for k, row in enumerate(r["rows"]):
            if row is not None:
                p4[i, k] = [_f(v) for v in row]
                scale[i, k] = _f(r["scale"][k])
        for s in range(n_steps):
            if r["q"][s] is not None:
                q[i, s], bands[i, s] = _f(r["q"][s]), _f(r["bands"][s])
    return p4, scale, q, bands, status


@exact
def build_fixture() -> dict:
    """Every array of ``kin_exact.npz``.  Per chain ``c`` (one ``attpc_kin_calculate`` launch): c_masses, c_beam [n],
    c_ex / c_th / c_ph [n, steps], c_p4 [n, rows, 4] (exact rows rounded to the nearest f64, NaN where there is none),
    c_scale [n, rows] (S_row), c_q / c_band [n, steps], c_status [n], c_class [n] (index into ``classes``).  Per
    explicit-parent set ``d`` (one ``attpc_decay_calculate`` launch): d_m [2], d_parent [n, 4], d_ex / d_th / d_ph [n],
    d_p4 [n, 2, 4], d_scale [n, 2], d_q / d_band [n, 1], d_status, d_class.  A hair case that is exactly forbidden
    keeps its nonzero status and holds the rows of p* = 0 (``exact_step(at_threshold=True)``)."""
    chains, decays = build_cases()
    out = {"classes": np.array(CLASSES), "chains": np.array([c.name for c in chains]),
           "decay_sets": np.array([d.name for d in decays])}
    hair = CLASSES.index("hair")
    for c in chains:
        res = [exact_chain(c.masses, c.beam[i], c.ex[i], c.th[i], c.ph[i], at_threshold=c.cls[i] == hair)
               for i in range(len(c.beam))]
        p4, scale, q, bands, status = _pack(res, len(c.masses), c.n_steps)
        for key, val in (("masses", c.masses), ("beam", np.array(c.beam)), ("ex", np.array(c.ex)), ("th", np.array(c.th)),
                         ("ph", np.array(c.ph)), ("p4", p4), ("scale", scale), ("q", q), ("band", bands),
                         ("status", status), ("class", np.array(c.cls, dtype=np.uint8))):
            out[f"{c.name}_{key}"] = val
    for d in decays:
        res = [exact_decay(d.parent[i], d.m[0], d.m[1], d.ex[i], d.th[i], d.ph[i], at_threshold=d.cls[i] == hair)
               for i in range(len(d.ex))]
        p4, scale, q, bands, status = _pack(res, 2, 1)
        for key, val in (("m", d.m), ("parent", np.array(d.parent)), ("ex", np.array(d.ex)), ("th", np.array(d.th)),
                         ("ph", np.array(d.ph)), ("p4", p4), ("scale", scale), ("q", q), ("band", bands),
                         ("status", status), ("class", np.array(d.cls, dtype=np.uint8))):
            out[f"{d.name}_{key}"] = val
    _check_decided(out)
    return out


def _check_decided(fx: dict) -> None:
    """A decided case stays 16 bands away from every threshold it passes, so f64 decides it as exact arithmetic does."""
    hair = CLASSES.index("hair")
    for name in list(fx["chains"]) + list(fx["decay_sets"]):
        decided = fx[f"{name}_class"] != hair
        q, bd = fx[f"{name}_q"][decided], fx[f"{name}_band"][decided]
        seen = ~np.isnan(q)
        assert (np.abs(q[seen]) >= 15.999 * bd[seen]).all(), name


if __name__ == "__main__":
    fixture = build_fixture()
    np.savez_compressed(GOLDEN / "kin_exact.npz", **fixture)
    total = 0
    for name in list(fixture["chains"]) + list(fixture["decay_sets"]):
        cls = fixture[f"{name}_class"]
        total += len(cls)
        print(name, len(cls), {c: int((cls == i).sum()) for i, c in enumerate(CLASSES) if (cls == i).any()},
              "statuses", sorted(set(fixture[f"{name}_status"].tolist())))
    print("cases", total, "bytes", (GOLDEN / "kin_exact.npz").stat().st_size)
