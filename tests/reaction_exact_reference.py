"""The reaction reconstruction in exact arithmetic (mpmath, 60 digits) and the cases of
``tests/golden/reaction_exact.npz``.

The contract's value -- beam energy at the vertex, missing mass, centre-of-mass angle -- as a function of f64 inputs,
every f64 taken as exact, evaluated without a rounding that matters; the angle from mpmath's atan2, not from the
written arctangent.  The inputs are made here too: a two-body step solved exactly in the centre of mass, carried to
the lab and rounded to f64, so that they are what a perfect track would give.

The scales the tests hold the f64 restatement to, for a case with total energy E, beam momentum pb, residual mass m_r:

    Ex:        S_ex = 2^-53 E^2 / m_r                 (M2 is a difference of terms of size E^2; Ex = sqrt(M2) - m_r
                                                       divides their rounding by 2 sqrt(M2) ~ 2 m_r)
    theta_cm:  X = gamma (pz - beta E_e) is a difference of terms of size gamma (|pz| + beta E_e), so
               dX ~ 2^-53 gamma (|pz| + beta E_e), and atan2(pt, X) moves by pt dX / (pt^2 + X^2); the written
               arctangent and pi - theta add roundings of size 2^-53 pi:
               S_th = 2^-53 [ gamma (|pz| + beta E_e) pt / (pt^2 + X^2) + pi ]

``python tests/reaction_exact_reference.py`` writes the fixture; tests/test_reaction_cpu.py (numpy only) reads it."""
from __future__ import annotations

from pathlib import Path

import numpy as np
from mpmath import mp, mpf

GOLDEN = Path(__file__).resolve().parent / "golden"
DPS = 60
U = mpf(2) ** -53
PI64 = 3.141592653589793
REACTIONS = {"be10dp": "be10dp_inverse", "o16aa": "o16aa_a12c"}  # the sets of tests/golden/kinematics.npz
TARGETS = {"none": None, "two": 2, "long": 2049}
Z_RANGE = (0.0, 1.0)
EX_FRACTIONS = (0.0, 0.03, 0.25, 0.5, 0.9, 0.999)
POLAR = (0.0, 1e-9, 0.02, 0.3, 1.0, 1.5707963267948966, 2.0, 2.9, 3.12, 3.141592653589793)
VERTICES = (0.0, 1.0, 0.37, 0.5 + 2.0 ** -30, -0.05, 1.2)  # both ends, inside, outside on either side


def _x(v) -> mpf:
    return mpf(float(v))


def eloss_table(n: int, beam: float) -> np.ndarray:
    """A smooth, slightly convex energy loss over the target, a quarter of the beam energy at its end."""
    s = np.linspace(0.0, 1.0, n)
    return 0.25 * beam * (0.8 * s + 0.2 * s * s)


def exact_beam_ke(beam, z, z_min, z_max, eloss):
    if eloss is None:
        return _x(beam)
    n = len(eloss)
    t = (_x(z) - _x(z_min)) / (_x(z_max) - _x(z_min)) * (n - 1)
    i = min(max(int(mp.floor(t)), 0), n - 2)
    f = t - i
    return _x(beam) - (_x(eloss[i]) + f * (_x(eloss[i + 1]) - _x(eloss[i])))


def exact_value(masses, row, t_b, px, py, pz):
    """-> (ex, theta_cm, E, gamma (|pz| + beta E_e), X, pt), the angle with the f64 PI of the contract for row 3."""
    m_t, m_p, m_e, m_r = _x(masses[0]), _x(masses[1]), _x(masses[row]), _x(masses[5 - row])
    e = t_b + m_p + m_t
    pb2 = t_b * (t_b + 2 * m_p)
    pb = mp.sqrt(pb2)
    pt2 = px * px + py * py
    p2 = pt2 + pz * pz
    e_e = mp.sqrt(p2 + m_e * m_e)
    m2 = (e - e_e) ** 2 - (pb2 + p2 - 2 * pb * pz)
    ex = mp.sqrt(m2) - m_r
    beta, gamma = pb / e, e / mp.sqrt(e * e - pb2)
    pt = mp.sqrt(pt2)
    x = gamma * (pz - beta * e_e)
    th = mp.atan2(pt, x)
    return ex, (_x(PI64) - th if row == 3 else th), e, gamma * (abs(pz) + beta * e_e), x, pt


def lab_momentum(masses, row, t_b, ex, polar, azimuth):
    """The lab momentum of the nucleus of ``row`` for the ejectile's CM angle ``polar`` and the residual's excitation
    ``ex``, exact; (px, py, pz) as f64."""
    m_t, m_p, m_e, m_r = (_x(m) for m in masses[:4])
    e = t_b + m_p + m_t
    pb = mp.sqrt(t_b * (t_b + 2 * m_p))
    e_cm = mp.sqrt(e * e - pb * pb)
    beta, gamma = pb / e, e / e_cm
    e_star = (e_cm ** 2 + m_e ** 2 - (m_r + ex) ** 2) / (2 * e_cm)
    p_star = mp.sqrt(e_star ** 2 - m_e ** 2)
    th, ph = _x(polar), _x(azimuth)
    on_axis = polar in (0.0, PI64)  # exactly forward or backward: no transverse momentum at all
    pt = mpf(0) if on_axis else p_star * mp.sin(th)
    pz_star = p_star * (1 if polar == 0.0 else -1 if polar == PI64 else mp.cos(th))
    if row == 3:  # the residual goes the other way, with the rest of the energy
        pz_star, e_star, ph = -pz_star, e_cm - e_star, ph + mp.pi
    pz = gamma * (pz_star + beta * e_star)
    return float(pt * mp.cos(ph)), float(pt * mp.sin(ph)), float(pz)


def threshold_ex(masses, t_b):
    m_t, m_p, m_e, m_r = (_x(m) for m in masses[:4])
    e = t_b + m_p + m_t
    return mp.sqrt(e * e - t_b * (t_b + 2 * m_p)) - m_e - m_r


def build() -> dict:
    kin = np.load(GOLDEN / "kinematics.npz")
    out = {"reactions": np.array(list(REACTIONS)), "targets": np.array(list(TARGETS))}
    rng = np.random.default_rng(35)
    with mp.workdps(DPS):
        for name, key in REACTIONS.items():
            masses = kin[f"{key}_masses"][:4].astype(np.float64)
            beam = float(np.median(kin[f"{key}_beam"]))
            out[f"{name}_masses"], out[f"{name}_beam"] = masses, np.float64(beam)
            for target, nodes in TARGETS.items():
                eloss = None if nodes is None else eloss_table(nodes, beam)
                if eloss is not None:
                    out[f"{name}_{target}_eloss"] = eloss
                for row in (2, 3):
                    rows = []
                    for z in VERTICES:
                        t_b = exact_beam_ke(beam, z, *Z_RANGE, eloss)
                        top = threshold_ex(masses, t_b)
                        for frac in EX_FRACTIONS:
                            for polar in POLAR:
                                ex = _x(float(top * _x(frac)))
                                px, py, pz = lab_momentum(masses, row, t_b, ex, polar, rng.uniform(0.0, 6.28))
                                got = exact_value(masses, row, t_b, _x(px), _x(py), _x(pz))
                                e_tot, spread, x, pt = got[2], got[3], got[4], got[5]
                                s_ex = U * e_tot ** 2 / _x(masses[5 - row])
                                s_th = U * ((spread * pt / (pt * pt + x * x) if pt > 0 else mpf(0)) + mp.pi)
                                rows.append([z, px, py, pz, float(t_b), float(got[0]), float(got[1]), float(s_ex),
                                             float(s_th), float(ex), polar])
                    out[f"{name}_{target}_row{row}"] = np.array(rows, dtype=np.float64)
    return out


COLUMNS = ("z", "px", "py", "pz", "beam_ke", "ex", "theta_cm", "scale_ex", "scale_theta", "ex_thrown", "polar_thrown")


if __name__ == "__main__":
    data = build()
    np.savez_compressed(GOLDEN / "reaction_exact.npz", columns=np.array(COLUMNS), **data)
    print("wrote", GOLDEN / "reaction_exact.npz", sum(v.shape[0] for k, v in data.items() if "_row" in k), "cases")
