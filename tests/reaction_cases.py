"""Synthetic inputs of the reaction reconstruction for the CPU and the GPU tests: source records (fit or estimate), pid
records, truth 4-vectors, vertices and kinematics status that reach every status bit, every way the slot is chosen, the
spectra with all events in one cell and with every event in a cell of its own, and values exactly on the edges of the
bins.  The reference of every case is tests/reaction_reference.py on the same arrays, computed once per process."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from attpc_engine_amd._abi import (EST_EMPTY, EST_FEW, ESTIMATE_DTYPE, FIT_DTYPE, FIT_EMPTY, FIT_FEW, FIT_NO_PID,
                                   FIT_NO_START, FIT_NOT_CONVERGED, PID_DTYPE)
from tests import reaction_reference as pref

GOLDEN = Path(__file__).resolve().parent / "golden"
NAN = float("nan")
EVENT_COUNTS = (1, 63, 64, 65, 130)
PID_MODES = (None, "own", "absent", "slot7", "twice")
N_ROWS = 4


@dataclass
class Case:
    settings: pref.Settings
    fits: np.ndarray | None
    estimates: np.ndarray | None
    pid: np.ndarray | None
    p4: np.ndarray
    vertex: np.ndarray
    status: np.ndarray

    def arrays(self) -> dict:
        return {"fits": self.fits, "estimates": self.estimates, "pid": self.pid, "p4": self.p4, "vertex": self.vertex,
                "status": self.status}


@functools.lru_cache(maxsize=None)
def fixture() -> dict:
    return dict(np.load(GOLDEN / "reaction_exact.npz"))


def base_settings(reaction="be10dp", target="long", **kw) -> pref.Settings:
    z = fixture()
    eloss = None if target == "none" else z[f"{reaction}_{target}_eloss"]
    charge = {"be10dp": {2: 1, 3: 4}, "o16aa": {2: 2, 3: 8}}[reaction][kw.get("observed_row", 2)]
    return pref.Settings(z[f"{reaction}_masses"], charge, float(z[f"{reaction}_beam"]), 0.0, 1.0, eloss, **kw)


def lab_momentum(s: pref.Settings, z, ex, polar, azimuth):
    """f64 two-body kinematics: the lab momentum of the observed nucleus for the ejectile's CM angle ``polar`` and the
    residual's excitation ``ex`` at the vertex z (plain numpy, good to a few ulps: an input, not a reference)."""
    m_t, m_p, m_e, m_r = s.masses[0], s.masses[1], s.masses[2], s.masses[3]
    t_b = pref.beam_ke(s, z)
    e = t_b + m_p + m_t
    pb = np.sqrt(t_b * (t_b + 2.0 * m_p))
    e_cm = np.sqrt(e * e - pb * pb)
    beta, gamma = pb / e, e / e_cm
    e_star = (e_cm ** 2 + m_e ** 2 - (m_r + ex) ** 2) / (2.0 * e_cm)
    p_star = np.sqrt(e_star ** 2 - m_e ** 2)
    pt, pz_star = p_star * np.sin(polar), p_star * np.cos(polar)
    if s.observed_row == 3:
        pz_star, e_star, azimuth = -pz_star, e_cm - e_star, azimuth + np.pi
    return pt * np.cos(azimuth), pt * np.sin(azimuth), gamma * (pz_star + beta * e_star)


def source_records(s: pref.Settings, px, py, pz, z, n_sim, slot):
    """Fit or estimate records [n, n_sim] whose slot ``slot`` [n] holds the momentum (px, py, pz) and the vertex z (m);
    the other slots hold another track (a valid one, so that reading the wrong slot shows)."""
    n = len(px)
    rows = np.arange(n)
    if s.source == pref.FROM_FIT:
        rec = np.zeros((n, n_sim), dtype=FIT_DTYPE)
        m_e = s.masses[s.observed_row]
        rec["g"] = np.array([0.01, -0.02, 0.05])
        rec["vertex"] = np.array([1.0, -1.0, 250.0])
        rec["g"][rows, slot] = np.stack([px, py, pz], axis=-1) / m_e
        rec["vertex"][rows, slot, 2] = z * 1000.0
        rec["ke"], rec["brho"], rec["f"], rec["lambda"], rec["path"] = 1.0, 0.5, 1e-6, 1e-3, 0.3
        rec["status"][:, ::2] = FIT_NOT_CONVERGED  # (a bit that does not matter)
        rec["status"][rows, slot] = 0
        return rec
    rec = np.zeros((n, n_sim), dtype=ESTIMATE_DTYPE)
    rec["brho"], rec["slope"], rec["vz"] = 0.4, 0.7, 250.0
    pt = np.sqrt(px * px + py * py)
    with np.errstate(all="ignore"):
        rec["brho"][rows, slot] = np.sqrt(pt * pt + pz * pz) / (pref.P_PER_BRHO * s.charge)
        rec["slope"][rows, slot] = pz / pt
    rec["vz"][rows, slot] = z * 1000.0
    return rec


def pid_records(mode, n, n_sim, track):
    """-> (pid [n, n_sim] or None, the slot every event's track is in, -1: none)."""
    if mode is None:
        return None, np.full(n, track, dtype=np.int64)
    pid = np.zeros((n, n_sim), dtype=PID_DTYPE)
    pid["position"] = -1
    pid["species"] = -1
    slot = np.full(n, -1, dtype=np.int64)
    events = np.arange(n)
    if mode == "own":  # every slot got its own position
        pid["position"] = np.arange(n_sim)
        slot[:] = track
    elif mode == "slot7":  # the track's position in the last slot, other positions before it
        pid["position"][:, :-1] = (track + 1 + np.arange(n_sim - 1)) % max(n_sim, 2) if n_sim > 1 else -1
        pid["position"][pid["position"] == track] = -1
        pid["position"][:, -1] = track
        slot[:] = n_sim - 1
    elif mode == "twice":  # twice in an event: the first slot counts
        first = events % n_sim
        second = (first + 1 + events % max(n_sim - 1, 1)) % n_sim
        pid["position"][events, first] = track
        pid["position"][events, second] = track
        slot[:] = np.minimum(first, second)
    elif mode != "absent":
        raise ValueError(mode)
    return pid, slot


def physics(s: pref.Settings, n, rng, cells=None):
    """Truth (z, ex, polar) of n events and a smeared observation of them -> (truth momenta, observed momenta, z_truth,
    z_observed).  ``cells`` = "one": every event the same; "own": event i at the centre of a (Ex, theta) cell of its own."""
    top = 8.0 if s.masses[1] < 12000.0 else 16.0  # below the threshold of either reaction at the end of the target
    if cells == "one":
        z, ex, polar = np.full(n, 0.4), np.full(n, 2.0), np.full(n, 1.1)
        azimuth = np.full(n, 0.3)
    elif cells == "own":
        i = np.arange(n)
        first = int(np.ceil((0.0 - s.ex_lo) * s.ex_inv_width))
        span = int((top - s.ex_lo) * s.ex_inv_width) - first
        ex = s.ex_lo + (first + i % span + 0.5) / s.ex_inv_width
        polar = ((i * 7) % s.n_theta + 0.5) / s.theta_inv_width
        z, azimuth = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 6.28, n)
        assert len(set(zip((i % span).tolist(), ((i * 7) % s.n_theta).tolist()))) == n
    else:
        z, ex = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, top, n)
        polar, azimuth = np.arccos(rng.uniform(-1.0, 1.0, n)), rng.uniform(0.0, 6.28, n)
    truth = lab_momentum(s, z, ex, polar, azimuth)
    if cells is not None:
        return truth, truth, z, z
    smear = 1.0 + rng.normal(0.0, 0.01, (3, n))
    return truth, tuple(t * f for t, f in zip(truth, smear)), z, z + rng.normal(0.0, 0.004, n)


def make(n, n_sim=1, source=pref.FROM_FIT, pid_mode=None, observed_row=2, reaction="be10dp", target="long", track=0,
         cells=None, flags=True, seed=0, **bins) -> Case:
    """A case of n events.  ``flags``: a share of the events gets each way to a status bit."""
    rng = np.random.default_rng(1000 * n + 10 * n_sim + seed)
    s = base_settings(reaction, target, source=source, observed_row=observed_row, track=track, **bins)
    truth, seen, z_truth, z_seen = physics(s, n, rng, cells)
    pid, slot = pid_records(pid_mode, n, n_sim, track)
    rec = source_records(s, *seen, z_seen, n_sim, np.where(slot >= 0, slot, 0))
    p4 = np.zeros((n, N_ROWS, 4))
    p4[:, :, 3] = s.masses[:4]
    p4[:, s.observed_row, :3] = np.stack(truth, axis=-1)
    p4[:, s.observed_row, 3] = np.sqrt(sum(t * t for t in truth) + s.masses[s.observed_row] ** 2)
    vertex = np.stack([rng.normal(0.0, 0.003, n), rng.normal(0.0, 0.003, n), z_truth], axis=-1)
    status = np.zeros(n, dtype=np.int32)
    if flags and n >= 8:
        kind = rng.integers(0, 24, n)
        at = (np.arange(n), np.where(slot >= 0, slot, 0))
        bad_bits = (FIT_EMPTY, FIT_FEW, FIT_NO_START, FIT_NO_PID) if source == pref.FROM_FIT else (EST_EMPTY, EST_FEW, EST_EMPTY, EST_FEW)
        for k, bit in enumerate(bad_bits):  # NO_TRACK by the source's status
            rec["status"][at[0][kind == k], at[1][kind == k]] |= bit
        value = "g" if source == pref.FROM_FIT else "brho"
        hit = kind == 4  # NO_TRACK by a value that is not a number
        if source == pref.FROM_FIT:
            rec["g"][at[0][hit], at[1][hit], 1] = NAN
        else:
            rec[value][at[0][hit], at[1][hit]] = NAN
        hit = kind == 5  # OUTSIDE_TARGET, below and above
        zz = np.where(np.arange(n) % 2 == 0, -30.0, 1100.0)
        if source == pref.FROM_FIT:
            rec["vertex"][at[0][hit], at[1][hit], 2] = zz[hit]
        else:
            rec["vz"][at[0][hit], at[1][hit]] = zz[hit]
        hit = kind == 6  # UNPHYSICAL: more momentum than the beam brought
        if source == pref.FROM_FIT:
            rec["g"][at[0][hit], at[1][hit], 2] *= 400.0
        else:
            rec["brho"][at[0][hit], at[1][hit]] *= 400.0
        hit = kind == 7  # NO_TRUTH: the kinematics gave up
        status[hit] = 1
        p4[hit] = NAN
        hit = kind == 8  # NO_TRUTH and NO_TRACK together
        status[hit] = 1
        rec["status"][at[0][hit], at[1][hit]] |= bad_bits[0]
    return Case(s, rec if source == pref.FROM_FIT else None, rec if source == pref.FROM_ESTIMATE else None, pid, p4, vertex, status)


def reference(case: Case, mutant=None):
    return pref.records(case.settings, case.p4, case.vertex, case.status, case.fits, case.estimates, case.pid, mutant=mutant)


def right_angle_g(s: pref.Settings, t_b: float, gx: float) -> float:
    """A g_z for which gamma (pz - beta E_e) is exactly 0 in the contract's arithmetic with (px, py, pz) = m_e (gx, 0,
    g_z), so that theta_cm is exactly 1.5707963267948966: found by walking the doubles around the solution (beta E_e
    moves by less than pz does, so some double near it meets it)."""
    m_e = s.masses[s.observed_row]
    e = (t_b + s.masses[1]) + s.masses[0]
    pb2 = t_b * (t_b + 2.0 * s.masses[1])
    beta = np.sqrt(pb2) / e
    px = m_e * gx
    start = beta * np.sqrt(px * px + m_e * m_e) / np.sqrt(1.0 - beta * beta) / m_e
    for toward in (np.inf, -np.inf):
        cand = start
        for _ in range(20000):
            pz = m_e * cand
            if pz - beta * np.sqrt((px * px + pz * pz) + m_e * m_e) == 0.0:
                return float(cand)
            cand = np.nextafter(cand, toward)
    raise AssertionError("no g_z gives a right angle exactly")


def edge_case(source=pref.FROM_FIT) -> Case:
    """Values exactly on the edges of the bins.  theta_cm of the truth (and, with the fit source, of the record): 0
    (pt = 0, forward), PI = the upper edge (pt = 0, backward in the CM; the lab momentum still points forward), PI / 2 =
    an interior edge of an even number of bins; Ex: ``edge_variants`` takes ex_lo and ex_hi from the values two of the
    case's events have, so one event is at lo exactly, one at hi exactly, and with ``hi = nextafter(value)`` one at the
    largest double below hi; NaN from an unphysical record."""
    base = make(16, 1, source, flags=False, seed=5)
    s = base.settings
    m_e = s.masses[2]
    t_b = float(pref.beam_ke(s, np.array([0.5]))[0])
    gx = 30.0 / m_e
    edges = [(0.0, 120.0 / m_e), (0.0, 0.02), (gx, right_angle_g(s, t_b, gx))]
    for e, (g0, g2) in enumerate(edges):
        base.p4[e, 2, :3] = (m_e * g0, 0.0, m_e * g2)
        base.vertex[e, 2] = 0.5
    if source == pref.FROM_FIT:
        for e, (g0, g2) in enumerate(edges):
            base.fits["g"][e, 0] = (g0, 0.0, g2)
            base.fits["vertex"][e, 0, 2] = 500.0
        base.fits["g"][3, 0, 2] *= 400.0  # unphysical: NaN
    else:
        base.estimates["slope"][0, 0] = np.inf  # st = 0, ct = NaN: not a track
        base.estimates["brho"][3, 0] *= 400.0
    return base


def edge_variants(case: Case) -> list:
    """The case with Ex bins whose lower / upper edge is a value of one of its events."""
    ex = reference(case)[0]["ex"]
    order = np.argsort(np.where(np.isnan(ex), np.inf, ex))
    lo, hi = float(ex[order[1]]), float(ex[order[np.count_nonzero(~np.isnan(ex)) - 2]])
    out = []
    for top in (hi, float(np.nextafter(hi, np.inf))):
        for n_ex in (1, 7, 64):
            s = pref.Settings(case.settings.masses, case.settings.charge, case.settings.beam_energy, case.settings.z_min,
                              case.settings.z_max, case.settings.eloss, case.settings.track, case.settings.observed_row,
                              case.settings.source, lo, top, n_ex, 36)
            out.append(Case(s, case.fits, case.estimates, case.pid, case.p4, case.vertex, case.status))
    return out


def to_settings(s: pref.Settings):
    """The ``detector.reaction.ReactionSettings`` of a restatement's settings."""
    from attpc_engine_amd.detector.reaction import ReactionSettings

    target = None if s.eloss is None else (s.z_min, s.z_max, s.eloss)
    return ReactionSettings(s.masses, s.charge, s.beam_energy, target, s.track, s.observed_row,
                            {pref.FROM_FIT: "fit", pref.FROM_ESTIMATE: "estimate"}[s.source], (s.ex_lo, s.ex_hi), s.n_ex, s.n_theta)
