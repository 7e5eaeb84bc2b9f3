"""The reaction reconstruction (include/attpc_engine.h, "reaction reconstruction") restated in numpy: every operation
in the contract's order, one rounding each (numpy's f64 + - * / and sqrt round once and never fuse), the angle from the
written arctangent of tests/helix_reference.py.  ``records`` gives the records and the spectra's cells of a batch;
``mutant`` names one deliberate error (``MUTANTS``), each of which the tests must catch."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd._abi import (EST_EMPTY, EST_FEW, ESTIMATE_DTYPE, FIT_DTYPE, FIT_EMPTY, FIT_FEW, FIT_NO_PID,
                                   FIT_NO_START, REACTION_DTYPE)
from tests.helix_reference import atan2w

NAN = float("nan")
PI = 3.141592653589793
P_PER_BRHO = 299.792458
NO_TRACK, OUTSIDE_TARGET, UNPHYSICAL, NO_TRUTH = 1, 2, 4, 8
FROM_FIT, FROM_ESTIMATE = 0, 1
MUTANTS = ("classical beam momentum", "no energy loss", "sign of pz", "masses swapped", "round for floor", "hi inclusive",
           "truth of the reconstructed only", "response transposed")


class Settings:
    """The fields of an attpc_reaction_desc.  ``eloss`` None: no target."""

    def __init__(self, masses, charge, beam_energy, z_min=0.0, z_max=0.0, eloss=None, track=0, observed_row=2,
                 source=FROM_FIT, ex_lo=-2.0, ex_hi=14.0, n_ex=64, n_theta=36):
        self.masses = [float(m) for m in masses]
        self.charge, self.beam_energy = int(charge), float(beam_energy)
        self.z_min, self.z_max = float(z_min), float(z_max)
        self.eloss = None if eloss is None else np.asarray(eloss, dtype=np.float64)
        self.track, self.observed_row, self.source = int(track), int(observed_row), int(source)
        self.ex_lo, self.ex_hi, self.n_ex, self.n_theta = float(ex_lo), float(ex_hi), int(n_ex), int(n_theta)
        self.ex_inv_width = float(self.n_ex) / (self.ex_hi - self.ex_lo)
        self.theta_inv_width = float(self.n_theta) / PI

    @property
    def n_cells(self):
        return 3 * self.n_ex * self.n_theta + self.n_ex * self.n_ex + 3

    @classmethod
    def of(cls, s):
        """From a ``detector.reaction.ReactionSettings``."""
        return cls(s.masses, s.charge, s.beam_energy, s.z_min, s.z_max, s.eloss, s.track, s.observed_row,
                   {"fit": FROM_FIT, "estimate": FROM_ESTIMATE}[s.source], s.ex_lo, s.ex_hi, s.ex_bins, s.theta_bins)


def beam_ke(s: Settings, z, mutant=None):
    """T_b at the vertices z (m)."""
    z = np.asarray(z, dtype=np.float64)
    if s.eloss is None or mutant == "no energy loss":
        return np.full(z.shape, s.beam_energy)
    n = len(s.eloss)
    with np.errstate(all="ignore"):
        t = (z - s.z_min) / (s.z_max - s.z_min) * float(n - 1)
        i = np.where(t >= 0.0, np.minimum(np.floor(np.where(t >= 0.0, t, 0.0)), float(n - 2)), 0.0).astype(np.int64)
        f = t - i.astype(np.float64)
        loss = s.eloss[i] + f * (s.eloss[i + 1] - s.eloss[i])
        return s.beam_energy - loss


def value(s: Settings, t_b, px, py, pz, mutant=None):
    """-> (ex, theta_cm, m2), NaN where the value is not physical (m2 is returned as computed)."""
    t_b, px, py, pz = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(t_b, px, py, pz))
    m_t, m_p = s.masses[0], s.masses[1]
    m_e, m_r = s.masses[s.observed_row], s.masses[5 - s.observed_row]
    if mutant == "masses swapped":
        m_e, m_r = m_r, m_e
    with np.errstate(all="ignore"):
        e = (t_b + m_p) + m_t
        pb2 = t_b * (t_b + 2.0 * m_p)
        if mutant == "classical beam momentum":
            pb2 = t_b * (2.0 * m_p)
        pb = np.sqrt(pb2)
        pt2 = px * px + py * py
        p2 = pt2 + pz * pz
        e_e = np.sqrt(p2 + m_e * m_e)
        de = e - e_e
        cross = (2.0 * pb) * pz
        m2 = de * de - ((pb2 + p2) + cross if mutant == "sign of pz" else (pb2 + p2) - cross)
        ex = np.sqrt(m2) - m_r
        beta = pb / e
        gamma = e / np.sqrt(e * e - pb2)
        pt = np.sqrt(pt2)
        th = atan2w(pt, gamma * (pz - beta * e_e))
        theta = PI - th if s.observed_row == 3 else th
        physical = (m2 > 0.0) & np.isfinite(ex) & np.isfinite(theta)
    return np.where(physical, ex, NAN), np.where(physical, theta, NAN), m2


def bins(v, lo, hi, inv_width, n, mutant=None):
    """The bin of every v, -1: outside."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        inside = (v >= lo) & ((v <= hi) if mutant == "hi inclusive" else (v < hi))
        scaled = (np.where(inside, v, lo) - lo) * inv_width
        b = np.rint(scaled) if mutant == "round for floor" else np.floor(scaled)
    return np.where(inside, np.minimum(b, float(n - 1)), -1.0).astype(np.int64)


def slots(s: Settings, pid, n, n_sim):
    """The slot every event reads, -1: none."""
    if pid is None:
        return np.full(n, s.track if s.track < n_sim else -1, dtype=np.int64)
    match = np.asarray(pid["position"]) == s.track
    return np.where(match.any(axis=1), match.argmax(axis=1), -1).astype(np.int64)


def records(s: Settings, p4, vertex, status=None, fits=None, estimates=None, pid=None, mutant=None):
    """-> (records [n] REACTION_DTYPE, cells [n_cells] uint64)."""
    source = np.asarray(fits, dtype=FIT_DTYPE) if s.source == FROM_FIT else np.asarray(estimates, dtype=ESTIMATE_DTYPE)
    n, n_sim = source.shape
    p4, vertex = np.asarray(p4, dtype=np.float64), np.asarray(vertex, dtype=np.float64).reshape(n, 3)
    kin = np.zeros(n, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
    slot = slots(s, pid, n, n_sim)
    have = slot >= 0
    rec = source[np.arange(n), np.where(have, slot, 0)]
    with np.errstate(all="ignore"):
        if s.source == FROM_FIT:
            have &= (rec["status"] & (FIT_EMPTY | FIT_FEW | FIT_NO_START | FIT_NO_PID)) == 0
            m_e = s.masses[s.observed_row]
            px, py, pz = m_e * rec["g"][:, 0], m_e * rec["g"][:, 1], m_e * rec["g"][:, 2]
            z = rec["vertex"][:, 2] / 1000.0
        else:
            have &= (rec["status"] & (EST_EMPTY | EST_FEW)) == 0
            pmag = P_PER_BRHO * float(s.charge) * rec["brho"]
            b = rec["slope"]
            w = np.sqrt(1.0 + b * b)
            st, ct = 1.0 / w, b / w
            px, py, pz = pmag * st, np.zeros(n), pmag * ct
            z = rec["vz"] / 1000.0
        have &= np.isfinite(px) & np.isfinite(py) & np.isfinite(pz) & np.isfinite(z)
        out = np.zeros(n, dtype=REACTION_DTYPE)
        t_b = beam_ke(s, z, mutant)
        ex, theta, _ = value(s, t_b, px, py, pz, mutant)
        unphysical = have & np.isnan(ex)
        outside = have & (s.eloss is not None) & ~((z >= s.z_min) & (z <= s.z_max))
        t_truth = beam_ke(s, vertex[:, 2], mutant)
        row = p4[:, s.observed_row]
        tex, ttheta, _ = value(s, t_truth, row[:, 0], row[:, 1], row[:, 2], mutant)
    no_truth = (kin != 0) | np.isnan(tex)
    out["status"] = (np.where(~have, NO_TRACK, 0) | np.where(outside, OUTSIDE_TARGET, 0) | np.where(unphysical, UNPHYSICAL, 0)
                     | np.where(no_truth, NO_TRUTH, 0))
    out["slot"] = slot
    out["beam_ke"] = np.where(have, t_b, NAN)
    out["ex"] = np.where(have, ex, NAN)
    out["theta_cm"] = np.where(have, theta, NAN)
    out["truth_beam_ke"] = np.where(no_truth, NAN, t_truth)
    out["truth_ex"] = np.where(no_truth, NAN, tex)
    out["truth_theta_cm"] = np.where(no_truth, NAN, ttheta)
    return out, cells(s, out, mutant)


def cells(s: Settings, rec, mutant=None):
    """The spectra of the records ``rec``."""
    n_ex, n_theta = s.n_ex, s.n_theta
    plane = n_ex * n_theta
    first_outside = 3 * plane + n_ex * n_ex
    out = np.zeros(s.n_cells, dtype=np.uint64)
    has_truth, good = (rec["status"] & NO_TRUTH) == 0, rec["status"] == 0
    te = bins(rec["truth_ex"], s.ex_lo, s.ex_hi, s.ex_inv_width, n_ex, mutant)
    tt = bins(rec["truth_theta_cm"], 0.0, PI, s.theta_inv_width, n_theta, mutant)
    re = bins(rec["ex"], s.ex_lo, s.ex_hi, s.ex_inv_width, n_ex, mutant)
    rt = bins(rec["theta_cm"], 0.0, PI, s.theta_inv_width, n_theta, mutant)
    thrown = has_truth & good if mutant == "truth of the reconstructed only" else has_truth
    t_in, r_in, x_in = (te >= 0) & (tt >= 0), (re >= 0) & (rt >= 0), (te >= 0) & (re >= 0)
    np.add.at(out, (te * n_theta + tt)[thrown & t_in], 1)
    out[first_outside] = np.count_nonzero(thrown & ~t_in)
    np.add.at(out, plane + (te * n_theta + tt)[has_truth & good & t_in], 1)
    np.add.at(out, 2 * plane + (re * n_theta + rt)[good & r_in], 1)
    out[first_outside + 1] = np.count_nonzero(good & ~r_in)
    response = re * n_ex + te if mutant == "response transposed" else te * n_ex + re
    np.add.at(out, 3 * plane + response[good & x_in], 1)
    out[first_outside + 2] = np.count_nonzero(good & ~x_in)
    return out


def same(a, b) -> bool:
    """Records equal byte for byte (NaN is NaN's equal)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
