"""Vectorised numpy restatement of the engine's samplers (test infrastructure) on the Philox restatements the suite
already has: the kinematics draws of an attempt and the whole-event rejection loop (csrc/kinematics.hip), the Fano draw
of a track sample (csrc/tracks.hip), the time-bucket jitter and the Monte-Carlo position of a primary electron
(csrc/scatter.hip).  ``test_laws_cpu.py`` ties it to the oracle and then runs it with one law broken at a time
(``mutant=``) to show that the checks of ``tests/law_analysis.py`` can fail."""
from __future__ import annotations

import numpy as np

from tests.peaks_reference import DOMAIN_JITTER
from tests.peaks_reference import jitter_uniform as _jitter_uniform
from tests.trace_noise_reference import philox4x32_10

TWO_PI = 2.0 * np.pi
DOMAIN_KIN, DOMAIN_FANO0, DOMAIN_MC, KIN_SLOTS = 0, 1, 0x200, 64
EX_GAUSSIAN, EX_UNIFORM, EX_TABLE = 0, 1, 2
POLAR_UNIFORM, POLAR_ARBITRARY = 0, 1

KIN_MUTANTS = ("sigma_fwhm", "theta_uniform", "rho_rayleigh", "azimuth_z_same", "ex1_slot0", "offset_from_bin",
               "resample_failed_step", "attempt_not_in_counter")
FANO_MUTANTS = ("round", "sigma_sqrt_mu", "sigma_f_sqrt_mu", "odd_reuses_even", "one_domain", "event_hi_ignored")
JITTER_MUTANTS = ("no_tb", "no_pad", "no_seed_hi")
MC_MUTANTS = ("sigma_2pc", "same_branch")


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def rng_pair(seed: int, event, index, domain):
    """Two uniforms in [0, 1) of (seed, event, index, domain): Philox4x32-10, counter (event lo, event hi, index,
    domain), key (seed lo, seed hi).  ``event``, ``index`` and ``domain`` broadcast."""
    event = np.asarray(event, dtype=np.uint64)
    r = philox4x32_10(event & np.uint64(0xFFFFFFFF), event >> np.uint64(32), index, domain,
                      int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return _u53(r[0], r[1]), _u53(r[2], r[3])


def normal_from(ua, ub):
    return np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(TWO_PI * ub)


# ------------------------------------------------------------------------------------------------ kinematics ----
class KinModel:
    """The sampler's inputs read off a ``KinDesc`` (what the device and the oracle are configured with)."""

    def __init__(self, desc):
        self.n_steps = int(desc.n_steps)
        self.n_rows = 4 + 2 * (self.n_steps - 1)
        self.masses = np.array([desc.masses[i] for i in range(self.n_rows)], dtype=np.float64)
        self.sample_limit = int(desc.sample_limit)
        self.beam_energy = float(desc.beam_energy)
        self.has_target = bool(desc.has_target)
        if self.has_target:
            self.rho_sigma, self.z_min, self.z_max = float(desc.rho_sigma), float(desc.z_min), float(desc.z_max)
            self.eloss = np.ctypeslib.as_array(desc.eloss, shape=(desc.eloss_len,)).copy()
        self.excitation, self.polar = [], []
        for s in range(self.n_steps):
            e, p = desc.excitation[s], desc.polar[s]
            ex = {"kind": int(e.kind), "p0": float(e.p0), "p1": float(e.p1)}
            if ex["kind"] == EX_TABLE:
                ex["x"] = np.ctypeslib.as_array(e.table_x, shape=(e.table_len,)).copy()
                ex["cdf"] = np.ctypeslib.as_array(e.table_cdf, shape=(e.table_len,)).copy()
            po = {"kind": int(p.kind), "cos_min": float(p.cos_min), "cos_max": float(p.cos_max),
                  "bin_width": float(p.bin_width)}
            if po["kind"] == POLAR_ARBITRARY:
                po["angles"] = np.ctypeslib.as_array(p.angles, shape=(p.table_len,)).copy()
                po["cdf"] = np.ctypeslib.as_array(p.cdf, shape=(p.table_len,)).copy()
            self.excitation.append(ex)
            self.polar.append(po)


def sample_excitation(d: dict, ua, ub, mutant=None):
    if d["kind"] == EX_GAUSSIAN:
        sigma = d["p1"] * 2.355 if mutant == "sigma_fwhm" else d["p1"]
        return d["p0"] + sigma * normal_from(ua, ub)
    if d["kind"] == EX_UNIFORM:
        return d["p0"] + (d["p1"] - d["p0"]) * ua
    x, cdf = d["x"], d["cdf"]
    hi = np.clip(np.searchsorted(cdf, ua, side="right"), 1, len(cdf) - 1)  # cdf[lo] <= ua < cdf[hi]
    lo = hi - 1
    w = cdf[hi] - cdf[lo]
    f = np.where(w > 0.0, (ua - cdf[lo]) / np.where(w > 0.0, w, 1.0), 0.0)
    return np.where(ua <= cdf[0], x[0], x[lo] + f * (x[hi] - x[lo])) - d["p0"]


def sample_polar(d: dict, ua, ub, mutant=None):
    if d["kind"] == POLAR_UNIFORM:
        if mutant == "theta_uniform":
            lo, hi = np.arccos(d["cos_max"]), np.arccos(d["cos_min"])
            return lo + (hi - lo) * ua
        return np.arccos(d["cos_min"] + (d["cos_max"] - d["cos_min"]) * ua)
    lo = np.minimum(np.searchsorted(d["cdf"], ua, side="right"), len(d["cdf"]) - 1)
    return d["angles"][lo] + (ua if mutant == "offset_from_bin" else ub) * d["bin_width"]


def _boost(p, bx, by, bz):
    """``vector``'s boost_beta3 as the kernel writes it; p [..., 4] = (x, y, z, t)."""
    bp2 = bx * bx + by * by + bz * bz
    gam = 1.0 / np.sqrt(1.0 - bp2)
    bgam = gam * gam / (1.0 + gam)
    xx, yy, zz = 1.0 + bgam * bx * bx, 1.0 + bgam * by * by, 1.0 + bgam * bz * bz
    xy, xz, yz = bgam * bx * by, bgam * bx * bz, bgam * by * bz
    xt, yt, zt = gam * bx, gam * by, gam * bz
    x, y, z, t = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    return np.stack([xx * x + xy * y + xz * z + xt * t, xy * x + yy * y + yz * z + yt * t,
                     xz * x + yz * y + zz * z + zt * t, xt * x + yt * y + zt * z + gam * t], axis=-1)


def inv_mass(p):
    m2 = p[..., 3] ** 2 - (p[..., 0] ** 2 + p[..., 1] ** 2 + p[..., 2] ** 2)
    return np.sign(m2) * np.sqrt(np.abs(m2))


def two_body(parent, m_out, m_other, ex, polar, azim):
    ibt = 1.0 / parent[..., 3]
    bx, by, bz = parent[..., 0] * ibt, parent[..., 1] * ibt, parent[..., 2] * ibt
    ecm = _boost(parent, -bx, -by, -bz)[..., 3]
    mo = m_other + ex
    e_a = (m_out * m_out - mo * mo + ecm * ecm) / (2.0 * ecm)
    p_a = np.sqrt(np.maximum(e_a * e_a - m_out * m_out, 0.0))
    cm = np.stack([p_a * np.sin(polar) * np.cos(azim), p_a * np.sin(polar) * np.sin(azim), p_a * np.cos(polar), e_a],
                  axis=-1)
    a = _boost(cm, bx, by, bz)
    return a, parent - a


def reaction_allowed(m, t, ex):
    pz = np.sqrt(t * (t + 2.0 * m[1]))
    s = m[0] + t + m[1]
    return (m[2] + m[3] + ex) < np.sqrt(s * s - pz * pz)


def below_nr_threshold(m, t, ex):
    q = m[0] + m[1] - (m[2] + m[3] + ex)
    return t < -q * (m[2] + m[3]) / (m[2] + m[3] - m[1])


def _eloss_lookup(k: KinModel, z):
    t = (z - k.z_min) / (k.z_max - k.z_min) * (len(k.eloss) - 1)
    i = np.clip(np.floor(t).astype(np.int64), 0, len(k.eloss) - 2)
    return k.eloss[i] + (t - i) * (k.eloss[i + 1] - k.eloss[i])


def kin_run(k: KinModel, seed: int, first_event: int, n: int, mutant: str | None = None):
    """-> (vertex [n,3], p4 [n,rows,4], status [n], attempts [n]) of kin_run_kernel: draw index = attempt * 64 + slot
    (slots 0..2 the vertex, 3 + 4 s / 4 + 4 s / 5 + 4 s the excitation, polar angle and azimuth of step s), any refusal
    resamples the whole event.  Every pending event is computed to its end each round; a step's refusal is looked at
    afterwards, which gives the kernel's numbers because a draw depends on nothing but its counter."""
    assert mutant is None or mutant in KIN_MUTANTS, mutant
    m = k.masses
    vertex = np.zeros((n, 3))
    p4 = np.full((n, k.n_rows, 4), np.nan)
    status = np.zeros(n, dtype=np.int32)
    tries = np.zeros(n, dtype=np.uint32)
    att = np.zeros((n, k.n_steps), dtype=np.uint64)  # the attempt whose draws step s uses (all equal unless mutated)
    pending = np.arange(n)
    with np.errstate(all="ignore"):
        while pending.size:
            over = tries[pending] >= k.sample_limit
            status[pending[over]] = 1
            pending = pending[~over]
            if not pending.size:
                break
            ev = np.uint64(first_event) + pending.astype(np.uint64)
            tries[pending] += 1

            def draw(step, slot):
                return rng_pair(seed, ev, att[pending, step] * np.uint64(KIN_SLOTS) + np.uint64(slot), DOMAIN_KIN)

            e_beam = np.full(pending.size, k.beam_energy)
            v = np.zeros((pending.size, 3))
            if k.has_target:
                ua, ub = draw(0, 0)
                rho = k.rho_sigma * (np.sqrt(-2.0 * np.log(1.0 - ua)) if mutant == "rho_rayleigh"
                                     else np.abs(normal_from(ua, ub)))
                ua1, _ = draw(0, 1)
                v[:, 0], v[:, 1] = rho * np.cos(TWO_PI * ua1), rho * np.sin(TWO_PI * ua1)
                ua2, _ = draw(0, 2)
                v[:, 2] = k.z_min + (k.z_max - k.z_min) * (ua1 if mutant == "azimuth_z_same" else ua2)
                e_beam = e_beam - _eloss_lookup(k, v[:, 2])
            failed = np.full(pending.size, -1)
            ex = sample_excitation(k.excitation[0], *draw(0, 3), mutant)
            failed[~reaction_allowed(m, e_beam, ex) | below_nr_threshold(m, e_beam, ex)] = 0
            th = sample_polar(k.polar[0], *draw(0, 4), mutant)
            ph = TWO_PI * draw(0, 5)[0]
            rows = np.zeros((pending.size, k.n_rows, 4))
            rows[:, 0, 3] = m[0]
            rows[:, 1, 2], rows[:, 1, 3] = np.sqrt(e_beam * (e_beam + 2.0 * m[1])), e_beam + m[1]
            rows[:, 2], rows[:, 3] = two_body(rows[:, 0] + rows[:, 1], m[2], m[3], ex, th, ph)
            prev = rows[:, 3]
            for s in range(1, k.n_steps):
                m1, m2 = m[4 + 2 * (s - 1)], m[5 + 2 * (s - 1)]
                slot = 3 if (mutant == "ex1_slot0" and s == 1) else 3 + 4 * s
                ex = sample_excitation(k.excitation[s], *draw(0 if slot == 3 else s, slot), mutant)
                bad = ~((inv_mass(prev) - (m1 + m2 + ex)) > 0.0)
                failed[bad & (failed < 0)] = s
                th = sample_polar(k.polar[s], *draw(s, 4 + 4 * s), mutant)
                ph = TWO_PI * draw(s, 5 + 4 * s)[0]
                rows[:, 4 + 2 * (s - 1)], rows[:, 5 + 2 * (s - 1)] = two_body(prev, m1, m2, ex, th, ph)
                prev = rows[:, 5 + 2 * (s - 1)]
            good = failed < 0
            p4[pending[good]] = rows[good]
            vertex[pending] = v  # the kernel leaves the last attempt's vertex behind, also beside status 1
            again = pending[~good]
            if mutant == "resample_failed_step":
                att[again, failed[~good]] += np.uint64(1)
            elif mutant != "attempt_not_in_counter":
                att[again] += np.uint64(1)
            pending = again
    return vertex, p4, status, tries


# ------------------------------------------------------------------------------------------------------ Fano ----
def fano_electrons(mu, k, seed: int, event, domain, fano: float, mutant: str | None = None) -> np.ndarray:
    """Electrons of track samples with mean ``mu`` at ODE row ``k`` of (event, domain = 1 + row of the nucleus):
    trunc(mu + sqrt(F mu) Z) toward zero, Z the Box-Muller cosine branch of Philox index k >> 1 for an even k, the
    sine branch for an odd one.  All arguments broadcast."""
    assert mutant is None or mutant in FANO_MUTANTS, mutant
    mu = np.asarray(mu, dtype=np.float64)
    k = np.asarray(k, dtype=np.uint64)
    event = np.asarray(event, dtype=np.uint64)
    if mutant == "event_hi_ignored":
        event = event & np.uint64(0xFFFFFFFF)
    if mutant == "one_domain":
        domain = DOMAIN_FANO0
    ua, ub = rng_pair(seed, event, k >> np.uint64(1), domain)
    rad = np.sqrt(-2.0 * np.log(1.0 - ua))
    odd = (k & np.uint64(1)).astype(bool) & (mutant != "odd_reuses_even")
    z = rad * np.where(odd, np.sin(TWO_PI * ub), np.cos(TWO_PI * ub))
    sigma = {"sigma_sqrt_mu": np.sqrt(mu), "sigma_f_sqrt_mu": fano * np.sqrt(mu)}.get(mutant, np.sqrt(fano * mu))
    draw = mu + sigma * z
    return (np.floor(draw + 0.5) if mutant == "round" else np.trunc(draw)).astype(np.int64)


def kinetic_energy(track, mass: float):
    """The oracle's expression on trajectory rows (x, y, z, gamma beta x, gamma beta y, gamma beta z)."""
    gv = np.sqrt(track[:, 3] ** 2 + track[:, 4] ** 2 + track[:, 5] ** 2)
    beta = np.sqrt(gv * gv / (1.0 + gv * gv))
    return mass * (gv / beta - 1.0)


def fano_mu(track, mass: float, w_value: float) -> np.ndarray:
    """Mean electrons of every trajectory row: |KE_k - KE_(k-1)| 1e6 / W, 0 for row 0."""
    e = kinetic_energy(np.asarray(track, dtype=np.float64), mass)
    mu = np.zeros(len(e))
    mu[1:] = np.abs(e[1:] - e[:-1])
    return mu * (1.0e6 / w_value)


# ---------------------------------------------------------------------------------------------------- jitter ----
def jitter(seed: int, event: int, pad, tb, mutant: str | None = None) -> np.ndarray:
    """U[0, 1) added to the time bucket of the cloud point (pad, tb) of (seed, event): Philox2x32-7 keyed by
    tb << 14 | pad."""
    assert mutant is None or mutant in JITTER_MUTANTS, mutant
    pad = np.asarray(pad, dtype=np.uint64)
    tb = np.asarray(tb, dtype=np.uint64)
    key = (np.zeros_like(tb) if mutant == "no_tb" else tb << np.uint64(14)) | (np.zeros_like(pad) if mutant == "no_pad" else pad)
    if mutant == "no_seed_hi":
        seed = int(seed) & 0xFFFFFFFF
    return _jitter_uniform(seed, event, key, DOMAIN_JITTER)


# ----------------------------------------------------------------------------------- Monte-Carlo diffusion ----
class PadPlane:
    """The whole-mm look-up table of a detector descriptor (unfolded) and the beam pads."""

    def __init__(self, det_raw, beam_pads):
        self.lo, self.n = int(det_raw.lut_lo), int(det_raw.lut_n)
        self.lut = np.ctypeslib.as_array(det_raw.pad_lut, shape=(self.n * self.n,)).astype(np.int64).reshape(self.n, self.n)
        self.beam = np.asarray(beam_pads, dtype=np.int64)

    def pad_of(self, x_m, y_m) -> np.ndarray:
        """Pad under a position in metres; -1 off the plane, in a gap or on a beam pad (no charge is collected)."""
        fx, fy = np.floor(x_m * 1000.0), np.floor(y_m * 1000.0)
        inside = (fx >= self.lo) & (fx < self.lo + self.n) & (fy >= self.lo) & (fy < self.lo + self.n)
        ix = np.where(inside, fx - self.lo, 0).astype(np.int64)
        iy = np.where(inside, fy - self.lo, 0).astype(np.int64)
        pad = np.where(inside, self.lut[ix, iy], -1)
        return np.where(np.isin(pad, self.beam), -1, pad)


def mc_sigma(time_bucket, diffusion: float, drift_velocity: float, efield: float):
    return np.sqrt(2.0 * diffusion * drift_velocity * np.asarray(time_bucket, dtype=np.float64) / efield)


def mc_pad_counts(plane: PadPlane, cx: float, cy: float, sigma: float, n_primary: int, seed: int, event: int,
                  entry: int, mutant: str | None = None) -> dict:
    """Primary electrons per pad of one track sample (entry number ``entry`` of the event): electron k lands at
    (cx + sigma N_x, cy + sigma N_y), Box-Muller cos / sin of the Philox pair (index k, domain 0x200 + entry)."""
    assert mutant is None or mutant in MC_MUTANTS, mutant
    ua, ub = rng_pair(seed, event, np.arange(n_primary, dtype=np.uint64), DOMAIN_MC + entry)
    # (ua where 1 - ua belongs changes nothing: both are uniform; it is not a mutant)
    rad = np.sqrt(-2.0 * np.log(1.0 - ua))
    if mutant == "sigma_2pc":
        sigma = 1.02 * sigma
    x = cx + sigma * (rad * np.cos(TWO_PI * ub))
    y = cy + sigma * (rad * (np.cos if mutant == "same_branch" else np.sin)(TWO_PI * ub))
    pad = plane.pad_of(x, y)
    pads, counts = np.unique(pad[pad >= 0], return_counts=True)
    return dict(zip(pads.tolist(), counts.tolist()))
