"""What a user gets back -> the sampled parameters -> the checks of their laws (test infrastructure).  Everything here
takes arrays and does not care who made them: ``test_laws_cpu.py`` hands it the oracle's and the restatement's output
(unmutated and with one law broken), ``test_gpu_laws.py`` the device's.  f64 numpy; the statistics are those of
``tests/law_checks.py``.  A check returns its figures (size, statistic, p or corr_z); the tests print them and assert
by the one rule of law_checks."""
from __future__ import annotations

import math

import numpy as np

from tests import law_checks as lc

TWO_PI = 2.0 * np.pi


# -------------------------------------------------------------------------------- parameters from 4-vectors ----
def inv_mass(p):
    m2 = p[..., 3] ** 2 - (p[..., 0] ** 2 + p[..., 1] ** 2 + p[..., 2] ** 2)
    return np.sign(m2) * np.sqrt(np.abs(m2))


def rest_frame(parent, p):
    """``p`` [n,4] boosted into the rest frame of ``parent`` [n,4] with the rotation-free boost (the formula of
    tests/kin_exact_reference.py): p* = p + beta (gamma^2 / (gamma + 1) beta.p - gamma E), beta = P / E_parent."""
    big_m = inv_mass(parent)
    beta = parent[:, :3] / parent[:, 3:4]
    gamma = parent[:, 3] / big_m
    bp = (beta * p[:, :3]).sum(axis=1)
    return p[:, :3] + beta * (gamma * gamma / (gamma + 1.0) * bp - gamma * p[:, 3])[:, None]


def step_rows(s: int) -> tuple[int, int]:
    return (2, 3) if s == 0 else (4 + 2 * (s - 1), 5 + 2 * (s - 1))


def recover(p4, masses) -> list[dict]:
    """Per step: ex (invariant mass of the decaying row minus its ground-state mass), theta and phi of the ejectile in
    its parent's rest frame."""
    p4 = np.asarray(p4, dtype=np.float64)
    n_steps = 1 + (p4.shape[1] - 4) // 2
    out = []
    for s in range(n_steps):
        eject, resid = step_rows(s)
        parent = p4[:, 0] + p4[:, 1] if s == 0 else p4[:, step_rows(s - 1)[1]]
        q = rest_frame(parent, p4[:, eject])
        out.append({"ex": inv_mass(p4[:, resid]) - masses[resid],
                    "theta": np.arctan2(np.hypot(q[:, 0], q[:, 1]), q[:, 2]),
                    "cos": q[:, 2] / np.sqrt((q * q).sum(axis=1)),
                    "phi": np.mod(np.arctan2(q[:, 1], q[:, 0]), TWO_PI)})
    return out


def _unit(u):
    return np.clip(u, 0.0, 1.0)


def ks_all(columns: dict) -> dict:
    """{name: (n, D, p)} of every PIT column against U(0, 1)."""
    return {k: (len(v),) + lc.ks_uniform(_unit(v)) for k, v in columns.items()}


def lag1(columns: dict) -> dict:
    """{name: corr_z of the column with itself one event id later}."""
    return {k: lc.corr_z(v[:-1], v[1:]) for k, v in columns.items()}


def cross(columns_a: dict, columns_b: dict) -> tuple[float, tuple[str, str]]:
    """Largest |corr_z| between any column of one run and any column of another (equal event ids)."""
    def scores(columns):
        z = np.stack([lc.ndtri(v) for v in columns.values()])
        z -= z.mean(axis=1, keepdims=True)
        return z / np.sqrt((z * z).sum(axis=1, keepdims=True))

    a, b = scores(columns_a), scores(columns_b)
    c = np.abs(a @ b.T) * math.sqrt(a.shape[1])
    i, j = np.unravel_index(c.argmax(), c.shape)
    return float(c[i, j]), (list(columns_a)[i], list(columns_b)[j])


# --------------------------------------------------------------------------------------------------- K1 ----
def k1_columns(vertex, p4, masses, rho_sigma: float, z_range, ex_centre: float, ex_sigma: float) -> dict:
    """PIT columns of a Reaction + Decay with a target, Gaussian ex of step 0 and PolarUniform(0, pi) on both steps."""
    vertex = np.asarray(vertex, dtype=np.float64)
    par = recover(p4, masses)
    cols = {"rho": lc.halfnormal_cdf(np.hypot(vertex[:, 0], vertex[:, 1]) / rho_sigma),
            "azimuth": np.mod(np.arctan2(vertex[:, 1], vertex[:, 0]), TWO_PI) / TWO_PI,
            "z": (vertex[:, 2] - z_range[0]) / (z_range[1] - z_range[0]),
            "ex0": lc.ndtr((par[0]["ex"] - ex_centre) / ex_sigma)}
    for s in (0, 1):
        cols[f"cos{s}"] = (par[s]["cos"] + 1.0) / 2.0
        cols[f"phi{s}"] = par[s]["phi"] / TWO_PI
    return cols


# --------------------------------------------------------------------------------------------------- K2 ----
def reaction_ex_max(m, t: float) -> float:
    """Largest excitation the reaction step accepts at beam energy ``t``: the smaller of the relativistic bound
    E_cm - m2 - m3 (reaction_allowed) and the bound of the non-relativistic threshold test (below_nr_threshold, linear
    in ex)."""
    pz = math.sqrt(t * (t + 2.0 * m[1]))
    s = m[0] + t + m[1]
    rel = math.sqrt(s * s - pz * pz) - m[2] - m[3]
    nr = m[0] + m[1] - m[2] - m[3] + t * (m[2] + m[3] - m[1]) / (m[2] + m[3])
    return min(rel, nr)


def bw_cdf(ex, rest_mass: float, centroid: float, width: float):
    """CDF of ExcitationBreitWigner(rest_mass, centroid, width) in ex = E_tot - rest_mass."""
    return lc.rel_breitwigner_cdf((np.asarray(ex, dtype=np.float64) + rest_mass) / width, (rest_mass + centroid) / width)


def geometric_chi2(attempts, p: float, n_cells: int):
    """chi-square of the counts of attempts = 1 .. n_cells - 1 and >= n_cells against the geometric law."""
    attempts = np.asarray(attempts, dtype=np.int64)
    obs = np.bincount(np.minimum(attempts, n_cells), minlength=n_cells + 1)[1:]
    k = np.arange(1, n_cells + 1)
    prob = p * (1.0 - p) ** (k - 1.0)
    prob[-1] = (1.0 - p) ** (n_cells - 1.0)
    return lc.chi2_p(obs, prob * attempts.size)


def k2_checks(p4, attempts, masses, beam: float, bw: tuple, angles, probs, width: float, pit_seed: int) -> dict:
    par = recover(p4, masses)[0]
    ex_max = reaction_ex_max(masses, beam)
    f_max = float(bw_cdf(ex_max, *bw))
    out = {"ex": (len(p4),) + lc.ks_uniform(_unit(bw_cdf(par["ex"], *bw) / f_max)),
           "attempts": geometric_chi2(attempts, f_max, 3)}
    bins = np.clip(np.floor((par["theta"] - angles[0]) / width).astype(np.int64), 0, len(angles) - 1)
    out["bin"] = lc.chi2_p(np.bincount(bins, minlength=len(angles)), np.asarray(probs) / np.sum(probs) * len(bins))
    offset = (par["theta"] - angles[bins]) / width
    out["offset"] = (len(bins),) + lc.ks_uniform(_unit(offset))
    cdf = np.concatenate([[0.0], np.cumsum(probs) / np.sum(probs)])
    v = np.random.default_rng(pit_seed).random(len(bins))
    out["bin_offset_z"] = lc.corr_z(lc.pit_discrete(bins, cdf[bins], cdf[bins + 1], v), _unit(offset))
    out["mean_attempts"] = (float(np.mean(attempts)), 1.0 / f_max)
    return out


# --------------------------------------------------------------------------------------------------- K3 ----
class K3Law:
    """Two steps with ExcitationUniform(a0, b0), (a1, b1), PolarUniform(0, pi) and no target.  Step 0 allows
    ex0 < ex_max0; step 1 allows ex1 < ex0 + q1, q1 = m(residual) - m1 - m2 (the parent's mass is m(residual) + ex0).
    The accepted events have the proposal's law restricted to that set: ex0 has density proportional to
    g(ex0) = clip((ex0 + q1 - a1) / (b1 - a1), 0, 1) on (a0, min(b0, ex_max0)), ex1 given ex0 is uniform on
    (a1, min(b1, ex0 + q1))."""

    def __init__(self, masses, beam: float, range0, range1):
        self.m = np.asarray(masses, dtype=np.float64)
        self.beam = beam
        (self.a0, self.b0), (self.a1, self.b1) = range0, range1
        self.ex_max0 = reaction_ex_max(self.m, beam)
        self.top0 = min(self.b0, self.ex_max0)
        self.q1 = self.m[3] - self.m[4] - self.m[5]
        self.p_step0 = (self.top0 - self.a0) / (self.b0 - self.a0)
        self.p_step1 = (self._h(self.top0) - self._h(self.a0)) / (self.top0 - self.a0)  # given that step 0 passed
        self.p_accept = self.p_step0 * self.p_step1

    def _h(self, x):
        """Integral of g from -inf to x: 0, then (x + c)^2 / (2 w), then w / 2 + (x - t1); c = q1 - a1, w = b1 - a1."""
        x = np.asarray(x, dtype=np.float64)
        c, w = self.q1 - self.a1, self.b1 - self.a1
        t = np.clip(x + c, 0.0, w)
        return t * t / (2.0 * w) + np.maximum(x + c - w, 0.0)

    def allowed(self, ex0, ex1):
        """The kernel's three tests in numpy on recovered parameters."""
        m, t = self.m, self.beam
        pz = np.sqrt(t * (t + 2.0 * m[1]))
        s = m[0] + t + m[1]
        ok = (m[2] + m[3] + ex0) < np.sqrt(s * s - pz * pz)                                  # reaction_allowed
        q = m[0] + m[1] - (m[2] + m[3] + ex0)
        ok &= ~(t < -q * (m[2] + m[3]) / (m[2] + m[3] - m[1]))                               # below_nr_threshold
        return ok & (((m[3] + ex0) - (m[4] + m[5] + ex1)) > 0.0)                             # inv_mass(prev) - (...) > 0

    def checks(self, p4, attempts, n_cells: int = 41) -> dict:
        par = recover(p4, self.m)
        ex0, ex1 = par[0]["ex"], par[1]["ex"]
        # (the recovered ex carry ~1e-11 MeV of rounding: the set is tested that much inside its edges)
        inside = self.allowed(ex0 - 1e-9, ex1 + 1e-9) | self.allowed(ex0 + 1e-9, ex1 - 1e-9)
        cols = {"ex0": (self._h(ex0) - self._h(self.a0)) / (self._h(self.top0) - self._h(self.a0)),
                "ex1": (ex1 - self.a1) / (np.minimum(self.b1, ex0 + self.q1) - self.a1)}
        for s in (0, 1):
            cols[f"cos{s}"] = (par[s]["cos"] + 1.0) / 2.0
            cols[f"phi{s}"] = par[s]["phi"] / TWO_PI
        out = {"outside_allowed_set": int((~inside).sum()), "ks": ks_all(cols),
               "attempts": geometric_chi2(attempts, self.p_accept, n_cells)}
        retried = np.asarray(attempts) >= 2
        out["ks_retried"] = ks_all({k: cols[k][retried] for k in ("cos0", "phi0", "cos1", "phi1")})
        worst, pair = 0.0, ("", "")
        for e in ("ex0", "ex1"):
            for a in ("cos0", "phi0", "cos1", "phi1"):
                z = abs(lc.corr_z(cols[e][retried], cols[a][retried]))
                if z > worst:
                    worst, pair = z, (e, a)
        out["angles_vs_ex_retried"] = (int(retried.sum()), worst, pair)
        out["ex0_ex1_z"] = lc.corr_z(cols["ex0"], cols["ex1"])
        return out


# ------------------------------------------------------------------------------------------------- Fano ----
def align_kept(track_xyt, kept_xyt, tol: float = 1e-9) -> np.ndarray:
    """Trajectory row of every kept sample.  generate_point_cloud keeps the rows with at least one electron, in
    order, so the kept samples are a subsequence of the rows: walk both, a row whose (x, y, time bucket) is not the
    next kept sample's was dropped.  AssertionError unless every kept sample finds its row."""
    rows = np.empty(len(kept_xyt), dtype=np.int64)
    k = 0
    for j in range(len(kept_xyt)):
        while k < len(track_xyt) and not np.abs(track_xyt[k] - kept_xyt[j]).max() <= tol:
            k += 1
        assert k < len(track_xyt), ("kept sample without a trajectory row", j)
        rows[j] = k
        k += 1
    return rows


def align_kept_fast(track_xyt, kept_xyt, tol: float = 1e-9) -> np.ndarray:
    """``align_kept`` without the Python loop where nothing was dropped in the middle (the common case)."""
    n = len(kept_xyt)
    for first in (1, 0):  # row 0 never makes electrons
        if first + n <= len(track_xyt) and (n == 0 or np.abs(track_xyt[first:first + n] - kept_xyt).max() <= tol):
            return np.arange(first, first + n, dtype=np.int64)
    return align_kept(track_xyt, kept_xyt, tol)


class FanoSamples:
    """Flat arrays over kept samples: event, row of the nucleus, trajectory row k, mean mu, electrons n."""

    def __init__(self):
        self.parts = []

    def add(self, event: int, row: int, k, mu, n):
        k = np.asarray(k, dtype=np.int64)
        self.parts.append((np.full(len(k), event, dtype=np.int64), np.full(len(k), row, dtype=np.int64), k,
                           np.asarray(mu, dtype=np.float64), np.asarray(n, dtype=np.int64)))

    def arrays(self):
        return tuple(np.concatenate([p[i] for p in self.parts]) for i in range(5))


def _paired(key_a, key_b):
    """Indices of equal keys in two arrays of unique keys."""
    _, ia, ib = np.intersect1d(key_a, key_b, assume_unique=True, return_indices=True)
    return ia, ib


def fano_checks(samples: FanoSamples, fano: float, pit_seed: int) -> dict:
    """n = trunc(mu + sqrt(F mu) Z): P(n <= k) = Phi((k + 1 - mu) / sigma) on the samples with mu - 9 sigma > 1 (a draw
    is at most 8.6 sigma from mu, so there the draw is positive and the sample is always kept)."""
    event, row, k, mu, n = samples.arrays()
    sigma = np.sqrt(fano * mu)
    use = mu - 9.0 * sigma > 1.0
    event, row, k, mu, n, sigma = (a[use] for a in (event, row, k, mu, n, sigma))
    v = np.random.default_rng(pit_seed).random(len(n))
    u = lc.pit_discrete(n, lc.ndtr((n - mu) / sigma), lc.ndtr((n + 1 - mu) / sigma), v)
    out = {"ks": (len(u),) + lc.ks_uniform(_unit(u))}
    # consecutive samples of one track: key = (event, row, k)
    key = (event * 32 + row) * 16384 + k
    order = np.argsort(key)
    key, ko, uo = key[order], k[order], u[order]
    nxt = np.flatnonzero(key[1:] == key[:-1] + 1)
    shared = ko[nxt] % 2 == 0  # (k, k + 1) with k even: the cos and sin branch of one Philox call
    for name, sel in (("lag1_shared_call", nxt[shared]), ("lag1_other", nxt[~shared])):
        out[name] = (len(sel), lc.corr_z(uo[sel], uo[sel + 1]))
    # equal k of two nuclei of one event
    rows = np.unique(row)
    a_all, b_all = [], []
    for i, ra in enumerate(rows):
        for rb in rows[i + 1:]:
            sa, sb = np.flatnonzero(row == ra), np.flatnonzero(row == rb)
            ia, ib = _paired(event[sa] * 16384 + k[sa], event[sb] * 16384 + k[sb])
            a_all.append(u[sa][ia])
            b_all.append(u[sb][ib])
    a_all, b_all = np.concatenate(a_all), np.concatenate(b_all)
    out["nuclei_equal_k"] = (len(a_all), lc.corr_z(a_all, b_all))
    # equal (row, k) of events e and e + 1
    rk = row * 16384 + k
    a_all, b_all = [], []
    for e in np.unique(event)[:-1]:
        sa, sb = np.flatnonzero(event == e), np.flatnonzero(event == e + 1)
        if len(sa) and len(sb):
            ia, ib = _paired(rk[sa], rk[sb])
            a_all.append(u[sa][ia])
            b_all.append(u[sb][ib])
    a_all, b_all = np.concatenate(a_all), np.concatenate(b_all)
    out["events_equal_row_k"] = (len(a_all), lc.corr_z(a_all, b_all))
    out["u"] = (event, row, k, u)
    return out


def fano_same_samples_z(checks_a: dict, checks_b: dict) -> tuple[int, float]:
    """corr_z between two runs of the same tracks (other event ids or seed) at equal (event index, row, k)."""
    ea, ra, ka, ua = checks_a["u"]
    eb, rb, kb, ub = checks_b["u"]
    ia, ib = _paired((ea * 32 + ra) * 16384 + ka, (eb * 32 + rb) * 16384 + kb)
    return len(ia), lc.corr_z(ua[ia], ub[ib])


# ----------------------------------------------------------------------------------------------- jitter ----
def split_cloud(points):
    """Cloud rows (pad, time bucket + jitter, charge) -> (pad, tb, jitter)."""
    pad = points[:, 0].astype(np.int64)
    tb = np.floor(points[:, 1]).astype(np.int64)
    return pad, tb, points[:, 1] - tb


def _key(pad, tb):
    return tb * 16384 + pad


def jitter_within(offsets, points) -> dict:
    """Over the events of a CSR cloud: the jitter's law, and its corr_z between (pad, tb) and (pad, tb + 1) and
    between (pad, tb) and (pad + 1, tb) of one event."""
    pad, tb, jit = split_cloud(points)
    out = {"ks": (len(jit),) + lc.ks_uniform(jit)}
    pairs = {"tb_next": ([], []), "pad_next": ([], [])}
    for e in range(len(offsets) - 1):
        s = slice(offsets[e], offsets[e + 1])
        key = _key(pad[s], tb[s])
        for name, other in (("tb_next", _key(pad[s], tb[s] + 1)), ("pad_next", _key(pad[s] + 1, tb[s]))):
            ia, ib = _paired(other, key)
            pairs[name][0].append(jit[s][ia])
            pairs[name][1].append(jit[s][ib])
    for name, (a, b) in pairs.items():
        a, b = np.concatenate(a), np.concatenate(b)
        out[name] = (len(a), lc.corr_z(a, b))
    return out


def jitter_equal_keys(offsets_a, points_a, offsets_b, points_b, shift: int = 0) -> tuple[int, float]:
    """corr_z of the jitter at equal (pad, tb) between event i + shift of cloud a and event i of cloud b."""
    pa, ta, ja = split_cloud(points_a)
    pb, tb_, jb = split_cloud(points_b)
    xs, ys = [], []
    for e in range(len(offsets_b) - 1 - shift):
        sa = slice(offsets_a[e + shift], offsets_a[e + shift + 1])
        sb = slice(offsets_b[e], offsets_b[e + 1])
        ia, ib = _paired(_key(pa[sa], ta[sa]), _key(pb[sb], tb_[sb]))
        xs.append(ja[sa][ia])
        ys.append(jb[sb][ib])
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    return len(xs), lc.corr_z(xs, ys)


# ------------------------------------------------------------------------------- Monte-Carlo diffusion ----
def mc_expected(plane, cx: float, cy: float, sigmas, n_primary: int, reach: float = 10.0) -> tuple[dict, float]:
    """({pad: expected primaries}, expected lost) over samples at one centre: for every sample the exact masses
    [Phi((x_(i+1) - cx) / sigma) - Phi((x_i - cx) / sigma)] [same in y] of the whole-mm cells within ``reach`` sigma,
    summed per pad of the look-up table; cells of beam pads, gaps and off the plane count as lost (as does the
    1e-23 beyond the reach)."""
    expect: dict = {}
    for sigma in np.atleast_1d(sigmas):
        def masses(c):
            lo = math.floor((c - reach * sigma) * 1000.0)
            hi = math.floor((c + reach * sigma) * 1000.0) + 1
            edges = np.arange(lo, hi + 1, dtype=np.float64) * 1.0e-3
            return edges[:-1], np.diff(lc.ndtr((edges - c) / sigma))
        x0, mx = masses(cx)
        y0, my = masses(cy)
        gx, gy = np.meshgrid(x0 + 0.5e-3, y0 + 0.5e-3, indexing="ij")  # cell centres: floor() gives the cell back
        pad = plane.pad_of(gx, gy)
        mass = np.outer(mx, my) * n_primary
        pads, inverse = np.unique(pad.ravel(), return_inverse=True)
        for p, w in zip(pads, np.bincount(inverse.ravel(), weights=mass.ravel())):
            if p >= 0:
                expect[int(p)] = expect.get(int(p), 0.0) + float(w)
    total = float(n_primary) * len(np.atleast_1d(sigmas))
    return expect, total - sum(expect.values())


def mc_checks(observed: dict, expect: dict, lost: float, total: int) -> dict:
    """observed {pad: primaries} -> chi-square over the pads and the lost cell; pads hit that the law gives nothing."""
    unexpected = sorted(set(observed) - set(expect))
    pads = sorted(expect)
    obs = np.array([observed.get(p, 0) for p in pads] + [total - sum(observed.values())], dtype=np.float64)
    exp = np.array([expect[p] for p in pads] + [lost])
    return {"chi2": lc.chi2_p(obs, exp), "unexpected": unexpected, "pads_hit": len(observed),
            "lost_fraction": lost / total}
