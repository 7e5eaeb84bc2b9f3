"""Statistics for the tests of the laws of the engine's random draws (tests/law_analysis.py, test_laws_cpu.py,
test_gpu_laws.py): numpy, math and torch on the CPU only, no scipy, and none of the engine's arithmetic.
``test_laws_cpu.py`` holds every function here to scipy where scipy imports.

One rule for every check built on these (fixed before anything was run): an unmutated law asserts p >= ``P_PASS``, an
unmutated independence check |corr_z| <= ``Z_PASS``; a mutant has to reach p < ``P_MUTANT`` or |corr_z| > ``Z_MUTANT``
at the same size."""
from __future__ import annotations

import math

import numpy as np
import torch

P_PASS, Z_PASS = 1.0e-6, 5.0
P_MUTANT, Z_MUTANT = 1.0e-12, 8.0


# ------------------------------------------------------------------------------------------ closed-form CDFs ----
def ndtr(x) -> np.ndarray:
    """Phi(x), f64."""
    return torch.special.ndtr(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy()


def ndtri(u) -> np.ndarray:
    """Phi^-1(u), f64; u is kept inside (0, 1) by a step of the engine's 53-bit uniforms, so a value of exactly 0 or 1
    maps to -+8.2 and not to -+inf."""
    u = np.clip(np.asarray(u, dtype=np.float64), 2.0 ** -53, 1.0 - 2.0 ** -53)
    return torch.special.ndtri(torch.as_tensor(u)).numpy()


def halfnormal_cdf(x) -> np.ndarray:
    """P(|Z| <= x) = erf(x / sqrt 2), x >= 0."""
    x = np.asarray(x, dtype=np.float64)
    return torch.special.erf(torch.as_tensor(np.maximum(x, 0.0) / math.sqrt(2.0))).numpy()


def rel_breitwigner_cdf(x, rho: float) -> np.ndarray:
    """CDF of scipy's ``rel_breitwigner(rho)`` (density proportional to 1 / ((x^2 - rho^2)^2 + rho^2) on x > 0), written
    out in arctan and log.  The quartic factors as (x^2 + s x + r)(x^2 - s x + r), r = rho sqrt(rho^2 + 1),
    s = sqrt(2 (r + rho^2)); with w = sqrt(2 (r - rho^2)) each factor is (x +- s/2)^2 + w^2 / 4, and

        G(x) = [ 1/2 ln((x^2 + s x + r) / (x^2 - s x + r)) + (s / w) (atan((2x + s) / w) + atan((2x - s) / w)) ] / (2 s r)

    has G(0) = 0 and G(inf) = pi / (2 w r).  r - rho^2 is taken as rho / (sqrt(rho^2 + 1) + rho): the difference itself
    loses 8 digits at the rho ~ 1e4 of a nuclear state."""
    x = np.asarray(x, dtype=np.float64)
    root = math.sqrt(rho * rho + 1.0)
    r = rho * root
    s = math.sqrt(2.0 * (r + rho * rho))
    w = math.sqrt(2.0 * rho / (root + rho))
    plus = (x + 0.5 * s) ** 2 + 0.25 * w * w
    minus = (x - 0.5 * s) ** 2 + 0.25 * w * w
    g = 0.5 * np.log(plus / minus) + (s / w) * (np.arctan((2.0 * x + s) / w) + np.arctan((2.0 * x - s) / w))
    return np.where(x > 0.0, g * (w / (s * math.pi)), 0.0)  # G / (2 s r) / (pi / (2 w r))


# -------------------------------------------------------------------------------------------------- p-values ----
def kolmogorov_sf(x: float) -> float:
    """Q(x) = P(sqrt(n) D > x) for n -> infinity: the alternating series 2 sum (-1)^(k-1) exp(-2 k^2 x^2) where it
    converges fast, the theta-function form 1 - sqrt(2 pi) / x sum exp(-(2k-1)^2 pi^2 / (8 x^2)) below x = 1."""
    if x <= 0.0:
        return 1.0
    if x < 1.0:
        t = sum(math.exp(-((2 * k - 1) ** 2) * math.pi ** 2 / (8.0 * x * x)) for k in range(1, 8))
        return 1.0 - math.sqrt(2.0 * math.pi) / x * t
    return 2.0 * sum((-1.0) ** (k - 1) * math.exp(-2.0 * k * k * x * x) for k in range(1, 8))


def ks_uniform(u) -> tuple[float, float]:
    """(D, p) of the two-sided Kolmogorov-Smirnov test of ``u`` against U(0, 1).  p is the limiting law
    Q(sqrt(n) D) with NO finite-n correction (Stephens' sqrt(n) + 0.12 + 0.11 / sqrt(n) moves x by less than 1e-3 of
    itself at the n >= 1e4 of every check here)."""
    u = np.sort(np.asarray(u, dtype=np.float64).ravel())
    n = u.size
    assert n > 0 and u[0] >= 0.0 and u[-1] <= 1.0, (n, u[0] if n else None, u[-1] if n else None)
    i = np.arange(1, n + 1, dtype=np.float64)
    d = float(max((i / n - u).max(), (u - (i - 1.0) / n).max()))
    return d, kolmogorov_sf(math.sqrt(n) * d)


def gammaincc(a: float, x: float) -> float:
    """Regularised upper incomplete gamma Q(a, x): the series of P for x < a + 1, Lentz's continued fraction of Q
    above (Numerical Recipes' gser / gcf), in plain floats; relative accuracy ~1e-13 down to the smallest normal."""
    if x <= 0.0:
        return 1.0
    log_front = -x + a * math.log(x) - math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        k = a
        for _ in range(100000):
            k += 1.0
            term *= x / k
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return 1.0 - total * math.exp(log_front)
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * math.exp(log_front)


def chi2_sf(chi2: float, dof: int) -> float:
    return gammaincc(0.5 * dof, 0.5 * chi2)


def wilson_hilferty_sf(chi2: float, dof: int) -> float:
    """The tail tests/test_gpu_trace_noise.py uses: (chi2 / dof)^(1/3) is close to normal with mean 1 - 2 / (9 dof) and
    variance 2 / (9 dof).  Good to a few per cent near its 1e-6 threshold; its relative error grows without bound
    in the far tail (test_laws_cpu.py prints it), so ``chi2_p`` does not use it: a mutant is judged at 1e-12."""
    z = ((chi2 / dof) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * dof))) / math.sqrt(2.0 / (9.0 * dof))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


POOL_BELOW = 20.0


def chi2_p(obs, exp) -> tuple[float, int, float]:
    """(chi2, dof, p) of Pearson's chi-square of the counts ``obs`` against the expectations ``exp`` (same total):
    cells with an expectation below 20 are pooled into one, dof = cells - 1, p from the exact chi-square tail
    (``chi2_sf``)."""
    obs = np.asarray(obs, dtype=np.float64).ravel()
    exp = np.asarray(exp, dtype=np.float64).ravel()
    assert obs.shape == exp.shape and abs(obs.sum() - exp.sum()) <= 1e-9 * max(1.0, exp.sum()), (obs.sum(), exp.sum())
    small = exp < POOL_BELOW
    if small.any():
        obs = np.append(obs[~small], obs[small].sum())
        exp = np.append(exp[~small], exp[small].sum())
        if exp[-1] == 0.0:  # the pooled cell holds nothing but impossible outcomes
            assert obs[-1] == 0.0, obs[-1]
            obs, exp = obs[:-1], exp[:-1]
    dof = len(obs) - 1
    assert dof >= 1, dof
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    return chi2, dof, chi2_sf(chi2, dof)


# --------------------------------------------------------------------------------------------- independence ----
def corr_z(a, b) -> float:
    """Pearson r of the normal scores Phi^-1(a), Phi^-1(b) of two columns of probability-integral-transformed values,
    times sqrt(n): standard normal for independent columns."""
    a = ndtri(np.asarray(a).ravel())
    b = ndtri(np.asarray(b).ravel())
    assert a.shape == b.shape and a.size >= 3, (a.shape, b.shape)
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()) * math.sqrt(a.size))


def corr_matrix_z(columns: dict) -> tuple[float, tuple[str, str]]:
    """Largest off-diagonal |corr_z| of named PIT columns and the pair that has it."""
    names = list(columns)
    z = np.stack([ndtri(columns[k]) for k in names])
    z -= z.mean(axis=1, keepdims=True)
    z /= np.sqrt((z * z).sum(axis=1, keepdims=True))
    c = (z @ z.T) * math.sqrt(z.shape[1])
    np.fill_diagonal(c, 0.0)
    i, j = np.unravel_index(np.abs(c).argmax(), c.shape)
    return float(abs(c[i, j])), (names[i], names[j])


def pit_discrete(k, cdf_lo, cdf_hi, v) -> np.ndarray:
    """Randomised probability-integral transform of the integer draws ``k``: lo + v (hi - lo) with lo = P(n < k),
    hi = P(n <= k) and v uniform from ``numpy.random.default_rng`` at a seed written in the test; U(0, 1) iff k has
    the law the two CDF values came from."""
    k = np.asarray(k)
    assert (k == np.trunc(k)).all()
    cdf_lo = np.asarray(cdf_lo, dtype=np.float64)
    assert cdf_lo.shape == k.shape
    return cdf_lo + np.asarray(v, dtype=np.float64) * (np.asarray(cdf_hi, dtype=np.float64) - cdf_lo)
