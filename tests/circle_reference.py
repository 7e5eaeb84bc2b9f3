"""The contract of the geometric circle fit (include/attpc_engine.h, "geometric circle fit") restated in numpy, on top
of ``tests/estimate_reference.py``: the per-point terms as f64 arrays (one rounding per numpy operation, sqrt correctly
rounded), the order of summation with its lane partition and xor tree, the 3x3 elimination and the iteration with Python
floats in the header's order of operations.  ``records`` returns ``ESTIMATE_DTYPE`` records to compare bit for bit."""
import math

import numpy as np

from attpc_engine_amd._abi import (ESTIMATE_DTYPE, EST_CAPPED, EST_MAX_FIT, EST_NOT_CONVERGED, EST_NO_CIRCLE, EST_NO_SLOPE,
                                   EST_ON_AXIS, EST_RANGE)
from tests import estimate_reference as est

NAN = float("nan")
LAMBDA0, LAMBDA_ACCEPT, LAMBDA_REJECT = 2.0 ** -10, 0.04, 10.0
SUMS = ("f", "uu", "uv", "vv", "u", "v", "gu", "gv", "g")
LANES = np.arange(64)


class Settings:
    def __init__(self, max_evaluations=32, tolerance=2.0 ** -7):
        self.max_evaluations, self.tolerance = int(max_evaluations), float(tolerance)


def lane_sum(terms):
    """The contract's sum of ``terms`` (rank order): rank i to lane i mod 64, each lane ascending onto +0.0, then
    s[lane] + s[lane xor off] for off = 32 .. 1.  (A lane's partial sum is never -0.0, so the +0.0 that pads the last
    row changes no bit.)"""
    terms = np.asarray(terms, dtype=np.float64)
    padded = np.zeros(-(-len(terms) // 64) * 64, dtype=np.float64)
    padded[:len(terms)] = terms
    lanes = np.zeros(64, dtype=np.float64)
    for row in padded.reshape(-1, 64):
        lanes = lanes + row
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[LANES ^ off]
    assert np.all(lanes.view(np.int64) == lanes.view(np.int64)[0]) or np.all(np.isnan(lanes))
    return float(lanes[0])


def evaluate(u, v, a, b, R):
    """The nine sums at p = (a, b, R) for the integer arrays u, v."""
    with np.errstate(all="ignore"):
        dx, dy = u.astype(np.float64) - a, v.astype(np.float64) - b
        r = np.sqrt(dx * dx + dy * dy)
        zero = r == 0.0
        U = np.where(zero, 0.0, dx / np.where(zero, 1.0, r))
        V = np.where(zero, 0.0, dy / np.where(zero, 1.0, r))
        g = r - R
        terms = dict(f=g * g, uu=U * U, uv=U * V, vv=V * V, u=U, v=V, gu=g * U, gv=g * V, g=g)
        return {name: lane_sum(terms[name]) for name in SUMS}


def _div(x, y):
    """x / y as IEEE does it (Python raises at y == 0)."""
    with np.errstate(all="ignore"):
        return float(np.float64(x) / np.float64(y))


def step(k, M, lam):
    """d of (N + lambda diag N) d = rhs, by the header's elimination."""
    m00, m11, m22 = k["uu"] + lam * k["uu"], k["vv"] + lam * k["vv"], M + lam * M
    l10, l20 = _div(k["uv"], m00), _div(k["u"], m00)
    a11, a12, b1 = m11 - l10 * k["uv"], k["v"] - l10 * k["u"], k["gv"] - l10 * k["gu"]
    a22, b2 = m22 - l20 * k["u"], k["g"] - l20 * k["gu"]
    l21 = _div(a12, a11)
    c22, c2 = a22 - l21 * a12, b2 - l21 * b1
    d2 = _div(c2, c22)
    d1 = _div(b1 - a12 * d2, a11)
    d0 = _div(k["gu"] - k["uv"] * d1 - k["u"] * d2, m00)
    return d0, d1, d2


def fit(u, v, start, settings, trace=None):
    """The iteration from ``start`` = (a, b, R) on the integer arrays u, v -> (a, b, R, evaluations, converged, F).
    ``trace``: a list that receives (accepted, lambda) of every trial."""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    a, b, R = (float(x) for x in start)
    k = evaluate(u, v, a, b, R)
    evaluations, lam, M = 1, LAMBDA0, float(len(u))
    while evaluations < settings.max_evaluations:
        d = step(k, M, lam)
        ta, tb, tR = a + d[0], b + d[1], R + d[2]
        kt = evaluate(u, v, ta, tb, tR)
        evaluations += 1
        accepted = kt["f"] <= k["f"] and tR > 0.0
        if trace is not None:
            trace.append((accepted, lam))
        if accepted:
            a, b, R, k = ta, tb, tR, kt
            lam = LAMBDA_ACCEPT * lam
            if max(abs(d[0]), abs(d[1]), abs(d[2])) <= settings.tolerance:
                return a, b, R, evaluations, True, k["f"]
        else:
            lam = LAMBDA_REJECT * lam
    return a, b, R, evaluations, False, k["f"]


def kasa(m, k):
    """(uc, vc, r2) of step 6 on the integer sums, or None (NO_CIRCLE)."""
    m = float(m)
    Su, Sv, Suu, Suv, Svv = (float(k[n]) for n in ("u", "v", "uu", "uv", "vv"))
    Suuu, Suvv, Svvv, Svuu = (float(k[n]) for n in ("uuu", "uvv", "vvv", "vuu"))
    A = m * Suu - Su * Su
    B = m * Suv - Su * Sv
    C = m * Svv - Sv * Sv
    D = (m * (Suvv + Suuu) - Su * (Suu + Svv)) / 2.0
    E = (m * (Svuu + Svvv) - Sv * (Suu + Svv)) / 2.0
    den = A * C - B * B
    if den == 0.0:
        return None
    uc = (D * C - B * E) / den
    vc = (A * E - B * D) / den
    r2 = (Suu + Svv - 2.0 * uc * Su - 2.0 * vc * Sv) / m + uc * uc + vc * vc
    return (uc, vc, r2) if r2 > 0.0 else None


def integer_sums(u, v):
    """The sums of step 5 that the Kasa circle needs, exact."""
    u, v = [int(x) for x in u], [int(x) for x in v]
    return dict(u=sum(u), v=sum(v), uu=sum(x * x for x in u), uv=sum(x * y for x, y in zip(u, v)), vv=sum(y * y for y in v),
                uuu=sum(x ** 3 for x in u), uvv=sum(x * y * y for x, y in zip(u, v)), vvv=sum(y ** 3 for y in v),
                vuu=sum(y * x * x for x, y in zip(u, v)))


def from_circle(rec, circle, X0, Y0, Z0, m, k_S, k_w, field):
    """cx .. vz and brho of ``rec`` (the Kasa record: slope, means and dedx stay) from the circle (a, b, R), and the
    status bits ON_AXIS again, as step 6 makes them."""
    a, b, R = circle
    X0, Y0, Z0, m = float(X0), float(Y0), float(Z0), float(m)
    out = dict(rec)
    out["status"] &= ~EST_ON_AXIS
    for name in ("vx", "vy", "vz", "brho"):
        out[name] = NAN
    out["cx"], out["cy"], out["radius"] = (X0 + a) / 16.0, (Y0 + b) / 16.0, R / 16.0
    c = math.sqrt(out["cx"] * out["cx"] + out["cy"] * out["cy"])
    vertex = c != 0.0
    if not vertex:
        out["status"] |= EST_ON_AXIS
    else:
        out["vx"] = out["cx"] * (1.0 - out["radius"] / c)
        out["vy"] = out["cy"] * (1.0 - out["radius"] / c)
    if not out["status"] & EST_NO_SLOPE:
        slope = out["slope"]
        if vertex:
            a0 = (float(k_w) - slope * float(k_S)) / m
            gx, gy = X0 - 16.0 * out["vx"], Y0 - 16.0 * out["vy"]
            chord0 = math.sqrt(gx * gx + gy * gy)
            out["vz"] = (Z0 + a0 - slope * chord0) / 16.0
        out["brho"] = field * out["radius"] * 1.0e-3 * math.sqrt(1.0 + slope * slope)
    return out


def segment(rows, params):
    """The fit segment of steps 1 to 4: int64 [m, 4] (X, Y, Z, I) in the direction of travel, or None (no fit)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    x, y, z, integral = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) <= 320.0) & (np.abs(y) <= 320.0) & (np.abs(z) <= 8192.0) & (np.abs(integral) < 2147483648.0)
    q = np.rint(np.where(ok[:, None], np.stack([16.0 * x, 16.0 * y, 16.0 * z, integral], axis=1), 0.0)).astype(np.int64)
    rb = min(int(np.rint(16.0 * params.beam_region_radius)), (1 << 31) - 1)
    used = q[ok & (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] >= rb * rb)]
    if len(used) < params.min_points:
        return None
    rho = used[:, 0] ** 2 + used[:, 1] ** 2
    if rho[0] > rho[-1]:
        used = used[::-1]
    return used[:min(max((len(used) + 1) // 2, params.min_points), EST_MAX_FIT)]


def track_record(rows, params, settings):
    """The record of one (event, position) with the stage on."""
    rec = est.track_record(rows, params)
    seg = segment(rows, params)
    if seg is None or rec["status"] & EST_NO_CIRCLE:
        return rec
    assert len(seg) == rec["n_fit"]
    u, v, w = seg[:, 0] - seg[0, 0], seg[:, 1] - seg[0, 1], seg[:, 2] - seg[0, 2]
    uc, vc, r2 = kasa(len(seg), integer_sums(u, v))
    a, b, R, evaluations, converged, _ = fit(u, v, (uc, vc, math.sqrt(r2)), settings)
    # S_i again for the two sums the vertex needs
    S = np.concatenate([[0], np.cumsum([int(np.rint(math.sqrt(float(dx * dx + dy * dy))))
                                         for dx, dy in zip(np.diff(seg[:, 0]), np.diff(seg[:, 1]))])]).astype(np.int64)
    out = from_circle(rec, (a, b, R), seg[0, 0], seg[0, 1], seg[0, 2], len(seg), int(S.sum()), int(w.sum()), params.magnetic_field)
    out["reserved"] = evaluations
    if not converged:
        out["status"] |= EST_NOT_CONVERGED
    return out


def records(offsets, rows, labels, indices, params, settings):
    """Records [n_events, len(indices)] of rows in CSR form with the stage on."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    labels = np.asarray(labels, dtype=np.int64)
    out = np.zeros((len(offsets) - 1, len(indices)), dtype=ESTIMATE_DTYPE)
    for e in range(len(offsets) - 1):
        ev_rows, ev_labels = rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        for s, index in enumerate(indices):
            first = list(indices).index(index) == s  # a label given twice goes to its first position
            rec = track_record(ev_rows[ev_labels == index], params, settings) if first and index >= 0 else est.no_fit(0, 0, False)
            for name, value in rec.items():
                out[e, s][name] = value
    return out


# ---------------------------------------------------------------- hand-made point sets ----
def arc_points(m, radius=4800.0, centre=(700.0, -300.0), start=0.4, arc_deg=20.0, jitter=0.0, rng=None):
    """Integer (u, v) of m points on an arc (units), relative to the first: what step 5 hands the fit."""
    t = start + np.radians(arc_deg) * np.arange(m) / max(m - 1, 1)
    x, y = centre[0] + radius * np.cos(t), centre[1] + radius * np.sin(t)
    if jitter:
        x, y = x + rng.normal(0.0, jitter, m), y + rng.normal(0.0, jitter, m)
    X, Y = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    return X - X[0], Y - Y[0]


def kasa_start(u, v):
    """(a, b, R) of the Kasa circle of the points, or None."""
    k = kasa(len(u), integer_sums(u, v))
    return None if k is None else (k[0], k[1], math.sqrt(k[2]))
