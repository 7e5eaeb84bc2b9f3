"""The contract of the track estimates (include/attpc_engine.h, "track estimates of the trace rows") restated in
numpy: quantisation and the choice of the rows in int64 arrays, the moment sums as exact integers (asserted to fit
int64), the closed form with Python floats in the header's order of operations -- one rounding per operation, math.sqrt
correctly rounded.  ``records`` returns ``ESTIMATE_DTYPE`` records [n_events, n_sim] to compare bit for bit."""
import math

import numpy as np

from attpc_engine_amd._abi import (ESTIMATE_DTYPE, EST_CAPPED, EST_EMPTY, EST_FEW, EST_MAX_FIT, EST_NO_CIRCLE, EST_NO_SLOPE,
                                   EST_ON_AXIS, EST_RANGE)

NAN = float("nan")
F64_FIELDS = ("cx", "cy", "radius", "vx", "vy", "vz", "slope", "x_mean", "y_mean", "dedx", "brho")
INT_FIELDS = ("n_rows", "n_used", "n_fit", "status", "direction", "reserved", "charge", "arc")
I64_MAX = (1 << 63) - 1


class Params:
    def __init__(self, beam_region_radius=25.0, min_points=30, magnetic_field=2.85):
        self.beam_region_radius, self.min_points, self.magnetic_field = float(beam_region_radius), int(min_points), float(magnetic_field)


def no_fit(n_rows, n_used, out_of_range):
    rec = dict.fromkeys(F64_FIELDS, NAN)
    rec.update(n_rows=n_rows, n_used=n_used, n_fit=0, direction=0, reserved=0, charge=0, arc=0,
               status=(EST_EMPTY if n_rows == 0 else EST_FEW) | (EST_RANGE if out_of_range else 0))
    return rec


def closed_form(m, X0, Y0, Z0, k, arc, field):
    """Step 6 on the integer sums ``k`` -> (status bits, the f64 fields)."""
    m, X0, Y0, Z0 = float(m), float(X0), float(Y0), float(Z0)
    Su, Sv, Suu, Suv, Svv = (float(k[n]) for n in ("u", "v", "uu", "uv", "vv"))
    Suuu, Suvv, Svvv, Svuu = (float(k[n]) for n in ("uuu", "uvv", "vvv", "vuu"))
    SS, Sw, SSS, SSw = (float(k[n]) for n in ("S", "w", "SS", "Sw"))
    status = 0
    out = dict.fromkeys(F64_FIELDS, NAN)
    A = m * Suu - Su * Su
    B = m * Suv - Su * Sv
    C = m * Svv - Sv * Sv
    D = (m * (Suvv + Suuu) - Su * (Suu + Svv)) / 2.0
    E = (m * (Svuu + Svvv) - Sv * (Suu + Svv)) / 2.0
    den = A * C - B * B
    circle = den != 0.0
    if circle:
        uc = (D * C - B * E) / den
        vc = (A * E - B * D) / den
        r2 = (Suu + Svv - 2.0 * uc * Su - 2.0 * vc * Sv) / m + uc * uc + vc * vc
        circle = r2 > 0.0
        if circle:
            out["cx"] = (X0 + uc) / 16.0
            out["cy"] = (Y0 + vc) / 16.0
            out["radius"] = math.sqrt(r2) / 16.0
    vertex = circle
    if not circle:
        status |= EST_NO_CIRCLE
    else:
        c = math.sqrt(out["cx"] * out["cx"] + out["cy"] * out["cy"])
        if c == 0.0:
            status |= EST_ON_AXIS
            vertex = False
        else:
            out["vx"] = out["cx"] * (1.0 - out["radius"] / c)
            out["vy"] = out["cy"] * (1.0 - out["radius"] / c)
    sden = m * SSS - SS * SS
    if sden == 0.0:
        status |= EST_NO_SLOPE
    else:
        b = (m * SSw - SS * Sw) / sden
        out["slope"] = b
        if vertex:
            a0 = (Sw - b * SS) / m
            gx = X0 - 16.0 * out["vx"]
            gy = Y0 - 16.0 * out["vy"]
            chord0 = math.sqrt(gx * gx + gy * gy)
            out["vz"] = (Z0 + a0 - b * chord0) / 16.0
        if circle:
            out["brho"] = field * out["radius"] * 1.0e-3 * math.sqrt(1.0 + b * b)
    out["x_mean"] = (X0 + Su / m) / 16.0
    out["y_mean"] = (Y0 + Sv / m) / 16.0
    out["dedx"] = NAN if arc == 0 else float(k["I"]) / (float(arc) / 16.0)
    return status, out


def track_record(rows, params):
    """The record of one (event, position): ``rows`` [n, 8] are the event's rows of the label, in delivered order."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    x, y, z, integral = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) <= 320.0) & (np.abs(y) <= 320.0) & (np.abs(z) <= 8192.0) & (np.abs(integral) < 2147483648.0)
    q = np.where(ok[:, None], np.stack([16.0 * x, 16.0 * y, 16.0 * z, integral], axis=1), 0.0)
    q = np.rint(q).astype(np.int64)  # half to even
    rb = min(int(np.rint(16.0 * params.beam_region_radius)), (1 << 31) - 1)
    used = ok & (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] >= rb * rb)
    n_rows, n_used, out_of_range = len(rows), int(used.sum()), bool((~ok).any())
    if n_used < params.min_points:
        return no_fit(n_rows, n_used, out_of_range)
    u_rows = q[used]
    rho = u_rows[:, 0] ** 2 + u_rows[:, 1] ** 2
    direction = 1 if rho[0] <= rho[-1] else -1
    if direction < 0:
        u_rows = u_rows[::-1]
    m_full = max((n_used + 1) // 2, params.min_points)
    m = min(m_full, EST_MAX_FIT)
    seg = [[int(v) for v in row] for row in u_rows[:m]]
    X0, Y0, Z0, _ = seg[0]
    k = dict.fromkeys(("u", "v", "uu", "uv", "vv", "uuu", "uvv", "vvv", "vuu", "S", "w", "SS", "Sw", "I"), 0)
    S = 0
    for i, (X, Y, Z, I) in enumerate(seg):
        if i:
            dx, dy = X - seg[i - 1][0], Y - seg[i - 1][1]
            S += int(np.rint(math.sqrt(float(dx * dx + dy * dy))))
        u, v, w = X - X0, Y - Y0, Z - Z0
        for name, term in (("u", u), ("v", v), ("uu", u * u), ("uv", u * v), ("vv", v * v), ("uuu", u * u * u),
                           ("uvv", u * v * v), ("vvv", v * v * v), ("vuu", v * u * u), ("S", S), ("w", w), ("SS", S * S),
                           ("Sw", S * w), ("I", I)):
            k[name] += term
    assert all(abs(v) <= I64_MAX for v in k.values())  # the header's bound
    status, f64 = closed_form(m, X0, Y0, Z0, k, S, params.magnetic_field)
    status |= (EST_RANGE if out_of_range else 0) | (EST_CAPPED if m_full > EST_MAX_FIT else 0)
    return dict(f64, n_rows=n_rows, n_used=n_used, n_fit=m, status=status, direction=direction, reserved=0,
                charge=k["I"], arc=S)


def records(offsets, rows, labels, indices, params):
    """Records [n_events, len(indices)] of rows in CSR form."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    labels = np.asarray(labels, dtype=np.int64)
    out = np.zeros((len(offsets) - 1, len(indices)), dtype=ESTIMATE_DTYPE)
    for e in range(len(offsets) - 1):
        ev_rows, ev_labels = rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        for s, index in enumerate(indices):
            first = list(indices).index(index) == s  # a label given twice goes to its first position
            rec = track_record(ev_rows[ev_labels == index], params) if first and index >= 0 else no_fit(0, 0, False)
            for name, value in rec.items():
                out[e, s][name] = value
    return out


def assert_same_records(got, want):
    """Integer fields equal, f64 fields bit for bit with NaN in the same places."""
    assert got.shape == want.shape and got.dtype == want.dtype == ESTIMATE_DTYPE
    for name in INT_FIELDS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for name in F64_FIELDS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=name)
        keep = ~np.isnan(a)
        np.testing.assert_array_equal(a.view(np.int64)[keep], b.view(np.int64)[keep], err_msg=name)


# ---------------------------------------------------------------- hand-made tracks ----
def spyral_rows(X, Y, Z, integral=100.0):
    """Rows [n, 8] with the given coordinates in UNITS (1/16 mm), exact in f64."""
    X, Y, Z = (np.asarray(v, dtype=np.float64) for v in (X, Y, Z))
    rows = np.zeros((len(X), 8), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2] = X / 16.0, Y / 16.0, Z / 16.0
    rows[:, 3], rows[:, 4] = 50.0, integral
    return rows


def arc_track(n, radius_mm=140.0, centre_mm=(150.0, 20.0), turn=0.9, z0_mm=100.0, dz_mm=2.5, phase=3.3, jitter=0.0, rng=None):
    """n rows along a circle arc that starts near the beam axis, z rising; off the quantisation grid (the kernel
    quantises), optionally scattered by ``jitter`` mm."""
    t = phase - turn * np.arange(n) / max(n - 1, 1)
    x = centre_mm[0] + radius_mm * np.cos(t)
    y = centre_mm[1] + radius_mm * np.sin(t)
    z = z0_mm + dz_mm * np.arange(n)
    if jitter:
        x, y = x + rng.normal(0.0, jitter, n), y + rng.normal(0.0, jitter, n)
    rows = np.zeros((n, 8), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = x, y, z, 80.0
    rows[:, 4] = 500.0 + 3.0 * np.arange(n) + 0.5  # (ties of rint: half to even)
    return rows
