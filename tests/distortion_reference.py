"""The drift distortion of one track record (include/attpc_engine.h, "drift distortion") restated in numpy, on its
own: nothing of the package's ``detector.distortion`` is used.  Every operation is one numpy f64 operation, in the
written order of the contract, so the result is the contract's to the last bit.

``Map`` is the descriptor (steps, origin, the three tables or None); ``shift_records(map, records)`` gives the shifted
records [n, 4].  ``mutant`` names one deliberate departure from the contract (``MUTANTS``): each is what a plausible
slip in the kernel would compute, and tests/test_distortion_cpu.py shows that the bit-for-bit comparison catches it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MUTANTS = ("swapped_weights", "azimuthal_sign", "clamp_as_cell", "no_tb_origin", "shift_on_axis")


@dataclass
class Map:
    rho_step: float
    tau_step: float
    tb_origin: float
    radial: np.ndarray | None     # [n_rho, n_tau] m
    azimuthal: np.ndarray | None  # [n_rho, n_tau] m of arc
    time: np.ndarray | None       # [n_rho, n_tau] time buckets

    @property
    def shape(self):
        return next(t.shape for t in (self.radial, self.azimuthal, self.time) if t is not None)


def _cell(v, step, n, mutant):
    """Step 2: (cell, weight) of v / step clamped to [0, n - 1]."""
    a = v / step
    a = np.where(a > float(n - 1), float(n - 1), a)
    a = np.where(a < 0.0, 0.0, a)
    whole = np.floor(a).astype(np.int64)
    if mutant == "clamp_as_cell":  # the clamped node taken as the cell: the last node reads past its row
        cell = np.minimum(whole, n - 1)
        return cell, a - cell
    cell = np.minimum(whole, n - 2)
    return cell, a - cell


def _value(table, i, j, fr, fs, shape):
    """Step 3 for one table (None: zeros)."""
    if table is None:
        return np.zeros(len(i))
    n_rho, n_tau = shape
    # (behind the table: what the clamp_as_cell mutant reads there is not a number, as nothing says what lies there)
    flat = np.concatenate([np.asarray(table, dtype=np.float64).ravel(), np.full(n_tau + 2, np.nan)])
    at = i * n_tau + j
    t00, t01, t10, t11 = flat[at], flat[at + 1], flat[at + n_tau], flat[at + n_tau + 1]
    lo = t00 + fs * (t01 - t00)
    hi = t10 + fs * (t11 - t10)
    return lo + fr * (hi - lo)


def shift_records(m: Map, records, mutant: str | None = None) -> np.ndarray:
    assert mutant is None or mutant in MUTANTS, mutant
    records = np.array(records, dtype=np.float64).reshape(-1, 4)
    out = records.copy()
    x, y, tb = records[:, 0], records[:, 1], records[:, 2]
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(tb)
    x, y, tb = x[finite], y[finite], tb[finite]
    n_rho, n_tau = m.shape
    with np.errstate(all="ignore"):
        xx = x * x
        yy = y * y
        rho = np.sqrt(xx + yy)
        tau = tb if mutant == "no_tb_origin" else tb - m.tb_origin
        i, fr = _cell(rho, m.rho_step, n_rho, mutant)
        j, fs = _cell(tau, m.tau_step, n_tau, mutant)
        if mutant == "swapped_weights":
            fr, fs = fs, fr
        dr = _value(m.radial, i, j, fr, fs, m.shape)
        da = _value(m.azimuthal, i, j, fr, fs, m.shape)
        dt = _value(m.time, i, j, fr, fs, m.shape)
        on_axis = rho == 0.0
        safe = np.where(on_axis, 1.0, rho)
        ux = np.where(on_axis, 0.0, x / safe)
        uy = np.where(on_axis, 0.0, y / safe)
        if mutant == "shift_on_axis":  # the shift applied where there is no direction: 0 / 0
            ux, uy = x / rho, y / rho
        if mutant == "azimuthal_sign":
            da = -da
        rx = dr * ux
        ry = dr * uy
        ax = da * uy
        ay = da * ux
        new_x = (x + rx) - ax
        new_y = (y + ry) + ay
        new_tb = tb + dt
    out[finite, 0], out[finite, 1], out[finite, 2] = new_x, new_y, new_tb
    return out


def same_bits(a, b) -> bool:
    """Equal as bit patterns (NaNs and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
