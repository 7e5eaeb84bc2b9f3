"""The drift correction of trace rows (include/attpc_engine.h, "drift correction") restated in numpy, on its own:
nothing of the package is used, and the forward map is that of tests/distortion_reference.py.  Every operation is one
numpy f64 operation, in the written order of the contract, so the result is the contract's to the last bit.

``Settings`` is the descriptor; ``undistort(settings, offsets, rows, labels)`` gives the corrected, re-sorted rows and
labels, ``order`` (the input row of every output row) and the four counts.  ``mutant`` names one deliberate departure
from the contract (``MUTANTS``): each is what a plausible slip in the kernel would compute, and
tests/test_undistort_cpu.py shows that the bit-for-bit comparison on the case set catches it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import distortion_reference as dref

MUTANTS = ("one_iteration_fewer", "no_resort", "tie_descending_index", "skipped_in_place", "z_from_uncorrected_time")
COUNTS = ("n_rows", "n_skipped", "n_unconverged", "n_moved")


@dataclass
class Settings:
    map: dref.Map
    windows_edge: int
    micromegas_edge: int
    length: float
    iterations: int = 12
    tolerance_xy: float = 1e-6
    tolerance_tb: float = 1e-3


def correct_points(s: Settings, sx, sy, st, iterations: int | None = None):
    """Steps 3 and 4 on finite observed points: (x, y, t) and the last (dx, dy, dt)."""
    sx, sy, st = (np.array(v, dtype=np.float64) for v in (sx, sy, st))
    x, y, t = sx.copy(), sy.copy(), st.copy()
    dx = dy = dt = np.zeros_like(sx)
    zeros = np.zeros_like(sx)
    with np.errstate(all="ignore"):
        for _ in range(s.iterations if iterations is None else iterations):
            f = dref.shift_records(s.map, np.stack([x, y, t, zeros], axis=1))
            dx = f[:, 0] - sx
            dy = f[:, 1] - sy
            dt = f[:, 2] - st
            x = x - dx
            y = y - dy
            t = t - dt
    return x, y, t, (dx, dy, dt)


def z_of(s: Settings, t):
    """Step 5, column 2: the trace rows' own expression."""
    with np.errstate(all="ignore"):
        return ((float(s.windows_edge) - t) / float(s.windows_edge - s.micromegas_edge)) * s.length * 1000.0


def undistort(s: Settings, offsets, rows, labels, mutant: str | None = None):
    assert mutant is None or mutant in MUTANTS, mutant
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.array(rows, dtype=np.float64).reshape(-1, 8)
    labels = np.array(labels, dtype=np.int64).reshape(-1)
    out_rows, out_labels = rows.copy(), labels.copy()
    order = np.arange(len(rows), dtype=np.int64)
    info = dict.fromkeys(COUNTS, 0)
    iterations = s.iterations - 1 if mutant == "one_iteration_fewer" else s.iterations
    for e in range(len(offsets) - 1):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        ev = rows[lo:hi]
        n = hi - lo
        info["n_rows"] += n
        if n == 0:
            continue
        finite = np.isfinite(ev[:, 0]) & np.isfinite(ev[:, 1]) & np.isfinite(ev[:, 6])
        good, skipped = np.flatnonzero(finite), np.flatnonzero(~finite)
        info["n_skipped"] += len(skipped)
        sx, sy, st = ev[good, 0] / 1000.0, ev[good, 1] / 1000.0, ev[good, 6]
        x, y, t, (dx, dy, dt) = correct_points(s, sx, sy, st, iterations)
        info["n_unconverged"] += int(((np.abs(dx) > s.tolerance_xy) | (np.abs(dy) > s.tolerance_xy)
                                      | (np.abs(dt) > s.tolerance_tb)).sum())
        new = ev.copy()
        new[good, 0] = x * 1000.0
        new[good, 1] = y * 1000.0
        new[good, 2] = z_of(s, st if mutant == "z_from_uncorrected_time" else t)
        if mutant == "no_resort":
            ranked = np.arange(len(good))
        elif mutant == "tie_descending_index":
            ranked = np.lexsort((-np.arange(len(good)), -t))
        else:
            ranked = np.argsort(-t, kind="stable")  # descending t, equal t in input order
        if mutant == "skipped_in_place":
            src = np.arange(n)
            src[good] = good[ranked]
        else:
            src = np.concatenate([good[ranked], skipped])
        info["n_moved"] += int((src != np.arange(n)).sum())
        out_rows[lo:hi] = new[src]
        out_labels[lo:hi] = labels[lo:hi][src]
        order[lo:hi] = lo + src
    return out_rows, out_labels, order, info
