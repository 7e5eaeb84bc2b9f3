"""What the fused Spyral path must deliver (spyral_count_kernel / spyral_write_kernel of csrc/spyral.hip), restated in
numpy and plain Python: an event-ordered cloud -> response, row layout, ADC threshold, z-sort.  Every column but the
integral is the single-rounded f64 expression of the reference (response.py:35-57, writer.py:61-112, :232-238), one
numpy operation per rounding, and is compared EXACTLY; the integral is the sum of the 512 products ``response[i] * q``,
each formed and clipped at 4095 in f64 as the reference's loop forms them, added in extended precision (or exactly,
math.fsum) and rounded once.
``integral_sequential`` is that loop's own f64 sum.  tests/test_spyral_cpu.py pins this file to the rows the
reference's code made and to the CPU oracle; tests/test_gpu_spyral_edges.py compares the device with this file."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from tests.peaks_reference import Geometry  # pad centres and sizes, the two time-bucket edges, the length

NUM_TB = 512
ADC_MAX = 4095.0
BLOCK = 4096  # rows of 512 products held at a time (16 MiB)


class FusedRows(NamedTuple):
    offsets: np.ndarray       # [n + 1] rows kept per event, as CSR offsets
    rows: np.ndarray          # [P', 8] x, y, z (mm), amplitude, integral, pad, time bucket, pad scale
    labels: np.ndarray        # [P']
    event_points: np.ndarray  # [n] cloud rows per event BEFORE the threshold


def bipolar_response() -> np.ndarray:
    """A shaper with negative lobes (226 negative samples), about as high as the default response."""
    t = np.arange(NUM_TB) / 6.0
    return 3.2e-5 * np.exp(-3.0 * t / 4.0) * (t / 4.0) ** 3 * np.sin(t / 4.0) / 0.044


def amplitude(response: np.ndarray, q: np.ndarray) -> np.ndarray:
    """max_i min(response[i] q, 4095) = min(max(response) q, 4095) for q >= 0: one product, one comparison."""
    return np.minimum(float(np.max(response)) * np.asarray(q, dtype=np.float64), ADC_MAX)


def clipped_products(response: np.ndarray, q: np.ndarray) -> np.ndarray:
    """[len(q), 512]: response[i] * q in f64, clipped at 4095 (response.py:55-56)."""
    return np.minimum(np.asarray(response, dtype=np.float64)[None, :] * np.asarray(q, dtype=np.float64)[:, None], ADC_MAX)


def clipped_count(response: np.ndarray, q: np.ndarray) -> np.ndarray:
    """k of every charge: the number of samples the clip changes, response[i] * q > 4095."""
    q = np.asarray(q, dtype=np.float64)
    out = np.empty(len(q), dtype=np.int64)
    for lo in range(0, len(q), BLOCK):
        out[lo:lo + BLOCK] = (np.asarray(response, dtype=np.float64)[None, :] * q[lo:lo + BLOCK, None] > ADC_MAX).sum(axis=1)
    return out


def _per_distinct_charge(response: np.ndarray, q: np.ndarray, fn) -> np.ndarray:
    """fn([m, 512] clipped products) -> [m], evaluated once per distinct charge, a block of charges at a time."""
    q = np.asarray(q, dtype=np.float64)
    distinct, inverse = np.unique(q, return_inverse=True)
    out = np.empty(len(distinct), dtype=np.float64)
    for lo in range(0, len(distinct), BLOCK):
        out[lo:lo + BLOCK] = fn(clipped_products(response, distinct[lo:lo + BLOCK]))
    return out[inverse.reshape(q.shape)]


def integral_exact(response: np.ndarray, q: np.ndarray) -> np.ndarray:
    """The sum of the 512 clipped f64 products, rounded once to f64: added in extended precision where numpy has it (a
    64-bit mantissa: 512 terms are good to 3e-17 before the rounding), without any rounding on the way (math.fsum) where
    it has not."""
    if np.finfo(np.longdouble).nmant >= 63:
        return _per_distinct_charge(response, q, lambda prod: prod.astype(np.longdouble).sum(axis=1).astype(np.float64))
    return _per_distinct_charge(response, q, lambda prod: np.array([math.fsum(row) for row in prod.tolist()], dtype=np.float64))


def integral_sequential(response: np.ndarray, q: np.ndarray) -> np.ndarray:
    """The reference's own sum: the clipped products added one after the other in f64, sample 0 first."""
    return _per_distinct_charge(response, q, lambda prod: np.cumsum(prod, axis=1)[:, -1] if len(prod) else np.empty(0))


def z_mm(tb: np.ndarray, geo: Geometry) -> np.ndarray:
    """writer.py:103-105, in that order: (window_edge - tb) / (window_edge - mm_edge) * length * 1000.0."""
    window, mm = float(geo.windows_edge), float(geo.micromegas_edge)
    return (window - np.asarray(tb, dtype=np.float64)) / (window - mm) * float(geo.length) * 1000.0


def convert(points: np.ndarray, response: np.ndarray, geo: Geometry, integral=integral_exact) -> np.ndarray:
    """writer.py:61-112 on a cloud [P, 3] (pad, time bucket, electrons) -> rows [P, 8], nothing dropped or sorted."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pad = points[:, 0].astype(np.int64)
    rows = np.empty((len(points), 8), dtype=np.float64)
    rows[:, 0] = np.asarray(geo.pad_centers, dtype=np.float64)[pad, 0]
    rows[:, 1] = np.asarray(geo.pad_centers, dtype=np.float64)[pad, 1]
    rows[:, 2] = z_mm(points[:, 1], geo)
    rows[:, 3] = amplitude(response, points[:, 2])
    rows[:, 4] = integral(response, points[:, 2])
    rows[:, 5] = points[:, 0]
    rows[:, 6] = points[:, 1]
    rows[:, 7] = np.asarray(geo.pad_sizes, dtype=np.float64)[pad]
    return rows


def fused_rows(offsets, points, labels, response, geo: Geometry, threshold: float, integral=integral_exact,
               converted=None) -> FusedRows:
    """The fused path on an event-ordered cloud (CSR ``offsets``, ``points`` [P, 3], ``labels`` [P]): the rows of every
    event with amplitude > threshold (strict, writer.py:232-234) in descending time bucket, rows of equal time bucket in
    cloud order -- that is ascending z (writer.py:236-238), which is asserted.  ``converted``: ``convert(points, ...)``
    where the caller has it already (the same cloud at another threshold)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    labels = np.asarray(labels)
    rows = convert(points, response, geo, integral) if converted is None else converted
    threshold = float(threshold)
    order = []
    kept = np.zeros(len(offsets) - 1, dtype=np.int64)
    for e in range(len(offsets) - 1):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        keep = lo + np.flatnonzero(rows[lo:hi, 3] > threshold)
        keep = keep[np.argsort(-rows[keep, 6], kind="stable")]
        assert (np.diff(rows[keep, 2]) >= 0).all(), f"event {e}: z is not non-decreasing in descending time bucket"
        kept[e] = len(keep)
        order.append(keep)
    order = np.concatenate(order) if order else np.empty(0, dtype=np.int64)
    return FusedRows(np.concatenate([[0], np.cumsum(kept)]).astype(np.int64), rows[order], labels[order], np.diff(offsets))
