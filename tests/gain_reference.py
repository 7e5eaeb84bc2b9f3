"""numpy restatement of the micromegas gain of the pad traces (include/attpc_engine.h, test infrastructure): the
Philox4x32-10 draw of every cloud row from (seed, global event id, pad, time bucket), the interpolated quantile, the
Wilson-Hilferty cube and the pad's gain factor, every operation a numpy f64 operation of its own (rounded once; numpy's
division and square root are the correctly rounded ones).  The Philox is the one tests/trace_noise_reference.py checks
against known-answer vectors."""
from __future__ import annotations

import numpy as np

from tests.trace_noise_reference import philox4x32_10

NUM_TB = 512
NUM_PADS = 10240
KNOTS = 4097
DOMAIN_TRACE_GAIN = 0x40000000


class Gain:
    """A gain configuration: rel_variance f, quantiles Z [4097] (needed when f > 0), pad_gain [10240] or None, stream."""

    def __init__(self, rel_variance: float = 0.0, quantiles=None, pad_gain=None, stream: int = 0):
        self.f = float(rel_variance)
        self.z = None if quantiles is None else np.asarray(quantiles, dtype=np.float64)
        assert self.f == 0.0 or (self.z is not None and self.z.shape == (KNOTS,))
        self.pad_gain = None if pad_gain is None else np.asarray(pad_gain, dtype=np.float64)
        self.stream = int(stream)
        self.c = np.float64(self.f) / np.float64(9.0)

    def uniforms(self, seed: int, event: int, pad, t) -> np.ndarray:
        """u (word 0 of the contract's Philox call) of the rows (pad, t) of global event ``event``."""
        index = np.asarray(pad, dtype=np.uint64) * np.uint64(NUM_TB) + np.asarray(t, dtype=np.uint64)
        return philox4x32_10(event & 0xFFFFFFFF, event >> 32, index, DOMAIN_TRACE_GAIN | self.stream,
                             seed & 0xFFFFFFFF, seed >> 32)[0]

    def fluctuate(self, u, q) -> np.ndarray:
        """q' of charges q under the uniforms u (u32 values): the contract's steps, one numpy operation each."""
        q = np.asarray(q, dtype=np.float64)
        if self.f == 0.0:
            return q.copy()
        u = np.broadcast_to(np.asarray(u, dtype=np.uint64), q.shape)
        i = (u >> np.uint64(20)).astype(np.int64)
        w = np.multiply((u & np.uint64(0xFFFFF)).astype(np.float64), 2.0 ** -20)
        z = np.add(self.z[i], np.multiply(np.subtract(self.z[i + 1], self.z[i]), w))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = np.divide(self.c, q)
            s = np.sqrt(r)
            y = np.add(np.subtract(1.0, r), np.multiply(z, s))
            x = np.where(y > 0.0, y, 0.0)
            out = np.multiply(np.multiply(np.multiply(q, x), x), x)
        return np.where(q == 0.0, 0.0, out)

    def rows(self, seed: int, event: int, pad, t, q) -> np.ndarray:
        """q'' of the rows (pad, t, q) of global event ``event``."""
        pad = np.asarray(pad, dtype=np.int64)
        q = np.asarray(q, dtype=np.float64)
        u = self.uniforms(seed, event, pad, t) if self.f > 0.0 and len(q) else np.zeros(q.shape, dtype=np.uint64)
        out = self.fluctuate(u, q)
        return out if self.pad_gain is None else np.multiply(out, self.pad_gain[pad])

    def cloud(self, offsets, points, seed: int = 0, first_event: int = 0) -> np.ndarray:
        """CSR cloud (offsets [n+1], points [P,3]) -> q'' [P]; rows outside the offsets' range keep 0."""
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(len(points), dtype=np.float64)
        for e in range(len(offsets) - 1):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            p = points[lo:hi]
            out[lo:hi] = self.rows(seed, first_event + e, p[:, 0].astype(np.int64), np.floor(p[:, 1]).astype(np.int64), p[:, 2])
        return out

    def gained_points(self, offsets, points, seed: int = 0, first_event: int = 0) -> np.ndarray:
        """The cloud with its charges replaced by q'' (what the trace contract then sums)."""
        out = np.array(points, dtype=np.float64).reshape(-1, 3)
        out[:, 2] = self.cloud(offsets, out, seed, first_event)
        return out


def labels_by_pad(points, labels) -> dict:
    """{pad: label} of one event's cloud rows by the trace contract's label rule on the cloud's own charges: the label
    of the pad's row with the largest q, the smallest t on a tie."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pad, t, q = points[:, 0].astype(np.int64), np.floor(points[:, 1]).astype(np.int64), points[:, 2]
    out = {}
    for i in np.lexsort((t, -q, pad))[::-1]:  # the last one written per pad is its first in (pad, -q, t) order
        out[int(pad[i])] = int(labels[i])
    return out


def traces_with_gain(offsets, points, labels, gain: Gain, seed: int, first_event: int, traces_of):
    """The trace contract with the gain on, from the restatements of the traces as they are: ``traces_of(points)`` ->
    (offsets [n+1], pads, samples, labels, sums) is one of them (tests/trace_reference.py, or the noise / readout ones)
    on the given charges.  Pads, samples and sums come from the cloud with its charges replaced by q''; the labels are
    those of the original cloud (the label rule keeps the cloud's own charge), -1 for a noise-only pad."""
    off, pads, samples, _, sums = traces_of(gain.gained_points(offsets, points, seed, first_event))
    labs = np.full(len(pads), -1, dtype=np.int64)
    for e in range(len(offsets) - 1):
        of_pad = labels_by_pad(points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]])
        for r in range(off[e], off[e + 1]):
            labs[r] = of_pad.get(int(pads[r]), -1)
    return off, pads, samples, labs, sums
