"""numpy restatement of the electronic noise and pedestals of the pad traces (include/attpc_engine.h, test
infrastructure): Philox4x32-10 in numpy uint64 arithmetic, the draw of every sample from (seed, global event id, pad,
sample), the table lookup, the pedestal, the clip and the threshold above the pedestal, built on
``trace_reference.pad_trace`` for the noiseless samples s_p."""
from __future__ import annotations

import numpy as np

from tests.trace_reference import NUM_TB, U64, pad_trace

MASK = np.uint64(0xFFFFFFFF)
DOMAIN_TRACE_NOISE = 0x80000000
_J = np.arange(NUM_TB, dtype=np.int64)
_J_INDEX = (2 * (_J % 64) + _J // 256).astype(np.uint64)  # the sample's part of the counter word 2
_J_WORD = (_J // 64) % 4                                    # the output word of sample j


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast) of 32-bit values; every product of two 32-bit words fits a uint64."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=np.uint64) & MASK
    k1 = np.asarray(k1, dtype=np.uint64) & MASK
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c


class Noise:
    """A noise configuration: cdf [n_levels - 1] u32, min_level, n_levels (0 = no draw), pedestals [10240] or None,
    stream."""

    def __init__(self, cdf=(), min_level: int = 0, n_levels: int | None = None, pedestals=None, stream: int = 0):
        self.cdf = np.asarray(cdf, dtype=np.uint32)
        self.min_level = int(min_level)
        self.n_levels = (self.cdf.size + 1 if (self.cdf.size or self.min_level) else 0) if n_levels is None else n_levels
        self.pedestals = None if pedestals is None else np.asarray(pedestals, dtype=np.int64)
        self.stream = int(stream)

    def uniforms(self, seed: int, event: int, pads) -> np.ndarray:
        """u [len(pads), 512] of the contract's draw."""
        pads = np.asarray(pads, dtype=np.uint64).reshape(-1, 1)
        index = pads * np.uint64(128) + _J_INDEX[None, :]
        out = philox4x32_10(event & 0xFFFFFFFF, event >> 32, index, DOMAIN_TRACE_NOISE | self.stream,
                            seed & 0xFFFFFFFF, seed >> 32)
        return np.choose(np.broadcast_to(_J_WORD, index.shape), out)

    def values(self, seed: int, event: int, pads) -> np.ndarray:
        """n_p[j] [len(pads), 512]: min_level + #{k : cdf[k] <= u}; zeros without a noise table."""
        if self.n_levels == 0:
            return np.zeros((len(np.atleast_1d(pads)), NUM_TB), dtype=np.int64)
        u = self.uniforms(seed, event, pads)
        return self.min_level + np.searchsorted(self.cdf.astype(np.uint64), u, side="right").astype(np.int64)

    def pedestal(self, pad: int) -> int:
        return 0 if self.pedestals is None else int(self.pedestals[pad])


def noisy(s_p: np.ndarray, ped: int, n_p: np.ndarray) -> np.ndarray:
    """trace_p[j] = min(max(s_p[j] + ped_p + n_p[j], 0), 4095), integer arithmetic."""
    return np.clip(s_p.astype(np.int64) + ped + n_p, 0, 4095)


def event_traces(points, labels, response, threshold: float, offset: int, noise: Noise, seed: int, event: int):
    """One event's cloud rows [P,3], labels [P] -> kept (pads [R], samples [R,512], labels [R]), pads ascending."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pad = points[:, 0].astype(np.int64)
    t = np.floor(points[:, 1]).astype(np.int64)
    q = points[:, 2]
    hit = np.unique(pad)
    n_all = noise.values(seed, event, hit) if len(hit) else None
    out_pads, out_samples, out_labels = [], [], []
    for i, p in enumerate(hit):
        sel = np.nonzero(pad == p)[0]
        ped = noise.pedestal(p)
        trace = noisy(pad_trace(t[sel], q[sel], response, offset), ped, n_all[i])
        if not (trace - ped).max() > threshold:
            continue
        best = sel[np.lexsort((t[sel], -q[sel]))[0]]  # largest q, smallest t on a tie
        out_pads.append(p)
        out_samples.append(trace.astype(np.int16))
        out_labels.append(int(labels[best]))
    return (np.array(out_pads, dtype=np.int32), np.array(out_samples, dtype=np.int16).reshape(-1, NUM_TB),
            np.array(out_labels, dtype=np.int64))


def traces(offsets, points, labels, response, threshold: float, offset: int, noise: Noise, seed: int = 0,
           first_event: int = 0):
    """CSR cloud -> (offsets [n+1], pads, samples, labels, {n_rows, sample_checksum, pad_checksum}); event i of the call
    is the global event first_event + i (its noise and its term of the pad checksum)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    response = np.asarray(response, dtype=np.float64)
    n = len(offsets) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    pads, samples, labs = [], [], []
    pad_sum = 0
    for e in range(n):
        lo, hi = offsets[e], offsets[e + 1]
        p, s, lab = event_traces(points[lo:hi], labels[lo:hi], response, threshold, offset, noise, seed,
                                 first_event + e)
        pads.append(p)
        samples.append(s)
        labs.append(lab)
        out_off[e + 1] = out_off[e] + len(p)
        pad_sum += sum(((first_event + e) << 14) + int(v) for v in p)
    pads = np.concatenate(pads) if pads else np.zeros(0, dtype=np.int32)
    samples = np.concatenate(samples) if samples else np.zeros((0, NUM_TB), dtype=np.int16)
    labs = np.concatenate(labs) if labs else np.zeros(0, dtype=np.int64)
    sample_sum = int((samples.astype(np.int64) @ np.arange(1, NUM_TB + 1, dtype=np.int64)).sum(dtype=np.int64)) % U64
    return out_off, pads, samples, labs, {"n_rows": int(out_off[-1]), "sample_checksum": sample_sum,
                                          "pad_checksum": pad_sum % U64}


def level_masses(cdf, n_levels: int) -> np.ndarray:
    """Probability of every level index 0 .. n_levels - 1 under u uniform on [0, 2^32)."""
    cdf = np.asarray(cdf, dtype=np.float64)
    assert cdf.size == n_levels - 1
    return np.diff(np.concatenate([[0.0], cdf, [2.0 ** 32]])) / 2.0 ** 32
