"""numpy restatement of the readout of noise-only pads (include/attpc_engine.h, test infrastructure), on top of
``trace_noise_reference``: partial readout (every pad of the readout set S is a candidate, a pad without rows has
s_p = 0, kept iff max_j (trace_p[j] - ped_p) > thr, rows on pads outside S dropped) and full readout (every pad of S
kept), noise-only rows labelled -1, rows in ascending pad.  The decision is the brute-force maximum over all 512
samples, not the decision rule the kernels use."""
from __future__ import annotations

import numpy as np

from tests.trace_noise_reference import DOMAIN_TRACE_NOISE, Noise, noisy, philox4x32_10
from tests.trace_noise_reference import traces as hit_traces
from tests.trace_reference import NUM_TB, U64, pad_trace

PARTIAL, FULL = 1, 2
_J = np.arange(NUM_TB)
_J_INDEX = 2 * (_J % 64) + _J // 256
_J_WORD = (_J // 64) % 4


def uniforms(noise: Noise, seed: int, event: int, pads) -> np.ndarray:
    """u [len(pads), 512] of the contract's draw, one Philox call per counter (128 per pad, 4 words each) instead of
    ``Noise.uniforms``' one per sample: the same numbers, a quarter of the work for the full pad plane."""
    pads = np.asarray(pads, dtype=np.uint64).reshape(-1, 1)
    index = pads * np.uint64(128) + np.arange(128, dtype=np.uint64)[None, :]
    out = philox4x32_10(event & 0xFFFFFFFF, event >> 32, index, DOMAIN_TRACE_NOISE | noise.stream,
                        seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(out)  # [4, P, 128]
    return words[_J_WORD, :, _J_INDEX].T.astype(np.uint32)


def values(noise: Noise, seed: int, event: int, pads) -> np.ndarray:
    """n_p[j] [len(pads), 512], as ``Noise.values``."""
    pads = np.atleast_1d(pads)
    if noise.n_levels == 0:
        return np.zeros((len(pads), NUM_TB), dtype=np.int64)
    u = uniforms(noise, seed, event, pads).astype(np.uint64)
    return noise.min_level + np.searchsorted(noise.cdf.astype(np.uint64), u, side="right").astype(np.int64)


def pedestals(noise: Noise, pads) -> np.ndarray:
    pads = np.asarray(pads, dtype=np.int64)
    return np.zeros(len(pads), dtype=np.int64) if noise.pedestals is None else noise.pedestals[pads].astype(np.int64)


def event_readout(points, labels, response, threshold: float, offset: int, noise: Noise, seed: int, event: int,
                  mode: int, channels):
    """One event's cloud rows [P,3], labels [P] -> kept (pads [R], samples [R,512], labels [R]) of readout ``mode``
    (PARTIAL or FULL) of the set ``channels`` (bool [10240]), pads ascending."""
    channels = np.asarray(channels, dtype=bool)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    pad = points[:, 0].astype(np.int64)
    keep_rows = channels[pad] if len(pad) else np.zeros(0, dtype=bool)
    points, labels, pad = points[keep_rows], labels[keep_rows], pad[keep_rows]  # a dead channel
    t = np.floor(points[:, 1]).astype(np.int64)
    q = points[:, 2]
    cand = np.flatnonzero(channels)
    ped = pedestals(noise, cand)
    n_all = values(noise, seed, event, cand)
    s = np.zeros((len(cand), NUM_TB), dtype=np.int64)
    lab = np.full(len(cand), -1, dtype=np.int64)
    where = {int(p): i for i, p in enumerate(cand)}
    for p in np.unique(pad):
        sel = np.nonzero(pad == p)[0]
        i = where[int(p)]
        s[i] = pad_trace(t[sel], q[sel], response, offset)
        lab[i] = int(labels[sel[np.lexsort((t[sel], -q[sel]))[0]]])  # largest q, smallest t on a tie
    trace = noisy(s, ped[:, None], n_all)
    kept = np.ones(len(cand), dtype=bool) if mode == FULL else (trace - ped[:, None]).max(axis=1) > threshold
    return cand[kept].astype(np.int32), trace[kept].astype(np.int16), lab[kept]


def traces(offsets, points, labels, response, threshold: float, offset: int, noise: Noise, seed: int = 0,
           first_event: int = 0, mode: int = 0, channels=None):
    """CSR cloud -> (offsets [n+1], pads, samples, labels, {n_rows, sample_checksum, pad_checksum}) of the readout
    ``mode`` (0 = hit: ``trace_noise_reference.traces``) of the set ``channels`` (bool [10240]); event i of the call is
    the global event first_event + i."""
    response = np.asarray(response, dtype=np.float64)
    if mode == 0:
        return hit_traces(offsets, points, labels, response, threshold, offset, noise, seed, first_event)
    offsets = np.asarray(offsets, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    pads, samples, labs = [], [], []
    pad_sum = 0
    for e in range(n):
        lo, hi = offsets[e], offsets[e + 1]
        p, s, lab = event_readout(points[lo:hi], labels[lo:hi], response, threshold, offset, noise, seed,
                                  first_event + e, mode, channels)
        pads.append(p)
        samples.append(s)
        labs.append(lab)
        out_off[e + 1] = out_off[e] + len(p)
        pad_sum += len(p) * ((first_event + e) << 14) + int(p.astype(np.int64).sum())
    pads = np.concatenate(pads) if pads else np.zeros(0, dtype=np.int32)
    samples = np.concatenate(samples) if samples else np.zeros((0, NUM_TB), dtype=np.int16)
    labs = np.concatenate(labs) if labs else np.zeros(0, dtype=np.int64)
    sample_sum = int((samples.astype(np.int64) @ np.arange(1, NUM_TB + 1, dtype=np.int64)).sum(dtype=np.int64)) % U64
    return out_off, pads, samples, labs, {"n_rows": int(out_off[-1]), "sample_checksum": sample_sum,
                                          "pad_checksum": pad_sum % U64}
