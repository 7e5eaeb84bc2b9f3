"""numpy restatement of the common-mode noise of the pad traces (include/attpc_engine.h, test infrastructure): the draw
of every sample of every group from (seed, global event id, group, sample) -- the pad noise's layout with the group in
the pad's place and a domain of its own --, added to the pad noise before the clamp for every pad with a group, in hit
mode, partial and full readout.  Built on ``trace_noise_reference`` (Philox, the pad noise, the clamp) and
``trace_reference.pad_trace`` (the noiseless samples s_p); the verdict is the brute-force maximum over all 512 samples,
not the decision rule the kernels use."""
from __future__ import annotations

import numpy as np

from tests.trace_noise_reference import Noise, noisy, philox4x32_10
from tests.trace_reference import NUM_TB, U64, pad_trace

DOMAIN_TRACE_COMMON = 0x20000000
NO_GROUP = 255
HIT, PARTIAL, FULL = 0, 1, 2
_J = np.arange(NUM_TB)
_J_INDEX = 2 * (_J % 64) + _J // 256
_J_WORD = (_J // 64) % 4


def values(seed: int, event: int, groups_in_use, table, stream: int = 0) -> np.ndarray:
    """c_g[j] [len(groups_in_use), 512] int64 of the groups ``groups_in_use``; ``table`` = (cdf [n_levels - 1],
    min_level).  One Philox call per counter (128 per group, 4 words each)."""
    cdf, min_level = table
    groups = np.asarray(groups_in_use, dtype=np.uint64).reshape(-1, 1)
    index = groups * np.uint64(128) + np.arange(128, dtype=np.uint64)[None, :]
    out = philox4x32_10(event & 0xFFFFFFFF, event >> 32, index, DOMAIN_TRACE_COMMON | stream, seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack(out)[_J_WORD, :, _J_INDEX].T  # [G, 512] uint64
    return int(min_level) + np.searchsorted(np.asarray(cdf, dtype=np.uint64), u, side="right").astype(np.int64)


class CommonMode:
    """A common-mode configuration: ``table`` = (cdf, min_level), ``groups`` ([10240] uint8, 255 = no term; None =
    every pad in group 0), ``stream``."""

    def __init__(self, table, groups=None, stream: int = 0):
        self.table = (np.asarray(table[0], dtype=np.uint32), int(table[1]))
        self.groups = np.zeros(10240, dtype=np.uint8) if groups is None else np.asarray(groups, dtype=np.uint8)
        self.stream = int(stream)
        used = self.groups[self.groups != NO_GROUP]
        self.n_groups = int(used.max()) + 1 if used.size else 0

    def all_values(self, seed: int, event: int) -> np.ndarray:
        """[n_groups, 512]: what ``common_mode_values`` returns for one event."""
        return values(seed, event, np.arange(self.n_groups), self.table, self.stream)

    def of_pads(self, seed: int, event: int, pads) -> np.ndarray:
        """The term of every pad of ``pads`` [len(pads), 512]: its group's values, zeros for group 255."""
        g = self.groups[np.asarray(pads, dtype=np.int64)].astype(np.int64)
        out = np.zeros((len(g), NUM_TB), dtype=np.int64)
        if (g != NO_GROUP).any():
            used = np.unique(g[g != NO_GROUP])
            c = values(seed, event, used, self.table, self.stream)
            has = g != NO_GROUP
            out[has] = c[np.searchsorted(used, g[has])]
        return out


def event_traces(points, labels, response, threshold: float, offset: int, noise: Noise, common: CommonMode | None,
                 seed: int, event: int, mode: int = HIT, channels=None):
    """One event's cloud rows [P,3], labels [P] -> kept (pads [R], samples [R,512], labels [R]), pads ascending.  Hit
    mode: the pads with rows are the candidates; PARTIAL / FULL: every pad of ``channels`` (bool [10240]), rows on pads
    outside it dropped, noise-only rows labelled -1."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    pad = points[:, 0].astype(np.int64)
    if mode != HIT:
        channels = np.asarray(channels, dtype=bool)
        inside = channels[pad] if len(pad) else np.zeros(0, dtype=bool)
        points, labels, pad = points[inside], labels[inside], pad[inside]
    t = np.floor(points[:, 1]).astype(np.int64)
    q = points[:, 2]
    cand = np.unique(pad) if mode == HIT else np.flatnonzero(channels)
    if not len(cand):
        return np.zeros(0, dtype=np.int32), np.zeros((0, NUM_TB), dtype=np.int16), np.zeros(0, dtype=np.int64)
    ped = np.array([noise.pedestal(int(p)) for p in cand], dtype=np.int64)
    n = noise.values(seed, event, cand)
    if common is not None:
        n = n + common.of_pads(seed, event, cand)
    s = np.zeros((len(cand), NUM_TB), dtype=np.int64)
    lab = np.full(len(cand), -1, dtype=np.int64)
    for i, p in enumerate(cand):
        sel = np.nonzero(pad == p)[0]
        if len(sel):
            s[i] = pad_trace(t[sel], q[sel], response, offset)
            lab[i] = int(labels[sel[np.lexsort((t[sel], -q[sel]))[0]]])  # largest q, smallest t on a tie
    trace = noisy(s, ped[:, None], n)
    kept = np.ones(len(cand), dtype=bool) if mode == FULL else (trace - ped[:, None]).max(axis=1) > threshold
    return cand[kept].astype(np.int32), trace[kept].astype(np.int16), lab[kept]


def traces(offsets, points, labels, response, threshold: float, offset: int, noise: Noise | None,
           common: CommonMode | None, seed: int = 0, first_event: int = 0, mode: int = HIT, channels=None):
    """CSR cloud -> (offsets [n+1], pads, samples, labels, {n_rows, sample_checksum, pad_checksum}) with the pad noise
    ``noise`` (None: no table, no pedestals) and the common-mode noise ``common`` (None: off); event i of the call is the
    global event first_event + i."""
    noise = Noise() if noise is None else noise
    offsets = np.asarray(offsets, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    response = np.asarray(response, dtype=np.float64)
    n = len(offsets) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    pads, samples, labs = [], [], []
    pad_sum = 0
    for e in range(n):
        lo, hi = offsets[e], offsets[e + 1]
        p, s, lab = event_traces(points[lo:hi], labels[lo:hi], response, threshold, offset, noise, common, seed,
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
