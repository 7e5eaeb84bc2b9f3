"""The trace-row contract of include/attpc_engine.h restated in numpy and plain Python (no scipy: it runs wherever the
GPU tests run): kept pad traces -> peaks -> Spyral rows.  Integers stay integers, every f64 operation is one Python
float operation (one rounding), and the centroid jitter is a numpy Philox2x32-7 that takes its key constant as an
argument (0x100 is the cloud's jitter, which the CPU oracle computes too; 0x300 is the peaks').
tests/test_peaks_cpu.py checks this file against scipy stage by stage; tests/test_gpu_peaks.py checks the device
against this file."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

NUM_TB = 512
U32 = 0xFFFFFFFF
DOMAIN_JITTER = 0x100
DOMAIN_PEAK_JITTER = 0x300


class Peaks(NamedTuple):
    """attpc_peak_desc with the Python defaults of the package."""
    separation: float = 50.0
    prominence: float = 20.0
    min_width: float = 1.0
    max_width: float = 50.0
    rel_height: float = 0.95
    threshold: float = 40.0


class Geometry(NamedTuple):
    """What attpc_spyral_configure uploads of the geometry."""
    pad_centers: np.ndarray  # [n_pads, 2] mm
    pad_sizes: np.ndarray    # [n_pads]
    windows_edge: int
    micromegas_edge: int
    length: float            # m

    @classmethod
    def of(cls, config):
        return cls(np.asarray(config.pad_centers, dtype=np.float64), np.asarray(config.pad_sizes, dtype=np.float64),
                   int(config.elec_params.windows_edge), int(config.elec_params.micromegas_edge),
                   float(config.det_params.length))


def philox2x32_7(c0, c1, key):
    """Philox2x32-7 on arrays (or scalars) of counter words, one key word -> (out0, out1) as uint64 arrays < 2^32."""
    c0 = np.asarray(c0, dtype=np.uint64) & np.uint64(U32)
    c1 = np.asarray(c1, dtype=np.uint64) & np.uint64(U32)
    k = int(key) & U32
    for _ in range(7):
        prod = c0 * np.uint64(0xD256D193)  # < 2^64: both factors are below 2^32
        hi, lo = prod >> np.uint64(32), prod & np.uint64(U32)
        c0 = hi ^ np.uint64(k) ^ c1
        c1 = lo
        k = (k + 0x9E3779B9) & U32
    return c0, c1


def jitter_uniform(seed: int, event: int, key24, domain: int = DOMAIN_PEAK_JITTER):
    """U[0, 1) of the jitter generator: counter (event[31:0], event[39:32] << 24 | key24), key word
    seed[31:0] ^ rotl(seed[63:32], 13) ^ domain, U = ((out0 >> 5) 2^26 + (out1 >> 6)) / 2^53."""
    seed, event = int(seed), int(event)
    hi = (seed >> 32) & U32
    key = (seed & U32) ^ (((hi << 13) | (hi >> 19)) & U32) ^ domain
    key24 = np.asarray(key24, dtype=np.uint64)
    c1 = np.uint64(((event >> 32) & 0xFF) << 24) | key24
    a, b = philox2x32_7(np.full(key24.shape, event & U32, dtype=np.uint64), c1, key)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def local_maxima(y: np.ndarray) -> np.ndarray:
    """Step 2: strict local maxima, a flat top once at (first + last) // 2, never sample 0 or the last one."""
    d = np.diff(y)
    rise = np.flatnonzero(d > 0) + 1          # y[j - 1] < y[j]
    change = np.flatnonzero(d != 0)           # y[i + 1] != y[i]
    at = np.searchsorted(change, rise)        # the plateau that starts at j ends at the first change i >= j
    ok = at < len(change)                     # (none: it runs to the last sample)
    rise, last = rise[ok], change[at[ok]]
    fall = d[last] < 0
    return (rise[fall] + last[fall]) // 2


def select_by_separation(y: np.ndarray, cand: np.ndarray, separation: float) -> np.ndarray:
    """Step 3: from the highest priority down (height, the later candidate on a tie), a kept candidate drops every
    other one closer than ceil(separation) samples."""
    distance = math.ceil(separation)
    keep = np.ones(len(cand), dtype=bool)
    order = np.lexsort((np.arange(len(cand)), y[cand]))
    for j in order[::-1]:
        if keep[j]:
            near = np.abs(cand - cand[j]) < distance
            near[j] = False
            keep[near] = False
    return cand[keep]


def prominence_of(y, k: int):
    """Step 4 -> (prominence, left_base, right_base); ``y`` a list of Python ints."""
    top = y[k]
    i, left_min, left_base = k, top, k
    while i >= 0 and y[i] <= top:
        if y[i] < left_min:
            left_min, left_base = y[i], i
        i -= 1
    i, right_min, right_base = k, top, k
    while i < len(y) and y[i] <= top:
        if y[i] < right_min:
            right_min, right_base = y[i], i
        i += 1
    return top - max(left_min, right_min), left_base, right_base


def width_of(y, k: int, prominence: int, left_base: int, right_base: int, rel_height: float):
    """Step 5 -> (left_ip, right_ip)."""
    h = float(y[k]) - float(prominence) * rel_height
    i = k
    while left_base < i and h < y[i]:
        i -= 1
    left_ip = float(i)
    if y[i] < h:
        left_ip += (h - y[i]) / (y[i + 1] - y[i])
    i = k
    while i < right_base and h < y[i]:
        i += 1
    right_ip = float(i)
    if y[i] < h:
        right_ip -= (h - y[i]) / (y[i - 1] - y[i])
    return left_ip, right_ip


def staged_peaks(y: np.ndarray, pk: Peaks):
    """Steps 2 to 5 on one baseline-subtracted trace -> [(k, prominence, left_ip, right_ip)] in ascending k."""
    y = np.asarray(y, dtype=np.int64)
    cand = select_by_separation(y, local_maxima(y), pk.separation)
    ylist = y.tolist()
    out = []
    for k in cand.tolist():
        prom, lb, rb = prominence_of(ylist, k)
        if not prom >= pk.prominence:
            continue
        left_ip, right_ip = width_of(ylist, k, prom, lb, rb, pk.rel_height)
        if not pk.min_width <= right_ip - left_ip <= pk.max_width:
            continue
        out.append((k, prom, left_ip, right_ip))
    return out


def trace_points(y: np.ndarray, pk: Peaks):
    """Steps 2 to 6 -> [(k, amplitude, integral, prominence, left_ip, right_ip)] in ascending k."""
    y = np.asarray(y, dtype=np.int64)
    out = []
    for k, prom, left_ip, right_ip in staged_peaks(y, pk):
        if not y[k] > pk.threshold:
            continue
        integral = int(np.abs(y[math.floor(left_ip): math.ceil(right_ip)]).sum())
        out.append((k, int(y[k]), integral, prom, left_ip, right_ip))
    return out


def trace_rows(offsets, pads, samples, labels, pk: Peaks, geo: Geometry, seed: int, first_event: int = 0, pedestals=None):
    """Kept trace rows in CSR form (as the trace entry points deliver them) -> (offsets [n+1], rows [R,8], labels [R],
    {n_rows, row_checksum}): steps 1 to 8 of the contract."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    out_offsets = np.zeros(n + 1, dtype=np.int64)
    all_rows, all_labels, checksum = [], [], 0
    span = geo.windows_edge - geo.micromegas_edge
    for e in range(n):
        event = int(first_event) + e
        ks, ps, amps, ints, labs = [], [], [], [], []
        for r in range(int(offsets[e]), int(offsets[e + 1])):
            p = int(pads[r])
            ped = 0 if pedestals is None else int(pedestals[p])
            for k, amp, integral, *_ in trace_points(np.asarray(samples[r], dtype=np.int64) - ped, pk):
                ks.append(k), ps.append(p), amps.append(amp), ints.append(integral), labs.append(int(labels[r]))
        ks, ps = np.array(ks, dtype=np.int64), np.array(ps, dtype=np.int64)
        centroid = ks.astype(np.float64) + jitter_uniform(seed, event, (ks << 14 | ps).astype(np.uint64))
        order = np.lexsort((ps, -centroid))
        rows = np.empty((len(ks), 8), dtype=np.float64)
        for i, j in enumerate(order.tolist()):
            c, p = float(centroid[j]), int(ps[j])
            z = (geo.windows_edge - c) / span * geo.length * 1000.0
            rows[i] = (geo.pad_centers[p, 0], geo.pad_centers[p, 1], z, amps[j], ints[j], p, c, geo.pad_sizes[p])
            checksum += (event << 23) + (p << 9) + int(ks[j])
        all_rows.append(rows)
        all_labels.append(np.array(labs, dtype=np.int64)[order])
        out_offsets[e + 1] = out_offsets[e] + len(ks)
    rows = np.concatenate(all_rows) if all_rows else np.zeros((0, 8))
    labels_out = np.concatenate(all_labels) if all_labels else np.zeros(0, dtype=np.int64)
    return out_offsets, rows.reshape(-1, 8), labels_out.astype(np.int64), {"n_rows": int(out_offsets[-1]),
                                                                         "row_checksum": checksum % (1 << 64)}
