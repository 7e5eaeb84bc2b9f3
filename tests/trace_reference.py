"""numpy restatement of the pad-trace contract of include/attpc_engine.h (test infrastructure): a loop over every pad's
rows in ascending integer time bucket, each product rounded (``np.multiply``) and then added (``np.add``) in f64 from
+0.0, the summed signal clipped at 4095, rounded half to even, kept iff its largest sample exceeds the threshold."""
from __future__ import annotations

import numpy as np

NUM_TB = 512
U64 = 1 << 64
_J = np.arange(NUM_TB)


def pad_trace(t: np.ndarray, q: np.ndarray, response: np.ndarray, offset: int) -> np.ndarray:
    """One pad: rows (integer time bucket t, electrons q) -> int16 trace [512]."""
    acc = np.zeros(NUM_TB, dtype=np.float64)
    for i in np.argsort(t, kind="stable"):
        k = _J + offset - int(t[i])
        m = (k >= 0) & (k < NUM_TB)
        prod = np.multiply(np.float64(q[i]), response[k[m]])
        acc[m] = np.add(acc[m], prod)
    return np.rint(np.minimum(acc, 4095.0)).astype(np.int16)


def event_traces(points: np.ndarray, labels: np.ndarray, response: np.ndarray, threshold: float, offset: int):
    """One event's cloud rows [P,3] (pad, tau, electrons), labels [P] -> kept (pads [R], samples [R,512], labels [R]),
    pads ascending."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pad = points[:, 0].astype(np.int64)
    t = np.floor(points[:, 1]).astype(np.int64)
    q = points[:, 2]
    out_pads, out_samples, out_labels = [], [], []
    for p in np.unique(pad):
        sel = np.nonzero(pad == p)[0]
        trace = pad_trace(t[sel], q[sel], response, offset)
        if not trace.max() > threshold:
            continue
        best = sel[np.lexsort((t[sel], -q[sel]))[0]]  # largest q, smallest t on a tie
        out_pads.append(p)
        out_samples.append(trace)
        out_labels.append(int(labels[best]))
    return (np.array(out_pads, dtype=np.int32), np.array(out_samples, dtype=np.int16).reshape(-1, NUM_TB),
            np.array(out_labels, dtype=np.int64))


def traces(offsets, points, labels, response, threshold: float, offset: int, first_event: int = 0):
    """CSR cloud -> (offsets [n+1], pads, samples, labels, {n_rows, sample_checksum, pad_checksum}); the pad checksum
    counts events from ``first_event``."""
    offsets = np.asarray(offsets, dtype=np.int64)
    response = np.asarray(response, dtype=np.float64)
    n = len(offsets) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    pads, samples, labs = [], [], []
    pad_sum = 0
    for e in range(n):
        lo, hi = offsets[e], offsets[e + 1]
        p, s, lab = event_traces(points[lo:hi], labels[lo:hi], response, threshold, offset)
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
