"""Hand-made clouds that reach every corner of the trace-row contract (include/attpc_engine.h), one event per case,
shared by tests/test_peaks_cpu.py (asserted on the restatement) and tests/test_gpu_peaks.py (device against
restatement).  The response is a box of three samples, R = (1, 1, 1, 0, ...), offset 0: an arrival of q electrons at
bucket t adds q to samples t, t + 1, t + 2, so every trace below is known sample by sample.  adc_threshold -1 keeps
every hit pad, the all-zero row included; pad 13 has a pedestal of 300 and no pad has noise.  The peak parameters are
the package's defaults (separation 50, prominence 20, width 1 .. 50 at 0.95, threshold 40)."""
from __future__ import annotations

import numpy as np

NUM_PADS = 10240


def box_response() -> np.ndarray:
    resp = np.zeros(512)
    resp[:3] = 1.0
    return resp


def pedestals() -> np.ndarray:
    ped = np.zeros(NUM_PADS, dtype=np.int16)
    ped[13] = 300
    return ped


TRACE_THRESHOLD = -1.0
TRACE_OFFSET = 0


def _rows(pad, arrivals):
    return [[float(pad), t + 0.25, float(q)] for t, q in arrivals]


def hand_cases():
    """[(name, points [P,3], labels [P], expected)]: ``expected`` the event's points as [(pad, sample, amplitude)] in
    any order."""
    base = [(t, 100) for t in range(10, 200, 3)]  # a plateau of 100 over samples 10 .. 201
    cases = [
        ("flat_top_odd", _rows(1, [(50, 100)]), [(1, 51, 100)]),                       # 100 at 50, 51, 52
        ("flat_top_even", _rows(2, [(50, 100), (53, 100)]), [(2, 52, 100)]),           # 100 at 50 .. 55
        ("lower_within_separation_dropped", _rows(3, [(100, 100), (130, 200)]), [(3, 131, 200)]),
        ("equal_height_earlier_dropped", _rows(4, [(100, 150), (130, 150)]), [(4, 131, 150)]),
        # a pulse of 500 (far wider than max_width at its 5 % height: dropped), the plateau, and a bump of +20 / +19 on
        # it 80 samples later: the bump's prominence is exactly 20 / 19 (higher ground on the left, the plateau between)
        ("prominence_at_limit_kept", _rows(5, base + [(20, 400), (101, 20)]), [(5, 102, 120)]),
        ("prominence_below_limit_dropped", _rows(6, base + [(20, 400), (101, 19)]), []),
        # a track along the drift direction: 81 consecutive buckets on one pad, a flat top 79 samples long
        ("width_above_max_dropped", _rows(7, [(t, 100) for t in range(300, 381)]), []),
        ("amplitude_at_threshold_dropped", _rows(8, [(50, 40)]), []),
        ("amplitude_above_threshold_kept", _rows(9, [(50, 41)]), [(9, 51, 41)]),
        ("peak_at_sample_1", _rows(10, [(0, 50), (1, 60)]), [(10, 1, 110)]),           # 50, 110, 110, 60
        ("peak_at_sample_510", _rows(11, [(508, 80), (510, 70)]), [(11, 510, 150)]),   # .., 80, 80, 150, 70
        ("all_zero_row", _rows(12, [(77, 0)]), []),
        # the sum saturates at 4095 counts including the pedestal: flat at 4095 - 300 over two samples
        ("saturated_flat_at_4095_minus_pedestal", _rows(13, [(200, 3000), (201, 3000)]), [(13, 201, 3795)]),
        ("empty_event", [], []),
        # several pads in one event: the rows come in descending centroid
        ("several_pads", _rows(20, [(300, 90)]) + _rows(21, [(10, 60), (400, 70)]) + _rows(22, [(300, 55)]),
         [(20, 301, 90), (21, 11, 60), (21, 401, 70), (22, 301, 55)]),
    ]
    out = []
    for i, (name, rows, expected) in enumerate(cases):
        points = np.array(rows, dtype=np.float64).reshape(-1, 3)
        out.append((name, points, np.full(len(points), i % 7, dtype=np.int64), expected))
    return out


def hand_cloud():
    """The cases as one CSR cloud -> (offsets, points, labels)."""
    cases = hand_cases()
    offsets = np.zeros(len(cases) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(p) for _, p, _, _ in cases])
    return (offsets, np.concatenate([p for _, p, _, _ in cases]).reshape(-1, 3),
            np.concatenate([lab for _, _, lab, _ in cases]).astype(np.int64))
