"""Hand-made tracks for the helix slope, shared by tests/test_helix_cpu.py (the host C++ against the restatement) and
tests/test_gpu_helix.py (the device against the restatement): helices off the quantisation grid with a known turning
angle per point, so that a wrap of the angle falls between two chosen ranks of the fit segment."""
import math

import numpy as np

from tests import estimate_reference as est
from tests import helix_reference as ref

INDICES8 = [2, 5, 3, 2, 7, 9, 11, 4]  # n_sim = 8: every wave takes two positions; label 2 is given twice
WRAP_63_64 = math.pi / 63.5  # turning angle a point: rank 63 is short of half a turn, rank 64 is past it
WRAP_64_65 = math.pi / 64.5


def track(n, dphi, sense=1, backward=False, radius_mm=60.0, z_step_mm=2.0, azimuth=0.3, jitter_mm=0.0, rng=None, unused=()):
    """``n`` used rows of a helix that turns ``dphi`` rad a point, in ascending z; ``backward``: it travels towards low z
    (its start, the end nearest the axis, is its last row); ``unused``: (position, count) runs of rows inside a 25 mm
    beam region put in front of the used row at that position."""
    polar = math.atan(dphi * radius_mm / z_step_mm)
    rows = ref.helix_rows(n, radius_mm, math.pi - polar if backward else polar, z_step_mm, sense, azimuth, jitter_mm=jitter_mm, rng=rng)
    assert (np.hypot(rows[:, 0], rows[:, 1]) > 25.5).all() and np.abs(rows[:, :2]).max() <= 320.0 and np.abs(rows[:, 2]).max() <= 8192.0
    if backward:
        rows = rows[::-1].copy()
    rng = rng or np.random.default_rng(n)
    for at, count in sorted(unused, reverse=True):
        inside = np.zeros((count, 8))
        inside[:, 0], inside[:, 1] = rng.uniform(-15.0, 15.0, count), rng.uniform(-15.0, 15.0, count)
        inside[:, 2], inside[:, 4] = rows[min(at, n - 1), 2], 77.0
        rows = np.concatenate([rows[:at], inside, rows[at:]])
    return rows


def centre_first(extra=4):
    """The first point AT the centre of the Kasa circle of the segment (m = 5 of 9 rows with min_points 3): the four
    others of the segment lie symmetric about it, so uc = vc = 0 exactly; every turning angle is atan2w(0, 0)."""
    X = [800, 960, 800, 640, 800] + [1200 + 40 * i for i in range(extra)]
    Y = [0, 0, 160, 0, -160] + [300 + 10 * i for i in range(extra)]
    return est.spyral_rows(X, Y, 100 + 40 * np.arange(len(X)))


def collinear(n=45):
    i = np.arange(n)
    return est.spyral_rows(480 + 9 * i, 12 * i, 300 + 21 * i)


def flat(n=41):
    """All z equal: Sww = 0, so the path against z (regressor 2) has nothing to regress on."""
    rows = track(n, 0.05)
    rows[:, 2] = 250.0
    return rows


def interleave(tracks, noise_rows=0, rng=None):
    """The rows of ``tracks`` [(rows, label)] row by row in turn, with ``noise_rows`` rows of label -1 between them."""
    tracks = list(tracks)
    if noise_rows:
        noise = np.zeros((noise_rows, 8))
        noise[:, :3], noise[:, 4] = rng.uniform(-250.0, 250.0, (noise_rows, 3)), 30.0
        tracks.append((noise, -1))
    order = np.argsort(np.concatenate([np.arange(len(r)) * 1.0 + 0.01 * i for i, (r, _) in enumerate(tracks)]), kind="stable")
    rows = np.concatenate([r for r, _ in tracks])[order]
    labels = np.concatenate([np.full(len(r), label, dtype=np.int64) for r, label in tracks])[order]
    return rows, labels


def one(rows, label):
    return rows, np.full(len(rows), label, dtype=np.int64)


def hand_events(rng):
    """With min_points = 3 the segment has m = (n_used + 1) div 2 rows: m = 3, 63, 64, 65, 129, 2048 and the cut at 2048.
    name -> (rows, labels)."""
    unused = [(1, 1), (5, 3), (60, 10), (70, 100), (139, 2)]  # single ones, a run across a tile edge, more than a tile
    events = {
        "m 3 63 64": interleave([(track(5, 0.2), 2), (track(125, 0.04, sense=-1, jitter_mm=0.4, rng=rng), 5),
                                 (track(127, 0.03, backward=True, jitter_mm=0.4, rng=rng, azimuth=2.0), 3)]),
        "wraps": interleave([(track(129, WRAP_63_64, azimuth=1.1), 7),
                             (track(257, WRAP_64_65, sense=-1, backward=True, azimuth=4.0), 9)], 40, rng),
        "turns, unused rows": one(track(140, 0.3, unused=unused, jitter_mm=0.3, rng=rng), 4),
        "backward, unused rows": one(track(140, 0.11, sense=-1, backward=True, unused=[(0, 5), (80, 70), (139, 1)], jitter_mm=0.3,
                                           rng=rng, azimuth=5.0), 3),
        "collinear": one(collinear(), 9),
        "empty": (np.zeros((0, 8)), np.zeros(0, dtype=np.int64)),
        # all eight positions in one event: waves take positions s and s + 4; label 2 is given twice
        "eight": interleave([(track(40 + 13 * s, 0.02 + 0.03 * s, sense=1 - 2 * (s % 2), backward=bool(s % 3 == 1), azimuth=0.7 * s,
                                    jitter_mm=0.3, rng=rng), label) for s, label in enumerate((2, 5, 3, 7, 9, 11, 4))], 25, rng),
        "centre, flat": interleave([(centre_first(), 2), (flat(), 5)]),
        "capped": one(track(4100, 0.004, z_step_mm=0.4, jitter_mm=0.2, rng=rng), 11),
        "turn cap": one(track(4096, 0.13, sense=-1, z_step_mm=0.4), 4),  # m = 2048 points of 0.13 rad: 266 rad
    }
    return events


def csr(events):
    events = list(events.values()) if isinstance(events, dict) else events
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in events])])
    return offsets, np.concatenate([r for r, _ in events]), np.concatenate([l for _, l in events])
