"""The summary contract of include/attpc_engine.h restated in numpy (test infrastructure only): a plain loop over events
and labels on a CSR cloud, plus the track part from the arrays of ``attpc_det_tracks``."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd import _abi


def _cloud_part(rec, points, min_electrons, centers=None):
    """n_points, n_kept, n_pads, tb_min, tb_max, charge (and rho2_max with ``centers``) of ``points`` into ``rec``."""
    q = points[:, 2]
    kept = q >= min_electrons
    pads = points[kept, 0].astype(np.int64)
    tb = np.floor(points[kept, 1]).astype(np.int64)
    rec["n_points"] = len(points)
    rec["n_kept"] = int(kept.sum())
    rec["n_pads"] = len(np.unique(pads))
    rec["tb_min"] = tb.min() if len(tb) else -1
    rec["tb_max"] = tb.max() if len(tb) else -1
    rec["charge"] = int(q.astype(np.int64).sum())
    if centers is not None:
        x, y = centers[pads, 0], centers[pads, 1]
        rho2 = x * x + y * y  # numpy rounds every product, then adds
        rec["rho2_max"] = rho2.max() if len(rho2) else -1.0


def summary(offsets, points, labels, indices, min_electrons, centers, samples=None, counts=None, n_steps=None):
    """(events [n], tracks [n, n_sim]) of the CSR cloud ``offsets`` / ``points`` [P,3] / ``labels`` [P] for the layout
    positions ``indices``.  ``samples`` [n * n_sim, S, 4], ``counts``, ``n_steps`` [n * n_sim]: the arrays of
    ``attpc_det_tracks`` (None: the empty track part)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    centers = np.asarray(centers, dtype=np.float64)
    n, n_sim = len(offsets) - 1, len(indices)
    events = np.zeros(n, dtype=_abi.EVENT_SUMMARY_DTYPE)
    tracks = np.zeros((n, n_sim), dtype=_abi.TRACK_SUMMARY_DTYPE)
    for e in range(n):
        pts, lab = points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        _cloud_part(events[e], pts, min_electrons)
        for s, row in enumerate(indices):
            rec = tracks[e, s]
            first = list(indices).index(row) == s  # a row that occurs twice: its cloud goes to the first position
            _cloud_part(rec, pts[lab == row] if first else pts[:0], min_electrons, centers)
            rec["end_x"] = rec["end_y"] = rec["end_tb"] = np.nan
            if counts is None:
                continue
            t = e * n_sim + s
            c = int(counts[t])
            rec["n_steps"] = n_steps[t]
            rec["n_samples"] = c
            rec["electrons"] = int(samples[t, :c, 3].astype(np.int64).sum())
            if c:
                rec["end_x"], rec["end_y"], rec["end_tb"] = samples[t, c - 1, :3]
    return events, tracks


def assert_same_records(got, ref, what=""):
    """Structured record arrays, field by field: integers equal, doubles bit-equal, NaN where NaN."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    for name in got.dtype.names:
        a, b = got[name], ref[name]
        if a.dtype.kind == "f":
            np.testing.assert_array_equal(a.view(np.uint64) * ~np.isnan(a), b.view(np.uint64) * ~np.isnan(b),
                                          err_msg=f"{what} {name} (bits)")
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what} {name} (NaN)")
        else:
            np.testing.assert_array_equal(a, b, err_msg=f"{what} {name}")


def hand_made_events():
    """(events, indices, min_electrons, expected): hand-made clouds with known answers -- cells shared by two tracks
    (the later label owns the row, charge and all), an event with no kept row, a label outside ``indices``, an empty
    event, a row that occurs twice in ``indices``.  ``expected``: {(event, field): value} / {(event, position, field):
    value} of records worked out by hand, with pad centres (x, y) = (pad, 2 pad) mm."""
    indices = [2, 5, 2]
    min_electrons = 100
    ev = []
    # 0: two tracks; the row on (pad 7, t 10) carries label 5 although both touched it
    ev.append((np.array([[7.0, 10.4, 500.0], [8.0, 11.9, 99.0], [7.0, 12.0, 100.0], [9.0, 3.2, 1000.0], [9.0, 4.7, 250.0]]),
               np.array([5, 2, 2, 5, 5])))
    # 1: rows, none kept
    ev.append((np.array([[100.0, 50.5, 99.0], [101.0, 51.5, 0.0]]), np.array([2, 5])))
    # 2: a label outside indices beside one inside
    ev.append((np.array([[3.0, 0.0, 300.0], [4.0, 511.99, 400.0], [3.0, 7.5, 150.0]]), np.array([4, 2, 17])))
    # 3: empty
    ev.append((np.zeros((0, 3)), np.zeros(0, dtype=np.int64)))
    # 4: pads 0 and 10239, a label beyond the row range
    ev.append((np.array([[0.0, 1.5, 100.0], [10239.0, 2.5, 101.0], [5.0, 3.5, 7.0e9]]), np.array([2, 5, 40])))
    expected = {
        (0, "n_points"): 5, (0, "n_kept"): 4, (0, "n_pads"): 2, (0, "tb_min"): 3, (0, "tb_max"): 12, (0, "charge"): 1949,
        (0, 0, "n_points"): 2, (0, 0, "n_kept"): 1, (0, 0, "n_pads"): 1, (0, 0, "tb_min"): 12, (0, 0, "tb_max"): 12,
        (0, 0, "charge"): 199, (0, 0, "rho2_max"): 7.0 * 7.0 + 14.0 * 14.0,
        (0, 1, "n_points"): 3, (0, 1, "n_kept"): 3, (0, 1, "n_pads"): 2, (0, 1, "tb_min"): 3, (0, 1, "tb_max"): 10,
        (0, 1, "charge"): 1750, (0, 1, "rho2_max"): 9.0 * 9.0 + 18.0 * 18.0,
        (0, 2, "n_points"): 0, (0, 2, "n_kept"): 0, (0, 2, "tb_min"): -1, (0, 2, "rho2_max"): -1.0,  # 2 again: empty
        (1, "n_points"): 2, (1, "n_kept"): 0, (1, "n_pads"): 0, (1, "tb_min"): -1, (1, "tb_max"): -1, (1, "charge"): 99,
        (1, 0, "n_points"): 1, (1, 0, "n_kept"): 0, (1, 0, "rho2_max"): -1.0, (1, 0, "charge"): 99,
        (2, "n_points"): 3, (2, "n_kept"): 3, (2, "n_pads"): 2, (2, "tb_min"): 0, (2, "tb_max"): 511, (2, "charge"): 850,
        (2, 0, "n_points"): 1, (2, 0, "tb_min"): 511, (2, 0, "charge"): 400, (2, 1, "n_points"): 0,
        (3, "n_points"): 0, (3, "n_kept"): 0, (3, "tb_min"): -1, (3, "charge"): 0, (3, 0, "n_points"): 0,
        (4, "n_points"): 3, (4, "n_kept"): 3, (4, "n_pads"): 3, (4, "charge"): 7000000201,
        (4, 1, "rho2_max"): 10239.0 * 10239.0 + 20478.0 * 20478.0, (4, 0, "rho2_max"): 0.0,
    }
    return ev, indices, min_electrons, expected


def hand_made_centers():
    pads = np.arange(_abi.NUM_PADS, dtype=np.float64)
    return np.column_stack([pads, 2.0 * pads])


def csr(events):
    offsets = np.zeros(len(events) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(p) for p, _ in events])
    points = np.concatenate([p for p, _ in events]).reshape(-1, 3)
    labels = np.concatenate([lab for _, lab in events]).astype(np.int64)
    return offsets, points, labels


def check_expected(events, tracks, expected):
    for key, value in expected.items():
        got = events[key[0]][key[1]] if len(key) == 2 else tracks[key[0], key[1]][key[2]]
        assert got == value, (key, got, value)
