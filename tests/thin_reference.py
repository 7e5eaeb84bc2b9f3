"""The contract of the thinned track points (include/attpc_engine.h, "thinned track points") restated in numpy: the
quantisation of the estimates, bins by integer floor division, runs of equal bin cut at 4096 rows, the sums as exact
int64 (asserted to keep the header's bounds) and the centroid C(S) = (2 S + W) // (2 W).  ``thin`` returns what
``attpc_rows_thin`` delivers, to compare for equality; ``band_track`` makes the synthetic band of rows on which the
method itself is judged."""
import numpy as np

from attpc_engine_amd._abi import THIN_INFO_DTYPE, THIN_MAX_RUN


def step_units(z_step):
    """H of the contract (the desc check: 1/16 <= z_step <= 512)."""
    assert np.isfinite(z_step) and 1.0 / 16.0 <= z_step <= 512.0
    return int(np.rint(16.0 * float(z_step)))


def floor_bin(Z, H):
    return Z // H  # (Python and numpy divide integers with floor semantics)


def centroid(S, W):
    return (2 * S + W) // (2 * W)


def quantise(rows):
    """Step 1 of the estimate contract -> (ok [n], X, Y, Z, I as int64 [n], 0 where not ok)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    x, y, z, integral = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) <= 320.0) & (np.abs(y) <= 320.0) & (np.abs(z) <= 8192.0) & (np.abs(integral) < 2147483648.0)
    q = np.where(ok[:, None], np.stack([16.0 * x, 16.0 * y, 16.0 * z, integral], axis=1), 0.0)
    q = np.rint(q).astype(np.int64)  # half to even
    return ok, q[:, 0], q[:, 1], q[:, 2], q[:, 3]


def label_points(rows, H):
    """The points of one (event, position): ``rows`` [n, 8] are the event's rows of the label in delivered order ->
    (points [p, 8], n_dropped, n_split)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    ok, X, Y, Z, I = quantise(rows)
    n_dropped = int((~ok).sum())
    X, Y, Z, I, amplitude = X[ok], Y[ok], Z[ok], I[ok], rows[ok, 3]
    n = len(X)
    if n == 0:
        return np.zeros((0, 8)), n_dropped, 0
    bins = floor_bin(Z, H)
    w = np.maximum(I, 1)
    head = np.ones(n, dtype=bool)
    head[1:] = bins[1:] != bins[:-1]
    run_start = np.flatnonzero(head)
    run_rows = np.diff(np.append(run_start, n))
    starts, closed_by_split, n_split = [], [], 0
    for start, length in zip(run_start.tolist(), run_rows.tolist()):
        pieces = -(-length // THIN_MAX_RUN)
        starts += [start + THIN_MAX_RUN * j for j in range(pieces)]
        closed_by_split += [1] * (pieces - 1) + [0]
        n_split += pieces if pieces > 1 else 0
    starts = np.asarray(starts, dtype=np.int64)
    count = np.diff(np.append(starts, n))
    assert count.max() <= THIN_MAX_RUN and w.max() < 1 << 31 and np.abs(Z).max() <= 1 << 17 and max(np.abs(X).max(), np.abs(Y).max()) <= 5120
    W, Sx, Sy, Sz, SI = (np.add.reduceat(v, starts) for v in (w, w * X, w * Y, w * Z, I))
    assert np.abs(Sz).max() < 1 << 60 and W.max() < 1 << 43  # the header's bounds: nothing wrapped
    points = np.zeros((len(starts), 8))
    points[:, 0], points[:, 1], points[:, 2] = centroid(Sx, W) / 16.0, centroid(Sy, W) / 16.0, centroid(Sz, W) / 16.0
    points[:, 3] = np.fmax.reduceat(amplitude, starts)  # NaN ignored
    points[:, 4], points[:, 5], points[:, 6], points[:, 7] = SI, count, bins[starts], closed_by_split
    return points, n_dropped, n_split


def thin(offsets, rows, labels, indices, z_step):
    """(point_offsets [n + 1], points [P, 8], point_labels [P], info [n, len(indices)]) of rows in CSR form."""
    H = step_units(z_step)
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    info = np.zeros((n, len(indices)), dtype=THIN_INFO_DTYPE)
    point_offsets, points, point_labels = np.zeros(n + 1, dtype=np.int64), [np.zeros((0, 8))], [np.zeros(0, dtype=np.int64)]
    for e in range(n):
        ev_rows, ev_labels = rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        total = 0
        for s, index in enumerate(indices):
            if index < 0 or list(indices).index(index) != s:  # a label given twice goes to its first position
                continue
            mine = ev_rows[ev_labels == index]
            pts, n_dropped, n_split = label_points(mine, H)
            info[e, s] = (len(mine), len(pts), n_dropped, n_split)
            points.append(pts)
            point_labels.append(np.full(len(pts), index, dtype=np.int64))
            total += len(pts)
        point_offsets[e + 1] = point_offsets[e] + total
    return point_offsets, np.concatenate(points), np.concatenate(point_labels), info


def assert_same_points(got, want):
    """Offsets, labels and info equal; the point rows equal with NaN (amplitude) in the same places."""
    for g, w, name in zip(got, want, ("point_offsets", "points", "point_labels", "info")):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)  # (NaN == NaN here)


# ---------------------------------------------------------------- the synthetic band ----
BAND_RADIUS, BAND_CENTRE = 140.0, (150.0, 20.0)


def band_track(rng, n_z, turn, dz):
    """Rows [n, 8] of a track as the pad plane sees it: at every one of ``n_z`` z steps up to seven rows across the
    circle of radius 140 mm about (150, 20), 4.9 mm apart with a Gaussian charge profile, sorted by z."""
    i = np.arange(n_z)
    angle = 3.3 - turn * i / (n_z - 1)
    z = 100.0 + dz * i + rng.uniform(0.0, 0.9 * dz, n_z)
    off = np.arange(-3, 4)[None, :] * 4.9 + rng.uniform(-1.5, 1.5, (n_z, 7))
    g = np.exp(-off * off / 18.0)
    radius = BAND_RADIUS + off
    x, y = BAND_CENTRE[0] + radius * np.cos(angle)[:, None], BAND_CENTRE[1] + radius * np.sin(angle)[:, None]
    keep = g >= 0.02
    rows = np.zeros((int(keep.sum()), 8))
    rows[:, 0], rows[:, 1], rows[:, 2] = x[keep], y[keep], np.broadcast_to(z[:, None], g.shape)[keep]
    rows[:, 3], rows[:, 4] = 50.0 * g[keep] + 5.0, 2000.0 * g[keep] + 0.5
    return rows[np.argsort(rows[:, 2], kind="stable")]


def band_slope(n_z, turn, dz):
    """dz per mm of path of ``band_track``."""
    return dz * (n_z - 1) / (BAND_RADIUS * turn)


def fused_records(offsets, rows, labels, indices, z_step, params, circle=None):
    """The records of a trace-row call with the estimates and thinning both on: the estimate contract on the event's
    point rows, ATTPC_EST_RANGE OR-ed in where thinning dropped a row of the label.  ``circle`` (a
    ``circle_reference.Settings``): with the geometric circle fit on as well."""
    from attpc_engine_amd._abi import EST_RANGE
    from tests import estimate_reference as est

    point_offsets, points, point_labels, info = thin(offsets, rows, labels, indices, z_step)
    if circle is not None:
        from tests import circle_reference

        records = circle_reference.records(point_offsets, points, point_labels, indices, params, circle)
    else:
        records = est.records(point_offsets, points, point_labels, indices, params)
    records["status"] |= np.where(info["n_dropped"] > 0, EST_RANGE, 0).astype(np.int32)
    return records
