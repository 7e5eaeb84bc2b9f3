"""The settings and row sets of the drift-correction tests (tests/test_undistort_cpu.py, tests/test_gpu_undistort.py).
The map is M of tests/distortion_cases.py in its drift (time-bucket edges 10 / 560, length 1 m).

``stage_cases()`` is the case set of the stage alone: one CSR array of events, each built to hold one way the kernel can
go wrong, with empty events between them.  Rows are made from apparent points (x m, y m, time bucket): columns 0, 1 in
mm, column 2 through the trace rows' relation, column 6 the time; columns 3, 4, 5, 7 carry a running number so that a row
that moved is seen.  Events come in descending apparent time, as the trace rows do, unless said otherwise."""
from __future__ import annotations

import numpy as np

from tests import distortion_cases as dc
from tests import distortion_reference as dref
from tests import undistort_reference as uref

SIZES = (0, 1, 63, 64, 65, 257, 1025)


def settings(m: dref.Map | None = None, **changes) -> uref.Settings:
    return uref.Settings(dc.reference_map() if m is None else m, dc.WIN_EDGE, dc.MM_EDGE, dc.LENGTH, **changes)


def rows_of(points: np.ndarray, first_number: int = 0) -> np.ndarray:
    """[n, 8] rows of apparent points [n, 3]."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    rows = np.empty((len(points), 8))
    with np.errstate(all="ignore"):
        rows[:, 0], rows[:, 1] = points[:, 0] * 1000.0, points[:, 1] * 1000.0
        rows[:, 2] = (dc.WIN_EDGE - points[:, 2]) / (dc.WIN_EDGE - dc.MM_EDGE) * dc.LENGTH * 1000.0
    number = first_number + np.arange(len(points), dtype=np.float64)
    rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 7] = number, 2.0 * number, number % 10240.0, 0.5
    rows[:, 6] = points[:, 2]
    return rows


def apparent_points(n: int, seed: int, tb=(dc.MM_EDGE, dc.WIN_EDGE), rho_limit: float = 0.28, sort: bool = True) -> np.ndarray:
    """[n, 3]: true points uniform in the disc and in ``tb``, moved by M; in descending apparent time if ``sort``."""
    rng = np.random.default_rng(seed)
    rho = rho_limit * np.sqrt(rng.uniform(size=n))
    phi = rng.uniform(0.0, 2.0 * np.pi, size=n)
    truth = np.stack([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(*tb, size=n), np.zeros(n)], axis=1)
    seen = dref.shift_records(dc.reference_map(), truth)[:, :3]
    return seen[np.argsort(-seen[:, 2], kind="stable")] if sort else seen


def stage_cases():
    """(offsets [n + 1], rows [R, 8], labels [R], names [n]) of the stage-alone case set."""
    events, names = [], []

    def add(name, rows):
        events.append(np.asarray(rows, dtype=np.float64).reshape(-1, 8))
        names.append(name)
        events.append(np.empty((0, 8)))
        names.append("empty")

    for k, n in enumerate(SIZES):  # the sizes around a wave, a tile of the workgroup and several tiles
        add(f"{n} rows", rows_of(apparent_points(n, 10 + k)))
    # one t for every row: the order is the input order (x, y and t are one point, the payload tells the rows apart)
    add("one t", rows_of(np.tile([[0.11, -0.07, 300.25]], (130, 1))))
    # two values of t, interleaved: ties inside a bin beside a second key
    add("two t", rows_of(np.array([[0.11, -0.07, 300.25], [0.11, -0.07, 300.2501]])[np.arange(150) % 2]))
    # every corrected t below 0 / above 511: the clamped end bins (M's time shift is at most 4 buckets)
    add("all below 0", rows_of(apparent_points(200, 30, tb=(-40.0, -6.0))))
    add("all above 511", rows_of(apparent_points(200, 31, tb=(518.0, 559.0))))
    add("across 0 and 512", rows_of(apparent_points(300, 32, tb=(-8.0, 530.0), sort=False)))
    # the map's edges, from the geometry of edge_records: rho = 0, on and beyond the nodes, the non-finite records
    edge = dc.edge_records()[:, :3]
    add("edges", rows_of(edge))
    # non-finite rows between good ones, NaN payloads in columns 3 .. 7 of good and of skipped rows
    mixed = rows_of(apparent_points(90, 33))
    payload = np.array([0x7FF8000000ABCDEF, 0xFFF8000000000001, 0x7FF0000000000000], dtype=np.uint64).view(np.float64)
    for k, i in enumerate(range(3, 90, 7)):
        mixed[i, (0, 1, 6)[k % 3]] = (np.nan, np.inf, -np.inf)[k % 3]
    for k, i in enumerate(range(0, 90, 5)):
        mixed[i, 3 + k % 5] = payload[k % 3]
    add("non-finite", mixed)
    add("all skipped", np.full((5, 8), np.nan))
    rows = np.concatenate(events)
    counts = np.array([len(e) for e in events], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    labels = (np.arange(len(rows), dtype=np.int64) * 7) % 5 - 1
    return offsets, np.ascontiguousarray(rows), labels, names


def steep_map() -> dref.Map:
    """A radial shift of 1.5 rho on a grid of 0.6 m (0.9 m at most, inside the 1 m cap): the fixed point diverges."""
    rho = np.linspace(0.0, 0.6, 33)
    radial = np.repeat((1.5 * rho)[:, None], 41, axis=1)
    return dref.Map(0.6 / 32, 550.0 / 40, 10.0, radial, None, None)


def bad_settings():
    """(field, value) of every way an attpc_undistort_desc can be wrong beside its map."""
    nan, inf = float("nan"), float("inf")
    return [("windows_edge", dc.MM_EDGE), ("windows_edge", dc.MM_EDGE - 1), ("length", 0.0), ("length", -1.0), ("length", nan),
            ("length", inf), ("iterations", 0), ("iterations", 65), ("iterations", -1), ("tolerance_xy", -1e-9),
            ("tolerance_xy", nan), ("tolerance_xy", inf), ("tolerance_tb", -1.0), ("tolerance_tb", nan), ("tolerance_tb", inf)]
