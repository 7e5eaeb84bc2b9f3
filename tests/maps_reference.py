"""The run-maps contract of include/attpc_engine.h restated in numpy (test infrastructure only): plain loops over the
events of a CSR cloud; ``np.unique`` on (event, pad) and on (event, t) makes the distinct counts."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.maps import RunMaps

OTHER = 1 << _abi.MAX_SIM
FULL_MASK = (OTHER << 1) - 1


def position_bits(labels, indices):
    """The mask bit of every row: that of the first position of ``indices`` that holds its label, else ``OTHER``."""
    indices = [int(i) for i in indices]
    bits = np.full(len(labels), OTHER, dtype=np.int64)
    for row in set(indices):
        bits[np.asarray(labels) == row] = 1 << indices.index(row)
    return bits


def maps(offsets, points, labels, indices, min_electrons, track_mask=FULL_MASK, passed=None) -> RunMaps:
    """The maps of the CSR cloud ``offsets`` / ``points`` [P,3] (pad, tau, q) / ``labels`` [P] for the layout positions
    ``indices``: the rows that count are those of the contributing events (``passed`` [n] bool, None: all) with
    q >= ``min_electrons`` and their position's bit in ``track_mask``."""
    offsets = np.asarray(offsets, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    passed = np.ones(n, dtype=bool) if passed is None else np.asarray(passed, dtype=bool)
    out = RunMaps()
    pairs_pad, pairs_tb = [], []
    for e in range(n):
        if not passed[e]:
            continue
        out.n_events += 1
        lo, hi = offsets[e], offsets[e + 1]
        pts, bits = points[lo:hi], position_bits(labels[lo:hi], indices)
        counted = (pts[:, 2] >= min_electrons) & ((bits & track_mask) != 0)
        if not counted.any():
            continue
        out.n_hit += 1
        for pad, tau, q in pts[counted]:
            pad, t, q = int(pad), int(np.floor(tau)), int(q)
            out.pad_charge[pad] += q
            out.tb_rows[t] += 1
            out.tb_charge[t] += q
            pairs_pad.append((e, pad))
            pairs_tb.append((e, t))
    if pairs_pad:
        for _, pad in np.unique(np.array(pairs_pad, dtype=np.int64), axis=0):
            out.pad_events[pad] += 1
        for _, t in np.unique(np.array(pairs_tb, dtype=np.int64), axis=0):
            out.tb_events[t] += 1
    return out


def maps_fast(offsets, points, labels, indices, min_electrons, track_mask=FULL_MASK, passed=None) -> RunMaps:
    """``maps`` without the Python loop over rows (the same definition on whole arrays, for clouds of 1e6 rows)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    passed = np.ones(n, dtype=bool) if passed is None else np.asarray(passed, dtype=bool)
    lo, hi = (int(offsets[0]), int(offsets[-1])) if n else (0, 0)
    event = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    pts, lab = points[lo:hi], labels[lo:hi]
    counted = passed[event] & (pts[:, 2] >= min_electrons) & ((position_bits(lab, indices) & track_mask) != 0)
    event, pad = event[counted], pts[counted, 0].astype(np.int64)
    t, q = np.floor(pts[counted, 1]).astype(np.int64), pts[counted, 2].astype(np.int64)
    out = RunMaps(n_events=int(passed.sum()), n_hit=len(np.unique(event)))
    np.add.at(out.pad_charge, pad, q)
    np.add.at(out.tb_charge, t, q)
    np.add.at(out.tb_rows, t, np.uint64(1))
    np.add.at(out.pad_events, np.unique(event * _abi.NUM_PADS + pad) % _abi.NUM_PADS, np.uint64(1))
    np.add.at(out.tb_events, np.unique(event * _abi.NUM_TB + t) % _abi.NUM_TB, np.uint64(1))
    return out


def assert_same_maps(got: RunMaps, ref: RunMaps, what: str = "") -> None:
    for name in ("pad_events", "pad_charge", "tb_events", "tb_rows", "tb_charge"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype)
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {name}")
    assert (got.n_events, got.n_hit) == (ref.n_events, ref.n_hit), (what, got.n_events, got.n_hit, ref.n_events, ref.n_hit)


def hand_made_maps():
    """The non-zero cells of the maps of ``summary_reference.hand_made_events()`` (indices [2, 5, 2], min_electrons 100)
    worked out by hand, for the full mask, for position 0 alone, for position 2 alone (label 2 again: nothing) and for
    the other labels alone: {mask: {field: {cell: value}} plus n_events / n_hit}."""
    full = {
        # event 0: (7, 10, 500 | 5) (7, 12, 100 | 2) (9, 3, 1000 | 5) (9, 4, 250 | 5); the 99 on pad 8 is dropped
        # event 1: nothing kept; event 2: (3, 0, 300 | 4) (4, 511, 400 | 2) (3, 7, 150 | 17); event 3: empty
        # event 4: (0, 1, 100 | 2) (10239, 2, 101 | 5) (5, 3, 7e9 | 40)
        "pad_events": {7: 1, 9: 1, 3: 1, 4: 1, 0: 1, 10239: 1, 5: 1},
        "pad_charge": {7: 600, 9: 1250, 3: 450, 4: 400, 0: 100, 10239: 101, 5: 7000000000},
        "tb_events": {10: 1, 12: 1, 3: 2, 4: 1, 0: 1, 511: 1, 7: 1, 1: 1, 2: 1},
        "tb_rows": {10: 1, 12: 1, 3: 2, 4: 1, 0: 1, 511: 1, 7: 1, 1: 1, 2: 1},
        "tb_charge": {10: 500, 12: 100, 3: 7000001000, 4: 250, 0: 300, 511: 400, 7: 150, 1: 100, 2: 101},
        "n_events": 5, "n_hit": 3,
    }
    first = {  # label 2
        "pad_events": {7: 1, 4: 1, 0: 1}, "pad_charge": {7: 100, 4: 400, 0: 100},
        "tb_events": {12: 1, 511: 1, 1: 1}, "tb_rows": {12: 1, 511: 1, 1: 1}, "tb_charge": {12: 100, 511: 400, 1: 100},
        "n_events": 5, "n_hit": 3,
    }
    again = {"pad_events": {}, "pad_charge": {}, "tb_events": {}, "tb_rows": {}, "tb_charge": {}, "n_events": 5, "n_hit": 0}
    other = {  # labels 4, 17 and 40
        "pad_events": {3: 1, 5: 1}, "pad_charge": {3: 450, 5: 7000000000},
        "tb_events": {0: 1, 7: 1, 3: 1}, "tb_rows": {0: 1, 7: 1, 3: 1}, "tb_charge": {0: 300, 7: 150, 3: 7000000000},
        "n_events": 5, "n_hit": 2,
    }
    return {FULL_MASK: full, 1: first, 4: again, OTHER: other}


def from_cells(cells: dict) -> RunMaps:
    out = RunMaps(n_events=cells["n_events"], n_hit=cells["n_hit"])
    for name in ("pad_events", "pad_charge", "tb_events", "tb_rows", "tb_charge"):
        for cell, value in cells[name].items():
            getattr(out, name)[cell] = value
    return out
