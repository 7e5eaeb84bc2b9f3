"""The clustering of trace rows (include/attpc_engine.h, "clustering") restated in numpy by brute force, on its own:
nothing of the package is used, the metric is the full n x n matrix of an event -- no window, no sorted order assumed --
and the components come from scipy's ``connected_components`` (a plain flood fill where scipy is missing).  The
arithmetic is integer, so the result is the contract's exactly.

``Settings`` is the descriptor; ``cluster(settings, offsets, rows, labels, indices)`` gives the cluster label of every
row, the event records and the cluster records.  ``mutant`` names one deliberate departure from the contract
(``MUTANTS``), each a one-line change, each what a plausible slip in the kernel would compute; tests/test_cluster_cpu.py
shows that the exact comparison on the case set catches every one."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MUTANTS = ("self_not_counted", "strict_threshold", "eps_swapped", "border_lowest_index", "size_cut_core_only",
           "majority_tie_higher", "rank_tie_higher_id")
MAX_SIM = 8
CAPPED, INTERNAL = 1, 2
EVENT_DTYPE = np.dtype([("n_rows", "<i4"), ("n_range", "<i4"), ("n_core", "<i4"), ("n_border", "<i4"), ("n_noise", "<i4"),
                        ("n_clusters", "<i4"), ("n_small", "<i4"), ("n_split", "<i4"), ("n_fake", "<i4"), ("status", "<i4"),
                        ("reserved", "<i4", (2,)), ("truth_rows", "<u2", (MAX_SIM,))])
RECORD_DTYPE = np.dtype([("rows", "<i4"), ("core_rows", "<i4"), ("first_row", "<i4"), ("majority", "<i4"),
                         ("majority_rows", "<i4"), ("label", "<i4"), ("z_min", "<i4"), ("z_max", "<i4")])
assert EVENT_DTYPE.itemsize == 64 and RECORD_DTYPE.itemsize == 32


@dataclass
class Settings:
    eps_xy: float = 20.0
    eps_z: float = 20.0
    min_samples: int = 5
    min_cluster_size: int = 10
    max_rows: int = 16384
    match: str = "truth"  # or "rank"

    def units(self):
        """(Exy, Ez)"""
        return int(np.rint(16.0 * self.eps_xy)), int(np.rint(16.0 * self.eps_z))


def desc_error(s: Settings) -> bool:
    """The settings are outside the contract's ranges."""
    for eps in (s.eps_xy, s.eps_z):
        if not (np.isfinite(eps) and 1.0 / 16.0 <= eps <= 64.0):
            return True
    return (s.min_samples < 1 or s.min_cluster_size < 1 or not 1 <= s.max_rows <= 65535 or s.match not in ("truth", "rank"))


def quantise(rows):
    """Step 1 -> (ok [n], X, Y, Z int64 [n]; 0 where not ok)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    x, y, z, integral = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 4]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) <= 320.0) & (np.abs(y) <= 320.0) & (np.abs(z) <= 8192.0) & (np.abs(integral) < 2147483648.0)
    units = [np.where(ok, np.rint(16.0 * np.where(ok, v, 0.0)), 0.0).astype(np.int64) for v in (x, y, z)]
    return ok, *units


def metric(s: Settings, X, Y, Z, mutant=None):
    """Step 2 -> (d [n, n] int64, near [n, n] bool) of quantised rows that are all in range."""
    exy, ez = s.units()
    if mutant == "eps_swapped":
        exy, ez = ez, exy
    dx, dy, dz = (v[:, None] - v[None, :] for v in (X, Y, Z))
    d = (dx * dx + dy * dy) * (ez * ez) + dz * dz * (exy * exy)
    limit = exy * exy * ez * ez
    within = d < limit if mutant == "strict_threshold" else d <= limit
    return d, (np.abs(dz) <= ez) & within


def components(adjacent) -> np.ndarray:
    """The lowest index of the connected component of every node of a symmetric boolean matrix."""
    n = len(adjacent)
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components

        _, comp = connected_components(csr_matrix(adjacent), directed=False)
    except ImportError:
        comp = np.full(n, -1, dtype=np.int64)
        for start in range(n):
            if comp[start] >= 0:
                continue
            comp[start] = start
            todo = [start]
            while todo:
                a = todo.pop()
                for b in np.flatnonzero(adjacent[a] & (comp < 0)):
                    comp[b] = start
                    todo.append(int(b))
    lowest = np.full(n, n, dtype=np.int64)
    np.minimum.at(lowest, comp, np.arange(n))
    return lowest[comp]


def positions_of(labels, indices) -> np.ndarray:
    """Step 8: the position every truth label votes for, -1: none."""
    labels = np.asarray(labels, dtype=np.int64)
    pos = np.full(len(labels), -1, dtype=np.int64)
    for s in range(min(len(indices), MAX_SIM) - 1, -1, -1):
        if indices[s] >= 0:
            pos[labels == indices[s]] = s  # (descending s: the lowest position of a label given twice wins)
    return pos


def cluster_event(s: Settings, rows, labels, indices, mutant=None, detail: dict | None = None):
    """Steps 1 to 9 of one event -> (cluster labels [n] int64, its EVENT_DTYPE record, its RECORD_DTYPE records [8]).
    ``detail``, if given, receives the intermediate arrays of a clustered event (on its in-range rows ``row_of``): ``d``,
    ``near``, ``core``, ``cluster`` (the id of every row as an in-range index, -1: none, before the size cut) and
    ``ranked`` (the surviving ids by rank)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    n = len(rows)
    out = np.full(n, -1, dtype=np.int64)
    event = np.zeros((), dtype=EVENT_DTYPE)
    records = np.zeros(MAX_SIM, dtype=RECORD_DTYPE)
    records["first_row"] = -1
    pos = positions_of(labels, indices) if labels is not None else np.full(n, -1, dtype=np.int64)
    event["n_rows"] = n
    event["truth_rows"] = np.minimum(np.bincount(pos[pos >= 0], minlength=MAX_SIM), 65535)
    if n > s.max_rows:
        event["n_noise"], event["status"] = n, CAPPED
        return out, event, records
    ok, X, Y, Z = quantise(rows)
    event["n_range"] = int((~ok).sum())
    row_of = np.flatnonzero(ok)  # everything below is on the in-range rows; row_of is monotone
    X, Y, Z, pos_in = X[row_of], Y[row_of], Z[row_of], pos[row_of]
    m = len(row_of)
    d, near = metric(s, X, Y, Z, mutant)
    counts = near.sum(axis=1) - (1 if mutant == "self_not_counted" else 0)
    core = counts >= s.min_samples
    cluster = np.full(m, -1, dtype=np.int64)  # the id as an in-range index
    core_at = np.flatnonzero(core)
    if len(core_at):
        cluster[core_at] = core_at[components(near[np.ix_(core_at, core_at)])]
    reach = near & core[None, :]
    for i in np.flatnonzero(~core & reach.any(axis=1)):  # step 5
        candidates = np.flatnonzero(reach[i])
        j = candidates[0] if mutant == "border_lowest_index" else candidates[np.argmin(d[i, candidates])]
        cluster[i] = cluster[j]
    ids = np.unique(cluster[cluster >= 0])
    sizes = np.array([((cluster == c) & (core if mutant == "size_cut_core_only" else True)).sum() for c in ids], dtype=np.int64)
    kept = ids[sizes >= s.min_cluster_size]
    event["n_small"] = len(ids) - len(kept)
    event["n_clusters"] = len(kept)
    n_rows_of = np.array([(cluster == c).sum() for c in kept], dtype=np.int64)
    tie = kept if mutant != "rank_tie_higher_id" else -kept
    ranked = kept[np.lexsort((tie, -n_rows_of))]  # step 7: rows descending, id ascending
    if detail is not None:
        detail.update(row_of=row_of, d=d, near=near, core=core, cluster=cluster.copy(), ranked=ranked, sizes=n_rows_of)
    taken = set()
    for rank, c in enumerate(ranked):
        member = cluster == c
        votes = np.bincount(pos_in[member & (pos_in >= 0)], minlength=MAX_SIM)
        if votes.max() == 0:
            majority = -1
        elif mutant == "majority_tie_higher":
            majority = MAX_SIM - 1 - int(np.argmax(votes[::-1]))
        else:
            majority = int(np.argmax(votes))
        if s.match == "rank":
            label = indices[rank] if rank < min(len(indices), MAX_SIM) else -1
        elif majority >= 0 and majority not in taken:
            taken.add(majority)
            label = indices[majority]
        else:
            label = -1
            event["n_split" if majority >= 0 else "n_fake"] += 1
        out[row_of[member]] = label
        event["n_core"] += int((member & core).sum())
        event["n_border"] += int((member & ~core).sum())
        if rank < MAX_SIM:
            records[rank] = (int(member.sum()), int((member & core).sum()), int(row_of[c]), majority,
                             int(votes[majority]) if majority >= 0 else 0, label, int(Z[member].min()), int(Z[member].max()))
    event["n_noise"] = n - int(event["n_core"]) - int(event["n_border"])
    return out, event, records


def cluster(s: Settings, offsets, rows, labels, indices, mutant: str | None = None):
    """-> (cluster labels [R] int64, events [n] EVENT_DTYPE, records [n, 8] RECORD_DTYPE); rows outside the offsets -1."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert not desc_error(s), s
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    n = len(offsets) - 1
    out = np.full(len(rows), -1, dtype=np.int64)
    events = np.zeros(n, dtype=EVENT_DTYPE)
    records = np.zeros((n, MAX_SIM), dtype=RECORD_DTYPE)
    for e in range(n):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        out[lo:hi], events[e], records[e] = cluster_event(s, rows[lo:hi], None if labels is None else np.asarray(labels)[lo:hi],
                                                          list(indices), mutant)
    return out, events, records


def same(got, want) -> bool:
    """Labels, event records and cluster records equal, byte for byte (structured arrays of any equal layout)."""
    return (np.array_equal(np.asarray(got[0], dtype=np.int64), np.asarray(want[0], dtype=np.int64))
            and all(np.array_equal(np.asarray(g)[name], np.asarray(w)[name]) for g, w in zip(got[1:], want[1:])
                    for name in np.asarray(w).dtype.names))
