"""Small synthetic events at the shapes where the clustering (include/attpc_engine.h, "clustering") can go wrong, a
handful to 600 rows each, every coordinate a whole number of 1/16 mm so that nothing hangs on a rounding.  ``events()``
is the list; ``GROUPS`` names the settings every event is clustered under (both match modes, unequal linking lengths, a
small row cap, two values of min_samples); ``csr()`` is the list as one CSR array; ``reference()`` is the restatement of
every group, computed once; ``check_cases()`` asserts with the restatement that every situation the events are named
for actually occurs -- a border row with two candidate clusters, a rank tie and so on -- so a comparison on this set is
not empty where it matters.

The base linking length is 2 mm = 32 units in x, y and z; ``INDICES`` = (2, 0, 3): the truth label 2 belongs to
position 0, 0 to position 1, 3 to position 2, so a mix-up of label and position shows."""
from __future__ import annotations

import functools

import numpy as np

from tests import cluster_reference as cref

E = 32  # the base linking length in units
INDICES = (2, 0, 3)
GROUPS = {
    "base": cref.Settings(2.0, 2.0, 3, 5, 16384, "truth"),
    "rank": cref.Settings(2.0, 2.0, 3, 5, 16384, "rank"),
    "four": cref.Settings(2.0, 2.0, 4, 5, 16384, "truth"),   # min_samples 4: a border row can touch two clusters
    "aniso": cref.Settings(1.0, 3.0, 3, 5, 16384, "truth"),  # eps_xy != eps_z
    "capped": cref.Settings(2.0, 2.0, 3, 5, 256, "truth"),   # a small max_rows
}


def _event(points, labels, keep_order: bool = False):
    """Rows [n, 8] of points [n, 3] in units (sorted by z, stably, unless ``keep_order``) and their labels."""
    points = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    labels = np.broadcast_to(np.asarray(labels, dtype=np.int64), (len(points),)).copy()
    if not keep_order:
        order = np.argsort(points[:, 2], kind="stable")
        points, labels = points[order], labels[order]
    rows = np.zeros((len(points), 8))
    rows[:, :3] = points / 16.0
    rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6], rows[:, 7] = 50.0, 100.0, 1.0, 7.0, 1.0
    return rows, labels


def _line(n: int, step: int, x: int = 0, y: int = 0, z0: int = 0, wiggle: int = 0):
    """n points along z, ``step`` units apart, x wiggling by ``wiggle`` units."""
    k = np.arange(n)
    return np.stack([x + wiggle * (k % 2), np.full(n, y), z0 + step * k], axis=1)


def _snake(n: int, step: int, z: int = 160):
    """A chain of n points at one z: along x, up by two steps, back along x -- consecutive points ``step`` apart, no
    other pair closer than 2 * step - 2 or step * sqrt(2)."""
    half = (n - 2) // 2
    there = [(-4650 + step * k, 0) for k in range(half + 1)]
    x_end = there[-1][0]
    turn = [(x_end, step), (x_end, 2 * step)]
    back = [(x_end - step * k, 2 * step) for k in range(1, n - len(there) - len(turn) + 1)]
    xy = np.array(there + turn + back)
    return np.concatenate([xy, np.full((len(xy), 1), z)], axis=1)


def events():
    """[(name, rows [n, 8], labels [n])]"""
    rng = np.random.default_rng(20261021)
    out = []

    def add(name, points, labels, **kw):
        out.append((name, *_event(points, labels, **kw)))

    add("empty", np.zeros((0, 3)), np.zeros(0))
    add("one row", [[0, 0, 100]], 2)
    add("min_samples - 1 rows", [[0, 0, 100], [8, 0, 104]], 2)
    for n in (255, 256, 257):  # rows straddle a tile of the workgroup
        add(f"line of {n}", _line(n, 16, wiggle=5), 2)
    add("z chain of 600", _line(600, E - 1), 2)  # one unit under the linking length: three neighbours each
    snake = _snake(600, E - 1)
    add("shuffled chain of 600", snake[rng.permutation(600)], 0, keep_order=True)  # one z: any order is sorted
    gap = _line(600, E - 1)
    gap[300:, 2] += 1  # the step from row 299 to row 300 is exactly the linking length
    add("chain with a gap of the linking length", gap, 2)
    gap = gap.copy()
    gap[300:, 2] += 1  # ... and one unit more: two clusters of 300 rows, a rank tie
    add("chain with a gap one unit over", gap, 2)
    grid = np.stack(np.meshgrid(np.arange(18), np.arange(18)), axis=-1).reshape(-1, 2)[:300]
    add("blob of 300 at one z", np.concatenate([grid[rng.permutation(300)], np.full((300, 1), 480)], axis=1), 3,
        keep_order=True)
    # two clusters of four core rows (under min_samples 4) on the x axis; a border row in the middle at the linking
    # length from the first core row of each (B's has the lower index), and a border row above A whose nearest core row
    # (-32, 0) stands behind a farther one (-40, 0)
    b_rows = [[32, 0, 0], [40, 0, 0], [48, 0, 0], [56, 0, 0]]
    a_rows = [[-40, 0, 0], [-32, 0, 0], [-48, 0, 0], [-56, 0, 0]]
    add("border row between two clusters", b_rows + [[0, 0, 0]] + a_rows + [[-32, 30, 0]], [0] * 4 + [2] + [2] * 4 + [2],
        keep_order=True)
    # ... and a border row whose nearest core row (-32, of the later cluster) is not its first core neighbour (30)
    add("border row nearer to the later cluster", [[30, 0, 0], [38, 0, 0], [46, 0, 0], [54, 0, 0], [-2, 0, 0]] + a_rows, 2,
        keep_order=True)
    add("two clusters of equal size", np.concatenate([_line(10, 16, x=400), _line(10, 16, x=-400, z0=8)]), [0] * 10 + [2] * 10)
    ten = np.concatenate([_line(6 + k, 16, x=-2000 + 400 * k, z0=5 * k) for k in range(10)])
    add("ten clusters", ten, np.concatenate([np.full(6 + k, (2, 0, 3)[k % 3]) for k in range(10)]))
    add("majority tie", _line(10, 16), [2, 0] * 5)
    add("two clusters with one majority", np.concatenate([_line(12, 16, x=300), _line(8, 16, x=-300, z0=4)]), 2)
    add("cluster of noise rows only", np.concatenate([_line(9, 16, x=300), _line(7, 16, x=-300, z0=4)]), [-1] * 9 + [3] * 7)
    add("cluster one row under min_cluster_size", np.concatenate([_line(4, 8), _line(5, 8, x=900)]), 2)
    add("all noise", np.stack([np.arange(30) * 200 - 3000, np.arange(30) * 150 - 2000, np.arange(30) * 90], axis=1), -1)
    add("labels outside the layout", _line(12, 16), [2] * 5 + [7] * 7)
    # out-of-range rows in the middle and at the end
    rows, labels = _event(_line(24, 16), 2)
    rows[7, 0], rows[8, 1], rows[9, 0], rows[10, 4] = np.nan, np.inf, 320.0625, 2147483648.0
    rows[11, 2] = np.nan
    rows[20:, :3] = np.nan  # (as the drift correction leaves its skipped rows: behind the others)
    out.append(("out-of-range rows", rows, labels))
    # two tracks that meet at a vertex, a broken one, and uniform noise: random, on the unit grid
    t = np.arange(150)
    one = np.stack([6 * t, 2 * t, 12 * t], axis=1) + rng.integers(-3, 4, (150, 3))
    two = np.stack([-5 * t, 4 * t, 10 * t], axis=1) + rng.integers(-3, 4, (150, 3))
    three = np.stack([-1500 + 3 * t, -800 - 6 * t, 300 + 11 * t], axis=1)[np.r_[0:60, 75:150]] + rng.integers(-3, 4, (135, 3))
    noise = np.stack([rng.integers(-4000, 4000, 80), rng.integers(-4000, 4000, 80), rng.integers(0, 2000, 80)], axis=1)
    add("tracks and noise", np.concatenate([one, two, three, noise]), [2] * 150 + [0] * 150 + [3] * 135 + [-1] * 80)
    return out


@functools.lru_cache(maxsize=None)
def csr():
    """(offsets [n+1], rows [R, 8], labels [R], names [n]) of ``events()``; do not write into them."""
    evs = events()
    offsets = np.concatenate([[0], np.cumsum([len(rows) for _, rows, _ in evs])]).astype(np.int64)
    rows, labels = np.concatenate([r for _, r, _ in evs]), np.concatenate([lab for _, _, lab in evs])
    for a in (offsets, rows, labels):
        a.setflags(write=False)
    return offsets, rows, labels, tuple(name for name, _, _ in evs)


@functools.lru_cache(maxsize=None)
def reference():
    """{group: (cluster labels [R], events [n], records [n, 8])} of the restatement on ``csr()``, computed once."""
    offsets, rows, labels, _ = csr()
    return {group: cref.cluster(s, offsets, rows, labels, INDICES) for group, s in GROUPS.items()}


def event_detail(group: str, name: str) -> dict:
    """The restatement's intermediate arrays of one event under one group (see ``cluster_reference.cluster_event``)."""
    offsets, rows, labels, names = csr()
    e = names.index(name)
    detail = {}
    out = cref.cluster_event(GROUPS[group], rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]], list(INDICES),
                             detail=detail)
    detail["out"], detail["event"], detail["records"] = out
    return detail


def exact_threshold_pairs(group: str, name: str) -> int:
    """The pairs of an event's in-range rows whose d equals the threshold (sklearn compares rounded square roots there)."""
    detail = event_detail(group, name)
    exy, ez = GROUPS[group].units()
    return int((detail["d"] == exy * exy * ez * ez).sum()) if "d" in detail else 0


def check_cases() -> None:
    """Every situation the events are named for occurs, by the restatement."""
    offsets, rows, labels, names = csr()
    ref = reference()
    sizes = dict(zip(names, np.diff(offsets)))
    ev = {g: dict(zip(names, ref[g][1])) for g in GROUPS}
    rec = {g: dict(zip(names, ref[g][2])) for g in GROUPS}
    base, recs = ev["base"], rec["base"]
    assert sizes["empty"] == 0 and sizes["one row"] == 1 and sizes["min_samples - 1 rows"] == GROUPS["base"].min_samples - 1
    for name in ("empty", "one row", "min_samples - 1 rows", "all noise"):
        assert base[name]["n_clusters"] == 0 and base[name]["n_noise"] == sizes[name] and recs[name]["first_row"][0] == -1, name
    for n in (255, 256, 257):
        assert sizes[f"line of {n}"] == n and base[f"line of {n}"]["n_clusters"] == 1 and recs[f"line of {n}"]["rows"][0] == n
    # the chains: every inner row has exactly min_samples neighbours, the ends are border rows; one component of 598 core rows
    for name in ("z chain of 600", "shuffled chain of 600", "chain with a gap of the linking length"):
        d = event_detail("base", name)
        assert sizes[name] == 600 and np.all(d["near"].sum(axis=1) <= 3) and d["core"].sum() == 598, name
        assert base[name]["n_clusters"] == 1 and recs[name]["rows"][0] == 600 and base[name]["n_border"] == 2, name
    d = event_detail("base", "shuffled chain of 600")  # the chain's neighbours lie far apart in row order
    i, j = np.nonzero(np.triu(d["near"], 1))
    assert np.median(np.abs(i - j)) > 100 and len(np.unique(rows[offsets[names.index("shuffled chain of 600")]:][:600, 2])) == 1
    assert exact_threshold_pairs("base", "chain with a gap of the linking length") == 2  # (the pair, both ways)
    two = recs["chain with a gap one unit over"]
    assert base["chain with a gap one unit over"]["n_clusters"] == 2 and list(two["rows"][:2]) == [300, 300]
    assert list(two["first_row"][:2]) == [1, 301] and list(two["label"][:2]) == [2, -1]  # a rank tie: the lower id first
    assert base["chain with a gap one unit over"]["n_split"] == 1
    d = event_detail("base", "blob of 300 at one z")  # every row in every row's window
    assert sizes["blob of 300 at one z"] == 300 and d["near"].all() and recs["blob of 300 at one z"]["core_rows"][0] == 300
    # the border rows: under min_samples 4 row 4 has a core neighbour in each cluster at equal d, and goes to the lower row
    d = event_detail("four", "border row between two clusters")
    assert not d["core"][4] and not d["core"][9] and d["core"].sum() == 8
    cand = np.flatnonzero(d["near"][4] & d["core"])
    assert list(cand) == [0, 6] and d["d"][4, 0] == d["d"][4, 6] and d["cluster"][0] != d["cluster"][6] and d["cluster"][4] == d["cluster"][0]
    cand = np.flatnonzero(d["near"][9] & d["core"])  # ... and row 9's nearest core row is not its first
    assert list(cand) == [5, 6] and d["d"][9, 6] < d["d"][9, 5]
    four = rec["four"]["border row between two clusters"]
    assert ev["four"]["border row between two clusters"]["n_clusters"] == 2 and list(four["rows"][:2]) == [5, 5]
    assert list(four["core_rows"][:2]) == [4, 4]  # (the size cut counts the border rows: 4 core rows alone would not survive)
    assert ev["base"]["border row between two clusters"]["n_clusters"] == 1  # (min_samples 3: the middle row is core and joins them)
    d = event_detail("four", "border row nearer to the later cluster")
    cand = np.flatnonzero(d["near"][4] & d["core"])
    assert not d["core"][4] and list(cand) == [0, 6] and d["d"][4, 6] < d["d"][4, 0] and d["cluster"][4] == d["cluster"][6] != d["cluster"][0]
    assert ev["four"]["border row nearer to the later cluster"]["n_small"] == 1
    tie = recs["two clusters of equal size"]
    assert list(tie["rows"][:2]) == [10, 10] and tie["first_row"][0] < tie["first_row"][1] and list(tie["label"][:2]) == [0, 2]
    assert list(rec["rank"]["two clusters of equal size"]["label"][:2]) == [2, 0]  # (rank: position 0 to the first, whatever its truth)
    ten = base["ten clusters"]
    assert ten["n_clusters"] == 10 and np.all(recs["ten clusters"]["first_row"] >= 0) and list(recs["ten clusters"]["rows"]) == list(range(15, 7, -1))
    assert ten["n_split"] == 7 and ten["n_fake"] == 0
    assert list(rec["rank"]["ten clusters"]["label"]) == [2, 0, 3, -1, -1, -1, -1, -1] and ev["rank"]["ten clusters"]["n_split"] == 0
    major = recs["majority tie"]
    assert major["majority"][0] == 0 and major["majority_rows"][0] == 5 and major["rows"][0] == 10 and major["label"][0] == 2
    split = recs["two clusters with one majority"]
    assert base["two clusters with one majority"]["n_split"] == 1 and list(split["label"][:2]) == [2, -1] and list(split["majority"][:2]) == [0, 0]
    fake = recs["cluster of noise rows only"]
    assert base["cluster of noise rows only"]["n_fake"] == 1 and fake["majority"][0] == -1 and fake["label"][0] == -1 and fake["label"][1] == 3
    small = base["cluster one row under min_cluster_size"]
    assert small["n_small"] == 1 and small["n_clusters"] == 1 and small["n_noise"] == 4
    outside = recs["labels outside the layout"]
    assert outside["majority_rows"][0] == 5 and outside["rows"][0] == 12 and base["labels outside the layout"]["truth_rows"][0] == 5
    rng_ev = base["out-of-range rows"]
    assert rng_ev["n_range"] == 9 and rng_ev["n_clusters"] == 2 and rng_ev["n_noise"] == 9
    lo = offsets[names.index("out-of-range rows")]
    assert np.all(ref["base"][0][lo + 7:lo + 12] == -1) and np.all(ref["base"][0][lo + 20:lo + 24] == -1) and ref["base"][0][lo + 12] >= 0
    capped = ev["capped"]
    assert [capped[f"line of {n}"]["status"] for n in (255, 256, 257)] == [0, 0, cref.CAPPED]
    assert capped["line of 257"]["n_noise"] == 257 and capped["line of 257"]["truth_rows"][0] == 257 and capped["z chain of 600"]["status"] == cref.CAPPED
    assert not any(base[name]["status"] for name in names)
    # eps_xy != eps_z: the chain in the plane falls apart under an eps_xy of 1 mm, the chain along z holds
    assert ev["aniso"]["shuffled chain of 600"]["n_clusters"] == 0 and ev["aniso"]["z chain of 600"]["n_clusters"] == 1
    mixed = base["tracks and noise"]
    assert mixed["n_clusters"] >= 3 and mixed["n_noise"] >= 40 and mixed["n_split"] >= 1
    assert exact_threshold_pairs("base", "tracks and noise") == 0
    # the two match modes differ, and so do the settings groups
    for g in ("rank", "four", "aniso", "capped"):
        assert not cref.same(ref[g], ref["base"]), g
