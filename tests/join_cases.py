"""Small synthetic events at the shapes where the cluster joining (include/attpc_engine.h, "cluster joining") can go
wrong, built like tests/cluster_cases.py: every coordinate a whole number of 1/16 mm.  A track piece is an ARC: points
20 units apart on a circle in the pad plane, 2 units apart in z, so that its rows link under the clustering's 2 mm
(32 units); the pieces of one event are at least 200 units apart in z, so the clustering never links two of them.
``events()`` is the list; ``CLUSTERING`` the clustering every event gets (``RANK``: the same with match="rank");
``GROUPS`` the four groups of join settings; ``csr()`` the list as one CSR array; ``reference()`` the restatement of
every group, computed once; ``check_cases()`` asserts on the restatement's own intermediate values that every event is
what its name says, so a case cannot go empty silently.

``INDICES`` = (2, 0, 3) as in tests/cluster_cases.py.  The pair of events "overlap just above / below the ratio" is
found by moving one centre unit by unit (``_threshold_distance``); the two ratios A / (pi Rs^2) are in ``JUST`` and
asserted: 0.50037 at a distance of 647 units and 0.49964 at 648 (printed by check_cases)."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import cluster_reference as cref
from tests import join_reference as jref
from tests.cluster_cases import _event, _line

INDICES = (2, 0, 3)
CLUSTERING = cref.Settings(2.0, 2.0, 3, 5, 800, "truth")
RANK = cref.Settings(2.0, 2.0, 3, 5, 800, "rank")
GROUPS = {
    "defaults": jref.JoinSettings(),
    "ratio": jref.JoinSettings(radius_ratio=1.5),
    "quarter": jref.JoinSettings(overlap_ratio=0.25),
    "two": jref.JoinSettings(max_clusters=2),
}
# what every comparison runs: the four groups, the defaults under match="rank", and overlap_ratio 1, where the area
# comparison of step 6c meets equality ("two pieces over one another")
RUNS = {**{g: (CLUSTERING, j) for g, j in GROUPS.items()}, "rank": (RANK, GROUPS["defaults"]),
        "full": (CLUSTERING, jref.JoinSettings(overlap_ratio=1.0))}
GAP = 200  # units of z between two pieces of an event
JUST = {}  # {"above": ratio, "below": ratio, "distance": units}, filled by events()


def _arc(cx: int, cy: int, r: int, a0: float, a1: float, z0: int, n: int | None = None):
    """Points [n, 3] on the circle (cx, cy, r) from angle a0 to a1, about 20 units apart, z rising by 2 from z0."""
    n = n if n is not None else max(int(math.ceil(r * abs(a1 - a0) / 20.0)), 2)
    angle = np.linspace(a0, a1, n)
    x, y = np.rint(cx + r * np.cos(angle)), np.rint(cy + r * np.sin(angle))
    return np.stack([x, y, z0 + 2 * np.arange(n)], axis=1).astype(np.int64)


def _stack(*pieces):
    """The pieces one behind the other in z, GAP apart -> points [n, 3] (each piece's z starts where it is put)."""
    out, z = [], 0
    for piece in pieces:
        piece = piece.copy()
        piece[:, 2] += z - piece[:, 2].min()
        z = int(piece[:, 2].max()) + GAP
        out.append(piece)
    return np.concatenate(out)


def _threshold_distance(r: int, ratio: float):
    """The first whole distance of two arcs' centres (radius r, as ``_pair_at`` builds them) at which the fitted
    circles' A / (pi Rs^2) falls below ``ratio`` -> (distance, ratio one unit before, ratio there)."""
    before = None
    for d in range(int(0.70 * r), int(0.95 * r)):
        left, right = _pair_at(r, d)
        one = jref.circle(left[:, 0], left[:, 1], left[0, 0], left[0, 1])
        two = jref.circle(right[:, 0], right[:, 1], right[0, 0], right[0, 1])
        Rs, _, _, A = jref.overlap(one, two)
        now = A / (jref.PI * (Rs * Rs))
        if now < ratio and before is not None and before >= ratio:
            return d, before, now
        before = now
    raise AssertionError("no threshold found")


def _pair_at(r: int, d: int):
    """Two arcs of radius r whose centres are d apart: the left one opens to the left, the right one to the right."""
    return _arc(0, 0, r, math.pi - 1.2, math.pi + 1.2, 0), _arc(d, 0, r, -1.2, 1.2, 0)


def events():
    """[(name, rows [n, 8], labels [n])]"""
    out = []

    def add(name, pieces, labels):
        points = _stack(*pieces)
        labels = np.concatenate([np.full(len(p), lab) if np.isscalar(lab) else np.asarray(lab) for p, lab in zip(pieces, labels)])
        out.append((name, *_event(points, labels)))

    out.append(("empty", *_event(np.zeros((0, 3)), np.zeros(0))))
    add("two arcs of one circle", [_arc(0, 0, 1600, 0.0, 0.8, 0), _arc(0, 0, 1600, 1.0, 1.8, 0)], [2, 2])
    add("two arcs of well separated circles", [_arc(-3000, 0, 800, 0.0, 1.5, 0), _arc(3000, 0, 800, 2.0, 3.5, 0)], [2, 0])
    add("circles that overlap a little", [_arc(0, 0, 800, 1.0, 2.5, 0), _arc(1500, 0, 800, 4.0, 5.5, 0)], [2, 0])
    add("small circle enclosed in a large one", [_arc(0, 0, 2400, 0.0, 1.0, 0), _arc(500, 0, 400, 0.0, 4.0, 0)], [2, 2])
    d, above, below = _threshold_distance(800, 0.5)
    JUST.update(distance=d, above=above, below=below)
    add("overlap just above the ratio", list(_pair_at(800, d - 1)), [2, 2])
    add("overlap just below the ratio", list(_pair_at(800, d)), [2, 2])
    add("chain of three", [_arc(0, 0, 800, 0.0, 2.0, 0), _arc(500, 0, 800, 2.0, 4.0, 0), _arc(1000, 0, 800, 4.0, 6.0, 0)], [2, 2, 2])
    add("collinear cluster", [_line(40, 16, y=300)[:, [2, 1, 0]], _arc(0, 0, 800, 0.0, 2.0, 0)], [0, 2])
    add("circle under min_radius", [_arc(100, 0, 100, 0.0, 5.5, 0), _arc(0, 0, 800, 0.0, 2.0, 0)], [2, 2])
    # the same points in the pad plane twice: equal sums, equal circles, A = pi Rs^2 exactly -- equality at overlap_ratio 1
    add("two pieces over one another", [_arc(0, 0, 800, 0.0, 2.0, 0), _arc(0, 0, 800, 0.0, 2.0, 0)], [2, 2])
    # the join flips the majority: the first piece votes 16 : 14 for position 0, the second 30 : 0 for position 1
    add("join flips the majority", [_arc(0, 0, 1600, 0.0, 0.4, 0, n=30), _arc(0, 0, 1600, 0.6, 1.0, 0, n=30)],
        [[2] * 16 + [0] * 14, 0])
    # the join changes the ranking: 25 + 25 rows about a lone cluster of 50; the tie at 50 rows goes to the lower id
    add("join changes the ranking", [_arc(0, 0, 1600, 0.0, 0.3, 0, n=25), _arc(-3000, -2000, 800, 0.0, 1.3, 0, n=50),
                                    _arc(0, 0, 1600, 0.5, 0.8, 0, n=25)], [2, 0, 2])
    lines = [_line(6, 16, x=-4800 + 300 * k, y=-4000) for k in range(31)]
    pair = [_arc(0, 0, 1600, 0.0, 0.5, 0), _arc(0, 0, 1600, 0.7, 1.2, 0)]
    flat = [np.concatenate(lines[:30])]  # (the short lines side by side at one z range: one piece of the stack)
    add("exactly max_clusters candidates", flat + pair, [3, 2, 2])
    add("one candidate more than max_clusters", [np.concatenate(lines)] + pair, [3, 2, 2])
    add("more rows than max_rows", [_line(801, 16, wiggle=5)], [2])
    add("700 rows, a member of 400", [_arc(0, 0, 2400, 0.0, 2.5, 0, n=300), _arc(0, 0, 2400, 2.7, 6.0, 0, n=400)], [2, 2])
    rows, labels = _event(_stack(_arc(0, 0, 1600, 0.0, 0.8, 0), _arc(0, 0, 1600, 1.0, 1.8, 0)), 2)
    rows[10, 0], rows[11, 1], rows[70, 0], rows[71, 4] = np.nan, np.inf, 320.0625, 2147483648.0
    rows[-4:, :3] = np.nan  # (as the drift correction leaves its skipped rows: behind the others)
    out.append(("out-of-range rows", rows, labels))
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
    """{run: (cluster labels, events, records, join events, join records)} of the restatement on ``csr()``, once."""
    offsets, rows, labels, _ = csr()
    return {run: jref.join(s, j, offsets, rows, labels, INDICES) for run, (s, j) in RUNS.items()}


@functools.lru_cache(maxsize=None)
def clustering_alone():
    """{"truth" / "rank": the restatement of the clustering alone on ``csr()``}"""
    offsets, rows, labels, _ = csr()
    return {s.match: cref.cluster(s, offsets, rows, labels, INDICES) for s in (CLUSTERING, RANK)}


def event_detail(run: str, name: str) -> dict:
    """The restatement's intermediate values of one event under one run (see ``join_reference.join_event``)."""
    offsets, rows, labels, names = csr()
    e = names.index(name)
    detail = {}
    s, j = RUNS[run]
    out = jref.join_event(s, j, rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]], list(INDICES), detail=detail)
    detail["out"], detail["event"], detail["records"], detail["join_event"], detail["join_records"] = out
    return detail


def check_cases() -> None:
    """Every event is what its name says, by the restatement's own intermediate values."""
    offsets, rows, labels, names = csr()
    assert offsets[-1] < 6000
    ref, alone = reference(), clustering_alone()["truth"]
    sizes = dict(zip(names, np.diff(offsets)))
    at = {name: e for e, name in enumerate(names)}
    jev = {g: dict(zip(names, ref[g][3])) for g in RUNS}
    ev = {g: dict(zip(names, ref[g][1])) for g in RUNS}
    rec = {g: dict(zip(names, ref[g][2])) for g in RUNS}
    jrec = {g: dict(zip(names, ref[g][4])) for g in RUNS}
    alone_ev, alone_rec = dict(zip(names, alone[1])), dict(zip(names, alone[2]))
    base = jev["defaults"]
    print("overlap just above / below the ratio:", JUST)
    # two arcs of one circle: two clusters of one truth label, one split, joined to one
    name = "two arcs of one circle"
    assert alone_ev[name]["n_clusters"] == 2 and alone_ev[name]["n_split"] == 1
    assert tuple(base[name].tolist()[:6]) == (2, 2, 2, 1, 1, 0) and ev["defaults"][name]["n_clusters"] == 1 and ev["defaults"][name]["n_split"] == 0
    assert rec["defaults"][name]["rows"][0] == sizes[name] and jrec["defaults"][name]["parts"][0] == 2
    assert abs(jrec["defaults"][name]["radius"][0] - 100.0) < 0.5 and jrec["defaults"][name]["first_row"][0] == rec["defaults"][name]["first_row"][0]
    for name in ("two arcs of well separated circles", "circles that overlap a little"):
        d = event_detail("quarter", name)
        Rs, Rl, dist, A = jref.overlap(d["circles"][0], d["circles"][1])
        assert d["part"] == [True, True] and not d["pairs"] and base[name]["n_joined"] == 0 and jev["quarter"][name]["n_joined"] == 0, name
        assert (dist >= Rs + Rl and A == 0.0) if "separated" in name else (Rl - Rs < dist < Rs + Rl and 0.0 < d["ratio"][(0, 1)] < 0.25), name
    name = "small circle enclosed in a large one"
    d = event_detail("defaults", name)
    Rs, Rl, dist, A = jref.overlap(d["circles"][0], d["circles"][1])
    assert dist <= Rl - Rs and A == jref.PI * (Rs * Rs) and Rl > 1.5 * Rs and base[name]["n_joined"] == 1 and jev["ratio"][name]["n_joined"] == 0
    assert jev["ratio"][name]["n_taking_part"] == 2
    # just above and below: one unit of one centre apart
    assert JUST["above"] >= 0.5 > JUST["below"] and JUST["above"] - JUST["below"] < 0.002
    above, below = event_detail("defaults", "overlap just above the ratio"), event_detail("defaults", "overlap just below the ratio")
    assert above["ratio"][(0, 1)] == JUST["above"] and below["ratio"][(0, 1)] == JUST["below"]
    assert above["join_event"]["n_joined"] == 1 and below["join_event"]["n_joined"] == 0 and below["join_event"]["n_taking_part"] == 2
    name = "chain of three"
    d = event_detail("defaults", name)
    assert d["pairs"] == [(0, 1), (1, 2)] and d["ratio"][(0, 2)] < 0.5 and list(d["root"]) == [0, 0, 0]
    assert tuple(base[name].tolist()[:5]) == (3, 3, 3, 2, 2) and jrec["defaults"][name]["parts"][0] == 3
    assert rec["defaults"][name]["first_row"][0] == alone_rec[name]["first_row"][:3].min() >= 0 and rec["defaults"][name]["rows"][0] == sizes[name]
    name = "collinear cluster"
    d = event_detail("defaults", name)
    assert d["circles"][0] is not None and d["circles"][1] is None or d["circles"][0] is None and d["circles"][1] is not None
    assert tuple(base[name].tolist()[:5]) == (2, 1, 1, 0, 0)
    no_circle = [k for k in range(2) if np.isnan(jrec["defaults"][name]["radius"][k])]
    assert len(no_circle) == 1 and jrec["defaults"][name]["parts"][no_circle[0]] == 1
    name = "circle under min_radius"
    d = event_detail("defaults", name)
    small = min(c[2] for c in d["circles"])
    assert small < 10.0 and tuple(base[name].tolist()[:5]) == (2, 2, 1, 0, 0) and (0, 1) not in d["ratio"]
    Rs, Rl, dist, A = jref.overlap(d["circles"][0], d["circles"][1])
    assert dist <= Rl - Rs  # (it would join: it is enclosed)
    name = "two pieces over one another"
    d = event_detail("full", name)
    Rs, Rl, dist, A = jref.overlap(d["circles"][0], d["circles"][1])
    assert d["circles"][0] == d["circles"][1] and dist == 0.0 and A == 1.0 * (jref.PI * (Rs * Rs)) and jev["full"][name]["n_joined"] == 1
    assert jev["full"]["small circle enclosed in a large one"]["n_joined"] == 1 and jev["full"]["chain of three"]["n_joined"] == 0
    name = "join flips the majority"
    assert list(alone_rec[name]["majority"][:2]) == [0, 1] and alone_ev[name]["n_split"] == 0  # (30 rows each: the lower id ranks first)
    r = rec["defaults"][name]
    assert r["majority"][0] == 1 and r["majority_rows"][0] == 44 and r["rows"][0] == 60 and r["label"][0] == INDICES[1]
    first = alone_rec[name][np.argmin(alone_rec[name]["first_row"][:2])]
    assert first["majority"] == 0 and r["first_row"][0] == first["first_row"]  # the id's own member votes for position 0
    name = "join changes the ranking"
    a = alone_rec[name]
    assert list(a["rows"][:3]) == [50, 25, 25] and a["first_row"][1] < a["first_row"][0] < a["first_row"][2]
    r = rec["defaults"][name]
    assert list(r["rows"][:2]) == [50, 50] and r["first_row"][0] == a["first_row"][1] and r["first_row"][1] == a["first_row"][0]
    assert list(jrec["defaults"][name]["parts"][:2]) == [2, 1]
    name = "exactly max_clusters candidates"
    assert tuple(base[name].tolist()[:6]) == (32, 2, 2, 1, 1, 0) and ev["defaults"][name]["n_clusters"] == 31
    name = "one candidate more than max_clusters"
    assert tuple(base[name].tolist()[:6]) == (33, 0, 0, 0, 0, jref.JOIN_CAPPED) and alone_ev[name]["n_clusters"] == 33
    lo, hi = offsets[at[name]], offsets[at[name] + 1]
    assert np.array_equal(ref["defaults"][0][lo:hi], alone[0][lo:hi]) and ref["defaults"][1][at[name]] == alone[1][at[name]]
    assert np.array_equal(ref["defaults"][2][at[name]], alone[2][at[name]]) and np.all(jrec["defaults"][name]["first_row"] == -1)
    name = "more rows than max_rows"
    assert sizes[name] == 801 and ev["defaults"][name]["status"] == cref.CAPPED and tuple(base[name].tolist()[:6]) == (0, 0, 0, 0, 0, jref.JOIN_NOT_CLUSTERED)
    assert sizes["empty"] == 0 and tuple(base["empty"].tolist()[:6]) == (0, 0, 0, 0, 0, jref.JOIN_NOT_CLUSTERED)
    name = "700 rows, a member of 400"
    assert sizes[name] == 700 and sorted(alone_rec[name]["rows"][:2]) == [300, 400] and rec["defaults"][name]["rows"][0] == 700
    name = "out-of-range rows"
    # (a row out of range breaks its arc in two: four pieces, all of one circle)
    assert ev["defaults"][name]["n_range"] == 8 and tuple(base[name].tolist()[:5]) == (4, 4, 4, 6, 3) and ev["defaults"][name]["n_clusters"] == 1
    assert alone_ev[name]["n_split"] == 3 and ev["defaults"][name]["n_split"] == 0 and rec["defaults"][name]["rows"][0] == 120
    lo = offsets[at[name]]
    assert ref["defaults"][0][lo + 10] == -1 and ref["defaults"][0][lo + 12] == 2
    # match="rank": the joined cluster takes position 0, whatever its truth
    r = rec["rank"]["join flips the majority"]
    assert r["label"][0] == INDICES[0] and r["majority"][0] == 1 and r["rows"][0] == 60 and ev["rank"]["join flips the majority"]["n_split"] == 0
    # max_clusters 2: three candidates are one too many
    assert jev["two"]["chain of three"]["status"] == jref.JOIN_CAPPED and jev["two"]["two arcs of one circle"]["n_joined"] == 1
    assert jev["quarter"]["chain of three"]["n_pairs"] == 3  # (at a quarter the ends overlap enough)
    assert jev["quarter"]["overlap just below the ratio"]["n_joined"] == 1
    for g in ("ratio", "quarter", "two", "rank", "full"):
        assert not jref.same(ref[g], ref["defaults"]), g
    assert not any(ev["defaults"][name]["status"] for name in names if name != "more rows than max_rows")
