"""The cluster joining (include/attpc_engine.h, "cluster joining") restated in numpy and plain Python floats on top of
tests/cluster_reference.py, which is imported and not edited: steps 1 to 6 are its ``cluster_event`` (through ``detail``),
steps 6a to 9 are here.  The sums are Python integers, the circle and the overlap f64 in the written order -- a Python
float operation is one IEEE rounding --, the arctangent restated as tests/helix_reference.py restates it.  Nothing of
the package is used.  The contract is Spyral's cluster joining in structure, with every tie made definite; Spyral
iterates and this does not, and nothing is compared against Spyral.

``JoinSettings`` is the descriptor; ``join(cluster_settings, join_settings, offsets, rows, labels, indices)`` gives the
cluster labels, the cluster events and records, and the join events and records.  ``mutant`` names one deliberate
departure from the contract (``MUTANTS``); tests/test_join_cpu.py shows that the exact comparison on the case set catches
every one."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import cluster_reference as cref

MUTANTS = ("strict_threshold", "no_transitivity", "enclosed_missing", "larger_radius_in_denominator", "highest_member_id",
           "votes_not_summed", "circle_on_core_rows", "min_radius_ignored")
MAX_SIM = cref.MAX_SIM
JOIN_CAPPED, JOIN_NOT_CLUSTERED = 1, 2
PI, HALF_PI, QUARTER_PI, CUT = 3.141592653589793, 1.5707963267948966, 0.7853981633974483, 0.41421356237309503
COEFFICIENTS = [(-1.0) ** k / (2 * k + 1) for k in range(20)]  # the f64 quotients
JOIN_EVENT_DTYPE = np.dtype([("n_candidates", "<i4"), ("n_circles", "<i4"), ("n_taking_part", "<i4"), ("n_pairs", "<i4"),
                             ("n_joined", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))])
JOIN_DTYPE = np.dtype([("parts", "<i4"), ("first_row", "<i4"), ("a", "<f8"), ("b", "<f8"), ("radius", "<f8")])
assert JOIN_EVENT_DTYPE.itemsize == 32 and JOIN_DTYPE.itemsize == 32


@dataclass
class JoinSettings:
    overlap_ratio: float = 0.5
    min_radius: float = 10.0
    radius_ratio: float = 0.0  # 0: no condition
    max_clusters: int = 32


def desc_error(j: JoinSettings) -> bool:
    """The settings are outside the contract's ranges."""
    return (not (0.0 < j.overlap_ratio <= 1.0) or not (1.0 / 16.0 <= j.min_radius <= 5000.0)
            or not (j.radius_ratio == 0.0 or (j.radius_ratio >= 1.0 and math.isfinite(j.radius_ratio)))
            or not 2 <= j.max_clusters <= 64)


def atan2w(y: float, x: float) -> float:
    """The written arctangent of two finite numbers."""
    ax, ay = abs(x), abs(y)
    steep = ay > ax
    hi, lo = (ay, ax) if steep else (ax, ay)
    t = lo / (1.0 if hi == 0.0 else hi)
    upper = t > CUT
    r = ((t - 1.0) if upper else t) / ((t + 1.0) if upper else 1.0)
    z = r * r
    p = COEFFICIENTS[19]
    for k in range(18, -1, -1):
        p = p * z + COEFFICIENTS[k]
    at = (QUARTER_PI if upper else 0.0) + r * p
    at = HALF_PI - at if steep else at
    at = PI - at if x < 0.0 else at
    return -at if y < 0.0 else at


def acos_w(c: float) -> float:
    q = 1.0 - c * c
    return atan2w(math.sqrt(q if q > 0.0 else 0.0), c)


def _div(x: float, y: float) -> float:
    """x / y as IEEE gives it (y is not 0 where this is called with a finite x)."""
    try:
        return x / y
    except ZeroDivisionError:
        return math.nan if x == 0.0 or x != x else math.copysign(math.inf, x) * math.copysign(1.0, y)


def circle(X, Y, x_id: int, y_id: int):
    """Step 6b on the integer coordinates of a candidate's rows -> (a, b, R) in mm, or None: no circle."""
    m = len(X)
    if m < 3:
        return None
    u = [int(x) - int(x_id) for x in X]
    v = [int(y) - int(y_id) for y in Y]
    su, sv = sum(u), sum(v)
    suu, svv, suv = sum(a * a for a in u), sum(b * b for b in v), sum(a * b for a, b in zip(u, v))
    suq = sum(a * (a * a + b * b) for a, b in zip(u, v))
    svq = sum(b * (a * a + b * b) for a, b in zip(u, v))
    assert max(abs(t) for t in (su, sv, suu, svv, suv, suq, svq)) < 2**57
    M, Su, Sv, Suu, Svv, Suv, Suq, Svq = (float(t) for t in (m, su, sv, suu, svv, suv, suq, svq))
    A = M * Suu - Su * Su
    B = M * Suv - Su * Sv
    C = M * Svv - Sv * Sv
    D = (M * (0.0 + Suq) - Su * (Suu + Svv)) / 2.0
    E = (M * (0.0 + Svq) - Sv * (Suu + Svv)) / 2.0
    den = A * C - B * B
    if den == 0.0:
        return None
    uc = _div(D * C - B * E, den)
    vc = _div(A * E - B * D, den)
    r2 = (Suu + Svv - 2.0 * uc * Su - 2.0 * vc * Sv) / M + uc * uc + vc * vc
    if not r2 > 0.0:
        return None
    a, b, R = (float(x_id) + uc) / 16.0, (float(y_id) + vc) / 16.0, math.sqrt(r2) / 16.0
    return (a, b, R) if all(math.isfinite(t) for t in (a, b, R)) else None


def overlap_area(Rs: float, Rl: float, d: float, mutant=None) -> float:
    """Step 6c: the area two circles of radii Rs <= Rl share."""
    if d >= Rs + Rl:
        return 0.0
    if d <= Rl - Rs:
        return 0.0 if mutant == "enclosed_missing" else PI * (Rs * Rs)
    cs = (d * d + Rs * Rs - Rl * Rl) / (2.0 * d * Rs)
    cl = (d * d + Rl * Rl - Rs * Rs) / (2.0 * d * Rl)
    k = (-d + Rs + Rl) * (d + Rs - Rl) * (d - Rs + Rl) * (d + Rs + Rl)
    return Rs * Rs * acos_w(cs) + Rl * Rl * acos_w(cl) - 0.5 * math.sqrt(k if k > 0.0 else 0.0)


def overlap(lower, higher, mutant=None):
    """(Rs, Rl, d, A) of two circles (a, b, R), ``lower`` the one of the lower id."""
    swap = higher[2] < lower[2]
    Rs, Rl = (higher[2], lower[2]) if swap else (lower[2], higher[2])
    da, db = higher[0] - lower[0], higher[1] - lower[1]
    d = math.sqrt(da * da + db * db)
    return Rs, Rl, d, overlap_area(Rs, Rl, d, mutant)


def joined(j: JoinSettings, lower, higher, mutant=None) -> bool:
    Rs, Rl, d, A = overlap(lower, higher, mutant)
    bound = j.overlap_ratio * (PI * ((Rl * Rl) if mutant == "larger_radius_in_denominator" else (Rs * Rs)))
    if mutant == "strict_threshold":
        return A > bound and (j.radius_ratio == 0.0 or Rl <= j.radius_ratio * Rs)
    return A >= bound and (j.radius_ratio == 0.0 or Rl <= j.radius_ratio * Rs)


def _unused_join_records():
    records = np.zeros(MAX_SIM, dtype=JOIN_DTYPE)
    records["first_row"] = -1
    return records


def join_event(s: cref.Settings, j: JoinSettings, rows, labels, indices, mutant=None, detail: dict | None = None):
    """Steps 1 to 9 of one event with the joining -> (cluster labels [n], its cluster event, its cluster records [8], its
    join event, its join records [8]).  ``detail``, if given, receives the intermediate values of a joined event:
    ``candidates`` (ids as in-range indices), ``circles`` (per candidate (a, b, R) or None), ``part``, ``pairs`` (slot
    pairs joined), ``ratio`` ({(i, j): A / (pi Rs^2)} of the pairs that take part), ``root`` (per candidate the slot of
    its component's id) and ``ranked`` (component slots by rank)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    n = len(rows)
    d = {}
    out, event, records = cref.cluster_event(s, rows, labels, indices, detail=d)
    jevent = np.zeros((), dtype=JOIN_EVENT_DTYPE)
    jrecords = _unused_join_records()
    if n == 0 or event["status"] != 0:
        jevent["status"] = JOIN_NOT_CLUSTERED
        return out, event, records, jevent, jrecords
    candidates = sorted(int(c) for c in d["ranked"])  # 6a: ascending id
    K = len(candidates)
    jevent["n_candidates"] = K
    if K > j.max_clusters:
        jevent["status"] = JOIN_CAPPED
        return out, event, records, jevent, jrecords
    ok, X, Y, Z = cref.quantise(rows)
    row_of, cluster, core = d["row_of"], d["cluster"], d["core"]
    X, Y, Z = X[row_of], Y[row_of], Z[row_of]
    pos = cref.positions_of(labels, indices)[row_of] if labels is not None else np.full(len(row_of), -1, dtype=np.int64)
    members = [cluster == c for c in candidates]
    circles = []
    for c, member in zip(candidates, members):  # 6b
        fit_on = member & core if mutant == "circle_on_core_rows" else member
        circles.append(circle(X[fit_on], Y[fit_on], X[c], Y[c]))
    part = [c is not None and (mutant == "min_radius_ignored" or not c[2] < j.min_radius) for c in circles]
    jevent["n_circles"] = sum(c is not None for c in circles)
    jevent["n_taking_part"] = sum(part)
    adjacent = np.zeros((K, K), dtype=bool)
    ratio = {}
    for a in range(K):  # 6c
        for b in range(a + 1, K):
            if part[a] and part[b]:
                Rs, _, _, A = overlap(circles[a], circles[b])
                ratio[(a, b)] = A / (PI * (Rs * Rs))
                adjacent[a, b] = adjacent[b, a] = joined(j, circles[a], circles[b], mutant)
    jevent["n_pairs"] = int(adjacent.sum()) // 2
    if mutant == "no_transitivity":  # a candidate goes to its lowest direct partner only
        root = np.array([min([a] + list(np.flatnonzero(adjacent[a]))) for a in range(K)], dtype=np.int64)
        root = np.array([r if root[r] == r else a for a, r in enumerate(root)], dtype=np.int64)
    else:
        root = cref.components(adjacent | np.eye(K, dtype=bool)) if K else np.zeros(0, dtype=np.int64)  # 6d
    roots = [a for a in range(K) if root[a] == a]
    jevent["n_joined"] = K - len(roots)
    merged = {}
    for a in roots:
        slots = [b for b in range(K) if root[b] == a]
        member = np.zeros(len(cluster), dtype=bool)
        for b in slots:
            member |= members[b]
        vote_of = members[a] if mutant == "votes_not_summed" else member
        votes = np.bincount(pos[vote_of & (pos >= 0)], minlength=MAX_SIM)
        with_circle = [circles[b] for b in slots if circles[b] is not None]
        merged[a] = dict(id=candidates[max(slots) if mutant == "highest_member_id" else a], member=member, votes=votes,
                         parts=len(slots), circle=with_circle[0] if with_circle else None, rows=int(member.sum()))
    ranked = sorted(roots, key=lambda a: (-merged[a]["rows"], merged[a]["id"]))  # 7
    if detail is not None:
        detail.update(candidates=candidates, circles=circles, part=part, pairs=[tuple(p) for p in np.argwhere(np.triu(adjacent))],
                      ratio=ratio, root=root, ranked=ranked, cluster_detail=d, merged=merged)
    out = np.full(n, -1, dtype=np.int64)
    event = event.copy()
    event["n_clusters"], event["n_split"], event["n_fake"] = len(roots), 0, 0
    records = np.zeros(MAX_SIM, dtype=cref.RECORD_DTYPE)
    records["first_row"] = -1
    taken = set()
    for rank, a in enumerate(ranked):  # 8 and 9
        c = merged[a]
        votes, member = c["votes"], c["member"]
        majority = int(np.argmax(votes)) if votes.max() > 0 else -1
        if s.match == "rank":
            label = indices[rank] if rank < min(len(indices), MAX_SIM) else -1
        elif majority >= 0 and majority not in taken:
            taken.add(majority)
            label = indices[majority]
        else:
            label = -1
            event["n_split" if majority >= 0 else "n_fake"] += 1
        out[row_of[member]] = label
        if rank < MAX_SIM:
            records[rank] = (c["rows"], int((member & core).sum()), int(row_of[c["id"]]), majority,
                             int(votes[majority]) if majority >= 0 else 0, label, int(Z[member].min()), int(Z[member].max()))
            fit = c["circle"] or (math.nan, math.nan, math.nan)
            jrecords[rank] = (c["parts"], int(row_of[c["id"]]), *fit)
    return out, event, records, jevent, jrecords


def join(s: cref.Settings, j: JoinSettings, offsets, rows, labels, indices, mutant: str | None = None):
    """-> (cluster labels [R], events [n], records [n, 8], join events [n], join records [n, 8])."""
    assert mutant is None or mutant in MUTANTS, mutant
    assert not cref.desc_error(s) and not desc_error(j), (s, j)
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    n = len(offsets) - 1
    out = np.full(len(rows), -1, dtype=np.int64)
    events, records = np.zeros(n, dtype=cref.EVENT_DTYPE), np.zeros((n, MAX_SIM), dtype=cref.RECORD_DTYPE)
    jevents, jrecords = np.zeros(n, dtype=JOIN_EVENT_DTYPE), np.zeros((n, MAX_SIM), dtype=JOIN_DTYPE)
    for e in range(n):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        out[lo:hi], events[e], records[e], jevents[e], jrecords[e] = join_event(
            s, j, rows[lo:hi], None if labels is None else np.asarray(labels)[lo:hi], list(indices), mutant)
    return out, events, records, jevents, jrecords


def same(got, want) -> bool:
    """Labels and the four kinds of records equal; the f64 fields byte for byte, NaN slots included."""
    if not np.array_equal(np.asarray(got[0], dtype=np.int64), np.asarray(want[0], dtype=np.int64)):
        return False
    for g, w in zip(got[1:], want[1:]):
        g, w = np.asarray(g), np.asarray(w)
        for name in w.dtype.names:
            if np.ascontiguousarray(g[name]).astype(w[name].dtype).tobytes() != np.ascontiguousarray(w[name]).tobytes():
                return False
    return True
