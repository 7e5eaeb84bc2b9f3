"""Synthetic estimate records at the shapes where the particle identification (include/attpc_engine.h, "particle
identification") can go wrong.  Only ``brho`` and ``dedx`` of a record matter to the stage; every other field is
filled from a seeded generator.  Every coordinate of a gate and of a hand-made point is a small multiple of 1/4, so a
point "exactly on an edge" is exactly there in f64 (d == 0).

``GATES`` are the polygons; ``cases()`` the case set, name -> ``Case`` (n_sim, the eight gates, the mode, the estimate
records [n, n_sim], and for the hand-made events the name of each); ``reference()`` the restatement of every case,
computed once; ``check_cases()`` asserts on the restatement alone that the set holds what it names, so a case cannot go
empty silently.  Shapes: n_sim 1, 3 and 8; 0 events, 1 event, and 5 000 events -- the launch is capped at 2 048
workgroups of one event each, so 5 000 events are more than two passes of the grid stride with a ragged last one."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from attpc_engine_amd._abi import ESTIMATE_DTYPE
from tests import pid_reference as pref

NAN, INF = float("nan"), float("inf")
MANY = 5000


def _band():
    """32 vertices: a U-shaped (concave) band, the lower side left to right, the upper side back."""
    i = np.arange(16)
    lower = 1.0 + (i - 8.0) ** 2 / 16.0
    x = 1.0 + 0.5 * i
    return np.concatenate([np.stack([x, lower], axis=1), np.stack([x[::-1], lower[::-1] + 1.5], axis=1)])


GATES = {
    "triangle": np.array([(1.0, 1.0), (5.0, 2.0), (2.0, 6.0)]),
    "band": _band(),
    "hbox": np.array([(1.0, 1.0), (4.0, 1.0), (4.0, 3.0), (1.0, 3.0)]),           # horizontal edges at y = 1 and y = 3
    "wide": np.array([(-1.0, -1.0), (4.0, -1.0), (4.0, 4.0), (-1.0, 4.0)]),       # holds the origin: 0 and negative points
    "far": np.array([(2.0, 2.0), (6.0, 2.0), (6.0, 6.0), (2.0, 6.0)]),            # overlaps "wide" in (2 .. 4)^2
    "alpha": np.array([(0.5, 3.0), (2.0, 2.5), (3.0, 4.0), (2.5, 6.5), (1.0, 5.5)]),
    "carbon": np.array([(3.0, 0.5), (6.5, 0.25), (7.0, 2.0), (4.0, 2.25)]),
}
assert len(GATES["band"]) == 32

# hand-made points of the one-gate cases: name -> (brho, dedx); "edge:" marks a point exactly on an edge or a vertex
POINTS = {
    "triangle": {
        "inside": (3.0, 3.0), "outside": (6.0, 6.0), "inside level with a vertex": (3.0, 2.0),
        "edge: vertex 0": (1.0, 1.0), "edge: vertex 1": (5.0, 2.0), "edge: vertex 2": (2.0, 6.0),
        "edge: lower side": (3.0, 1.5), "edge: left side": (1.5, 3.5),
        "level with a vertex, right": (6.0, 2.0), "level with a vertex, left": (0.5, 2.0), "level with the lowest vertex": (0.25, 1.0),
        "level with the highest vertex, left": (0.25, 6.0), "level with the highest vertex, right": (7.0, 6.0),
        "nan brho": (NAN, 3.0), "nan dedx": (3.0, NAN), "inf brho": (INF, 3.0), "inf dedx": (3.0, INF), "-inf brho": (-INF, 3.0),
        "zero brho": (0.0, 3.0), "zero dedx": (3.0, 0.0), "negative brho": (-3.0, 3.0), "negative dedx": (3.0, -3.0),
    },
    "hbox": {
        "inside": (2.0, 2.0), "outside left": (0.5, 2.0), "outside right": (5.0, 2.0),
        "edge: left side": (1.0, 2.0), "edge: right side": (4.0, 2.0), "edge: bottom, horizontal": (2.0, 1.0),
        "edge: top, horizontal": (2.0, 3.0), "edge: vertex 0": (1.0, 1.0), "edge: vertex 1": (4.0, 1.0), "edge: vertex 2": (4.0, 3.0),
        "edge: vertex 3": (1.0, 3.0), "level with the bottom, right": (5.0, 1.0), "level with the bottom, left": (0.5, 1.0),
        "level with the top, right": (5.0, 3.0), "level with the top, left": (0.5, 3.0),
    },
    "band": {
        "inside at the bottom": (5.0, 1.5), "inside the left arm": (1.25, 5.5), "between the arms": (5.0, 4.0), "below": (5.0, 0.5),
        "edge: vertex 0": (1.0, 5.0), "edge: lowest vertex": (5.0, 1.0), "level with vertex 0, left": (0.5, 5.0),
        "level with the lowest vertex, left": (0.5, 1.0), "right of everything": (9.0, 3.0),
    },
    "wide": {  # a gate that holds the origin: what is not tested must not be accepted
        "inside": (1.0, 1.0), "zero brho": (0.0, 2.0), "zero dedx": (2.0, 0.0), "both zero": (0.0, 0.0),
        "negative brho": (-0.5, 2.0), "negative dedx": (2.0, -0.5), "-0.0": (-0.0, 2.0),
    },
}

# hand-made events of the assignment cases: name -> the (brho, dedx) of every slot
OVERLAP_EVENTS = {  # gates: position 0 "wide", position 1 "far", position 2 none
    "both, wide only, far only": [(3.0, 3.0), (1.0, 1.0), (5.0, 5.0)],     # AMBIGUOUS -> 0; TAKEN by slot 0; slot 2 -> 1
    "far only first": [(5.0, 5.0), (3.0, 3.0), (3.0, 3.5)],                 # 1; AMBIGUOUS -> 0; AMBIGUOUS and TAKEN
    "nothing holds": [(7.0, 7.0), (7.0, 0.5), (NAN, NAN)],
    "second slot only": [(NAN, 1.0), (1.0, 1.0), (0.0, 0.0)],
}
ALPHA_EVENTS = {  # gates: position 0 "carbon", positions 1 and 2 "alpha" (the two alphas of o16aa), position 3 none
    "carbon first": [(5.0, 1.0), (2.0, 4.0), (1.5, 4.5), (NAN, NAN)],
    "alphas first": [(2.0, 4.0), (1.5, 4.5), (5.0, 1.0), (NAN, NAN)],     # slots 0, 1 -> 1, 2; slot 2 -> 0
    "three alphas": [(2.0, 4.0), (1.5, 4.5), (2.0, 5.0), (5.0, 1.0)],     # the third: TAKEN and AMBIGUOUS; slot 3 -> 0
    "one alpha": [(NAN, NAN), (NAN, NAN), (2.0, 4.0), (NAN, NAN)],        # slot 2 -> 1
}


class Case(NamedTuple):
    n_sim: int
    gates: tuple       # [8] of None or vertices [n, 2]
    mode: int
    estimates: np.ndarray  # [n, n_sim] ESTIMATE_DTYPE
    names: tuple       # the hand-made events' names (empty for generated ones)


def _gates(*names):
    return tuple(None if n is None else GATES[n] for n in names) + (None,) * (8 - len(names))


def _records(points, rng) -> np.ndarray:
    """Estimate records [n, n_sim] with (brho, dedx) = points [n, n_sim, 2], every other field from ``rng``."""
    points = np.asarray(points, dtype=np.float64)
    out = np.zeros(points.shape[:2], dtype=ESTIMATE_DTYPE)
    for name in ESTIMATE_DTYPE.names:
        kind = ESTIMATE_DTYPE[name].kind
        out[name] = rng.integers(0, 1000, size=out.shape) if kind == "i" else rng.normal(size=out.shape)
    out["brho"], out["dedx"] = points[..., 0], points[..., 1]
    return out


def _generated(n, n_sim, rng):
    """Points on the grid of quarters in -1 .. 8 (many land exactly on an edge or a vertex), a share of them NaN,
    infinite, zero or negative."""
    points = rng.integers(-4, 33, size=(n, n_sim, 2)) / 4.0
    kind = rng.integers(0, 40, size=(n, n_sim))
    points[kind == 0] = NAN
    points[kind == 1, 0] = INF
    points[kind == 2, 1] = 0.0
    return points


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    rng = np.random.default_rng(20261021)
    out = {}
    for gate, points in POINTS.items():  # n_sim 1, one gate
        out[gate] = Case(1, _gates(gate), pref.ANY, _records(np.array(list(points.values()))[:, None, :], rng), tuple(points))
    overlap = np.array(list(OVERLAP_EVENTS.values()))
    out["overlap"] = Case(3, _gates("wide", "far", None), pref.ANY, _records(overlap, rng), tuple(OVERLAP_EVENTS))
    out["overlap, own"] = Case(3, _gates("wide", "far", None), pref.OWN, _records(overlap, rng), tuple(OVERLAP_EVENTS))
    alphas = np.array(list(ALPHA_EVENTS.values()))
    out["alphas"] = Case(4, _gates("carbon", "alpha", "alpha", None), pref.ANY, _records(alphas, rng), tuple(ALPHA_EVENTS))
    out["no events"] = Case(3, _gates("wide", "far", None), pref.ANY, _records(np.zeros((0, 3, 2)), rng), ())
    out["one event"] = Case(3, _gates("wide", "far", None), pref.ANY, _records(overlap[:1], rng), ())
    out["no gate at all"] = Case(3, _gates(None, None, None), pref.ANY, _records(overlap, rng), ())
    eight = _gates("triangle", "band", "hbox", "wide", "far", None, "alpha", "alpha")
    out["many, n_sim 1"] = Case(1, _gates("band"), pref.ANY, _records(_generated(MANY, 1, rng), rng), ())
    out["many, n_sim 3"] = Case(3, _gates("triangle", "far", "wide"), pref.ANY, _records(_generated(MANY, 3, rng), rng), ())
    out["many, n_sim 8"] = Case(8, eight, pref.ANY, _records(_generated(MANY, 8, rng), rng), ())
    out["many, n_sim 8, own"] = Case(8, eight, pref.OWN, _records(_generated(MANY, 8, rng), rng), ())
    for case in out.values():
        case.estimates.setflags(write=False)
    return out


def species_of(case: Case):
    """A species table for the case's positions (what the stand-alone host program is given): 10 + p, none at 1."""
    return [-1 if p == 1 else 10 + p for p in range(case.n_sim)]


@functools.lru_cache(maxsize=None)
def reference() -> dict:
    out = {name: pref.records(case.estimates, case.gates, case.mode) for name, case in cases().items()}
    for records in out.values():
        records.setflags(write=False)
    return out


def check_cases() -> None:
    """From the restatement alone: the case set holds what it names."""
    ref, all_cases = reference(), cases()
    status = np.concatenate([r["status"].ravel() for r in ref.values()])
    for bit in (pref.NO_ESTIMATE, pref.NONE, pref.TAKEN, pref.AMBIGUOUS):
        assert (status & bit).any(), bit
    held = np.concatenate([r["held"].ravel() for r in ref.values()])
    assert ((held & (held - 1)) != 0).any()  # two or more gates hold a point
    elsewhere = 0
    for name, records in ref.items():
        own = np.arange(records.shape[1])[None, :]
        elsewhere += int(((records["position"] >= 0) & (records["position"] != own)).sum())
    assert elsewhere > 0
    # a TAKEN that an earlier slot's claim caused: the hand-made event says which
    overlap = ref["overlap"][all_cases["overlap"].names.index("both, wide only, far only")]
    assert overlap["position"].tolist() == [0, -1, 1] and overlap["held"].tolist() == [3, 1, 2]
    assert overlap["status"].tolist() == [pref.AMBIGUOUS, pref.TAKEN, 0]
    own = ref["overlap, own"][all_cases["overlap, own"].names.index("both, wide only, far only")]
    assert own["position"].tolist() == [0, -1, -1] and own["status"].tolist() == [0, pref.NONE, pref.NONE]
    alphas = dict(zip(all_cases["alphas"].names, ref["alphas"]))
    assert alphas["alphas first"]["position"].tolist() == [1, 2, 0, -1]
    assert alphas["three alphas"]["position"].tolist() == [1, 2, -1, 0]
    assert alphas["three alphas"]["status"][2] == pref.TAKEN | pref.AMBIGUOUS and alphas["one alpha"]["position"][2] == 1
    assert np.all(ref["no gate at all"]["position"] == -1) and not (ref["no gate at all"]["status"] & ~(pref.NONE | pref.NO_ESTIMATE)).any()
    # the points on an edge or a vertex: both answers occur, and the table below pins which
    answers = {}
    for gate in POINTS:
        for name, record in zip(all_cases[gate].names, ref[gate]):
            answers[gate, name] = bool(record["held"][0])
    on_edge = {key: value for key, value in answers.items() if key[1].startswith("edge:")}
    assert any(on_edge.values()) and not all(on_edge.values())
    assert on_edge == ON_EDGE, on_edge
    for (gate, name), value in answers.items():
        if name.startswith(("inside",)):
            assert value, (gate, name)
        if name.startswith(("outside", "level", "nan", "inf", "-inf", "zero", "negative", "both zero", "-0.0", "between", "below", "right of")):
            assert not value, (gate, name)
    assert len(ref["no events"]) == 0 and len(ref["one event"]) == 1 and all(len(ref[name]) == MANY for name in ref if name.startswith("many"))
    assert {c.n_sim for c in all_cases.values()} >= {1, 3, 8}
    for name in ("many, n_sim 1", "many, n_sim 3", "many, n_sim 8", "many, n_sim 8, own"):
        assert (ref[name]["position"] >= 0).sum() > MANY // 20, name


# The answers the edge rule gives on an edge or a vertex, each worked by hand from the rule: an edge the point lies on
# has d == 0 and does not count, and an edge one of whose ends is level with the point straddles it iff the other end
# is above.  So what decides is whether an edge to the right of the point remains: the left side and the bottom of the
# box belong to it, its right side and top do not; the lower-right side of the triangle and its vertices have no edge
# left to count; the left arm of the band has its right arm beside it (three edges count), its lowest vertex nothing.
ON_EDGE = {
    ("triangle", "edge: vertex 0"): False, ("triangle", "edge: vertex 1"): False, ("triangle", "edge: vertex 2"): False,
    ("triangle", "edge: lower side"): False, ("triangle", "edge: left side"): True,
    ("hbox", "edge: left side"): True, ("hbox", "edge: right side"): False, ("hbox", "edge: bottom, horizontal"): True,
    ("hbox", "edge: top, horizontal"): False, ("hbox", "edge: vertex 0"): True, ("hbox", "edge: vertex 1"): False,
    ("hbox", "edge: vertex 2"): False, ("hbox", "edge: vertex 3"): False,
    ("band", "edge: vertex 0"): True, ("band", "edge: lowest vertex"): False,
}
