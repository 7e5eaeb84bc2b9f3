"""Clustering: an event's trace rows split into tracks without the truth labels, on the device
(``attpc_trace_configure_clustering``; the contract is in include/attpc_engine.h, "clustering",
``tests/cluster_reference.py`` restates it in numpy by brute force).  The algorithm is DBSCAN with every tie made
definite, in integers -- not Spyral's HDBSCAN, cluster joining and outlier-factor cleanup, and not compared against
Spyral, which is not at hand.  The stage is opt-in (``ClusterSettings``, ``clustering=``) and sits behind the drift
correction and in front of the thinning, the estimates, the circle fit, the helix slope and the track fit, which then
match the cluster labels in place of the truth labels.  The delivered ``labels`` stay the truth labels;
``run_trace_rows`` and ``run_estimates`` carry ``"clusters"`` (the event and the cluster records) and, where the rows
are fetched, ``"cluster_labels"``.  ``rows_to_clusters`` is the stage alone on any host rows; ``cluster_scores`` turns the
records into completeness and purity.  The writers do not store the records."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .._abi import CLUSTER_CAPPED, CLUSTER_DTYPE, CLUSTER_EVENT_DTYPE, CLUSTER_INTERNAL  # noqa: F401
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout

STATUS_BITS = {"CAPPED": CLUSTER_CAPPED, "INTERNAL": CLUSTER_INTERNAL}
MATCH = {"truth": _abi.CLUSTER_MATCH_TRUTH, "rank": _abi.CLUSTER_MATCH_RANK}
EPS_MIN, EPS_MAX = 1.0 / 16.0, 64.0  # mm


def _length(name: str, value) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"clustering {name} must be a number, got {value!r}")
    number = float(value)
    if not (math.isfinite(number) and EPS_MIN <= number <= EPS_MAX):
        raise ValueError(f"clustering {name} must be in 1/16 .. 64 mm, got {value!r}")
    return number


def _integer(name: str, value, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"clustering {name} must be an integer in {lo} .. {hi}, got {value!r}")
    return int(value)


class ClusterSettings:
    """The validated settings of the clustering (``attpc_cluster_desc``, include/attpc_engine.h): ``eps_xy`` and
    ``eps_z``, the linking lengths in mm (1/16 .. 64); ``min_samples``, the neighbours a core row needs, itself
    included; ``min_cluster_size``, the rows a cluster needs to survive; ``max_rows`` (1 .. 65535), the rows of an event
    above which it is not clustered; ``match``: "truth" -- a cluster gets the label of the position most of its rows
    carry by truth, the best-ranked cluster of every position wins, which stands in for a particle-identification gate
    and makes the estimates comparable slot by slot with a truth-labelled run -- or "rank" -- the label-free mode: the
    k-th largest cluster gets the k-th position's label.  The defaults of the four physical settings are a starting
    point, not a measurement (profiles/r31_clustering.md)."""

    slot, call = "clustering", "attpc_trace_configure_clustering"

    def __init__(self, eps_xy: float = 20.0, eps_z: float = 20.0, min_samples: int = 5, min_cluster_size: int = 10,
                 max_rows: int = _abi.CLUSTER_DEFAULT_MAX_ROWS, match: str = "truth"):
        self.eps_xy, self.eps_z = _length("eps_xy", eps_xy), _length("eps_z", eps_z)
        self.min_samples = _integer("min_samples", min_samples, 1, 2**31 - 1)
        self.min_cluster_size = _integer("min_cluster_size", min_cluster_size, 1, 2**31 - 1)
        self.max_rows = _integer("max_rows", max_rows, 1, _abi.CLUSTER_MAX_ROWS_LIMIT)
        if match not in MATCH:
            raise ValueError(f"clustering match must be one of {sorted(MATCH)}, got {match!r}")
        self.match = match

    def token(self):
        return (self.eps_xy, self.eps_z, self.min_samples, self.min_cluster_size, self.max_rows, self.match)

    def desc(self) -> _abi.ClusterDesc:
        return _abi.ClusterDesc(self.eps_xy, self.eps_z, self.min_samples, self.min_cluster_size, self.max_rows,
                                MATCH[self.match])


def configure_clustering(ctx: _abi.Context, clustering: ClusterSettings | None) -> None:
    """``attpc_trace_configure_clustering`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, ClusterSettings, checked(ClusterSettings, clustering, "clustering"))


def clusters_last(ctx: _abi.Context, n_events: int):
    """(events [n_events] ``CLUSTER_EVENT_DTYPE``, records [n_events, 8] ``CLUSTER_DTYPE``) of ctx's last trace-row call
    (``attpc_clusters_last``); RuntimeError if the stage was off for it."""
    events = np.empty(int(n_events), dtype=CLUSTER_EVENT_DTYPE)
    records = np.empty((int(n_events), _abi.MAX_SIM), dtype=CLUSTER_DTYPE)
    ctx.check(ctx.lib.attpc_clusters_last(ctx.handle, 0, len(events), _abi.iptr(events, _abi.ClusterEvent),
                                          _abi.iptr(records, _abi.ClusterRecord)), "attpc_clusters_last")
    return events, records


def cluster_labels_last(ctx: _abi.Context, n_rows: int) -> np.ndarray:
    """The cluster labels [n_rows] of the rows ctx's last trace-row call delivered (``attpc_cluster_labels_last``);
    RuntimeError if the stage was off for it or the rows were not fetched."""
    labels = np.empty(int(n_rows), dtype=np.int64)
    ctx.check(ctx.lib.attpc_cluster_labels_last(ctx.handle, 0, len(labels), _abi.iptr(labels, _abi.C.c_int64)),
              "attpc_cluster_labels_last")
    return labels


def clustering_result(ctx: _abi.Context, n_events: int, n_sim: int = 0, n_rows: int | None = None) -> dict:
    """``{"clusters": (events, records)}`` of ctx's last trace-row call if the ctx holds the stage, else {}; with
    ``n_rows`` (the rows the call fetched) also ``"cluster_labels"`` [n_rows]."""
    if ctx._tokens["clustering"] is None:
        return {}
    out = {"clusters": clusters_last(ctx, n_events)}
    if n_rows is not None:
        out["cluster_labels"] = cluster_labels_last(ctx, n_rows)
    return out


def rows_to_clusters(offsets, rows, labels, indices, settings: ClusterSettings, ctx: _abi.Context | None = None):
    """The stage alone on any host rows in CSR form (``attpc_rows_cluster``; the kernel of the fused path, no other
    configuration needed): offsets [n+1], rows [R,8] as ``run_trace_rows`` delivers them (per event the in-range rows in
    nondecreasing z: ValueError otherwise, from the library), labels [R] the truth labels or None (then nobody votes),
    ``indices`` (the nucleus of every track position, or an ``_abi.EventLayout``) -> (cluster_labels [R], events [n]
    ``CLUSTER_EVENT_DTYPE``, records [n, 8] ``CLUSTER_DTYPE``).  Rows outside offsets[0] .. offsets[n] get -1."""
    if not isinstance(settings, ClusterSettings):
        raise TypeError("rows_to_clusters needs a ClusterSettings")
    layout = _layout(indices)
    offsets, rows, labels, n = host_rows(offsets, rows, labels, optional_labels=True)
    out = np.full(len(rows), -1, dtype=np.int64)
    events = np.zeros(n, dtype=CLUSTER_EVENT_DTYPE)
    records = np.zeros((n, _abi.MAX_SIM), dtype=CLUSTER_DTYPE)
    i64 = _abi.C.c_int64
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_rows_cluster(ctx.handle, n, _abi.iptr(offsets, i64), _abi.dptr(rows),
                                         None if labels is None else _abi.iptr(labels, i64), layout, settings.desc(),
                                         _abi.iptr(out, i64), _abi.iptr(events, _abi.ClusterEvent),
                                         _abi.iptr(records, _abi.ClusterRecord)), "attpc_rows_cluster")
    return out, events, records


def cluster_scores(events, records):
    """Per (event, position) of the records of a "truth"-matched run -> (completeness, purity) [n, 8], NaN where the
    position has no cluster: completeness = the matched cluster's ``majority_rows`` / the position's ``truth_rows``,
    purity = ``majority_rows`` / ``rows`` of that cluster.  The slot's cluster is the one whose ``majority`` is the
    position and whose ``label`` is not -1: the best-ranked of that majority, if it is among the eight recorded.

    Records of a ``match="rank"`` run are not scored: there a label goes by rank, not by majority, so a slot's cluster
    is not the one of its majority and the result would sit in the wrong slots.  The records do not carry the mode;
    what only rank matching produces -- a labelled cluster without a majority, or two labelled clusters of one event
    with one majority -- raises ValueError, and for every other rank-matched input the result is undefined."""
    events, records = np.asarray(events), np.asarray(records)
    n = len(events)
    completeness = np.full((n, _abi.MAX_SIM), np.nan)
    purity = np.full((n, _abi.MAX_SIM), np.nan)
    labelled = (records["first_row"] >= 0) & (records["label"] >= 0)
    used = labelled & (records["majority"] >= 0)
    per_position = (used[:, :, None] & (records["majority"][:, :, None] == np.arange(_abi.MAX_SIM))).sum(axis=1)
    if np.any(labelled & ~used) or np.any(per_position > 1):
        raise ValueError('cluster_scores needs the records of a match="truth" run: these were matched by rank')
    for rank in range(records.shape[1] - 1, -1, -1):  # (a position has one labelled cluster; the order does not matter)
        rec = records[:, rank]
        ev = np.nonzero(used[:, rank])[0]
        pos = rec["majority"][ev]
        truth = events["truth_rows"][ev, pos].astype(np.float64)
        completeness[ev, pos] = rec["majority_rows"][ev] / truth
        purity[ev, pos] = rec["majority_rows"][ev] / rec["rows"][ev].astype(np.float64)
    return completeness, purity
