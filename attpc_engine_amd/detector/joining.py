"""Cluster joining: the pieces of a track that the clustering broke apart become one cluster again, on the device
(``attpc_trace_configure_cluster_join``; the contract is in include/attpc_engine.h, "cluster joining",
``tests/join_reference.py`` restates it).  Clusters whose circles in the pad plane overlap by ``overlap_ratio`` of the
smaller one are joined, transitively, in one round; the stage sits between the clustering's size cut and its ranking, so
the cluster labels that thinning, estimates, circle fit, helix slope and track fit read are the joined ones.  The
contract is Spyral's cluster joining in structure, with every tie made definite -- not Spyral's code: Spyral iterates
the joining with refitted circles and this stage does not, and nothing is compared against Spyral, which is not at
hand.  The stage is opt-in (``JoinSettings``, ``join=``) and does nothing unless the clustering is on.
``run_trace_rows`` and ``run_estimates`` carry ``"joins"`` (the join events and records) when both are on;
``rows_to_joined_clusters`` is the two stages alone on any host rows; ``cluster_scores`` works unchanged on joined
records.  The writers do not store the records."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .._abi import JOIN_CAPPED, JOIN_DTYPE, JOIN_EVENT_DTYPE, JOIN_NOT_CLUSTERED  # noqa: F401
from .clustering import ClusterSettings
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout

STATUS_BITS = {"CAPPED": JOIN_CAPPED, "NOT_CLUSTERED": JOIN_NOT_CLUSTERED}
RADIUS_MIN, RADIUS_MAX = 1.0 / 16.0, 5000.0  # mm


def _number(name: str, value) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"cluster joining {name} must be a number, got {value!r}")
    return float(value)


class JoinSettings:
    """The validated settings of the cluster joining (``attpc_join_desc``, include/attpc_engine.h): ``overlap_ratio`` in
    (0, 1], the share of the smaller circle's area that two clusters' circles must have in common; ``min_radius`` in mm
    (1/16 .. 5000), the radius below which a cluster's circle takes no part; ``radius_ratio``, None (no condition) or a
    number >= 1, the most the larger radius may be of the smaller; ``max_clusters`` (2 .. 64), the clusters of an event
    above which it is not joined.  The defaults are a starting point, not a tuning (profiles/r32_cluster_join.md)."""

    slot, call = "cluster_join", "attpc_trace_configure_cluster_join"

    def __init__(self, overlap_ratio: float = 0.5, min_radius: float = 10.0, radius_ratio: float | None = None,
                 max_clusters: int = 32):
        self.overlap_ratio = _number("overlap_ratio", overlap_ratio)
        if not 0.0 < self.overlap_ratio <= 1.0:  # (a NaN fails)
            raise ValueError(f"cluster joining overlap_ratio must be in (0, 1], got {overlap_ratio!r}")
        self.min_radius = _number("min_radius", min_radius)
        if not RADIUS_MIN <= self.min_radius <= RADIUS_MAX:
            raise ValueError(f"cluster joining min_radius must be in 1/16 .. 5000 mm, got {min_radius!r}")
        self.radius_ratio = None if radius_ratio is None else _number("radius_ratio", radius_ratio)
        if self.radius_ratio is not None and not (math.isfinite(self.radius_ratio) and self.radius_ratio >= 1.0):
            raise ValueError(f"cluster joining radius_ratio must be None or a finite number >= 1, got {radius_ratio!r}")
        if (isinstance(max_clusters, (bool, np.bool_)) or not isinstance(max_clusters, (int, np.integer))
                or not 2 <= max_clusters <= _abi.JOIN_MAX_CLUSTERS):
            raise ValueError(f"cluster joining max_clusters must be an integer in 2 .. {_abi.JOIN_MAX_CLUSTERS}, got {max_clusters!r}")
        self.max_clusters = int(max_clusters)

    def token(self):
        return (self.overlap_ratio, self.min_radius, self.radius_ratio, self.max_clusters)

    def desc(self) -> _abi.JoinDesc:
        return _abi.JoinDesc(self.overlap_ratio, self.min_radius, 0.0 if self.radius_ratio is None else self.radius_ratio,
                             self.max_clusters)


def configure_cluster_join(ctx: _abi.Context, join: JoinSettings | None) -> None:
    """``attpc_trace_configure_cluster_join`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, JoinSettings, checked(JoinSettings, join, "join"))


def joins_last(ctx: _abi.Context, n_events: int):
    """(events [n_events] ``JOIN_EVENT_DTYPE``, records [n_events, 8] ``JOIN_DTYPE``) of ctx's last trace-row call
    (``attpc_joins_last``); RuntimeError if this stage or the clustering was off for it."""
    events = np.empty(int(n_events), dtype=JOIN_EVENT_DTYPE)
    records = np.empty((int(n_events), _abi.MAX_SIM), dtype=JOIN_DTYPE)
    ctx.check(ctx.lib.attpc_joins_last(ctx.handle, 0, len(events), _abi.iptr(events, _abi.JoinEvent),
                                       _abi.iptr(records, _abi.JoinRecord)), "attpc_joins_last")
    return events, records


def join_result(ctx: _abi.Context, n_events: int, n_sim: int = 0, n_rows=None) -> dict:
    """``{"joins": (events, records)}`` of ctx's last trace-row call if the ctx holds this stage and the clustering,
    else {}."""
    if ctx._tokens["cluster_join"] is None or ctx._tokens["clustering"] is None:
        return {}
    return {"joins": joins_last(ctx, n_events)}


def rows_to_joined_clusters(offsets, rows, labels, indices, clustering: ClusterSettings, join: JoinSettings,
                            ctx: _abi.Context | None = None):
    """The clustering and the joining alone on any host rows in CSR form (``attpc_rows_cluster_join``; the kernels of
    the fused path, no other configuration needed), arguments as ``rows_to_clusters`` -> (cluster_labels [R], events [n]
    ``CLUSTER_EVENT_DTYPE``, records [n, 8] ``CLUSTER_DTYPE``, join_events [n] ``JOIN_EVENT_DTYPE``, join_records [n, 8]
    ``JOIN_DTYPE``).  Rows outside offsets[0] .. offsets[n] get -1."""
    if not isinstance(clustering, ClusterSettings):
        raise TypeError("rows_to_joined_clusters needs a ClusterSettings")
    if not isinstance(join, JoinSettings):
        raise TypeError("rows_to_joined_clusters needs a JoinSettings")
    layout = _layout(indices)
    offsets, rows, labels, n = host_rows(offsets, rows, labels, optional_labels=True)
    out = np.full(len(rows), -1, dtype=np.int64)
    events = np.zeros(n, dtype=_abi.CLUSTER_EVENT_DTYPE)
    records = np.zeros((n, _abi.MAX_SIM), dtype=_abi.CLUSTER_DTYPE)
    join_events = np.zeros(n, dtype=JOIN_EVENT_DTYPE)
    join_records = np.zeros((n, _abi.MAX_SIM), dtype=JOIN_DTYPE)
    i64 = _abi.C.c_int64
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_rows_cluster_join(ctx.handle, n, _abi.iptr(offsets, i64), _abi.dptr(rows),
                                              None if labels is None else _abi.iptr(labels, i64), layout, clustering.desc(),
                                              join.desc(), _abi.iptr(out, i64), _abi.iptr(events, _abi.ClusterEvent),
                                              _abi.iptr(records, _abi.ClusterRecord), _abi.iptr(join_events, _abi.JoinEvent),
                                              _abi.iptr(join_records, _abi.JoinRecord)), "attpc_rows_cluster_join")
    return out, events, records, join_events, join_records
