"""Thinned track points: every track's labelled trace rows reduced to one charge-weighted centroid per z bin, on the
device and in exact integer arithmetic, in front of the track estimates (``attpc_trace_configure_thinning``; the
contract is in include/attpc_engine.h, "thinned track points", ``tests/thin_reference.py`` restates it in numpy).  A
track lights several pads at every z; on such a band the estimates' path zig-zags and their circle shrinks, on one point
per z step they do not.  The stage is opt-in (``ThinSettings``, ``thinning=``) and takes effect only where the estimates
are on: their records are then those of the points, and ``min_points`` counts points.  ``rows_to_points`` is the stage
alone on any host rows; its point rows are valid input of ``detector.estimate.rows_to_estimates``."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .._abi import THIN_INFO_DTYPE, THIN_MAX_RUN  # noqa: F401
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout


class ThinSettings:
    """The validated settings of the thinning (``attpc_thin_desc``, include/attpc_engine.h): ``z_step`` in mm, finite,
    1/16 .. 512 -- the height of a z bin."""

    slot, call = "thinning", "attpc_trace_configure_thinning"

    def __init__(self, z_step: float = 5.0):
        if isinstance(z_step, (bool, np.bool_)) or not isinstance(z_step, (int, float, np.integer, np.floating)):
            raise ValueError(f"thinning z_step must be a number, got {z_step!r}")
        self.z_step = float(z_step)
        if not (math.isfinite(self.z_step) and 1.0 / 16.0 <= self.z_step <= 512.0):
            raise ValueError(f"thinning z_step must be finite and in 1/16 .. 512 mm, got {z_step!r}")

    def token(self):
        return (self.z_step,)

    def desc(self) -> _abi.ThinDesc:
        return _abi.ThinDesc(self.z_step, 0, 0)


def configure_thinning(ctx: _abi.Context, thinning: ThinSettings | None) -> None:
    """``attpc_trace_configure_thinning`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, ThinSettings, checked(ThinSettings, thinning, "thinning"))


def thinning_result(ctx: _abi.Context, n_events: int = 0, n_sim: int = 0, n_rows=None) -> dict:
    """``{"thinning": z_step}`` if the ctx holds both the estimates and the thinning -- the records of its last
    trace-row call are then those of thinned points --, else {}."""
    token = ctx._tokens["thinning"]
    return {"thinning": token[0]} if token is not None and ctx._tokens["estimates"] is not None else {}


def rows_to_points(offsets, rows, labels, indices, settings: ThinSettings, ctx: _abi.Context | None = None):
    """The thinning stage alone on any host rows in CSR form (``attpc_rows_thin``; the kernel of the fused path, no other
    configuration needed): offsets [n+1], rows [R,8] as ``run_trace_rows`` / ``run_spyral`` deliver them, labels [R],
    ``indices`` (the nucleus of every track position) -> (point_offsets [n+1], points [P,8], point_labels [P], info
    [n, len(indices)] of ``THIN_INFO_DTYPE``).  Per event the points come position by position and in run order; a
    point row is x, y, z (mm), amplitude, integral, rows, z bin, 1 if a split at 4096 rows closed it."""
    if not isinstance(settings, ThinSettings):
        raise TypeError("settings must be a ThinSettings")
    desc = settings.desc()
    layout = _layout(indices)
    offsets, rows, labels, n = host_rows(offsets, rows, labels)
    capacity = int(offsets[-1] - offsets[0])  # (a label has no more points than rows)
    point_offsets = np.zeros(n + 1, dtype=np.int64)
    points = np.empty((capacity, 8), dtype=np.float64)
    point_labels = np.empty(capacity, dtype=np.int64)
    info = np.zeros((n, layout.n_sim), dtype=THIN_INFO_DTYPE)
    needed = np.zeros(1, dtype=np.int64)
    i64 = _abi.C.c_int64
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_rows_thin(ctx.handle, n, _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64), layout,
                                      desc, capacity, _abi.iptr(point_offsets, i64), _abi.dptr(points),
                                      _abi.iptr(point_labels, i64), _abi.iptr(info, _abi.ThinInfo), _abi.iptr(needed, i64)),
              "attpc_rows_thin")
    total = int(point_offsets[-1])
    return point_offsets, points[:total], point_labels[:total], info
