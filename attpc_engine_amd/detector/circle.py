"""Geometric circle fit: the Kasa circle of the track estimates refined on the device by a least-squares fit of the
geometric distances of the fit segment's points to the circle (Levenberg-Marquardt from the Kasa circle;
``attpc_trace_configure_circle``; the contract is in include/attpc_engine.h, "geometric circle fit",
``tests/circle_reference.py`` restates it in numpy).  The algebraic fit pulls the radius low on a short noisy arc, the
geometric one does not.  The stage is opt-in (``CircleFitSettings``, ``circle=``) and takes effect only where the
estimates are on, with or without thinning: centre, radius, vertex and B rho of the records then come from the refined
circle, ``reserved`` carries the evaluations made and ``STATUS_BITS["NOT_CONVERGED"]`` marks a fit that spent them all.
``rows_to_estimates(..., circle=...)`` is the stage alone on any host rows."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .._abi import (CIRCLE_DEFAULT_EVALUATIONS, CIRCLE_DEFAULT_TOLERANCE, CIRCLE_MAX_EVALUATIONS,  # noqa: F401
                    CIRCLE_MIN_EVALUATIONS, EST_NOT_CONVERGED)
from .stage import checked, configure_stage


class CircleFitSettings:
    """The validated settings of the geometric circle fit (``attpc_circle_desc``, include/attpc_engine.h):
    ``max_evaluations`` (an integer in 2 .. 64: evaluations of the objective, the start included) and ``tolerance`` (in
    units of 1/16 mm, finite and > 0: the fit has converged on an accepted step no larger than this)."""

    slot, call = "circle", "attpc_trace_configure_circle"

    def __init__(self, max_evaluations: int = CIRCLE_DEFAULT_EVALUATIONS, tolerance: float = CIRCLE_DEFAULT_TOLERANCE):
        if (isinstance(max_evaluations, (bool, np.bool_)) or not isinstance(max_evaluations, (int, np.integer))
                or not CIRCLE_MIN_EVALUATIONS <= max_evaluations <= CIRCLE_MAX_EVALUATIONS):
            raise ValueError(f"circle max_evaluations must be an integer in {CIRCLE_MIN_EVALUATIONS} .. "
                             f"{CIRCLE_MAX_EVALUATIONS}, got {max_evaluations!r}")
        if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
            raise ValueError(f"circle tolerance must be a number, got {tolerance!r}")
        self.max_evaluations, self.tolerance = int(max_evaluations), float(tolerance)
        if not (math.isfinite(self.tolerance) and self.tolerance > 0.0):
            raise ValueError(f"circle tolerance must be finite and > 0, got {tolerance!r}")

    def token(self):
        return (self.tolerance, self.max_evaluations)

    def desc(self) -> _abi.CircleDesc:
        return _abi.CircleDesc(self.tolerance, self.max_evaluations, 0)


def configure_circle(ctx: _abi.Context, circle: CircleFitSettings | None) -> None:
    """``attpc_trace_configure_circle`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, CircleFitSettings, checked(CircleFitSettings, circle, "circle"))


def circle_result(ctx: _abi.Context, n_events: int = 0, n_sim: int = 0, n_rows=None) -> dict:
    """``{"circle": "geometric"}`` if the ctx holds both the estimates and the circle fit -- the circles of its last
    trace-row call are then the refined ones --, else {}."""
    return {"circle": "geometric"} if ctx._tokens["circle"] is not None and ctx._tokens["estimates"] is not None else {}
