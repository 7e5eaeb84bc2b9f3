"""Helix slope: the slope of the track estimates from the regression of z against the TURNING ANGLE of the fit
segment's points about the centre of the record's circle, in the place of z against the cumulated pad-plane distance
between consecutive points (``attpc_trace_configure_helix``; the contract is in include/attpc_engine.h, "helix slope",
``tests/helix_reference.py`` restates it in numpy).  Lateral scatter lengthens the zig-zag path and pulls the polar
angle towards pi/2; around the fitted centre the radial scatter drops out.  The stage is opt-in
(``HelixSlopeSettings``, ``helix=``) and takes effect only where the estimates are on, on raw rows and on thinned
points, behind the Kasa circle and behind the geometric circle fit: ``slope``, ``vz`` and ``brho`` of the records then
come from the helix, and ``STATUS_BITS["NO_HELIX"]`` marks a record in which the stage could not run (that record is
the stage-off one).  ``rows_to_estimates(..., helix=...)`` is the stage alone on any host rows."""
from __future__ import annotations

import numpy as np

from .. import _abi
from .._abi import EST_NO_HELIX, HELIX_AUTO, HELIX_PATH_ON_Z, HELIX_Z_ON_PATH  # noqa: F401
from .estimate import STATUS_BITS as _ESTIMATE_BITS
from .stage import checked, configure_stage

REGRESSORS = {"auto": HELIX_AUTO, "z_on_path": HELIX_Z_ON_PATH, "path_on_z": HELIX_PATH_ON_Z}
# the status bits of a record made with the stage on: those of ``detector.estimate.STATUS_BITS`` and NO_HELIX
STATUS_BITS = {**_ESTIMATE_BITS, "NO_HELIX": EST_NO_HELIX}


class HelixSlopeSettings:
    """The validated settings of the helix slope (``attpc_helix_desc``, include/attpc_engine.h): ``regressor``, which
    of the two coordinates the regression takes as given -- "z_on_path" (z against the path), "path_on_z" (the path
    against z) or "auto" (the one with the larger spread, the default); the numbers 1, 2 and 0 of the header say the
    same."""

    slot, call = "helix", "attpc_trace_configure_helix"

    def __init__(self, regressor="auto"):
        if isinstance(regressor, str):
            if regressor not in REGRESSORS:
                raise ValueError(f"helix regressor must be one of {sorted(REGRESSORS)} or 0 .. 2, got {regressor!r}")
            regressor = REGRESSORS[regressor]
        if (isinstance(regressor, (bool, np.bool_)) or not isinstance(regressor, (int, np.integer))
                or regressor not in REGRESSORS.values()):
            raise ValueError(f"helix regressor must be one of {sorted(REGRESSORS)} or 0 .. 2, got {regressor!r}")
        self.regressor = int(regressor)

    def token(self):
        return (self.regressor,)

    def desc(self) -> _abi.HelixDesc:
        return _abi.HelixDesc(self.regressor, 0)


def configure_helix(ctx: _abi.Context, helix: HelixSlopeSettings | None) -> None:
    """``attpc_trace_configure_helix`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, HelixSlopeSettings, checked(HelixSlopeSettings, helix, "helix"))


def helix_result(ctx: _abi.Context, n_events: int = 0, n_sim: int = 0, n_rows=None) -> dict:
    """``{"slope": "helix"}`` if the ctx holds both the estimates and the helix slope -- the slopes of its last
    trace-row call are then the helix's --, else {}."""
    return {"slope": "helix"} if ctx._tokens["helix"] is not None and ctx._tokens["estimates"] is not None else {}
