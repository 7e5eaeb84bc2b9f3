"""Track estimates of the trace rows: what Spyral's estimation phase computes for every cluster -- a circle in the pad
plane (radius -> B rho), the polar angle from z against the path, the vertex, dE/dx --, made on the device for every
simulated nucleus of every event from the labelled trace rows (``attpc_trace_configure_estimates``; the contract is in
include/attpc_engine.h, ``tests/estimate_reference.py`` restates it in numpy).  The stage is opt-in
(``EstimateSettings``, ``estimates=``): ``Engine.run_trace_rows`` / ``simulate_batch_trace_rows`` then return one
128-byte record per (event, position of ``indices``) under ``"estimates"`` (``ESTIMATE_DTYPE``), beside the ``p4`` and
``vertex`` of the same call, which are the truth (``truth_tracks``).  ``rows_to_estimates`` is the stage alone on any
host rows, the delivered rows of ``run_spyral`` included.  The trigonometry stays here: ``polar``, ``azimuthal``.
The writers do not store the records."""
from __future__ import annotations

import copy
import math

import numpy as np

from .. import _abi
from .._abi import (ESTIMATE_DTYPE, EST_CAPPED, EST_EMPTY, EST_FEW, EST_MAX_FIT, EST_NOT_CONVERGED, EST_NO_CIRCLE,  # noqa: F401
                    EST_NO_HELIX, EST_NO_SLOPE, EST_ON_AXIS, EST_RANGE)
from .circle import CircleFitSettings
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout

STATUS_BITS = {"EMPTY": EST_EMPTY, "FEW": EST_FEW, "RANGE": EST_RANGE, "CAPPED": EST_CAPPED, "NO_CIRCLE": EST_NO_CIRCLE,
               "ON_AXIS": EST_ON_AXIS, "NO_SLOPE": EST_NO_SLOPE, "NOT_CONVERGED": EST_NOT_CONVERGED}
# (the eight bits of the estimates and the circle fit; ``detector.helix.STATUS_BITS`` adds the helix slope's NO_HELIX)
C_MEV_PER_TM = 299.792458  # p [MeV/c] = 299.792458 Z B rho [T m]


class EstimateSettings:
    """The validated settings of the track estimates (``attpc_estimate_desc``, include/attpc_engine.h):
    ``beam_region_radius`` (mm, finite and >= 0: rows nearer the beam axis are not used) and ``min_points`` (an integer
    >= 3: fewer used rows give no estimate); the defaults are Spyral's.  The magnetic field comes from the config
    (``configure_estimates``, ``for_field``); ``magnetic_field`` gives it directly, to ``rows_to_estimates`` for one."""

    slot, call = "estimates", "attpc_trace_configure_estimates"

    def __init__(self, beam_region_radius: float = 25.0, min_points: int = 30, *, magnetic_field: float | None = None):
        self.beam_region_radius = float(beam_region_radius)
        if not (math.isfinite(self.beam_region_radius) and self.beam_region_radius >= 0.0):
            raise ValueError(f"estimate beam_region_radius must be finite and >= 0, got {beam_region_radius!r}")
        if isinstance(min_points, (bool, np.bool_)) or not isinstance(min_points, (int, np.integer)) or not 3 <= min_points < 1 << 31:
            raise ValueError(f"estimate min_points must be an integer >= 3, got {min_points!r}")
        self.min_points = int(min_points)
        self.magnetic_field = None if magnetic_field is None else float(magnetic_field)
        if self.magnetic_field is not None and math.isnan(self.magnetic_field):
            raise ValueError("estimate magnetic_field is NaN")

    def for_field(self, magnetic_field: float) -> "EstimateSettings":
        """The same settings in a field of ``magnetic_field`` tesla (one given to the constructor stays)."""
        if self.magnetic_field is not None:
            return self
        bound = copy.copy(self)
        bound.magnetic_field = float(magnetic_field)
        if math.isnan(bound.magnetic_field):
            raise ValueError("estimate magnetic_field is NaN")
        return bound

    def token(self):
        if self.magnetic_field is None:
            raise ValueError("the estimates need a magnetic field: EstimateSettings.for_field, or configure_estimates with a config")
        return (self.beam_region_radius, self.magnetic_field, self.min_points)

    def desc(self) -> _abi.EstimateDesc:
        return _abi.EstimateDesc(*self.token(), 0)


def configure_estimates(ctx: _abi.Context, estimates: EstimateSettings | None, config=None) -> None:
    """``attpc_trace_configure_estimates`` unless this ctx already holds the same settings (``None``: the stage off);
    the field is ``config.det_params.bfield`` unless the settings carry one."""
    if checked(EstimateSettings, estimates, "estimates") is not None and config is not None:
        estimates = estimates.for_field(config.det_params.bfield)
    configure_stage(ctx, EstimateSettings, estimates)


def estimates_result(ctx: _abi.Context, n_events: int, n_sim: int, n_rows=None) -> dict:
    """``{"estimates": records [n_events, n_sim]}`` of ctx's last trace-row call if the ctx holds the stage, else {}."""
    return {"estimates": ctx.estimates_last(n_events, n_sim)} if ctx._tokens["estimates"] is not None else {}


def rows_to_estimates(offsets, rows, labels, indices, settings: EstimateSettings, ctx: _abi.Context | None = None,
                      config=None, circle=None, helix=None) -> np.ndarray:
    """The estimate stage alone on any host rows in CSR form (``attpc_rows_estimate``; the kernel of the fused path, no
    other configuration needed): offsets [n+1], rows [R,8] as ``run_trace_rows`` / ``run_spyral`` deliver them, labels
    [R], ``indices`` (the nucleus of every track position) -> records [n, len(indices)] (``ESTIMATE_DTYPE``).  The field
    is the settings' own, else ``config.det_params.bfield``.  ``circle`` (a ``detector.circle.CircleFitSettings``; None =
    off): the geometric circle fit behind the Kasa circle (``attpc_rows_estimate_circle``).  ``helix`` (a
    ``detector.helix.HelixSlopeSettings``; None = off): the helix slope behind the circle, with or without ``circle``
    (``attpc_rows_estimate_helix``)."""
    from .helix import HelixSlopeSettings  # (that module reads the STATUS_BITS of this one)

    if not isinstance(settings, EstimateSettings):
        raise TypeError("settings must be an EstimateSettings")
    checked(CircleFitSettings, circle, "circle")
    checked(HelixSlopeSettings, helix, "helix")
    if config is not None:
        settings = settings.for_field(config.det_params.bfield)
    desc = settings.desc()
    layout = _layout(indices)
    offsets, rows, labels, n = host_rows(offsets, rows, labels)
    records = np.empty((n, layout.n_sim), dtype=ESTIMATE_DTYPE)
    ctx = ctx or _abi.default_context()
    if helix is not None:
        ctx.check(ctx.lib.attpc_rows_estimate_helix(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows),
                                                    _abi.iptr(labels, _abi.C.c_int64), layout, desc,
                                                    None if circle is None else circle.desc(), helix.desc(),
                                                    _abi.iptr(records, _abi.TrackEstimate)), "attpc_rows_estimate_helix")
        return records
    if circle is not None:
        ctx.check(ctx.lib.attpc_rows_estimate_circle(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows),
                                                     _abi.iptr(labels, _abi.C.c_int64), layout, desc, circle.desc(),
                                                     _abi.iptr(records, _abi.TrackEstimate)), "attpc_rows_estimate_circle")
        return records
    ctx.check(ctx.lib.attpc_rows_estimate(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows),
                                          _abi.iptr(labels, _abi.C.c_int64), layout, desc,
                                          _abi.iptr(records, _abi.TrackEstimate)), "attpc_rows_estimate")
    return records


def polar(est) -> np.ndarray:
    """The polar angle of the records in 0 .. pi: ``arctan2(1, slope)`` (slope = cot(theta); NaN stays NaN)."""
    slope = np.asarray(est["slope"], dtype=np.float64)
    return np.arctan2(np.ones_like(slope), slope)


def azimuthal(est) -> np.ndarray:
    """The azimuth of the records in 0 .. 2 pi, from the chord vertex -> mean of the fit segment."""
    return np.mod(np.arctan2(est["y_mean"] - est["vy"], est["x_mean"] - est["vx"]), 2.0 * np.pi)


def truth_tracks(p4, indices, proton_numbers) -> dict:
    """The truth beside the estimates: for ``p4`` [n, n_rows, 4] (px, py, pz, E in MeV) and the nuclei ``indices`` of
    charge ``proton_numbers[i]`` -> {"brho": |p| / (299.792458 Z) in T m (inf for Z = 0), "polar" in 0 .. pi,
    "azimuthal" in 0 .. 2 pi}, each [n, len(indices)]."""
    p = np.asarray(p4, dtype=np.float64)[:, [int(i) for i in indices], :3]
    z = np.asarray([proton_numbers[int(i)] for i in indices], dtype=np.float64)
    pt = np.hypot(p[..., 0], p[..., 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        brho = np.sqrt(pt * pt + p[..., 2] * p[..., 2]) / (C_MEV_PER_TM * z)
    return {"brho": brho, "polar": np.arctan2(pt, p[..., 2]),
            "azimuthal": np.mod(np.arctan2(p[..., 1], p[..., 0]), 2.0 * np.pi)}
