"""Track fit: the momentum and the vertex of every track from trial tracks integrated through the gas with the
species' stopping-power table, fitted to the label's points by Levenberg-Marquardt on the device
(``attpc_trace_configure_fit``; the contract is in include/attpc_engine.h, "track fit", ``tests/fit_reference.py``
restates it in numpy).  It is Spyral's solver phase behind the estimation phase: the estimate record of a track is the
start.  The stage is opt-in (``TrackFitSettings``, ``fit=``) and takes effect only where the estimates are on;
``run_trace_rows`` and ``run_estimates`` then carry ``"fits"`` [n, n_sim] (``FIT_DTYPE``) beside ``"estimates"``.
``rows_to_fit`` is the stage alone on any host rows.  Angles are made here, on the host: ``polar``, ``azimuthal``."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .._abi import (FIT_CAPPED, FIT_DTYPE, FIT_EMPTY, FIT_FEW, FIT_NO_START, FIT_NOT_CONVERGED, FIT_SINGULAR,  # noqa: F401
                    FIT_STEP_CAP)
from .estimate import EstimateSettings
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout

STATUS_BITS = {"EMPTY": FIT_EMPTY, "FEW": FIT_FEW, "CAPPED": FIT_CAPPED, "NO_START": FIT_NO_START,
               "SINGULAR": FIT_SINGULAR, "STEP_CAP": FIT_STEP_CAP, "NOT_CONVERGED": FIT_NOT_CONVERGED}
ENDS = {"stopped": _abi.FIT_END_STOPPED, "left": _abi.FIT_END_LEFT, "step_cap": _abi.FIT_END_STEP_CAP,
        "not_finite": _abi.FIT_END_NOT_FINITE}


def _positive(name: str, value) -> float:
    number = float(value)
    if not (math.isfinite(number) and number > 0.0):
        raise ValueError(f"fit {name} must be finite and > 0, got {value!r}")
    return number


def _integer(name: str, value, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"fit {name} must be an integer in {lo} .. {hi}, got {value!r}")
    return int(value)


class TrackFitSettings:
    """The validated settings of the track fit (``attpc_fit_desc``, include/attpc_engine.h): ``time_step`` (s, the fixed
    RK4 step of a trial; 1e-10 is the grid of the track kernel), ``max_steps`` (1 .. 10000 steps of a trial),
    ``max_evaluations`` (2 .. 32 evaluations of seven trials each), ``tolerance_momentum`` (the accepted step that ends
    the fit, relative to |gamma beta|) and ``tolerance_position`` (the same for the vertex, in metres)."""

    slot, call = "fit", "attpc_trace_configure_fit"

    def __init__(self, time_step: float = _abi.FIT_DEFAULT_TIME_STEP, max_steps: int = _abi.FIT_MAX_STEPS,
                 max_evaluations: int = _abi.FIT_DEFAULT_EVALUATIONS, tolerance_momentum: float = 1.0e-4,
                 tolerance_position: float = 1.0e-4):
        self.time_step = _positive("time_step", time_step)
        self.tolerance_momentum = _positive("tolerance_momentum", tolerance_momentum)
        self.tolerance_position = _positive("tolerance_position", tolerance_position)
        self.max_steps = _integer("max_steps", max_steps, 1, _abi.FIT_MAX_STEPS)
        self.max_evaluations = _integer("max_evaluations", max_evaluations, _abi.FIT_MIN_EVALUATIONS,
                                        _abi.FIT_MAX_EVALUATIONS)

    def token(self):
        return (self.time_step, self.tolerance_momentum, self.tolerance_position, self.max_steps, self.max_evaluations)

    def desc(self) -> _abi.FitDesc:
        return _abi.FitDesc(*self.token())


def _checked(fit):
    return checked(TrackFitSettings, fit, "fit")


def configure_track_fit(ctx: _abi.Context, fit: TrackFitSettings | None) -> None:
    """``attpc_trace_configure_fit`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, TrackFitSettings, _checked(fit))


def fits_last(ctx: _abi.Context, n_events: int, n_sim: int) -> np.ndarray:
    """The track fits [n_events, n_sim] (``FIT_DTYPE``) of ctx's last trace-row call (``attpc_fits_last``)."""
    records = np.empty((int(n_events), int(n_sim)), dtype=FIT_DTYPE)
    ctx.check(ctx.lib.attpc_fits_last(ctx.handle, 0, len(records), _abi.iptr(records, _abi.TrackFit)), "attpc_fits_last")
    return records


def fit_result(ctx: _abi.Context, n_events: int, n_sim: int, n_rows=None) -> dict:
    """``{"fits": records [n_events, n_sim]}`` of ctx's last trace-row call if the ctx holds both the estimates and the
    track fit, else {}."""
    if ctx._tokens["fit"] is None or ctx._tokens["estimates"] is None:
        return {}
    return {"fits": fits_last(ctx, n_events, n_sim)}


def rows_to_fit(offsets, rows, labels, indices, estimates, ctx: _abi.Context, settings: TrackFitSettings, start=None, *,
                estimate_settings=None, species_of_row=None, pid=None) -> np.ndarray:
    """The stage alone on any host rows in CSR form (``attpc_rows_fit``; the kernel of the fused path): offsets [n+1],
    rows [R,8], labels [R], ``indices`` (an ``_abi.EventLayout`` such as ``Engine.layout``, or the nucleus of every
    position with ``species_of_row``), ``estimates`` [n, n_sim] (``ESTIMATE_DTYPE``, of ``rows_to_estimates`` on the
    same rows with ``estimate_settings``) -> records [n, n_sim] (``FIT_DTYPE``).  ``start`` [n, n_sim, 6] = (gamma beta
    x, y, z, vertex x, y, z in metres) replaces the start from the estimates.  ``ctx`` must hold a configured detector:
    its species tables, masses, charges, fields and length are the model.  ``pid`` [n, n_sim] (``PID_DTYPE``, of
    ``detector.pid.estimates_to_pid`` on the same estimates): the fit behind the particle identification
    (``attpc_rows_fit_pid``) -- slot k is fitted as the nucleus of position ``pid["position"][e, k]``, and a slot without
    a position gets the record without a fit, ``FIT_NO_PID``."""
    if not isinstance(settings, TrackFitSettings):
        raise TypeError("settings must be a TrackFitSettings")
    estimate_settings = estimate_settings or EstimateSettings(magnetic_field=0.0)
    if not isinstance(estimate_settings, EstimateSettings):
        raise TypeError("estimate_settings must be an EstimateSettings")
    if estimate_settings.magnetic_field is None:
        estimate_settings = estimate_settings.for_field(0.0)  # (the fit reads the field of the detector, not this one)
    if species_of_row is None and not isinstance(indices, _abi.EventLayout):
        raise ValueError("rows_to_fit needs an EventLayout, or indices with species_of_row")
    layout = _layout(indices, species_of_row)
    offsets, rows, labels, n = host_rows(offsets, rows, labels)
    estimates = np.ascontiguousarray(estimates, dtype=_abi.ESTIMATE_DTYPE)
    if estimates.shape != (n, layout.n_sim):
        raise ValueError(f"estimates must be [{n}, {layout.n_sim}], got {estimates.shape}")
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64)
        if start.shape != (n, layout.n_sim, 6):
            raise ValueError(f"start must be [{n}, {layout.n_sim}, 6], got {start.shape}")
    records = np.empty((n, layout.n_sim), dtype=FIT_DTYPE)
    if pid is not None:
        pid = np.ascontiguousarray(pid, dtype=_abi.PID_DTYPE)
        if pid.shape != (n, layout.n_sim):
            raise ValueError(f"pid must be [{n}, {layout.n_sim}], got {pid.shape}")
        ctx.check(ctx.lib.attpc_rows_fit_pid(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows),
                                             _abi.iptr(labels, _abi.C.c_int64), layout, estimate_settings.desc(),
                                             _abi.iptr(estimates, _abi.TrackEstimate),
                                             None if start is None else _abi.dptr(start), settings.desc(),
                                             _abi.iptr(pid, _abi.PidRecord), _abi.iptr(records, _abi.TrackFit)),
                  "attpc_rows_fit_pid")
        return records
    ctx.check(ctx.lib.attpc_rows_fit(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows),
                                     _abi.iptr(labels, _abi.C.c_int64), layout, estimate_settings.desc(),
                                     _abi.iptr(estimates, _abi.TrackEstimate), None if start is None else _abi.dptr(start),
                                     settings.desc(), _abi.iptr(records, _abi.TrackFit)), "attpc_rows_fit")
    return records


def polar(fits) -> np.ndarray:
    """The polar angle of the fitted momentum in 0 .. pi (NaN stays NaN)."""
    g = np.asarray(fits["g"], dtype=np.float64)
    return np.arctan2(np.hypot(g[..., 0], g[..., 1]), g[..., 2])


def azimuthal(fits) -> np.ndarray:
    """The azimuth of the fitted momentum in 0 .. 2 pi."""
    g = np.asarray(fits["g"], dtype=np.float64)
    return np.mod(np.arctan2(g[..., 1], g[..., 0]), 2.0 * np.pi)
