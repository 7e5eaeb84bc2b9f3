"""Drift correction: the way back from the drift distortion, on the trace rows and on the device
(``attpc_trace_configure_correction``; the contract is in include/attpc_engine.h, "drift correction",
``tests/undistort_reference.py`` restates it in numpy).  Every row of a chunk is taken from its apparent (x, y, time) to
where its electrons were made, by fixed-point iteration on the forward map of a ``DistortionMap``, and the rows of every
event are sorted again by their corrected time -- a map with a time table changes z, and the thinning and the estimates
rely on ascending z.  The stage is opt-in (``CorrectionSettings``, ``correction=``) and sits between the kernel that
writes the rows and everything that reads them: thinning, estimates and delivery see the corrected rows.  The map is the
caller's and need not be the one the tracks were distorted with: what a wrong map costs is a use case.
``rows_to_correction`` is the stage alone on any host rows; ``DistortionMap.undistort_rows`` is the same correction in
numpy, without the re-sort and with the time taken from z."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .distortion import DistortionMap
from .stage import checked, host_rows

MAX_ITERATIONS = 64
COUNTS = ("n_rows", "n_skipped", "n_unconverged", "n_moved")


def _tolerance(what: str, value) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"correction {what} must be a number, got {value!r}")
    value = float(value)
    if not (value >= 0.0 and math.isfinite(value)):
        raise ValueError(f"correction {what} must be finite and >= 0, got {value}")
    return value


class CorrectionSettings:
    """The validated settings of the drift correction (``attpc_undistort_desc``, include/attpc_engine.h): ``map``, the
    ``DistortionMap`` to correct with; ``iterations`` of the fixed point, 1 .. 64; ``tolerance_xy`` (m) and
    ``tolerance_tb`` (time buckets), finite and >= 0: a row whose last step was larger counts in ``n_unconverged``."""

    slot, call = "correction", "attpc_trace_configure_correction"

    def __init__(self, map, iterations: int = 12, tolerance_xy: float = 1e-6, tolerance_tb: float = 1e-3):
        if not isinstance(map, DistortionMap):
            raise TypeError(f"the correction's map must be a DistortionMap, got {type(map).__name__}")
        if (isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer))
                or not 1 <= int(iterations) <= MAX_ITERATIONS):
            raise ValueError(f"correction iterations must be an integer in 1 .. {MAX_ITERATIONS}, got {iterations!r}")
        self.map, self.iterations = map, int(iterations)
        self.tolerance_xy, self.tolerance_tb = _tolerance("tolerance_xy", tolerance_xy), _tolerance("tolerance_tb", tolerance_tb)

    @property
    def on(self) -> bool:
        return self.map.on

    def _drift(self, config):
        if config is None:
            raise ValueError("a CorrectionSettings needs the run's config")
        mm, win = int(config.elec_params.micromegas_edge), int(config.elec_params.windows_edge)
        length = float(config.det_params.length)
        if not win > mm:
            raise ValueError("windows_edge <= micromegas_edge")
        if not (length > 0.0 and math.isfinite(length)):
            raise ValueError(f"the detector length must be finite and > 0, got {length}")
        return win, mm, length

    def token(self, config):
        """None: a map that shifts nothing, the stage off."""
        if not self.on:
            return None
        drift = self._drift(config)
        return (self.map.token(config), *drift, self.iterations, self.tolerance_xy, self.tolerance_tb)

    def desc(self, config) -> _abi.UndistortDesc:
        """The ``attpc_undistort_desc`` of these settings in the drift of ``config`` (it refers to the map's arrays)."""
        win, mm, length = self._drift(config)
        return _abi.UndistortDesc(self.map.desc(config), win, mm, length, self.iterations, self.tolerance_xy, self.tolerance_tb)


def configure_correction(ctx: _abi.Context, correction: CorrectionSettings | None, config=None) -> None:
    """``attpc_trace_configure_correction`` unless this ctx already holds the same settings in the same drift (``None``,
    or a map that is zero everywhere: the stage off).  ``config``: the run's Config, whose time-bucket edges and length
    place the map's nodes and give a corrected time its z."""
    correction = checked(CorrectionSettings, correction, "correction")
    token = None
    if correction is not None and correction.on:
        token = correction.token(config)
    ctx.configure(CorrectionSettings.slot, token, CorrectionSettings.call, None if token is None else correction.desc(config))


def correction_result(ctx: _abi.Context, n_events: int = 0, n_sim: int = 0, n_rows=None) -> dict:
    """``{"correction": {n_rows, n_skipped, n_unconverged, n_moved}}`` of the ctx's last trace-row call if it holds the
    stage, else {}."""
    return {"correction": ctx.correction_last()} if ctx._tokens["correction"] is not None else {}


def rows_to_correction(offsets, rows, labels, correction: CorrectionSettings, config, ctx: _abi.Context | None = None):
    """The stage alone on any host rows in CSR form (``attpc_rows_undistort``; the kernel of the fused path, no other
    configuration needed): offsets [n+1], rows [R,8] as ``run_trace_rows`` / ``run_spyral`` deliver them, labels [R] ->
    (rows [R,8] corrected and, per event, in ascending corrected z, labels [R] moved with them, order [R] = the input row
    of every output row, {n_rows, n_skipped, n_unconverged, n_moved}).  A map that shifts nothing runs like any other.
    It leaves the configured stage of ``ctx`` as it is."""
    if checked(CorrectionSettings, correction, "correction") is None:
        raise TypeError("rows_to_correction needs a CorrectionSettings")
    desc = correction.desc(config)
    offsets, rows, labels, n = host_rows(offsets, rows, labels)
    # (rows outside offsets[0] .. offsets[n] belong to no event: they come back as they are, in their place)
    out_rows, out_labels = rows.copy(), labels.copy()
    order = np.arange(len(rows), dtype=np.int64)
    info = _abi.UndistortInfo()
    i64 = _abi.C.c_int64
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_rows_undistort(ctx.handle, n, _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64), desc,
                                           _abi.dptr(out_rows), _abi.iptr(out_labels, i64), _abi.iptr(order, i64),
                                           _abi.C.byref(info)), "attpc_rows_undistort")
    return out_rows, out_labels, order, info.as_dict()
