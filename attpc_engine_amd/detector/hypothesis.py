"""Fit hypotheses: every slot of an event is fitted once per candidate species, and one kernel gives every slot the
position of the lowest objective ``f`` (``attpc_trace_configure_hypotheses``; the contract is in
include/attpc_engine.h, "fit hypotheses", ``tests/hypothesis_reference.py`` restates it).  A trial integrated with the
wrong stopping-power table cannot have the curvature and the range of the data at once, so the track fit itself is a
particle identification that needs no gate on the biased estimates; with the particle identification on as well its
gates only narrow the candidates (``pid.held``) and the fit decides among them.  Not a row of
``detector.traces.STAGES``: the stage is configured on the ``Engine`` (``Engine.configure_fit_hypotheses``), like the
reaction reconstruction, and takes effect only where the estimates and the track fit are on; ``run_trace_rows`` and
``run_estimates`` then carry ``"hypotheses"`` [n, n_sim] (``HYPOTHESIS_DTYPE``), ``"fits"`` are the chosen species'
records, and the reaction reconstruction reads this stage's positions.  ``rows_to_fit_hypotheses`` is the stage alone on
any host rows.  ``simulate_batch*``, ``configure_trace_rows``, ``run_fused``, ``run_simulation`` and the writers do not
take it."""
from __future__ import annotations

import numpy as np

from .. import _abi
from .._abi import HYP_DISPLACED, HYP_NO_CANDIDATE, HYP_NO_FIT, HYP_TAKEN, HYPOTHESIS_DTYPE  # noqa: F401
from .estimate import EstimateSettings
from .fit import TrackFitSettings
from .stage import checked, configure_stage, host_rows
from .stage import layout as _layout

STATUS_BITS = {"NO_CANDIDATE": HYP_NO_CANDIDATE, "NO_FIT": HYP_NO_FIT, "TAKEN": HYP_TAKEN, "DISPLACED": HYP_DISPLACED}
ALL_POSITIONS = (1 << _abi.MAX_SIM) - 1


class HypothesisSettings:
    """The validated settings of the fit hypotheses (``attpc_hypothesis_desc``): ``candidates``, the positions that may
    be chosen, as a bit mask (an int, bit p = position p) or a sequence of positions; None: all."""

    slot, call = "hypotheses", "attpc_trace_configure_hypotheses"

    def __init__(self, candidates=None):
        if candidates is None:
            mask = ALL_POSITIONS
        elif isinstance(candidates, (bool, np.bool_, str, bytes, float)):
            raise TypeError(f"candidates must be a bit mask, a sequence of positions or None, got {candidates!r}")
        elif isinstance(candidates, (int, np.integer)):
            mask = int(candidates)
        else:
            try:
                positions = list(candidates)
            except TypeError:
                raise TypeError(f"candidates must be a bit mask, a sequence of positions or None, got {candidates!r}") from None
            mask = 0
            for p in positions:
                if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, np.integer)) or not 0 <= p < _abi.MAX_SIM:
                    raise ValueError(f"a candidate position must be an integer in 0 .. {_abi.MAX_SIM - 1}, got {p!r}")
                mask |= 1 << int(p)
        if mask <= 0 or mask >> _abi.MAX_SIM:
            raise ValueError(f"candidates must name at least one position in 0 .. {_abi.MAX_SIM - 1}, got mask {mask:#x}")
        self.candidates = mask

    def token(self):
        return (self.candidates,)

    def desc(self) -> _abi.HypothesisDesc:
        return _abi.HypothesisDesc(self.candidates, 0)


def configure_fit_hypotheses(ctx: _abi.Context, settings: HypothesisSettings | None) -> None:
    """``attpc_trace_configure_hypotheses`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, HypothesisSettings, checked(HypothesisSettings, settings, "settings"))


def stage_on(ctx: _abi.Context) -> bool:
    """The ctx holds the stage and what it needs: the estimates and the track fit."""
    return all(ctx._tokens[slot] is not None for slot in ("hypotheses", "estimates", "fit"))


def hypotheses_last(ctx: _abi.Context, n_events: int, n_sim: int) -> np.ndarray:
    """The records [n_events, n_sim] (``HYPOTHESIS_DTYPE``) of ctx's last trace-row call (``attpc_hypotheses_last``);
    RuntimeError if the stage, the track fit or the estimates were off for it."""
    records = np.empty((int(n_events), int(n_sim)), dtype=HYPOTHESIS_DTYPE)
    ctx.check(ctx.lib.attpc_hypotheses_last(ctx.handle, 0, len(records), _abi.iptr(records, _abi.FitHypothesis)),
              "attpc_hypotheses_last")
    return records


def hypothesis_fits_last(ctx: _abi.Context, n_events: int, n_sim: int) -> np.ndarray:
    """The fit records of every hypothesis [n_events, n_sim, H] (``FIT_DTYPE``) of ctx's last trace-row call
    (``attpc_hypothesis_fits_last``)."""
    room = np.empty((int(n_events), int(n_sim), _abi.MAX_SIM), dtype=_abi.FIT_DTYPE)
    n_hyp = _abi.C.c_int32(0)
    ctx.check(ctx.lib.attpc_hypothesis_fits_last(ctx.handle, 0, len(room), _abi.C.byref(n_hyp), _abi.iptr(room, _abi.TrackFit)),
              "attpc_hypothesis_fits_last")
    return _tight(room, n_hyp.value)


def _tight(room: np.ndarray, n_hyp: int) -> np.ndarray:
    """[n, n_sim, H] records from the front of an array with room for MAX_SIM hypotheses per slot."""
    n, n_sim = room.shape[:2]
    return room.reshape(-1)[:n * n_sim * n_hyp].reshape(n, n_sim, n_hyp).copy()


def hypotheses_result(ctx: _abi.Context, n_events: int, n_sim: int) -> dict:
    """``{"hypotheses": records [n_events, n_sim]}`` of ctx's last trace-row call if the ctx holds the stage, the track
    fit and the estimates, else {}."""
    return {"hypotheses": hypotheses_last(ctx, n_events, n_sim)} if stage_on(ctx) else {}


def rows_to_fit_hypotheses(offsets, rows, labels, indices, estimates, ctx: _abi.Context, fit: TrackFitSettings,
                           settings: HypothesisSettings, start=None, *, estimate_settings=None, species_of_row=None, pid=None):
    """The stage alone on any host rows in CSR form (``attpc_rows_fit_hypotheses``; the two kernels of the fused path),
    with the arguments of ``detector.fit.rows_to_fit`` -> (records [n, n_sim] ``HYPOTHESIS_DTYPE``, fits [n, n_sim]
    ``FIT_DTYPE`` -- the chosen species' records --, all_fits [n, n_sim, H] -- the record of every (slot, hypothesis),
    ``FIT_NO_PID`` where the pair was no candidate --, species [H], the detector species of every hypothesis in the
    order of all_fits' last axis).  ``pid`` [n, n_sim] (``PID_DTYPE``) or None: its ``held`` narrows the candidates."""
    if not isinstance(fit, TrackFitSettings):
        raise TypeError("fit must be a TrackFitSettings")
    if not isinstance(settings, HypothesisSettings):
        raise TypeError("settings must be a HypothesisSettings")
    estimate_settings = estimate_settings or EstimateSettings(magnetic_field=0.0)
    if not isinstance(estimate_settings, EstimateSettings):
        raise TypeError("estimate_settings must be an EstimateSettings")
    if estimate_settings.magnetic_field is None:
        estimate_settings = estimate_settings.for_field(0.0)  # (the fit reads the field of the detector, not this one)
    if species_of_row is None and not isinstance(indices, _abi.EventLayout):
        raise ValueError("rows_to_fit_hypotheses needs an EventLayout, or indices with species_of_row")
    layout = _layout(indices, species_of_row)
    offsets, rows, labels, n = host_rows(offsets, rows, labels)
    estimates = np.ascontiguousarray(estimates, dtype=_abi.ESTIMATE_DTYPE)
    if estimates.shape != (n, layout.n_sim):
        raise ValueError(f"estimates must be [{n}, {layout.n_sim}], got {estimates.shape}")
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64)
        if start.shape != (n, layout.n_sim, 6):
            raise ValueError(f"start must be [{n}, {layout.n_sim}, 6], got {start.shape}")
    if pid is not None:
        pid = np.ascontiguousarray(pid, dtype=_abi.PID_DTYPE)
        if pid.shape != (n, layout.n_sim):
            raise ValueError(f"pid must be [{n}, {layout.n_sim}], got {pid.shape}")
    records = np.empty((n, layout.n_sim), dtype=HYPOTHESIS_DTYPE)
    fits = np.empty((n, layout.n_sim), dtype=_abi.FIT_DTYPE)
    room = np.empty((n, layout.n_sim, _abi.MAX_SIM), dtype=_abi.FIT_DTYPE)
    n_hyp, species = _abi.C.c_int32(0), np.full(_abi.MAX_SIM, -1, dtype=np.int32)
    ctx.check(ctx.lib.attpc_rows_fit_hypotheses(
        ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(rows), _abi.iptr(labels, _abi.C.c_int64), layout,
        estimate_settings.desc(), _abi.iptr(estimates, _abi.TrackEstimate), None if start is None else _abi.dptr(start),
        fit.desc(), settings.desc(), _abi.iptr(pid, _abi.PidRecord), _abi.iptr(records, _abi.FitHypothesis),
        _abi.iptr(fits, _abi.TrackFit), _abi.iptr(room, _abi.TrackFit), _abi.C.byref(n_hyp),
        _abi.iptr(species, _abi.C.c_int32)), "attpc_rows_fit_hypotheses")
    return records, fits, _tight(room, n_hyp.value), species[:n_hyp.value].copy()
