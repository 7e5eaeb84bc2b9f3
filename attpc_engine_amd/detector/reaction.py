"""Reaction reconstruction: excitation energy and centre-of-mass angle of the two-body first step from one observed
track, next to the same numbers from the truth, and the spectra of a call (include/attpc_engine.h, "reaction
reconstruction"; csrc/reaction.hip).  Not a row of ``detector.traces.STAGES``: the stage needs the reaction, which a
``TraceChain`` does not know, so it is configured on the ``Engine`` (``Engine.configure_reaction``) like the summary, the
selection and the maps."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .stage import checked, configure_stage

REACTION_DTYPE = _abi.REACTION_DTYPE
STATUS_BITS = {"NO_TRACK": _abi.REACTION_NO_TRACK, "OUTSIDE_TARGET": _abi.REACTION_OUTSIDE_TARGET,
               "UNPHYSICAL": _abi.REACTION_UNPHYSICAL, "NO_TRUTH": _abi.REACTION_NO_TRUTH}
SOURCES = {"fit": _abi.REACTION_FROM_FIT, "estimate": _abi.REACTION_FROM_ESTIMATE}
PI = 3.141592653589793  # the upper edge of the angle's bins


def _integer(value, name: str, lo: int, hi: int) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {value!r}")
    return int(value)


def _number(value, name: str, positive: bool = False) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {value!r}")
    value = float(value)
    if not math.isfinite(value) or (positive and not value > 0.0):
        raise ValueError(f"{name} must be finite{' and > 0' if positive else ''}, got {value!r}")
    return value


class ReactionSettings:
    """The validated settings of the reaction reconstruction (``attpc_reaction_desc``): ``masses`` (target, projectile,
    ejectile, residual; MeV), ``charge`` (Z of the observed nucleus), ``beam_energy`` (MeV), ``target`` = None or
    (z_min, z_max in m, eloss: the projectile's energy loss at the nodes from z_min to z_max, MeV), ``track`` (the layout
    position whose track is read), ``observed_row`` (2: the ejectile, 3: the residual), ``source`` ("fit" or
    "estimate"), ``ex_range`` = (lo, hi) in MeV with ``ex_bins`` <= 256 bins and ``theta_bins`` <= 180 bins over
    [0, pi].  Self-contained: nothing is read from the configured kinematics."""

    slot, call = "reaction", "attpc_reaction_configure"

    def __init__(self, masses, charge, beam_energy, target=None, track: int = 0, observed_row: int = 2,
                 source: str = "fit", ex_range=(-2.0, 14.0), ex_bins: int = 64, theta_bins: int = 36):
        masses = tuple(masses)
        if len(masses) != 4:
            raise ValueError(f"masses must be the four of target, projectile, ejectile and residual, got {len(masses)}")
        self.masses = tuple(_number(m, "a mass", positive=True) for m in masses)
        self.charge = _integer(charge, "charge", 1, 2**31 - 1)
        self.beam_energy = _number(beam_energy, "beam_energy", positive=True)
        if target is None:
            self.z_min = self.z_max = 0.0
            self.eloss = None
        else:
            z_min, z_max, eloss = target
            self.z_min, self.z_max = _number(z_min, "z_min"), _number(z_max, "z_max")
            if not self.z_max > self.z_min:
                raise ValueError(f"the target needs z_min < z_max, got {self.z_min} .. {self.z_max}")
            eloss = np.ascontiguousarray(eloss, dtype=np.float64)
            if eloss.ndim != 1 or not 2 <= eloss.size <= _abi.REACTION_MAX_ELOSS or not np.all(np.isfinite(eloss)):
                raise ValueError(f"eloss must be 2 .. {_abi.REACTION_MAX_ELOSS} finite nodes")
            self.eloss = eloss.copy()
            self.eloss.setflags(write=False)
        self.track = _integer(track, "track", 0, _abi.MAX_SIM - 1)
        if isinstance(observed_row, (bool, np.bool_)) or observed_row not in (2, 3):
            raise ValueError(f"observed_row must be 2 (the ejectile) or 3 (the residual), got {observed_row!r}")
        self.observed_row = int(observed_row)
        if not isinstance(source, str) or source not in SOURCES:
            raise ValueError(f"source must be 'fit' or 'estimate', got {source!r}")
        self.source = source
        lo, hi = ex_range
        self.ex_lo, self.ex_hi = _number(lo, "ex_range[0]"), _number(hi, "ex_range[1]")
        if not self.ex_hi > self.ex_lo:
            raise ValueError(f"ex_range needs lo < hi, got {self.ex_lo} .. {self.ex_hi}")
        self.ex_bins = _integer(ex_bins, "ex_bins", 1, _abi.REACTION_MAX_EX)
        self.theta_bins = _integer(theta_bins, "theta_bins", 1, _abi.REACTION_MAX_THETA)
        # computed once, here; the device multiplies by them
        self.ex_inv_width = float(self.ex_bins) / (self.ex_hi - self.ex_lo)
        self.theta_inv_width = float(self.theta_bins) / PI
        if not math.isfinite(self.ex_inv_width):
            raise ValueError("ex_range is too narrow for its bins")

    @classmethod
    def from_pipeline(cls, pipeline, track: int = 0, source: str = "fit", ex_range=(-2.0, 14.0), ex_bins: int = 64,
                      theta_bins: int = 36, indices=None) -> "ReactionSettings":
        """The settings of ``pipeline``'s reaction: masses, beam energy and the energy-loss table are what
        ``kinematics/_device.py`` uploads for it; the observed nucleus is the one at position ``track`` of ``indices``
        (default: the final products, as ``Engine``), which must be row 2 or 3."""
        from .simulator import default_indices

        kin, keep = pipeline.device_desc()
        z = pipeline.get_proton_numbers()
        indices = list(indices) if indices is not None else default_indices(len(z))
        track = _integer(track, "track", 0, len(indices) - 1)
        row = int(indices[track])
        if row not in (2, 3):
            raise ValueError(f"position {track} is row {row} of the kinematics; the reconstruction observes row 2 or 3")
        target = None
        if kin.has_target:
            target = (kin.z_min, kin.z_max, np.ctypeslib.as_array(kin.eloss, shape=(kin.eloss_len,)).copy())
        del keep
        return cls([kin.masses[i] for i in range(4)], int(z[row]), kin.beam_energy, target, track, row, source, ex_range,
                   ex_bins, theta_bins)

    def check_indices(self, indices) -> None:
        """ValueError unless position ``track`` of ``indices`` is the kinematics row ``observed_row``: the fit of one
        nucleus would otherwise be read with the mass and the truth row of another."""
        indices = list(indices)
        if self.track >= len(indices) or int(indices[self.track]) != self.observed_row:
            raise ValueError(f"track {self.track} of indices {indices} is not row {self.observed_row} of the kinematics")

    @property
    def n_cells(self) -> int:
        return 3 * self.ex_bins * self.theta_bins + self.ex_bins * self.ex_bins + 3

    def token(self):
        return (self.masses, self.charge, self.beam_energy, self.z_min, self.z_max,
                None if self.eloss is None else self.eloss.tobytes(), self.track, self.observed_row, self.source,
                self.ex_lo, self.ex_hi, self.ex_bins, self.theta_bins)

    def desc(self) -> _abi.ReactionDesc:
        desc = _abi.ReactionDesc()
        for i, m in enumerate(self.masses):
            desc.masses[i] = m
        desc.beam_energy, desc.z_min, desc.z_max = self.beam_energy, self.z_min, self.z_max
        desc.ex_lo, desc.ex_hi = self.ex_lo, self.ex_hi
        desc.ex_inv_width, desc.theta_inv_width = self.ex_inv_width, self.theta_inv_width
        desc.has_target = 0 if self.eloss is None else 1
        desc.eloss_len = 0 if self.eloss is None else self.eloss.size
        if self.eloss is not None:  # (the array lives as long as the settings; the library copies it in the call)
            desc.eloss = self.eloss.ctypes.data_as(_abi.C.POINTER(_abi.C.c_double))
        desc.charge, desc.track, desc.observed_row, desc.source = self.charge, self.track, self.observed_row, SOURCES[self.source]
        desc.n_ex, desc.n_theta, desc.reserved = self.ex_bins, self.theta_bins, 0
        return desc


class ReactionSpectra:
    """The spectra of a call, u64 counts: ``truth`` [ex_bins, theta_bins] (every event with truth),
    ``truth_reconstructed`` (those of it with a record of status 0, at the truth values), ``reconstructed`` (status 0, at
    the reconstructed values), ``ex_response`` [truth bin, reconstructed bin] and ``outside`` [3] (the events of truth /
    reconstructed / ex_response with a value outside the bins).  Spectra of disjoint id ranges add."""

    def __init__(self, settings: ReactionSettings, cells=None):
        self.settings = settings
        cells = np.zeros(settings.n_cells, dtype=np.uint64) if cells is None else np.ascontiguousarray(cells, dtype=np.uint64)
        if cells.shape != (settings.n_cells,):
            raise ValueError(f"the spectra of these bins have {settings.n_cells} cells, got {cells.shape}")
        self.cells = cells
        n_ex, n_theta = settings.ex_bins, settings.theta_bins
        plane = n_ex * n_theta
        self.truth = cells[:plane].reshape(n_ex, n_theta)
        self.truth_reconstructed = cells[plane:2 * plane].reshape(n_ex, n_theta)
        self.reconstructed = cells[2 * plane:3 * plane].reshape(n_ex, n_theta)
        self.ex_response = cells[3 * plane:3 * plane + n_ex * n_ex].reshape(n_ex, n_ex)
        self.outside = cells[3 * plane + n_ex * n_ex:]

    @property
    def ex_edges(self) -> np.ndarray:
        s = self.settings
        return s.ex_lo + np.arange(s.ex_bins + 1) / s.ex_inv_width

    @property
    def theta_edges(self) -> np.ndarray:
        s = self.settings
        return np.arange(s.theta_bins + 1) / s.theta_inv_width

    def efficiency(self) -> np.ndarray:
        """truth_reconstructed / truth per (Ex, theta_cm) cell, NaN where no event was thrown."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.truth > 0, self.truth_reconstructed / self.truth.astype(np.float64), np.nan)

    def __add__(self, other: "ReactionSpectra") -> "ReactionSpectra":
        if not isinstance(other, ReactionSpectra):
            return NotImplemented
        if other.settings.token() != self.settings.token():
            raise ValueError("spectra of different settings do not add")
        return ReactionSpectra(self.settings, self.cells + other.cells)

    def __eq__(self, other) -> bool:
        return (isinstance(other, ReactionSpectra) and other.settings.token() == self.settings.token()
                and np.array_equal(self.cells, other.cells))

    __hash__ = None


def configure_reaction(ctx: _abi.Context, settings: ReactionSettings | None) -> None:
    """``attpc_reaction_configure`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, ReactionSettings, checked(ReactionSettings, settings, "settings"))


def reaction_last(ctx: _abi.Context, n_events: int) -> np.ndarray:
    """The records [n_events] (``REACTION_DTYPE``) of ctx's last trace-row call (``attpc_reaction_last``); RuntimeError
    if the stage or its source was off for it."""
    records = np.empty(int(n_events), dtype=REACTION_DTYPE)
    ctx.check(ctx.lib.attpc_reaction_last(ctx.handle, 0, len(records), _abi.iptr(records, _abi.ReactionRecord)),
              "attpc_reaction_last")
    return records


def spectra_last(ctx: _abi.Context, settings: ReactionSettings) -> ReactionSpectra:
    """The spectra of ctx's last trace-row call (``attpc_reaction_spectra_last``)."""
    spectra = ReactionSpectra(settings)
    ctx.check(ctx.lib.attpc_reaction_spectra_last(ctx.handle, spectra.cells.size, _abi.iptr(spectra.cells, _abi.C.c_uint64)),
              "attpc_reaction_spectra_last")
    return spectra


def source_on(ctx: _abi.Context, settings: ReactionSettings | None) -> bool:
    """The ctx holds what the stage reads: the estimates, and for the fit source the track fit."""
    return (settings is not None and ctx._tokens["reaction"] is not None and ctx._tokens["estimates"] is not None
            and (settings.source == "estimate" or ctx._tokens["fit"] is not None))


def reaction_result(ctx: _abi.Context, settings: ReactionSettings | None, n_events: int, records: bool = True) -> dict:
    """``{"reaction": records [n_events], "spectra": ReactionSpectra}`` of ctx's last trace-row call if the stage and
    its source are on, else {}."""
    if not source_on(ctx, settings):
        return {}
    out = {"reaction": reaction_last(ctx, n_events)} if records else {}
    return {**out, "spectra": spectra_last(ctx, settings)}


def records_to_reaction(settings: ReactionSettings, p4, vertex, status=None, fits=None, estimates=None, pid=None,
                        ctx: _abi.Context | None = None):
    """The stage alone on host arrays (``attpc_reaction_records``, the kernel of the fused path, no other configuration
    needed): ``fits`` (source "fit", ``detector.fit.FIT_DTYPE``) or ``estimates`` (source "estimate") [n, n_sim], ``pid``
    [n, n_sim] or None, the truth ``p4`` [n, n_rows, 4], ``vertex`` [n, 3] (m) and the kinematics ``status`` [n] (None:
    all 0) -> (records [n] ``REACTION_DTYPE``, ``ReactionSpectra``)."""
    if not isinstance(settings, ReactionSettings):
        raise TypeError("records_to_reaction needs a ReactionSettings")
    source = fits if settings.source == "fit" else estimates
    if source is None:
        raise ValueError(f"source {settings.source!r} needs the {'fits' if settings.source == 'fit' else 'estimates'}")
    dtype, ctype = (_abi.FIT_DTYPE, _abi.TrackFit) if settings.source == "fit" else (_abi.ESTIMATE_DTYPE, _abi.TrackEstimate)
    source = np.ascontiguousarray(source, dtype=dtype)
    if source.ndim != 2 or not 1 <= source.shape[1] <= _abi.MAX_SIM:
        raise ValueError(f"the source records must be [n, 1 <= n_sim <= {_abi.MAX_SIM}], got {source.shape}")
    n, n_sim = source.shape
    p4 = np.ascontiguousarray(p4, dtype=np.float64)
    vertex = np.ascontiguousarray(vertex, dtype=np.float64)
    if p4.ndim != 3 or p4.shape[0] != n or p4.shape[2] != 4 or not 4 <= p4.shape[1] <= _abi.MAX_ROWS:
        raise ValueError(f"p4 must be [{n}, 4 <= n_rows <= {_abi.MAX_ROWS}, 4], got {p4.shape}")
    if vertex.shape != (n, 3):
        raise ValueError(f"vertex must be [{n}, 3], got {vertex.shape}")
    if status is not None:
        status = np.ascontiguousarray(status, dtype=np.int32)
        if status.shape != (n,):
            raise ValueError(f"status must be [{n}], got {status.shape}")
    if pid is not None:
        pid = np.ascontiguousarray(pid, dtype=_abi.PID_DTYPE)
        if pid.shape != (n, n_sim):
            raise ValueError(f"pid must be [{n}, {n_sim}], got {pid.shape}")
    elif settings.track >= n_sim:
        raise ValueError(f"track {settings.track} is not a slot of {n_sim}")
    records = np.empty(n, dtype=REACTION_DTYPE)
    spectra = ReactionSpectra(settings)
    fit_arg = _abi.iptr(source, ctype) if settings.source == "fit" else None
    est_arg = _abi.iptr(source, ctype) if settings.source == "estimate" else None
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_reaction_records(ctx.handle, n, n_sim, p4.shape[1], settings.desc(), fit_arg, est_arg,
                                             _abi.iptr(pid, _abi.PidRecord), _abi.dptr(p4), _abi.dptr(vertex),
                                             _abi.iptr(status, _abi.C.c_int32), _abi.iptr(records, _abi.ReactionRecord),
                                             spectra.cells.size, _abi.iptr(spectra.cells, _abi.C.c_uint64)),
              "attpc_reaction_records")
    return records, spectra
