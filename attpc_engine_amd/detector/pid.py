"""Particle identification: which position's species a track is, decided on the device by polygon gates in the plane
of its estimate record's dE/dx against B rho (``attpc_trace_configure_pid``; the contract is in
include/attpc_engine.h, "particle identification", ``tests/pid_reference.py`` restates it).  The stage sits behind the
estimate kernel and in front of the track fit: the fit of a slot then uses the species of the position the slot was
assigned, and a slot no gate holds is not fitted (``FIT_NO_PID``).  With the clustering in ``match="rank"`` the chain
clustering -> joining -> thinning -> estimates -> PID -> fit uses no truth label anywhere.  The stage is opt-in
(``PidSettings``, ``pid=``) and does nothing unless the estimates are on.  ``run_trace_rows`` and ``run_estimates``
carry ``"pid"`` [n, n_sim] (``PID_DTYPE``) when both are on; ``estimates_to_pid`` is the stage alone on any host
estimate records, ``detector.fit.rows_to_fit(..., pid=)`` the fit behind it.  ``Gate.from_band`` makes a gate from the
records of a truth-labelled calibration run, in plain numpy; gates drawn interactively or read from Spyral's files are
not supported.  The writers, ``run_simulation`` and ``run_fused`` do not take ``pid=`` (nor ``clustering=``) and do not
store the records."""
from __future__ import annotations

import numpy as np

from .. import _abi
from .._abi import (FIT_NO_PID, PID_AMBIGUOUS, PID_ANY, PID_DTYPE, PID_MAX_VERTICES, PID_NO_ESTIMATE, PID_NONE,  # noqa: F401
                    PID_OWN, PID_TAKEN)
from .stage import checked, configure_stage

STATUS_BITS = {"NO_ESTIMATE": PID_NO_ESTIMATE, "NONE": PID_NONE, "TAKEN": PID_TAKEN, "AMBIGUOUS": PID_AMBIGUOUS}
MODES = {"any": PID_ANY, "own": PID_OWN}


class Gate:
    """A polygon in the plane (B rho in T m, dE/dx in the units of the estimate records): ``vertices`` [3 .. 32, 2],
    finite.  The closing edge from the last vertex to the first is implied."""

    def __init__(self, vertices):
        try:
            v = np.array(vertices, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("a gate's vertices must be numbers [n, 2]") from None
        if v.ndim != 2 or v.shape[1] != 2 or not 3 <= len(v) <= PID_MAX_VERTICES:
            raise ValueError(f"a gate has 3 .. {PID_MAX_VERTICES} vertices (x, y), got an array of shape {v.shape}")
        if not np.all(np.isfinite(v)):
            raise ValueError("a gate's vertices must be finite")
        self.vertices = v
        self.vertices.setflags(write=False)

    def __len__(self) -> int:
        return len(self.vertices)

    def token(self):
        return self.vertices.tobytes()

    @classmethod
    def rectangle(cls, brho, dedx) -> "Gate":
        """The rectangle ``brho`` = (lo, hi) by ``dedx`` = (lo, hi)."""
        (x0, x1), (y0, y1) = brho, dedx
        return cls([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])

    @classmethod
    def from_band(cls, brho, dedx, bins: int = 12, coverage=(0.02, 0.98)) -> "Gate":
        """The band of a sample: ``bins`` (1 .. 15) quantile bins in B rho, and per bin the ``coverage`` quantiles of
        dE/dx as the lower and the upper side of the polygon -- a vertex per bin edge and side, placed so that every
        point of a bin between its two quantiles is inside; 2 * bins + 2 <= 32 vertices.  Records with a NaN, an infinity or a value <= 0
        in either quantity are ignored (the device does not test them).  This is how gates are made from the estimates
        of a truth-labelled calibration run (``estimates["brho"][:, p]``, ``estimates["dedx"][:, p]``)."""
        if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 15:
            raise ValueError(f"bins must be an integer in 1 .. 15, got {bins!r}")
        lo, hi = (float(c) for c in coverage)
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f"coverage must be two shares 0 <= lo < hi <= 1, got {coverage!r}")
        x, y = np.asarray(brho, dtype=np.float64).ravel(), np.asarray(dedx, dtype=np.float64).ravel()
        if x.shape != y.shape:
            raise ValueError(f"{x.size} values of B rho, {y.size} of dE/dx")
        keep = np.isfinite(x) & np.isfinite(y) & (x > 0.0) & (y > 0.0)
        x, y = x[keep], y[keep]
        if len(x) < 2 * bins:
            raise ValueError(f"a band of {bins} bins needs at least {2 * bins} usable records, got {len(x)}")
        edges = np.quantile(x, np.linspace(0.0, 1.0, bins + 1))
        edges[0], edges[-1] = np.nextafter(edges[0], -np.inf), np.nextafter(edges[-1], np.inf)  # (the extremes inside)
        if np.any(np.diff(edges) <= 0.0):
            raise ValueError("the sample's B rho has too few distinct values for this many bins")
        which = np.clip(np.searchsorted(edges, x, side="right") - 1, 0, bins - 1)
        lower, upper = np.empty(bins), np.empty(bins)
        for b in range(bins):
            values = y[which == b]
            if len(values) == 0:
                raise ValueError("a bin of the band is empty")
            lower[b], upper[b] = np.quantile(values, lo), np.quantile(values, hi)
            if upper[b] <= lower[b]:  # (a bin of one value: a sliver around it)
                lower[b], upper[b] = np.nextafter(lower[b], -np.inf), np.nextafter(upper[b], np.inf)
        # one vertex per bin edge on either side, at the outer of the two neighbouring bins' quantiles: the side between
        # two edges then lies outside the bin's own quantile, so the polygon holds every point between them
        low_x, low_y = [edges[0]], [lower[0]]
        for b in range(1, bins):
            low_x.append(edges[b])
            low_y.append(min(lower[b - 1], lower[b]))
        low_x.append(edges[-1])
        low_y.append(lower[-1])
        up_x, up_y = [edges[-1]], [upper[-1]]
        for b in range(bins - 1, 0, -1):
            up_x.append(edges[b])
            up_y.append(max(upper[b - 1], upper[b]))
        up_x.append(edges[0])
        up_y.append(upper[0])
        return cls(np.column_stack([low_x + up_x, low_y + up_y]))

    def contains(self, brho, dedx) -> np.ndarray:
        """The contract's inside test in numpy (the edge rule of the header), for host-side use; untestable points
        (not finite or <= 0) are outside."""
        x, y = np.broadcast_arrays(np.asarray(brho, dtype=np.float64), np.asarray(dedx, dtype=np.float64))
        inside = np.zeros(x.shape, dtype=bool)
        v = self.vertices
        with np.errstate(invalid="ignore"):
            for i in range(len(v)):
                (x0, y0), (x1, y1) = v[i], v[(i + 1) % len(v)]
                d = (x1 - x0) * (y - y0) - (x - x0) * (y1 - y0)
                inside ^= ((y0 > y) != (y1 > y)) & (d != 0.0) & ((d > 0.0) == (y1 > y0))
            return inside & np.isfinite(x) & np.isfinite(y) & (x > 0.0) & (y > 0.0)


class PidSettings:
    """The validated settings of the particle identification (``attpc_pid_desc``, include/attpc_engine.h): ``gates``, a
    sequence by position or a dict {position: gate} of ``Gate`` (or vertex arrays), None = no gate, the position is never
    assigned; ``mode``, "any" (a slot takes the lowest free position whose gate holds it) or "own" (slot k is tested
    against the gate of position k only: the efficiency of a gate on a truth-labelled run)."""

    slot, call = "pid", "attpc_trace_configure_pid"

    def __init__(self, gates, mode: str = "any"):
        if not isinstance(mode, str) or mode not in MODES:
            raise ValueError(f"pid mode must be 'any' or 'own', got {mode!r}")
        self.mode = mode
        if isinstance(gates, dict):
            for key in gates:
                if isinstance(key, (bool, np.bool_)) or not isinstance(key, (int, np.integer)) or not 0 <= key < _abi.MAX_SIM:
                    raise ValueError(f"a gate's position must be an integer in 0 .. {_abi.MAX_SIM - 1}, got {key!r}")
            listed = [gates.get(p) for p in range(_abi.MAX_SIM)]
        elif isinstance(gates, (list, tuple)):
            if len(gates) > _abi.MAX_SIM:
                raise ValueError(f"at most {_abi.MAX_SIM} gates, got {len(gates)}")
            listed = list(gates) + [None] * (_abi.MAX_SIM - len(gates))
        else:
            raise TypeError(f"gates must be a sequence or a dict by position, got {type(gates).__name__}")
        self.gates = tuple(g if g is None or isinstance(g, Gate) else Gate(g) for g in listed)

    def token(self):
        return (self.mode, tuple(None if g is None else g.token() for g in self.gates))

    def desc(self) -> _abi.PidDesc:
        desc = _abi.PidDesc()
        desc.mode, desc.reserved = MODES[self.mode], 0
        vertices = np.zeros((_abi.MAX_SIM, PID_MAX_VERTICES, 2), dtype=np.float64)
        for p, gate in enumerate(self.gates):
            desc.n_vertices[p] = 0 if gate is None else len(gate)
            if gate is not None:
                vertices[p, :len(gate)] = gate.vertices
        _abi.C.memmove(desc.vertices, vertices.ctypes.data, vertices.nbytes)
        return desc


def configure_pid(ctx: _abi.Context, pid: PidSettings | None) -> None:
    """``attpc_trace_configure_pid`` unless this ctx already holds the same settings (``None``: the stage off)."""
    configure_stage(ctx, PidSettings, checked(PidSettings, pid, "pid"))


def pid_last(ctx: _abi.Context, n_events: int, n_sim: int) -> np.ndarray:
    """The records [n_events, n_sim] (``PID_DTYPE``) of ctx's last trace-row call (``attpc_pid_last``); RuntimeError if
    this stage or the estimates were off for it."""
    records = np.empty((int(n_events), int(n_sim)), dtype=PID_DTYPE)
    ctx.check(ctx.lib.attpc_pid_last(ctx.handle, 0, len(records), _abi.iptr(records, _abi.PidRecord)), "attpc_pid_last")
    return records


def pid_result(ctx: _abi.Context, n_events: int, n_sim: int, n_rows=None) -> dict:
    """``{"pid": records [n_events, n_sim]}`` of ctx's last trace-row call if the ctx holds both the estimates and this
    stage, else {}."""
    if ctx._tokens["pid"] is None or ctx._tokens["estimates"] is None:
        return {}
    return {"pid": pid_last(ctx, n_events, n_sim)}


def estimates_to_pid(estimates, settings: PidSettings, ctx: _abi.Context | None = None) -> np.ndarray:
    """The stage alone on any host estimate records [n, n_sim] (``ESTIMATE_DTYPE``; ``attpc_estimates_pid``, the kernel
    of the fused path, no other configuration needed) -> records [n, n_sim] (``PID_DTYPE``).  There is no layout here,
    so ``species`` is -1 throughout."""
    if not isinstance(settings, PidSettings):
        raise TypeError("estimates_to_pid needs a PidSettings")
    estimates = np.ascontiguousarray(estimates, dtype=_abi.ESTIMATE_DTYPE)
    if estimates.ndim != 2 or estimates.shape[1] > _abi.MAX_SIM:
        raise ValueError(f"estimates must be [n, n_sim <= {_abi.MAX_SIM}], got {estimates.shape}")
    n, n_sim = estimates.shape
    records = np.empty((n, n_sim), dtype=PID_DTYPE)
    ctx = ctx or _abi.default_context()
    ctx.check(ctx.lib.attpc_estimates_pid(ctx.handle, n, n_sim, _abi.iptr(estimates, _abi.TrackEstimate), settings.desc(),
                                          _abi.iptr(records, _abi.PidRecord)), "attpc_estimates_pid")
    return records


def by_position(records, pid):
    """Records [n, n_sim] of any per-slot dtype with a ``status`` field (estimates, fits) re-ordered by the position the
    identification gave: -> (out [n, n_sim] with row p taken from the slot that got position p and a record of zeros
    with the EMPTY status bit (1) elsewhere, slot_of_position [n, n_sim], -1 where no slot got it).  The fits and the
    estimates of a rank-labelled run then compare position by position with those of a truth-labelled one."""
    records, pid = np.asarray(records), np.asarray(pid)
    if records.shape != pid.shape or records.ndim != 2:
        raise ValueError(f"records {records.shape} and pid {pid.shape} must both be [n, n_sim]")
    n, n_sim = records.shape
    out = np.zeros((n, n_sim), dtype=records.dtype)
    out["status"] = 1
    for name in out.dtype.names:
        if out.dtype[name].base.kind == "f":
            out[name] = np.nan
    slot_of_position = np.full((n, n_sim), -1, dtype=np.int64)
    position = pid["position"]
    events, slots = np.nonzero((position >= 0) & (position < n_sim))
    slot_of_position[events, position[events, slots]] = slots
    out[events, position[events, slots]] = records[events, slots]
    return out, slot_of_position
