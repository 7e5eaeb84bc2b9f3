"""Selected delivery: only the events that pass a selection on their summary records cross the link (EXTENSION: the
reference hands out every event's point cloud).

An acceptance study decides from the event and track records (``detector.summary``) which events the detector would
accept -- enough pads lit, enough time buckets spanned, a track that reaches far enough out or stops inside the volume
-- and then wants those events' clouds or Spyral rows and nothing else.  A selected run evaluates the decision on the
device, between a chunk's summary kernels and its assembly: the rows of a rejected event are never put in event order,
converted or copied, and the records of every event still come back (the efficiency denominator).  The contract is
written out in include/attpc_engine.h; ``tests/selection_reference.py`` restates the predicate as plain loops.

``Selection`` holds the validated cuts and evaluates them on host records (``passes``: what a user applies to
``run_summary`` output); ``simulate_batch_selected`` is ``simulate_batch`` / ``simulate_batch_spyral`` of the events
that pass (``attpc_det_run_selected``); ``clouds_to_selection`` is the predicate on any host cloud through the same
kernels (``attpc_cloud_select``); ``Engine.run_selected`` is the fused run.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from ..outputs import SelectedArrays
from .parameters import Config

U32_MAX, I64_MIN, I64_MAX = (1 << 32) - 1, -(1 << 63), (1 << 63) - 1
# cut -> (kind, open bounds); the names are those of attpc_select_desc without _lo / _hi
_OPEN = {"u32": (0, U32_MAX), "i64": (I64_MIN, I64_MAX), "f64": (-math.inf, math.inf)}
EVENT_CUTS = {"n_kept": "u32", "n_pads": "u32", "tb_span": "u32", "charge": "i64"}
TRACK_CUTS = {"track_n_kept": "u32", "track_n_pads": "u32", "track_n_samples": "u32", "track_rho2_max": "f64",
              "track_end_tb": "f64", "track_end_rho2": "f64"}
ROW_KINDS = {"cloud": 3, "spyral": 8}


def _bounds(name: str, kind: str, cut):
    """``cut`` = None (absent), (lo, hi) with None for an open end -> validated (lo, hi)."""
    lo_open, hi_open = _OPEN[kind]
    if cut is None:
        return lo_open, hi_open
    try:
        lo, hi = cut
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (lo, hi) pair, got {cut!r}") from None
    lo = lo_open if lo is None else lo
    hi = hi_open if hi is None else hi
    if kind == "f64":
        lo, hi = float(lo), float(hi)
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError(f"{name}: a NaN bound")
    else:
        if int(lo) != lo or int(hi) != hi:
            raise ValueError(f"{name}: bounds must be integers, got {cut!r}")
        lo, hi = int(lo), int(hi)
        if not (lo_open <= lo <= hi_open and lo_open <= hi <= hi_open):
            raise ValueError(f"{name}: bounds outside [{lo_open}, {hi_open}], got {cut!r}")
    if lo > hi:
        raise ValueError(f"{name}: lo > hi in {cut!r}")
    return lo, hi


class Selection:
    """A conjunction of inclusive ranges on the fields of an event's summary records (include/attpc_engine.h).

    Event cuts ``n_kept``, ``n_pads``, ``tb_span`` (``tb_max - tb_min + 1``, 0 without a kept row), ``charge``; track
    cuts ``track_n_kept``, ``track_n_pads``, ``track_n_samples``, ``track_rho2_max`` (mm^2), ``track_end_tb``,
    ``track_end_rho2`` (m^2), applied to the positions of the simulated nuclei in ``tracks`` (an iterable of positions
    of ``indices``, or the bit mask ``track_mask``).  Every cut is a ``(lo, hi)`` pair, None for an open end; a cut
    that is absent (or open at both ends) is not evaluated, so it lets a NaN end point through, while an evaluated
    range is false for NaN.  The event passes iff its event cuts hold and at least ``min_tracks`` masked positions pass
    all track cuts (default: all masked positions; 1 = any; 0 = the track cuts decide nothing)."""

    def __init__(self, *, tracks=None, track_mask: int | None = None, min_tracks: int | None = None, **cuts):
        unknown = set(cuts) - set(EVENT_CUTS) - set(TRACK_CUTS)
        if unknown:
            raise TypeError(f"unknown cuts {sorted(unknown)}; known: {sorted(EVENT_CUTS) + sorted(TRACK_CUTS)}")
        if tracks is not None and track_mask is not None:
            raise TypeError("give tracks or track_mask, not both")
        if tracks is not None:
            positions = [int(s) for s in tracks]
            if any(s < 0 for s in positions):
                raise ValueError(f"track positions must be >= 0, got {positions}")
            track_mask = 0
            for s in positions:
                track_mask |= 1 << s
        track_mask = 0 if track_mask is None else int(track_mask)
        if track_mask < 0 or track_mask >> _abi.MAX_SIM:
            raise ValueError(f"track_mask {track_mask:#x} has bits at or above {_abi.MAX_SIM}")
        self.track_mask = track_mask
        n_masked = bin(track_mask).count("1")
        self.min_tracks = n_masked if min_tracks is None else int(min_tracks)
        if not 0 <= self.min_tracks <= n_masked:
            raise ValueError(f"min_tracks {min_tracks} outside [0, {n_masked}] (the masked positions)")
        self.bounds = {name: _bounds(name, kind, cuts.get(name)) for name, kind in {**EVENT_CUTS, **TRACK_CUTS}.items()}

    def evaluated(self, name: str) -> bool:
        kind = {**EVENT_CUTS, **TRACK_CUTS}[name]
        return self.bounds[name] != _OPEN[kind]

    def token(self):
        return (self.track_mask, self.min_tracks, tuple(sorted(self.bounds.items())))

    def desc(self) -> _abi.SelectDesc:
        d = _abi.SelectDesc()
        d.track_mask, d.min_tracks = self.track_mask, self.min_tracks
        for name, (lo, hi) in self.bounds.items():
            setattr(d, name + "_lo", lo)
            setattr(d, name + "_hi", hi)
        return d

    def check_positions(self, n_sim: int) -> None:
        if self.track_mask >> n_sim:
            raise ValueError(f"track_mask {self.track_mask:#x} names positions at or above n_sim = {n_sim}")

    def passes(self, events: np.ndarray, tracks: np.ndarray) -> np.ndarray:
        """The predicate on host records: ``events`` [n] and ``tracks`` [n, n_sim] as ``run_summary`` returns them ->
        bool [n]."""
        events, tracks = np.asarray(events), np.asarray(tracks)
        n = len(events)
        tracks = tracks.reshape(n, -1)
        self.check_positions(tracks.shape[1])

        def within(name, values):
            if not self.evaluated(name):
                return np.ones(values.shape, dtype=bool)
            lo, hi = self.bounds[name]
            return (values >= lo) & (values <= hi)

        kept = events["n_kept"].astype(np.int64)
        span = np.where(kept > 0, events["tb_max"].astype(np.int64) - events["tb_min"].astype(np.int64) + 1, 0)
        ok = (within("n_kept", kept) & within("n_pads", events["n_pads"].astype(np.int64)) & within("tb_span", span)
              & within("charge", events["charge"].astype(np.int64)))
        good = np.zeros(n, dtype=np.int64)
        for s in range(tracks.shape[1]):
            if not (self.track_mask >> s) & 1:
                continue
            t = tracks[:, s]
            with np.errstate(invalid="ignore", over="ignore"):
                end_rho2 = t["end_x"] * t["end_x"] + t["end_y"] * t["end_y"]  # (two rounded products, then the sum)
                good += (within("track_n_kept", t["n_kept"].astype(np.int64))
                         & within("track_n_pads", t["n_pads"].astype(np.int64))
                         & within("track_n_samples", t["n_samples"].astype(np.int64))
                         & within("track_rho2_max", t["rho2_max"]) & within("track_end_tb", t["end_tb"])
                         & within("track_end_rho2", end_rho2))
        return ok & (good >= self.min_tracks)


def _selection(selection, cuts) -> Selection:
    if selection is not None and cuts:
        raise TypeError("give a Selection or its keywords, not both")
    if selection is None:
        return Selection(**cuts)
    if not isinstance(selection, Selection):
        raise TypeError(f"selection must be a Selection, got {type(selection).__name__}")
    return selection


def configure_selection(ctx: _abi.Context, selection: Selection | None = None, **cuts) -> Selection:
    """``attpc_select_configure`` unless this ctx already holds the same selection (decided on its content).  The
    settings are validated here, before any library call."""
    selection = _selection(selection, cuts)
    ctx.configure("select", selection.token(), "attpc_select_configure", selection.desc())
    return selection


def simulate_batch_selected(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config,
                            seed: int, indices: list[int], selection: Selection, kind: str = "cloud",
                            first_event: int = 0, ctx: _abi.Context | None = None, min_electrons: int | None = None,
                            response: np.ndarray | None = None, capacity_per_event: int | None = None,
                            straggling=None, distortion=None) -> dict:
    """simulate() for n events, delivering only the events that pass ``selection`` (``attpc_det_run_selected``):
    ``kind`` "cloud" -> points [P,3] as ``simulate_batch``, "spyral" -> rows [P',8] as ``simulate_batch_spyral``.
    Returns a dict: passed [n] bool, n_passed, n_rows, offsets [n+1] (a rejected event is an empty range), points or
    rows, labels, event_points [n] (cloud rows of every event before selection and threshold), events [n] and tracks
    [n, n_sim] (the records of all events, as ``simulate_batch_summary`` with ``min_electrons``), stats.  ``straggling``
    (a ``detector.straggling.StragglingSettings``; None = off): the track straggling.  ``distortion`` (a
    ``detector.distortion.DistortionMap``; None = off): the drift distortion; a cut on a track's end point sees the
    shifted, apparent one."""
    from .simulator import configure_spyral, run_batch
    from .summary import SummarySettings, configure_summary

    if kind not in ROW_KINDS:
        raise ValueError(f"kind must be one of {sorted(ROW_KINDS)}, got {kind!r}")
    selection = _selection(selection, {})
    selection.check_positions(len(indices))
    SummarySettings(min_electrons, config)  # (validated before the first library call)

    def configure(c):
        configure_summary(config, c, min_electrons)
        if kind == "spyral":
            configure_spyral(config, c, response)
        configure_selection(c, selection)

    per_event = capacity_per_event if capacity_per_event is not None else (16384 if kind == "cloud" else 8192)
    arrays, stats = run_batch("attpc_det_run_selected", momenta, vertices, proton_numbers, mass_numbers, config, seed,
                              list(indices), first_event, ctx, per_event, configure=configure, straggling=straggling,
                              distortion=distortion,
                              holder=SelectedArrays,
                              width=ROW_KINDS[kind], n_sim=len(indices), slack=1024)
    return selected_result(arrays, kind, stats.as_dict())


def selected_result(arrays: SelectedArrays, kind: str, stats: dict) -> dict:
    """The part of a selected call's result dict that the fused and the file-driven run share."""
    offsets, rows, labels = arrays.result()
    return {"passed": arrays.passed.astype(bool), "n_passed": int(arrays.out.n_passed), "n_rows": int(arrays.out.n_rows),
            "offsets": offsets, ("points" if kind == "cloud" else "rows"): rows, "labels": labels,
            "event_points": arrays.event_points, "events": arrays.events, "tracks": arrays.tracks,
            "stats": stats}


def clouds_to_selection(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, indices: list[int],
                        ctx: _abi.Context, n_rows: int | None = None):
    """The predicate on any host cloud in CSR form through the device's kernels (``attpc_cloud_select``; ``ctx``
    configured with ``configure_summary`` and ``configure_selection``), arguments as ``clouds_to_summary`` ->
    (passed [n] bool, events [n], tracks [n, len(indices)]; the track part of the records is empty)."""
    from ..outputs import SummaryArrays

    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0:
        raise ValueError("offsets needs n_events + 1 entries")
    if len(points) != len(labels) or (n and offsets[-1] > len(points)):
        raise ValueError("points / labels do not hold the rows the offsets name")
    indices = [int(i) for i in indices]
    if len(indices) > _abi.MAX_SIM:
        raise ValueError(f"at most {_abi.MAX_SIM} indices, got {len(indices)}")
    layout = _abi.EventLayout()
    layout.n_rows = int(n_rows) if n_rows is not None else max(indices, default=0) + 1
    layout.n_sim = len(indices)
    for s, row in enumerate(indices):
        layout.indices[s] = row
    arrays = SummaryArrays(n, n_sim=len(indices))
    passed = np.zeros(n, dtype=np.uint8)
    ctx.check(ctx.lib.attpc_cloud_select(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(points),
                                         _abi.iptr(labels, _abi.C.c_int64), layout, arrays.out,
                                         _abi.iptr(passed, _abi.C.c_uint8)), "attpc_cloud_select")
    return (passed.astype(bool), *arrays.result())
