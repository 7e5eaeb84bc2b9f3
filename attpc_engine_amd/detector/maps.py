"""Run maps: pad and time-bucket hit maps summed over the events of a device-resident run (EXTENSION: the reference
hands out point clouds only).

The summary records (``detector.summary``) say what each event looked like; the first plots of an acceptance,
trigger-region or threshold study ask what the *detector* looked like over a run -- how often each pad fires, how much
charge it collects, where in the drift window the kept charge sits, and how that changes for the events a cut keeps.
These are sums over events of integers, and everything they need lies in HBM behind a chunk's scatter: a maps run
accumulates them there (``csrc/maps.hip``) and 172 KiB cross the link per call, whatever its length.  The contract is
written out in include/attpc_engine.h; ``tests/maps_reference.py`` restates it as plain loops.

``MapsSettings`` holds the validated settings; ``RunMaps`` the result (maps of disjoint id ranges add: ``a + b``);
``simulate_batch_maps`` is ``simulate_batch_summary`` with the maps on top (``attpc_det_run_maps``);
``clouds_to_maps`` accumulates any host cloud through the same kernel (``attpc_cloud_maps``); ``Engine.run_maps`` is
the fused run.
"""
from __future__ import annotations

import numpy as np

from .. import _abi
from ..outputs import SummaryArrays
from .parameters import Config
from .stage import configure_stage

OTHER_LABELS = 1 << _abi.MAX_SIM            # the mask bit of rows whose label is in no position of ``indices``
FULL_MASK = (OTHER_LABELS << 1) - 1         # every position and the other labels
ARRAYS = (("pad_events", np.uint64, _abi.NUM_PADS), ("pad_charge", np.int64, _abi.NUM_PADS),
          ("tb_events", np.uint64, _abi.NUM_TB), ("tb_rows", np.uint64, _abi.NUM_TB), ("tb_charge", np.int64, _abi.NUM_TB))


class MapsSettings:
    """The validated settings of a maps configuration (``attpc_maps_desc``): ``tracks`` -- the positions of ``indices``
    whose rows contribute (an iterable; None: every position) --, ``other_labels`` -- rows whose label is in no position
    contribute as well --, ``selected`` -- only the events that pass the configured selection contribute."""

    slot, call = "maps", "attpc_maps_configure"

    def __init__(self, tracks=None, other_labels: bool = False, selected: bool = False):
        for name, value in (("other_labels", other_labels), ("selected", selected)):
            if not isinstance(value, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, got {value!r}")
        if tracks is None:
            mask = OTHER_LABELS - 1
        else:
            positions = [int(s) for s in tracks]
            if any(not 0 <= s < _abi.MAX_SIM for s in positions):
                raise ValueError(f"track positions must be in [0, {_abi.MAX_SIM}), got {positions}")
            mask = 0
            for s in positions:
                mask |= 1 << s
        if other_labels:
            mask |= OTHER_LABELS
        if mask == 0:
            raise ValueError("the maps need at least one track position or other_labels")
        self.track_mask, self.selected = mask, bool(selected)

    def token(self):
        return (self.track_mask, self.selected)

    def desc(self) -> _abi.MapsDesc:
        return _abi.MapsDesc(self.track_mask, int(self.selected))


class RunMaps:
    """The maps of a call (``attpc_maps_out``): ``pad_events`` u64 [NUM_PADS] -- events with a counted row on the pad --,
    ``pad_charge`` i64 [NUM_PADS], ``tb_events`` u64 [512], ``tb_rows`` u64 [512], ``tb_charge`` i64 [512], ``n_events``
    (the events that contributed) and ``n_hit`` (those with a counted row).  The maps of disjoint id ranges add."""

    def __init__(self, pad_events=None, pad_charge=None, tb_events=None, tb_rows=None, tb_charge=None, n_events: int = 0,
                 n_hit: int = 0):
        given = (pad_events, pad_charge, tb_events, tb_rows, tb_charge)
        for (name, dtype, size), value in zip(ARRAYS, given):
            array = np.zeros(size, dtype=dtype) if value is None else np.ascontiguousarray(value, dtype=dtype)
            if array.shape != (size,):
                raise ValueError(f"{name} must have shape ({size},), got {array.shape}")
            setattr(self, name, array)
        self.n_events, self.n_hit = int(n_events), int(n_hit)

    def out(self) -> _abi.MapsOut:
        """The ``attpc_maps_out`` that points at this object's arrays (``absorb`` takes its counts back)."""
        C = _abi.C
        return _abi.MapsOut(_abi.iptr(self.pad_events, C.c_uint64), _abi.iptr(self.pad_charge, C.c_int64),
                            _abi.iptr(self.tb_events, C.c_uint64), _abi.iptr(self.tb_rows, C.c_uint64),
                            _abi.iptr(self.tb_charge, C.c_int64), 0, 0)

    def absorb(self, out: _abi.MapsOut) -> "RunMaps":
        self.n_events, self.n_hit = int(out.n_events), int(out.n_hit)
        return self

    def __add__(self, other: "RunMaps") -> "RunMaps":
        if not isinstance(other, RunMaps):
            return NotImplemented
        return RunMaps(*(getattr(self, name) + getattr(other, name) for name, _, _ in ARRAYS),
                       n_events=self.n_events + other.n_events, n_hit=self.n_hit + other.n_hit)

    def __radd__(self, other):
        return self if other == 0 else NotImplemented  # (sum() of shards starts at 0)

    def __eq__(self, other) -> bool:
        if not isinstance(other, RunMaps):
            return NotImplemented
        return (self.n_events, self.n_hit) == (other.n_events, other.n_hit) and all(
            np.array_equal(getattr(self, name), getattr(other, name)) for name, _, _ in ARRAYS)

    __hash__ = None

    def occupancy(self) -> np.ndarray:
        """``pad_events / n_events``: the fraction of the contributing events in which every pad fired (zeros for a run
        without events)."""
        if self.n_events == 0:
            return np.zeros(_abi.NUM_PADS)
        return self.pad_events / float(self.n_events)


def configure_maps(ctx: _abi.Context, maps: MapsSettings | None = None, **parameters) -> MapsSettings | None:
    """``attpc_maps_configure`` unless this ctx already holds the same settings (decided on their content): a
    ``MapsSettings`` or its keywords; neither turns the mode off."""
    if maps is not None and parameters:
        raise TypeError("give a MapsSettings or its keywords, not both")
    if parameters:
        maps = MapsSettings(**parameters)
    if maps is not None and not isinstance(maps, MapsSettings):
        raise TypeError(f"maps must be a MapsSettings, got {type(maps).__name__}")
    configure_stage(ctx, MapsSettings, maps)
    return maps


def simulate_batch_maps(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config, seed: int,
                        indices: list[int], maps: MapsSettings | None = None, selection=None, first_event: int = 0,
                        ctx: _abi.Context | None = None, min_electrons: int | None = None, straggling=None,
                        distortion=None) -> dict:
    """simulate() for n events with the clouds left on the device and accumulated there (``attpc_det_run_maps``; ``maps``
    default ``MapsSettings()``, with ``maps.selected`` the ``selection``) -> a dict: maps (``RunMaps``), events [n] and
    tracks [n, n_sim] (the records of all events, as ``simulate_batch_summary``), passed [n] bool (the events that
    contributed), stats.  ``straggling`` (a ``detector.straggling.StragglingSettings``; None = off): the track
    straggling.  ``distortion`` (a ``detector.distortion.DistortionMap``; None = off): the drift distortion."""
    from .distortion import configure_distortion
    from .luts import build_layout, species_for
    from .selection import Selection, configure_selection
    from .simulator import configure_detector
    from .straggling import configure_straggling
    from .summary import SummarySettings, configure_summary

    maps = MapsSettings() if maps is None else maps
    if not isinstance(maps, MapsSettings):
        raise TypeError(f"maps must be a MapsSettings, got {type(maps).__name__}")
    if maps.selected:
        if not isinstance(selection, Selection):
            raise ValueError("maps of the selected events need a Selection")
        selection.check_positions(len(indices))
    SummarySettings(min_electrons, config)  # (validated before the first library call)
    ctx = ctx or _abi.default_context()
    momenta = np.ascontiguousarray(momenta, dtype=np.float64)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    seed, first_event, n = _abi.check_id_range(seed, first_event, momenta.shape[0])
    indices = list(indices)
    keys = species_for(proton_numbers, mass_numbers, indices)
    configure_detector(config, keys, ctx)
    configure_straggling(ctx, straggling, config)
    configure_distortion(ctx, distortion, config)
    configure_summary(config, ctx, min_electrons)
    if maps.selected:
        configure_selection(ctx, selection)
    configure_maps(ctx, maps)
    layout = build_layout(proton_numbers, mass_numbers, indices, keys)
    stats, result, arrays = _abi.RunStats(), RunMaps(), SummaryArrays(n, n_sim=len(indices))
    passed, out = np.zeros(n, dtype=np.uint8), result.out()
    ctx.check(ctx.lib.attpc_det_run_maps(ctx.handle, seed, first_event, n, layout, _abi.dptr(momenta), _abi.dptr(vertices),
                                         arrays.out, _abi.iptr(passed, _abi.C.c_uint8), out, stats), "attpc_det_run_maps")
    return {"maps": result.absorb(out), "events": arrays.events, "tracks": arrays.tracks, "passed": passed.astype(bool),
            "stats": stats.as_dict()}


def clouds_to_maps(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, indices: list[int], ctx: _abi.Context,
                   n_rows: int | None = None):
    """The maps of any host cloud in CSR form through the device's kernel (``attpc_cloud_maps``; ``ctx`` configured with
    ``configure_summary``, ``configure_maps`` and, for maps of the selected events, ``configure_selection``), arguments
    as ``clouds_to_summary`` -> (maps ``RunMaps``, passed [n] bool: the events that contributed, events [n],
    tracks [n, len(indices)]; the track part of the records is empty)."""
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
    result, arrays = RunMaps(), SummaryArrays(n, n_sim=len(indices))
    passed, out = np.zeros(n, dtype=np.uint8), result.out()
    ctx.check(ctx.lib.attpc_cloud_maps(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(points),
                                       _abi.iptr(labels, _abi.C.c_int64), layout, arrays.out,
                                       _abi.iptr(passed, _abi.C.c_uint8), out), "attpc_cloud_maps")
    return (result.absorb(out), passed.astype(bool), *arrays.result())
