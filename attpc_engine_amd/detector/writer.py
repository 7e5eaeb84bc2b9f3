"""Point-cloud writers (reference ``detector/writer.py``).

``SimulationWriter`` is the protocol ``run_simulation`` drives (write once per non-empty
event in event order, then close).  ``SpyralWriter`` produces the Spyral layout; the
per-point response scaling / row conversion runs on the device (``attpc_spyral_rows``; the
fused path ``Engine.run_spyral`` also thresholds and z-sorts there).  h5py is imported lazily;
without it the same datasets go to one ``.npz`` per run file, after a warning (the HDF5 layout is
"parity unpinned" in this container; tests drive it through a stand-in module).
"""
from __future__ import annotations

from pathlib import Path
from typing import Protocol

import numpy as np

from .. import _abi
from .parameters import Config
from .response import get_response
from .traces import (TRACE_PACK_FORMAT, NoiseSettings, ReadoutSettings, TraceChain, _packed_flag, clouds_to_trace_rows,
                     clouds_to_traces, pack_traces_host, trace_settings, unpack_traces)


class SimulationWriter(Protocol):
    """write(data [P,3], labels [P], config, event_number); get_directory_name(); close()
    (reference writer.py:12-58)."""

    def write(self, data: np.ndarray, labels: np.ndarray, config: Config, event_number: int) -> None: ...

    def get_directory_name(self) -> Path: ...

    def close(self) -> None: ...


def convert_to_spyral(points: np.ndarray, window_edge: int, mm_edge: int, length: float,
                      response: np.ndarray, pad_centers: np.ndarray, pad_sizes: np.ndarray,
                      ctx: _abi.Context | None = None) -> np.ndarray:
    """[P,3] (pad, tb, electrons) -> [P,8] (x mm, y mm, z mm, amplitude, integral, pad, tb,
    pad scale) on the device (reference writer.py:61-112)."""
    ctx = ctx or _abi.default_context()
    points = np.ascontiguousarray(points, dtype=np.float64)
    response = np.ascontiguousarray(response, dtype=np.float64)
    centers = np.ascontiguousarray(pad_centers, dtype=np.float64)
    sizes = np.ascontiguousarray(pad_sizes, dtype=np.float64)
    rows = np.empty((len(points), 8), dtype=np.float64)
    if len(points) == 0:
        return rows
    ctx.check(
        ctx.lib.attpc_spyral_rows(
            ctx.handle, len(points), _abi.dptr(points), _abi.dptr(response), _abi.dptr(centers),
            _abi.dptr(sizes), len(sizes), int(window_edge), int(mm_edge), float(length),
            _abi.dptr(rows),
        ),
        "attpc_spyral_rows",
    )
    return rows


class _NpzRunFile:
    """Fallback container when h5py is absent: same dataset names/attrs, one npz per run."""

    def __init__(self, path: Path, group: str = "cloud"):
        self.path = path.with_suffix(".npz")
        self.group = group
        self.arrays: dict[str, np.ndarray] = {}

    def create_dataset(self, name: str, data: np.ndarray, attrs: dict | None = None) -> None:
        self.arrays[f"{self.group}/{name}"] = np.asarray(data)
        for key, value in (attrs or {}).items():
            self.arrays[f"{self.group}/{name}@{key}"] = np.asarray(value)

    def set_attr(self, key: str, value) -> None:
        self.arrays[f"{self.group}@{key}"] = np.asarray(value)

    def close(self) -> None:
        np.savez_compressed(self.path, **self.arrays)


class _H5RunFile:
    def __init__(self, path: Path, h5, group: str = "cloud"):
        self.file = h5.File(path, "w")
        self.group = self.file.create_group(group)

    def create_dataset(self, name: str, data: np.ndarray, attrs: dict | None = None) -> None:
        dset = self.group.create_dataset(name, data=data)
        for key, value in (attrs or {}).items():
            dset.attrs[key] = value

    def set_attr(self, key: str, value) -> None:
        self.group.attrs[key] = value

    def close(self) -> None:
        self.file.close()


class _RollingWriter:
    """The file-rolling part of SpyralWriter and TraceWriter: ``run_%04d.h5`` (or ``.npz`` without h5py) with one group
    named ``group``, a new file after ``max_events_per_file`` events (reference writer.py:214-218), and min_event /
    max_event on the group when a file is closed."""

    group = "cloud"

    def __init__(self, directory_path: Path, max_events_per_file: int, first_run_number: int, npz_fallback: bool):
        self.directory_path = Path(directory_path)
        self.npz_fallback = npz_fallback  # without h5py: warn and write .npz (True) or raise (False)
        self.max_events_per_file = max_events_per_file
        self.run_number = first_run_number
        self.starting_event = 0
        self.last_event = 0
        self.events_written = 0
        self.file = self._open(self.run_number)

    def _open(self, run_number: int):
        from ..io import hdf5_or_fallback

        path = self.directory_path / f"run_{run_number:04d}.h5"
        h5py = hdf5_or_fallback(path, self.npz_fallback)
        return _H5RunFile(path, h5py, self.group) if h5py is not None else _NpzRunFile(path, self.group)

    def create_next_file(self) -> None:
        self.run_number += 1
        self.file = self._open(self.run_number)

    def _begin_event(self, event_number: int) -> None:
        """Roll over to the next file if this one is full."""
        if self.events_written == self.max_events_per_file:
            self.close()
            self.create_next_file()
            self.starting_event = event_number
            self.events_written = 0

    def _end_event(self, event_number: int) -> None:
        self.last_event = event_number
        self.events_written += 1

    def set_number_of_events(self) -> None:
        self.file.set_attr("min_event", self.starting_event)
        self.file.set_attr("max_event", self.last_event)

    def get_directory_name(self) -> Path:
        return self.directory_path

    def close(self) -> None:
        self.set_number_of_events()
        self.file.close()


class SpyralWriter(_RollingWriter):
    """Spyral-format output split into files of ``max_events_per_file`` events
    (reference writer.py:115-281): ``run_%04d.h5`` / group ``cloud`` / ``cloud_{event}``
    [P,8] + ``labels_{event}``, attrs orig_run, orig_event, ic_* = -1, and min_event /
    max_event on the group."""

    def __init__(self, directory_path: Path, config: Config, max_events_per_file: int = 5_000,
                 first_run_number: int = 0, npz_fallback: bool = True, *, peaks=None, baseline=None,
                 noise_seed: int = 0, gain=None, common_mode=None, correction=None, **trace_kwargs):
        """``peaks`` (keyword only; a ``detector.traces.PeakSettings``, default None = the reference's writer: one row
        per cloud point): the rows are the peaks of the event's digitised pad traces instead (EXTENSION, trace rows of
        include/attpc_engine.h), made on the device with the trace settings ``trace_kwargs`` (response, threshold,
        offset, noise_sigma / noise_table, pedestals, noise_stream, readout, readout_pads as
        ``detector.traces.configure_traces`` takes them); ``noise_seed`` keys the draws of ``write``, a run keys them on
        its own seed.  ``baseline`` (a ``detector.traces.BaselineSettings``, default None = the peaks stand on the
        configured pedestals): Spyral's Fourier baseline is removed from the traces first.  ``gain`` (a
        ``detector.traces.GainSettings``, default None = off): the micromegas gain of the traces, keyed like the noise.
        ``common_mode`` (a ``detector.traces.CommonModeSettings``, default None = off): the common-mode noise of the
        traces, keyed the same way.  ``correction`` (a ``detector.correction.CorrectionSettings``, default None = off):
        the drift correction of the rows, which are then stored corrected and in ascending corrected z.  The files have
        the same datasets either way."""
        self.response = get_response(config).copy()
        self.peaks, self.baseline, self.gain, self.chain = peaks, baseline, gain, None
        self.common_mode, self.correction = common_mode, correction
        if peaks is None and (trace_kwargs or noise_seed or baseline is not None or gain is not None or common_mode is not None
                              or correction is not None):
            given = (sorted(trace_kwargs) + (["noise_seed"] if noise_seed else []) + (["baseline"] if baseline is not None else [])
                     + (["gain"] if gain is not None else []) + (["common_mode"] if common_mode is not None else [])
                     + (["correction"] if correction is not None else []))
            raise TypeError(f"SpyralWriter takes trace settings only with peaks=: {given}")
        if peaks is not None:  # (the chain of a trace-row run; ``write`` uses it too)
            self.chain = TraceChain.from_kwargs(config, **trace_kwargs).replace(peaks=peaks, baseline=baseline, gain=gain,
                                                                                common_mode=common_mode, correction=correction)
            self.noise_seed = _abi.check_id_range(noise_seed, 0, 0)[0]
        self._trace_kwargs = dict(trace_kwargs)
        super().__init__(directory_path, max_events_per_file, first_run_number, npz_fallback)

    def trace_kwargs(self) -> dict:
        """The trace settings a writer with ``peaks`` was given, as ``configure_traces`` takes them."""
        return dict(self._trace_kwargs)

    def write(self, data: np.ndarray, labels: np.ndarray, config: Config, event_number: int) -> None:
        """[P,3] cloud -> Spyral rows (device), ADC threshold, z-sort, datasets (writer.py:194-255).  With ``peaks``:
        the cloud's traces and their peaks on the device (``clouds_to_trace_rows``) -> datasets."""
        if config.pad_centers is None:
            raise ValueError("Pad centers are not assigned at write!")
        if self.peaks is not None:
            ctx = _abi.default_context()
            self.chain.replace(config=config).configure(ctx, rows=True, keep=("trigger",))
            data = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, 3)
            _, rows, out_labels, _ = clouds_to_trace_rows(np.array([0, len(data)], dtype=np.int64), data, labels, ctx,
                                                          seed=self.noise_seed, first_event=event_number)
            self.write_rows(rows, out_labels, event_number, presorted=True)
            return
        rows = convert_to_spyral(
            data, config.elec_params.windows_edge, config.elec_params.micromegas_edge,
            config.det_params.length, self.response, config.pad_centers, config.pad_sizes,
        )
        keep = rows[:, 3] > config.elec_params.adc_threshold  # writer.py:232-234
        self.write_rows(rows[keep], labels[keep], event_number)

    def write_rows(self, rows: np.ndarray, labels: np.ndarray, event_number: int, presorted: bool = False) -> None:
        """Already converted and thresholded rows [P',8]: z-sort (writer.py:236-238) unless the rows
        come ``presorted`` from the device (``Engine.run_spyral``), file roll-over (:214-218), datasets
        and attributes (:240-251)."""
        self._begin_event(event_number)
        if not presorted:
            order = np.argsort(rows[:, 2])
            rows, labels = rows[order], labels[order]
        self.file.create_dataset(
            f"cloud_{event_number}", rows,
            {"orig_run": self.run_number, "orig_event": event_number, "ic_amplitude": -1.0,
             "ic_multiplicity": -1.0, "ic_integral": -1.0, "ic_centroid": -1.0},
        )
        self.file.create_dataset(f"labels_{event_number}", labels)
        self._end_event(event_number)


class TraceWriter(_RollingWriter):
    """Digitised GET pad traces (EXTENSION: the reference writes point clouds only) split into files of
    ``max_events_per_file`` events, with SpyralWriter's roll-over and ``.npz`` fallback: ``run_%04d.h5`` / group
    ``trace`` / per event ``trace_{event}`` [R,512] int16, ``pads_{event}`` [R] int32, ``labels_{event}`` [R] int64
    (attrs orig_run, orig_event), and min_event / max_event on the group.  ``response`` (default get_response(config)),
    ``threshold`` (default the ADC threshold) and ``offset`` are those of the trace contract, include/attpc_engine.h.
    ``noise_sigma`` / ``noise_table``, ``pedestals`` and ``noise_stream`` add electronic noise and pedestals (off by
    default; ``detector.traces.configure_traces``); ``noise_seed`` keys the noise of ``write`` (event ``event_number``),
    the runs that call ``write_traces`` key it on their own seed.  Every file of a writer with noise records it on the
    group: attributes noise_stream, noise_sigma (NaN for a custom table) and noise_min_level and the dataset noise_cdf;
    the dataset pedestals when pedestals are given.  Without noise the files are those of the noiseless writer.
    ``readout`` ("hit", "partial" or "full") and ``readout_pads`` read out noise-only pads as well (label -1;
    ``detector.traces.configure_traces``); off hit mode every file records the attribute readout and the dataset
    readout_pads (the pad ids of the readout set), in hit mode the files are those of a writer without them.
    ``gain`` (a ``detector.traces.GainSettings``, default None = off) is the micromegas gain of the traces, keyed like
    the noise; every file of a writer with a gain records the attributes gain_rel_variance and gain_stream, and the
    dataset pad_gain when a gain map is given.  ``common_mode`` (a ``detector.traces.CommonModeSettings``, default None
    = off) is the common-mode noise of the traces, keyed like the noise; every file of a writer with it records the
    attributes common_mode_stream, common_mode_sigma (NaN for a custom table) and common_mode_min_level, the dataset
    common_mode_cdf, and the dataset common_mode_groups when a map is given.
    ``packed=True``: an event's samples are stored as losslessly packed records (include/attpc_engine.h, "packed pad
    traces") -- ``trace_{event}_packed`` uint8 and ``trace_{event}_row_start`` [R+1] int64 (from 0) instead of
    ``trace_{event}`` -- and the group carries the attribute trace_format; ``read_traces`` reads either layout.  A
    run feeds such a writer from the packed entry points (``write_packed_traces``): the samples are never expanded
    on the host.  Without ``packed`` the files are those of a writer that does not know the flag."""

    group = "trace"

    def __init__(self, directory_path: Path, config: Config, max_events_per_file: int = 5_000,
                 first_run_number: int = 0, npz_fallback: bool = True, response: np.ndarray | None = None,
                 threshold: float | None = None, offset: int = 0, noise_sigma: float = 0.0, noise_table=None,
                 pedestals=None, noise_stream: int = 0, noise_seed: int = 0, readout: str = "hit",
                 readout_pads=None, gain=None, common_mode=None, packed: bool = False):
        self.packed = _packed_flag(packed)
        response, threshold, offset = trace_settings(config, response, threshold, offset)  # (this config's defaults in every run)
        noise = NoiseSettings(noise_sigma, noise_table, pedestals, noise_stream)
        self.chain = chain = TraceChain(config, response.copy(), threshold, offset, noise, ReadoutSettings(readout, readout_pads), gain,
                                        common_mode=common_mode)
        self.response, self.threshold, self.offset = chain.response, chain.threshold, chain.offset
        self.noise, self.readout, self.gain = chain.noise, chain.readout, chain.gain
        self.common_mode = chain.common_mode
        self.noise_seed = _abi.check_id_range(noise_seed, 0, 0)[0]
        super().__init__(directory_path, max_events_per_file, first_run_number, npz_fallback)

    def _open(self, run_number: int):
        f = super()._open(run_number)
        if self.packed:
            f.set_attr("trace_format", TRACE_PACK_FORMAT)
        if self.noise.n_levels:
            f.set_attr("noise_stream", self.noise.stream)
            f.set_attr("noise_sigma", self.noise.sigma)
            f.set_attr("noise_min_level", self.noise.min_level)
            f.create_dataset("noise_cdf", self.noise.cdf)
        if self.noise.pedestals is not None:
            f.create_dataset("pedestals", self.noise.pedestals)
        if self.readout.token() is not None:
            f.set_attr("readout", self.readout.name)
            f.create_dataset("readout_pads", self.readout.pads)
        if self.gain is not None and self.gain.on:
            f.set_attr("gain_rel_variance", self.gain.rel_variance)
            f.set_attr("gain_stream", self.gain.stream)
            if self.gain.pad_gain is not None:
                f.create_dataset("pad_gain", self.gain.pad_gain)
        if self.common_mode is not None and self.common_mode.on:
            f.set_attr("common_mode_stream", self.common_mode.stream)
            f.set_attr("common_mode_sigma", self.common_mode.sigma)
            f.set_attr("common_mode_min_level", self.common_mode.min_level)
            f.create_dataset("common_mode_cdf", self.common_mode.cdf)
            if self.common_mode.groups is not None:
                f.create_dataset("common_mode_groups", self.common_mode.groups)
        return f

    def noise_kwargs(self) -> dict:
        """The noise settings as ``configure_traces`` takes them."""
        n = self.noise
        return {"noise_table": (n.cdf, n.min_level) if n.n_levels else None, "pedestals": n.pedestals,
                "noise_stream": n.stream}

    def readout_kwargs(self) -> dict:
        """The readout settings as ``configure_traces`` takes them."""
        return {"readout": self.readout.name, "readout_pads": self.readout.channels.astype(bool)}

    def write(self, data: np.ndarray, labels: np.ndarray, config: Config, event_number: int) -> None:
        """One event's cloud [P,3] -> its traces on the device (``clouds_to_traces``) -> datasets."""
        ctx = _abi.default_context()
        self.chain.configure(ctx, keep=("trigger",))
        data = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, 3)
        offsets = np.array([0, len(data)], dtype=np.int64)
        if self.packed:
            _, pads, row_start, packed, out_labels, _ = clouds_to_traces(offsets, data, labels, ctx, seed=self.noise_seed,
                                                                         first_event=event_number, packed=True)
            self.write_packed_traces(pads, row_start, packed, out_labels, event_number)
            return
        _, pads, samples, out_labels, _ = clouds_to_traces(offsets, data, labels, ctx, seed=self.noise_seed,
                                                           first_event=event_number)
        self.write_traces(pads, samples, out_labels, event_number)

    def write_traces(self, pads: np.ndarray, samples: np.ndarray, labels: np.ndarray, event_number: int) -> None:
        """One event's kept pad rows, as the device makes them (``Engine.run_traces``, ``simulate_batch_traces``):
        file roll-over, datasets and attributes.  A ``packed`` writer packs them with the host encoder."""
        if self.packed:
            row_start, packed = pack_traces_host(np.asarray(samples).reshape(-1, _abi.NUM_TB))
            self.write_packed_traces(pads, row_start, packed, labels, event_number)
            return
        self._begin_event(event_number)
        self.file.create_dataset(f"trace_{event_number}", np.asarray(samples, dtype=np.int16).reshape(-1, _abi.NUM_TB),
                                 {"orig_run": self.run_number, "orig_event": event_number})
        self.file.create_dataset(f"pads_{event_number}", np.asarray(pads, dtype=np.int32))
        self.file.create_dataset(f"labels_{event_number}", np.asarray(labels, dtype=np.int64))
        self._end_event(event_number)

    def write_packed_traces(self, pads: np.ndarray, row_start: np.ndarray, packed: np.ndarray, labels: np.ndarray,
                            event_number: int) -> None:
        """One event's kept pad rows as packed records, as the packed entry points deliver them
        (``Engine.run_traces(packed=True)``): ``row_start`` [R+1] any R + 1 consecutive offsets of a call (stored from
        0), ``packed`` the bytes they point into.  Only a ``packed`` writer takes them."""
        if not self.packed:
            raise TypeError("write_packed_traces needs a TraceWriter(packed=True)")
        row_start = np.asarray(row_start, dtype=np.int64)
        records = np.asarray(packed, dtype=np.uint8)[int(row_start[0]):int(row_start[-1])]
        self._begin_event(event_number)
        self.file.create_dataset(f"trace_{event_number}_packed", records, {"orig_run": self.run_number, "orig_event": event_number})
        self.file.create_dataset(f"trace_{event_number}_row_start", row_start - row_start[0])
        self.file.create_dataset(f"pads_{event_number}", np.asarray(pads, dtype=np.int32))
        self.file.create_dataset(f"labels_{event_number}", np.asarray(labels, dtype=np.int64))
        self._end_event(event_number)


def read_traces(path, event: int):
    """One event of a TraceWriter file, ``.h5`` or ``.npz``, plain or packed -> (pads [R] i32, samples [R,512] i16,
    labels [R] i64).  A packed event is decoded on the host (``unpack_traces``); a file whose trace_format this
    package does not know is refused."""
    path = Path(path)
    if path.suffix == ".npz":
        with np.load(path) as f:
            names = set(f.files)
            get = lambda name: f[f"trace/{name}"]  # noqa: E731
            has = lambda name: f"trace/{name}" in names  # noqa: E731
            fmt = str(f["trace@trace_format"]) if "trace@trace_format" in names else None
            return _read_event(get, has, fmt, event)
    import h5py

    with h5py.File(path, "r") as f:
        group = f["trace"]
        fmt = group.attrs.get("trace_format")
        fmt = fmt.decode() if isinstance(fmt, bytes) else (None if fmt is None else str(fmt))
        return _read_event(lambda name: group[name][()], lambda name: name in group, fmt, event)


def _read_event(get, has, fmt, event: int):
    if fmt is not None and fmt != TRACE_PACK_FORMAT:
        raise ValueError(f"unknown trace_format {fmt!r} (this package reads {TRACE_PACK_FORMAT!r})")
    pads, labels = np.asarray(get(f"pads_{event}"), dtype=np.int32), np.asarray(get(f"labels_{event}"), dtype=np.int64)
    if has(f"trace_{event}_packed"):
        samples = unpack_traces(get(f"trace_{event}_row_start"), get(f"trace_{event}_packed"))
    else:
        samples = np.asarray(get(f"trace_{event}"), dtype=np.int16)
    return pads, samples, labels
