"""Detector simulation entry points (reference ``detector/simulator.py``), device backed.

``simulate`` keeps the reference signature for one event; ``simulate_batch`` is the same
operator over many events (one HIP launch sequence), and ``run_simulation`` drives a
kinematics file through it in batches, calling the writer once per non-empty event in
event order, exactly like the reference loop (simulator.py:183-208).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
from numpy.random import Generator, default_rng

from .. import _abi
from ..outputs import RowArrays, call_with_capacity
from .luts import build_det_desc, build_layout, species_for
from .parameters import Config
from .traces import PackedRows, TraceChain
from .writer import SimulationWriter


def default_indices(n_rows: int) -> list[int]:
    """All final products: rows 2, 4, 6, ... plus the last row (simulator.py:157-158)."""
    indices = [idx for idx in range(2, n_rows, 2)]
    indices.append(n_rows - 1)
    return indices


def _nuclear_map():
    from .. import nuclear_map

    return nuclear_map


def _digest(struct, arrays) -> bytes:
    """Content of a descriptor: its scalar fields and the arrays its pointers refer to (the pointer values
    themselves are left out -- they differ from build to build of the same content)."""
    import ctypes
    import hashlib

    copy = type(struct).from_buffer_copy(bytes(struct))
    for name, ctype in copy._fields_:
        if isinstance(getattr(copy, name), ctypes._Pointer):
            setattr(copy, name, ctypes.cast(None, ctype))
    if hasattr(copy, "species"):
        for sp in copy.species:
            sp.dedx = ctypes.cast(None, type(sp.dedx))
    h = hashlib.blake2b(bytes(copy), digest_size=16)
    for arr in arrays:
        h.update(np.ascontiguousarray(arr).tobytes())
    return h.digest()


def configure_detector(config: Config, species_keys: list[tuple[int, int]], ctx: _abi.Context,
                       ode_substeps: int = 1) -> None:
    """Upload Config + species tables unless this ctx already holds the same ones.  "The same" is decided on the
    CONTENT of the descriptor (every parameter, the pad look-up table, the stopping-power tables), not on object
    identity: a parameter changed in place on the same Config object is seen."""
    nuclei = [_nuclear_map().get_data(z, a) for (z, a) in species_keys]
    keys: list = []
    desc, keep = build_det_desc(config, nuclei, ode_substeps=ode_substeps, content_keys=keys)
    # (the tables are memoised on their inputs' content, luts.py: their keys stand for them; a table without a key --
    #  a target object that cannot be compared by value -- is hashed itself)
    token = (_digest(desc, [arr for arr, key in zip(keep, keys) if key is None]), tuple(keys))
    ctx.configure("det", token, "attpc_det_configure", desc)
    del keep


def configure_spyral(config: Config, ctx: _abi.Context, response: np.ndarray | None = None) -> None:
    """Upload what SpyralWriter.write needs per event (reference writer.py:164-181, 220-234) unless this ctx already
    holds the same: the GET response of the electronics (``response``: the writer's own, writer.py:176; default
    get_response(config)), pad centres / sizes, ADC threshold and time-bucket edges."""
    from .response import get_response

    if config.pad_centers is None:
        raise ValueError("Pad centers are not assigned at write!")  # writer.py:220-221
    response = np.ascontiguousarray(get_response(config) if response is None else response, dtype=np.float64)
    centers = np.ascontiguousarray(config.pad_centers, dtype=np.float64)
    sizes = np.ascontiguousarray(config.pad_sizes, dtype=np.float64)
    desc = _abi.SpyralDesc(_abi.dptr(response), _abi.dptr(centers), _abi.dptr(sizes), len(sizes),
                           int(config.elec_params.windows_edge), int(config.elec_params.micromegas_edge), 0,
                           float(config.det_params.length), float(config.elec_params.adc_threshold))
    ctx.configure("spyral", _digest(desc, [response, centers, sizes]), "attpc_spyral_configure", desc)


def run_batch(call: str, momenta, vertices, proton_numbers, mass_numbers, config: Config, seed, indices, first_event,
              ctx: _abi.Context | None, capacity_per_event: int, configure=None, straggling=None, distortion=None, **how):
    """What simulate_batch, simulate_batch_spyral and simulate_batch_traces share: the inputs as the C ABI takes them,
    the detector on ``ctx`` (``configure_detector``), then the mode's own settings (``configure(ctx)``, which may return
    the rows per event the mode is known to need), the layout and ``lib.<call>`` under ``call_with_capacity(**how)``
    -> (the output holder, the run's RunStats).  ``straggling`` (a ``detector.straggling.StragglingSettings``; None =
    off): the track straggling of the call's tracks, on the gas of ``config``.  ``distortion`` (a
    ``detector.distortion.DistortionMap``; None = off): the drift distortion of the call's track samples, in the drift of
    ``config``."""
    from .distortion import configure_distortion
    from .hypothesis import configure_fit_hypotheses
    from .reaction import configure_reaction
    from .straggling import configure_straggling

    ctx = ctx or _abi.default_context()
    momenta = np.ascontiguousarray(momenta, dtype=np.float64)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    seed, first_event, n = _abi.check_id_range(seed, first_event, momenta.shape[0])
    keys = species_for(proton_numbers, mass_numbers, indices)
    configure_detector(config, keys, ctx)
    configure_straggling(ctx, straggling, config)
    configure_distortion(ctx, distortion, config)
    configure_reaction(ctx, None)  # (an Engine's reaction reconstruction on this context: the entry points here do not take it)
    configure_fit_hypotheses(ctx, None)  # (nor its fit hypotheses)
    known = configure(ctx) if configure else None
    per_event = max(int(capacity_per_event), known or 0)
    layout = build_layout(proton_numbers, mass_numbers, indices, keys)
    stats = _abi.RunStats()

    def run(out):
        return getattr(ctx.lib, call)(ctx.handle, seed, first_event, n, layout, _abi.dptr(momenta), _abi.dptr(vertices),
                                      out, stats)

    return call_with_capacity(ctx, n, max(1024, per_event * n), run, call, stats, **how), stats


def simulate_batch(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers,
                   config: Config, seed: int, indices: list[int], first_event: int = 0,
                   ctx: _abi.Context | None = None, capacity_per_event: int = 16384, straggling=None,
                   distortion=None):
    """simulate() for n events: momenta [n,N,4], vertices [n,3] ->
    (offsets [n+1], points [P,3], labels [P], stats dict).  ``straggling`` and ``distortion``: as ``run_batch`` takes
    them."""
    arrays, stats = run_batch("attpc_det_run", momenta, vertices, proton_numbers, mass_numbers, config, seed, indices,
                              first_event, ctx, capacity_per_event, straggling=straggling, distortion=distortion,
                              holder=RowArrays, width=3, event_points=False, slack=1024)
    return (*arrays.result(), stats.as_dict())


def simulate_batch_spyral(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers,
                          config: Config, seed: int, indices: list[int], first_event: int = 0,
                          ctx: _abi.Context | None = None, response: np.ndarray | None = None,
                          capacity_per_event: int = 8192, straggling=None, distortion=None):
    """simulate() + what SpyralWriter.write does per event (convert_to_spyral, ADC threshold, z-sort; reference
    writer.py:194-238) for n events in one launch sequence, all on the device (``attpc_det_run_spyral``) ->
    (offsets [n+1], rows [P',8], labels [P'], event_points [n] = cloud rows of every event BEFORE the threshold,
    stats dict).  ``straggling`` and ``distortion``: as ``run_batch`` takes them."""
    arrays, stats = run_batch("attpc_det_run_spyral", momenta, vertices, proton_numbers, mass_numbers, config, seed,
                              indices, first_event, ctx, capacity_per_event, straggling=straggling, distortion=distortion,
                              configure=lambda ctx: configure_spyral(config, ctx, response), holder=RowArrays, width=8,
                              slack=1024)
    return (*arrays.result(), arrays.event_points, stats.as_dict())


def simulate(momenta: np.ndarray, vertex: np.ndarray, proton_numbers: np.ndarray,
             mass_numbers: np.ndarray, config: Config, rng: Generator, indices: list[int], straggling=None,
             distortion=None):
    """One kinematics event -> (points [P,3] = pad, time bucket, electrons; labels [P])
    (reference simulator.py:52-115).  ``rng`` seeds the device Philox streams (one draw).
    Row order is unspecified (the reference's is dict-insertion order); use
    ``np.lexsort((points[:,1], points[:,0]))`` for a canonical order.  ``straggling`` (a
    ``detector.straggling.StragglingSettings``; None = off): multiple scattering and energy-loss straggling of the
    tracks.  ``distortion`` (a ``detector.distortion.DistortionMap``; None = off): the drift distortion."""
    seed = int(rng.integers(0, 1 << 63))
    momenta = np.ascontiguousarray(momenta, dtype=np.float64)[None]
    vertex = np.ascontiguousarray(vertex, dtype=np.float64)[None]
    _, points, labels, _ = simulate_batch(momenta, vertex, proton_numbers, mass_numbers, config,
                                          seed, list(indices), straggling=straggling, distortion=distortion)
    return points, labels


def delivery_of(writer, config: Config):
    """What a run hands ``writer`` per event, chosen once from what the writer offers -> (kind, emit): "traces" with
    ``emit(pads, samples, labels, event)`` (TraceWriter.write_traces), "rows" with ``emit(rows, labels, event)``
    (presorted rows to SpyralWriter.write_rows), "trace_rows" with the same ``emit`` (a SpyralWriter with ``peaks``:
    its rows are the peaks of the pad traces) or "cloud" with ``emit(points, labels, event)`` (the plain ``write`` of
    any SimulationWriter)."""
    if callable(getattr(writer, "write_traces", None)):
        if writer_packed(writer):  # (pads, PackedRows, labels, event): the records as they crossed PCIe
            return "traces", lambda pads, rows, labels, event: writer.write_packed_traces(pads, rows.row_start, rows.packed,
                                                                                           labels, event)
        return "traces", writer.write_traces
    if callable(getattr(writer, "write_rows", None)):
        # (SpyralWriter(peaks=...): the rows are the peaks of the event's pad traces, made on the device)
        kind = "rows" if getattr(writer, "peaks", None) is None else "trace_rows"
        return kind, lambda rows, labels, event: writer.write_rows(rows, labels, event, presorted=True)
    return "cloud", lambda points, labels, event: writer.write(points, labels, config, event)


def writer_packed(writer) -> bool:
    """Does ``writer`` store packed pad traces (TraceWriter(packed=True))?  A run then takes the packed entry points."""
    return bool(getattr(writer, "packed", False)) and callable(getattr(writer, "write_packed_traces", None))


def plan_delivery(writer, config: Config, selection=None, trigger=None, gain=None, plain_clouds: bool = True,
                  common_mode=None, correction=None):
    """What run_simulation and run_fused may be asked for with ``writer`` -> (kind, emit, chain): ``delivery_of`` and,
    for a writer of traces or trace rows, the ``detector.traces.TraceChain`` to run (else None): ``writer.chain`` -- a
    writer without one: the TraceChain fields it has as attributes (``noise`` and ``readout`` as settings objects), the
    rest at their defaults -- on the run's ``config`` (it fills in a response or threshold the writer left unset), with
    ``trigger``, gated for trace rows, and ``gain`` and ``common_mode`` if given, else the writer's.  ValueError for a
    ``selection`` with a trace writer and for a ``trigger``, a ``gain`` or a ``common_mode`` with any other;
    ``correction`` (the drift correction, a ``detector.correction.CorrectionSettings``; else the writer's) goes with
    trace rows only, ValueError with any other writer.  AttributeError for plain clouds without a selection unless ``plain_clouds``."""
    kind, emit = delivery_of(writer, config)
    traces = kind in ("traces", "trace_rows")
    if selection is not None and traces:
        raise ValueError("a selection delivers Spyral rows or clouds: trace writers are not supported")
    if trigger is not None and not traces:
        raise ValueError("a trigger delivers traces or trace rows: writers of Spyral rows or clouds are not supported")
    if gain is not None and not traces:
        raise ValueError("a gain acts on traces or trace rows: writers of Spyral rows or clouds are not supported")
    if common_mode is not None and not traces:
        raise ValueError("common-mode noise acts on traces or trace rows: writers of Spyral rows or clouds are not supported")
    if correction is not None and kind != "trace_rows":
        raise ValueError("the drift correction acts on trace rows: only a SpyralWriter with peaks= is supported")
    if kind == "cloud" and selection is None and not plain_clouds:
        raise AttributeError("run_fused needs a writer that offers write_rows or write_traces")
    if not traces:
        return kind, emit, None
    names = ("response", "threshold", "offset", "noise", "readout", "gain", "peaks", "baseline", "common_mode", "correction")
    chain = getattr(writer, "chain", None) or TraceChain(config, **{n: getattr(writer, n) for n in names if hasattr(writer, n)})
    if trigger is not None and kind == "trace_rows":
        trigger = trigger.gated()
    return kind, emit, chain.replace(config=config, trigger=trigger, gain=chain.gain if gain is None else gain,
                                     common_mode=chain.common_mode if common_mode is None else common_mode,
                                     correction=chain.correction if correction is None else correction)


def selected_events(res: dict, key: str):
    """A selected call's result as ``deliver_events`` takes a batch (``key``: "rows" or "points"): event_points masked
    by passed, so that its loop skips the rejected events as it skips the empty ones."""
    return res["offsets"], np.where(res["passed"], res["event_points"], 0), res[key], res["labels"]


def fired_events(offsets, event_points, records, *arrays):
    """A triggered trace call's result as ``deliver_events`` takes a batch: event_points masked by ``records["fired"]``
    (the trigger records of the batch, None = no trigger), so that its loop skips the events that did not fire as it
    skips the empty ones."""
    if records is not None:
        event_points = np.where(records["fired"] != 0, event_points, 0)
    return (offsets, event_points, *arrays)


def deliver_events(writer, n_events: int, batch_size: int, batch, emit) -> None:
    """The event loop of run_simulation and run_fused: ``batch(start, stop)`` -> (offsets, event_points, *arrays) of
    the events start .. stop - 1 in CSR form; every non-empty event's slices go to ``emit`` in event order, then the
    writer is closed.  Empty (simulator.py:204-205) is decided on the cloud BEFORE any threshold, ``event_points[i] ==
    0``; a batch without event_points (None: a plain cloud) on its rows.  A selection or a trigger reaches this loop as
    event_points set to 0 for the events it rejects (``fired_events``): they are skipped, the others keep their
    numbers."""
    for start in range(0, n_events, batch_size):
        stop = min(n_events, start + batch_size)
        offsets, event_points, *arrays = batch(start, stop)
        for i in range(stop - start):
            lo, hi = offsets[i], offsets[i + 1]
            if (hi == lo) if event_points is None else (event_points[i] == 0):
                continue
            emit(*(a[lo:hi] for a in arrays), start + i)
    writer.close()


def run_simulation(config: Config, input_path: Path, writer: SimulationWriter,
                   indices: list[int] | None = None, batch_size: int = 16384,
                   seed: int | None = None, selection=None, trigger=None, gain=None, common_mode=None,
                   straggling=None, distortion=None, correction=None):
    """Apply the detector simulation to every event of a kinematics file (reference
    simulator.py:118-210): the writer is called once per event with a non-empty cloud, in event order, then
    closed.  A writer that offers ``write_rows`` (SpyralWriter) receives its rows ready to store: the response
    scaling, row conversion, ADC threshold and z-sort it would do per event in ``write`` (writer.py:194-238) run on
    the device, fused behind the scatter, before anything crosses PCIe (``attpc_det_run_spyral``) -- the same
    datasets as ``write`` produces, without one GPU round trip per event.  A writer that offers ``write_traces``
    (TraceWriter) receives every non-empty event's pad traces, made on the device (``attpc_det_run_traces``, with the
    writer's noise settings, the noise keyed on the run's seed and the global event ids).  Any other
    SimulationWriter gets
    ``write(points, labels, config, event)`` exactly as in the reference.  ``selection`` (a
    ``detector.selection.Selection``): only the events that pass it reach the writer (``attpc_det_run_selected``: the
    others are not assembled, converted or copied), with their original event numbers; a trace writer raises
    ValueError.  ``trigger`` (a ``detector.traces.TriggerSettings``): only the events the multiplicity trigger fires on
    reach the writer, with their original event numbers -- a writer that receives traces or trace rows (for the latter
    the device skips the peak work of the others too); any other raises ValueError.  ``gain`` (a
    ``detector.traces.GainSettings``; default: the writer's own ``gain``, None = off): the micromegas gain of the traces
    -- again a writer that receives traces or trace rows; any other raises ValueError.  ``common_mode`` (a
    ``detector.traces.CommonModeSettings``; default: the writer's own, None = off): the common-mode noise of the traces,
    under the same rule.  ``straggling`` (a ``detector.straggling.StragglingSettings``; None = off): multiple scattering
    and energy-loss straggling of every track, with any writer.  ``distortion`` (a
    ``detector.distortion.DistortionMap``; None = off): the drift distortion of every track sample, with any writer.
    ``correction`` (a ``detector.correction.CorrectionSettings``; default: the writer's own, None = off): the drift
    correction of the trace rows -- a SpyralWriter with ``peaks``; any other raises ValueError."""
    from ..io import KinematicsFileReader

    print("------- AT-TPC Simulation Engine (MI355X) -------")
    print(f"Applying detector effects to kinematics from file: {input_path}")
    reader = KinematicsFileReader(Path(input_path))
    proton_numbers, mass_numbers = reader.proton_numbers, reader.mass_numbers
    nuclei_to_sim = list(indices) if indices is not None else default_indices(len(proton_numbers))
    n_events = reader.n_events
    print(f"Found {n_events} kinematics events in {reader.n_chunks} {reader.chunk_size} event chunks.")
    print(f"Output will be written to {writer.get_directory_name()}.")
    rng = default_rng(seed)
    run_seed = int(rng.integers(0, 1 << 63))
    kind, emit, chain = plan_delivery(writer, config, selection, trigger, gain, common_mode=common_mode, correction=correction)

    def batch(start, stop):
        vertices, momenta = reader.read(start, stop)
        args = (momenta, vertices, proton_numbers, mass_numbers, config, run_seed, nuclei_to_sim)
        if selection is not None:
            from .selection import simulate_batch_selected

            res = simulate_batch_selected(*args, selection, kind="spyral" if kind == "rows" else "cloud", first_event=start,
                                          response=getattr(writer, "response", None), straggling=straggling,
                                          distortion=distortion)
            return selected_events(res, "rows" if kind == "rows" else "points")
        if chain is not None:  # the pad traces, or their peaks as Spyral rows, are made on the device behind the scatter
            packed = kind == "traces" and writer_packed(writer)
            offsets, *arrays, raw_points, stats = chain.run_batch(
                kind == "trace_rows", momenta, vertices, proton_numbers, mass_numbers, run_seed, nuclei_to_sim, start,
                packed=packed, straggling=straggling, distortion=distortion)
            if packed:  # (pads, row_start, packed, labels) -> the records as one row-indexed array
                arrays = [arrays[0], PackedRows(arrays[1], arrays[2]), arrays[3]]
            return fired_events(offsets, raw_points, stats.get("trigger"), *arrays)
        if kind == "rows":
            offsets, rows, labels, raw_points, _ = simulate_batch_spyral(
                *args, first_event=start, response=getattr(writer, "response", None), straggling=straggling,
                distortion=distortion)
            return offsets, raw_points, rows, labels
        offsets, points, labels, _ = simulate_batch(*args, first_event=start, straggling=straggling, distortion=distortion)
        return offsets, None, points, labels

    deliver_events(writer, n_events, batch_size, batch, emit)
    print("Done.")
    print("----------------------------------------")
