"""Fused driver: kinematics + detector simulation without the file in between.

The reference couples its two stages through an HDF5 file (``run_kinematics_pipeline``
then ``run_simulation``, reference kinematics/pipeline.py:429-495 and
detector/simulator.py:118-210).  ``Engine`` runs the same two operators back to back on
one GPU with the kinematics staying in HBM (``attpc_sim_run``); it is what the benchmark
and the multi-GPU sharding drive.  Events are identified by a *global* event id, so any
split of an id range over calls, chunks, processes or GPUs produces the same events.
"""
from __future__ import annotations

import numpy as np

from . import _abi, nuclear_map
from .detector.luts import build_det_desc, build_layout, species_for
from .detector.simulator import default_indices, deliver_events, fired_events, plan_delivery, selected_events, writer_packed
from .detector.traces import (BaselineSettings, CommonModeSettings, GainSettings, PackedRows, PeakSettings, TriggerSettings,
                              configure_baseline, configure_common_mode, configure_gain, configure_peaks, configure_traces,
                              configure_trigger, stage_results, trigger_result)
from .detector.estimate import EstimateSettings, configure_estimates
from .detector.circle import CircleFitSettings, configure_circle
from .detector.fit import TrackFitSettings, configure_track_fit
from .detector.clustering import ClusterSettings, configure_clustering
from .detector.joining import JoinSettings, configure_cluster_join
from .detector.pid import PidSettings, configure_pid
from .detector.hypothesis import HypothesisSettings, configure_fit_hypotheses, hypotheses_result
from .detector.reaction import ReactionSettings, configure_reaction, reaction_result, source_on
from .detector.helix import HelixSlopeSettings, configure_helix
from .detector.thinning import ThinSettings, configure_thinning
from .detector.straggling import StragglingSettings, configure_straggling
from .detector.distortion import DistortionMap, configure_distortion
from .detector.correction import CorrectionSettings, configure_correction
from .outputs import PackedTraceArrays, RowArrays, SelectedArrays, SummaryArrays, call_with_capacity


class Engine:
    def __init__(self, pipeline, config, indices: list[int] | None = None,
                 context: _abi.Context | None = None, chunk_events: int | None = None,
                 ode_substeps: int = 1):
        self.pipeline = pipeline
        self.config = config
        self.ctx = context or _abi.default_context()
        self.z = pipeline.get_proton_numbers()
        self.a = pipeline.get_mass_numbers()
        self.n_rows = len(self.z)
        self.indices = list(indices) if indices is not None else default_indices(self.n_rows)
        self._out_cache = None  # (key, arrays) of the last run with reuse_buffers (call_with_capacity)
        self._spyral_configured = self._traces_configured = self._peaks_configured = self._summary_configured = False
        self._selection = None  # the Selection configure_selection uploaded
        self._maps = None  # the MapsSettings configure_maps uploaded
        self._reaction = None  # the ReactionSettings configure_reaction uploaded
        self._hypotheses = None  # the HypothesisSettings configure_fit_hypotheses uploaded
        ctx = self.ctx
        kin, keep_k = pipeline.device_desc()
        ctx.check(ctx.lib.attpc_kin_configure(ctx.handle, kin), "attpc_kin_configure")
        ctx._kin_owner = id(pipeline)
        self.species = species_for(self.z, self.a, self.indices)
        nuclei = [nuclear_map.get_data(z, a) for z, a in self.species]
        det, keep_d = build_det_desc(config, nuclei, ode_substeps=ode_substeps)
        ctx.check(ctx.lib.attpc_det_configure(ctx.handle, det), "attpc_det_configure")
        ctx.forget("det")  # (what configure_detector last uploaded is no longer what the device holds)
        configure_straggling(ctx, None)  # a new engine starts without the track straggling an earlier one configured
        configure_distortion(ctx, None)  # ... and without its drift distortion
        configure_reaction(ctx, None)  # ... and without its reaction reconstruction, which was that engine's reaction
        configure_fit_hypotheses(ctx, None)  # ... and without its fit hypotheses
        self.layout = build_layout(self.z, self.a, self.indices, self.species)
        if chunk_events:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, int(chunk_events)), "attpc_set_chunk_events")
        del keep_k, keep_d

    def _deliver(self, call: str, n_events: int, seed: int, first_event: int, capacity: int, pinned: bool, **how):
        """One fetched run of ``lib.<call>`` -> (its output holder, the part of the result dict every mode has).
        ``how``: what call_with_capacity needs to know about the mode (holder, slack, reuse)."""
        ctx, stats = self.ctx, _abi.RunStats()
        p4 = np.empty((n_events, self.n_rows, 4), dtype=np.float64)
        vertex = np.empty((n_events, 3), dtype=np.float64)
        status = np.empty(n_events, dtype=np.int32)

        def run(out):
            return getattr(ctx.lib, call)(ctx.handle, seed, first_event, n_events, self.layout, _abi.dptr(p4),
                                          _abi.dptr(vertex), _abi.iptr(status, _abi.C.c_int32), out, stats)

        arrays = call_with_capacity(ctx, n_events, capacity, run, call, stats, pinned=pinned, **how)
        return arrays, {"vertex": vertex, "p4": p4, "status": status, "offsets": arrays.offsets,
                        "labels": arrays.result()[-1], "event_points": arrays.event_points, "stats": stats.as_dict()}

    def hint_next(self, n_events: int, seed: int = 0, first_event: int = 0) -> None:
        """Announce the ``run`` / ``run_spyral`` call after the next one (``attpc_sim_hint_next``): the next call then
        queues that call's first kinematics + track batch behind its own last scatter launches.  A scheduling hint
        only -- results never depend on it; ``n_events = 0`` withdraws it."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        ctx = self.ctx
        ctx.check(ctx.lib.attpc_sim_hint_next(ctx.handle, int(seed), int(first_event), int(n_events), self.layout),
                  "attpc_sim_hint_next")

    def run(self, n_events: int, seed: int = 0, first_event: int = 0, fetch: bool = False,
            capacity_per_event: int = 12288, pinned: bool = False, reuse_buffers: bool = False) -> dict:
        """Simulate events ``first_event .. first_event + n_events - 1``.

        ``fetch=False``: everything stays device resident (chunk buffers are overwritten);
        only the statistics / checksums come back.  ``fetch=True``: also returns vertex, p4,
        status and the point clouds in CSR form (offsets, points, labels); ``pinned`` puts the cloud
        arrays in page-locked host memory (the copy is PCIe bound), ``reuse_buffers`` reuses them
        from call to call (a consumer that is done with one batch before it asks for the next).
        Raises ``DataLossError`` if an event lost charge (``n_failed`` / ``n_inconsistent``)."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        ctx = self.ctx
        stats = _abi.RunStats()
        if not fetch:
            ctx.check(
                ctx.lib.attpc_sim_run(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                      None, None, None, None, stats),
                "attpc_sim_run",
            )
            return {"stats": stats.as_dict()}
        arrays, res = self._deliver("attpc_sim_run", n_events, seed, first_event,
                                    max(4096, int(capacity_per_event) * n_events), pinned, holder=RowArrays, width=3,
                                    slack=4096, cache=self, reuse=reuse_buffers)
        return {**res, "points": arrays.result()[1]}

    # ---------------------------------------------------------------- track straggling
    def configure_straggling(self, settings=None, **parameters) -> None:
        """Multiple scattering and energy-loss straggling of the tracks (include/attpc_engine.h, "track straggling"):
        a ``detector.straggling.StragglingSettings`` or its keywords (angular_scale, energy_scale, radiation_length,
        electron_density, stream) turn the stage on for every run function of this engine -- every recorded sample of
        every track gets a Gaussian kick of its direction and of its kinetic energy, a pure function of the run's seed,
        the global event id, the nucleus and the stream; a radiation length or an electron density left open is that
        of the config's gas target --, neither turns it off (the default)."""
        configure_straggling(self.ctx, _settings(StragglingSettings, settings, parameters), self.config)

    # ---------------------------------------------------------------- drift distortion
    def configure_distortion(self, distortion=None, **parameters) -> None:
        """The drift distortion of the track samples (include/attpc_engine.h, "drift distortion"): a
        ``detector.distortion.DistortionMap`` or its keywords (radial, azimuthal, time, rho_max, length) turn the stage
        on for every run function of this engine -- every kept sample of every track is moved radially, azimuthally and
        in time by the map before anything reads it, a pure function of the sample and the map; the map's drift-distance
        nodes are placed by the config's time-bucket edges --, neither turns it off (the default)."""
        configure_distortion(self.ctx, _settings(DistortionMap, distortion, parameters), self.config)

    # ---------------------------------------------------------------- drift correction of the trace rows
    def configure_correction(self, correction=None, **parameters) -> None:
        """The drift correction of the trace rows (include/attpc_engine.h, "drift correction"): a
        ``detector.correction.CorrectionSettings`` or its keywords (map, iterations, tolerance_xy, tolerance_tb) turn
        the stage on -- every row of ``run_trace_rows`` / ``run_estimates`` is taken back through the map on the device
        and every event's rows are sorted again by their corrected time, before the thinning, the estimates and the
        delivery read them; the counts come back under ``correction`` --, neither turns it off (the default).  The map
        need not be the one of ``configure_distortion``."""
        configure_correction(self.ctx, _settings(CorrectionSettings, correction, parameters), self.config)

    # ---------------------------------------------------------------- Spyral rows on the device
    def configure_spyral(self, config=None, response=None) -> None:
        """Upload what SpyralWriter needs (reference writer.py:164-181, 220-234): the GET response of
        the electronics (``response``, default get_response(config)), pad centres / sizes, ADC threshold and
        time-bucket edges."""
        from .detector.simulator import configure_spyral

        configure_spyral(config or self.config, self.ctx, response)
        self._spyral_configured = True

    def run_spyral(self, n_events: int, seed: int = 0, first_event: int = 0, capacity_per_event: int = 6144,
                   pinned: bool = False, reuse_buffers: bool = False) -> dict:
        """Fused kinematics + detector + (on the device) GET response, ADC threshold, Spyral row
        conversion and z-sort.  Returns rows [P', 8] (x mm, y mm, z mm, amplitude, integral, pad, tb,
        pad scale) in CSR form, the rows of every event in ascending z (reference writer.py:232-238), and
        ``event_points`` [n] = cloud rows of every event before the threshold (an event is "empty" for
        the writer only if that is 0, simulator.py:204-205)."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if not self._spyral_configured:
            self.configure_spyral()
        arrays, res = self._deliver("attpc_sim_run_spyral", n_events, seed, first_event,
                                    max(4096, int(capacity_per_event) * n_events), pinned, holder=RowArrays, width=8,
                                    slack=4096, cache=self, reuse=reuse_buffers)
        return {**res, "rows": arrays.result()[1]}

    # ---------------------------------------------------------------- digitised pad traces on the device
    def configure_traces(self, config=None, response=None, threshold=None, offset: int = 0, noise_sigma: float = 0.0,
                         noise_table=None, pedestals=None, noise_stream: int = 0, readout: str = "hit",
                         readout_pads=None) -> None:
        """Upload the trace settings (include/attpc_engine.h): the GET response (default get_response(config)), the ADC
        threshold (default ``ElectronicsParams.adc_threshold``; < 0 keeps every hit pad), the sample offset (0 =
        causal, argmax(response) = peak on the arrival bucket) and the electronic noise and pedestals (off by default:
        ``noise_sigma`` ADC counts of Gaussian noise or a ``noise_table`` (cdf, min_level), ``pedestals`` per pad,
        ``noise_stream``; see ``detector.traces.configure_traces``) and the readout ("hit" by default, "partial" or
        "full" of the pads ``readout_pads``, default every pad not in BEAM_PADS).  The noise of ``run_traces`` is keyed
        on its seed and the global event ids."""
        configure_traces(config or self.config, self.ctx, response, threshold, offset, noise_sigma, noise_table,
                         pedestals, noise_stream, readout, readout_pads)
        self._traces_configured = True

    def _configure_chain(self, chain, rows: bool = False) -> None:
        """What ``run_traces`` (``rows``: ``run_trace_rows``) needs, from one ``detector.traces.TraceChain``."""
        chain.configure(self.ctx, rows)
        self._traces_configured = True
        if rows:
            self._spyral_configured = self._peaks_configured = True

    def run_traces(self, n_events: int, seed: int = 0, first_event: int = 0, fetch: bool = True, pinned: bool = False,
                   capacity_per_event: int = 1024, packed: bool = False, packed_bytes_per_row: int = 512) -> dict:
        """Fused kinematics + detector + the digitised pad traces of every event, made on the device before anything
        crosses PCIe (``attpc_sim_run_traces``).  ``fetch=True``: offsets [n+1], pads [R] i32, samples [R,512] i16,
        labels [R] i64 (``pinned``: page-locked arrays), event_points [n] = cloud rows before the suppression, and the
        kinematics; ``fetch=False``: the traces stay on the device, only ``trace`` (n_rows and both checksums) and the
        cloud's ``stats`` come back.  Both: with a trigger configured (``configure_trigger``) its records [n] under
        ``trigger``.  ``packed=True`` (``attpc_sim_run_traces_packed``): the rows are packed losslessly on the device
        and cross PCIe as records -- ``row_start`` [R+1] i64 and ``packed`` uint8 (``detector.traces.unpack_traces``
        gives the samples back; format ``_abi.TRACE_PACK_FORMAT``) instead of ``samples``, and ``trace`` gains
        ``n_bytes``, with ``fetch=False`` too; ``packed_bytes_per_row`` sizes the first try's byte array (a row takes
        16 .. 784 bytes; too small costs one more run)."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if not isinstance(packed, (bool, np.bool_)):
            raise TypeError(f"packed must be a bool, got {packed!r}")
        if not self._traces_configured:
            self.configure_traces()
        ctx = self.ctx
        stats = _abi.RunStats()
        if not fetch and packed:
            out = _abi.TracePackedOut()
            ctx.check(ctx.lib.attpc_sim_run_traces_packed(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                                          None, None, None, out, stats), "attpc_sim_run_traces_packed")
            return {"stats": stats.as_dict(), "trace": {"n_rows": int(out.n_rows), "n_bytes": int(out.n_bytes),
                                                        "sample_checksum": int(out.sample_checksum),
                                                        "pad_checksum": int(out.pad_checksum)},
                    **trigger_result(ctx, n_events)}
        if not fetch:
            out = _abi.TraceOut()
            ctx.check(ctx.lib.attpc_sim_run_traces(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                                   None, None, None, out, stats), "attpc_sim_run_traces")
            return {"stats": stats.as_dict(), "trace": {"n_rows": int(out.n_rows),
                                                        "sample_checksum": int(out.sample_checksum),
                                                        "pad_checksum": int(out.pad_checksum)},
                    **trigger_result(ctx, n_events)}
        per_event = max(int(capacity_per_event), ctx._trace_readout_rows)  # full readout: |S|
        if packed:
            capacity = max(1024, per_event * n_events)
            arrays, res = self._deliver("attpc_sim_run_traces_packed", n_events, seed, first_event, capacity, pinned,
                                        holder=PackedTraceArrays, byte_capacity=capacity * max(16, int(packed_bytes_per_row)))
            _, pads, row_start, bytes_, _ = arrays.result()
            return {**res, "pads": pads, "row_start": row_start, "packed": bytes_, "trace": arrays.sums(),
                    **trigger_result(ctx, n_events)}
        arrays, res = self._deliver("attpc_sim_run_traces", n_events, seed, first_event, max(1024, per_event * n_events),
                                    pinned)
        _, pads, samples, _ = arrays.result()
        return {**res, "pads": pads, "samples": samples, "trace": arrays.sums(), **trigger_result(ctx, n_events)}

    # ---------------------------------------------------------------- micromegas gain of the pad traces
    def configure_gain(self, gain=None, **parameters) -> None:
        """The micromegas gain of the traces (include/attpc_engine.h): a ``detector.traces.GainSettings`` or its
        keywords (rel_variance or theta, pad_gain, stream) turn it on -- the traces of ``run_traces``,
        ``run_trace_rows`` and ``run_trigger`` are then made from every cloud row's gained charge (avalanche
        fluctuations and the pad's gain factor), keyed on the run's seed and the global event ids --, neither turns it
        off (the default).  The clouds of ``run`` and the rows of ``run_spyral`` never change."""
        configure_gain(self.ctx, _settings(GainSettings, gain, parameters))

    # ---------------------------------------------------------------- common-mode noise of the pad traces
    def configure_common_mode(self, common_mode=None, **parameters) -> None:
        """The common-mode noise of the traces (include/attpc_engine.h): a ``detector.traces.CommonModeSettings`` or its
        keywords (sigma or table, groups, stream) turn it on -- every pad with a group then gets its group's draw of
        every sample on top of its own noise in ``run_traces``, ``run_trace_rows`` and ``run_trigger``, keyed on the
        run's seed and the global event ids --, neither turns it off (the default).  It does not need
        ``configure_traces`` to have set a pad noise.  The clouds of ``run`` and the rows of ``run_spyral`` never
        change."""
        configure_common_mode(self.ctx, _settings(CommonModeSettings, common_mode, parameters))

    # ---------------------------------------------------------------- multiplicity trigger on the pad traces
    def configure_trigger(self, trigger=None, **parameters) -> None:
        """The multiplicity trigger of the traces (include/attpc_engine.h): a ``detector.traces.TriggerSettings`` or its
        keywords (threshold, window, group_multiplicity, min_groups, groups, gate) turn it on -- ``run_traces``,
        ``run_trace_rows`` and ``run_trigger`` then return one record per event under ``trigger``; with ``gate`` the
        events that did not fire get no trace rows --, neither turns it off (the default)."""
        configure_trigger(self.ctx, _settings(TriggerSettings, trigger, parameters))

    def run_trigger(self, n_events: int, seed: int = 0, first_event: int = 0) -> dict:
        """``run_traces(fetch=False)`` for its trigger records: the traces are made, triggered on and left on the
        device, 32 bytes per event cross PCIe (``trigger`` [n], ``detector.traces.TRIGGER_DTYPE``; ``trace`` and
        ``stats`` as ``run_traces``).  Raises if no trigger is configured."""
        if self.ctx._tokens["trigger"] is None:
            raise RuntimeError("run_trigger needs a trigger: call configure_trigger first")
        return self.run_traces(n_events, seed=seed, first_event=first_event, fetch=False)


    # ---------------------------------------------------------------- trace rows: peaks of the traces as Spyral rows
    def configure_peaks(self, peaks=None, **parameters) -> None:
        """Upload the peak parameters of the trace rows: a ``detector.traces.PeakSettings`` or its keywords
        (separation, prominence, min_width, max_width, rel_height, threshold; include/attpc_engine.h)."""
        configure_peaks(self.ctx, _settings(PeakSettings, peaks, parameters) or PeakSettings())
        self._peaks_configured = True

    def configure_baseline(self, baseline=None, window_scale: float | None = None) -> None:
        """The Fourier baseline of the trace rows (include/attpc_engine.h): a ``detector.traces.BaselineSettings`` or
        its ``window_scale`` turns it on -- the peaks of ``run_trace_rows`` then stand on Spyral's own estimate of the
        baseline instead of the configured pedestals --, neither turns it off (the default)."""
        parameters = {} if window_scale is None else {"window_scale": window_scale}
        configure_baseline(self.ctx, _settings(BaselineSettings, baseline, parameters, "window_scale"))

    def _trace_rows_defaults(self) -> None:
        """What a trace-row call needs and was not configured, with its defaults."""
        if not self._traces_configured:
            self.configure_traces()
        if not self._spyral_configured:
            self.configure_spyral()
        if not self._peaks_configured:
            self.configure_peaks()

    def run_trace_rows(self, n_events: int, seed: int = 0, first_event: int = 0, fetch: bool = True, pinned: bool = False,
                       capacity_per_event: int = 2048) -> dict:
        """Fused kinematics + detector + pad traces + the peaks of every kept trace as Spyral rows, all on the device
        (``attpc_sim_run_trace_rows``; the traces as ``configure_traces`` set them, the geometry of
        ``configure_spyral``, the peaks of ``configure_peaks``, each with its defaults if not called; the Fourier baseline
        of ``configure_baseline`` if that turned it on).  ``fetch=True``:
        offsets [n+1], rows [P,8] (x mm, y mm, z mm, amplitude, integral, pad, centroid, pad scale; every event in
        ascending z), labels [P], event_points [n] and the kinematics; ``fetch=False``: the rows stay on the device.
        Both: ``trace_rows`` = {n_rows, row_checksum}, the cloud's ``stats`` (``n_points`` = the rows) and, with a
        trigger configured (``configure_trigger``), its records [n] under ``trigger`` (with its ``gate`` an event that
        did not fire is an empty range of the offsets); with the track estimates configured (``configure_estimates``)
        their records [n, n_sim] under ``estimates`` (and with the track fit
        configured, ``configure_track_fit``, its records under ``fits``) -- with the thinning configured too (``configure_thinning``) those
        of the thinned points, and its z step under ``thinning``; with the geometric circle fit configured as well
        (``configure_circle_fit``) their circles are the refined ones, and ``circle`` is "geometric"; with the helix
        slope configured (``configure_helix_slope``) their slope, vz and B rho come from the turning angle about the
        circle's centre, and ``slope`` is "helix"; with the drift correction configured (``configure_correction``) the
        rows, labels and estimates are those of the corrected rows, and ``correction`` holds its counts (n_rows,
        n_skipped, n_unconverged, n_moved); with the fit hypotheses configured (``configure_fit_hypotheses``) beside the
        estimates and the track fit, their records [n, n_sim] under ``hypotheses``, and ``fits`` are the chosen species'."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        self._trace_rows_defaults()
        self._apply_reaction()
        self._apply_hypotheses()
        ctx = self.ctx
        if not fetch:
            stats, out = _abi.RunStats(), _abi.CloudOut()
            ctx.check(ctx.lib.attpc_sim_run_trace_rows(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                                       None, None, None, out, stats), "attpc_sim_run_trace_rows")
            return {"stats": stats.as_dict(), "trace_rows": ctx.trace_rows_last(),
                    **stage_results(ctx, n_events, len(self.indices)), **hypotheses_result(ctx, n_events, len(self.indices)),
                    **reaction_result(ctx, self._reaction, n_events)}
        per_event = max(int(capacity_per_event), 4 * ctx._trace_readout_rows)
        arrays, res = self._deliver("attpc_sim_run_trace_rows", n_events, seed, first_event, max(1024, per_event * n_events),
                                    pinned, holder=RowArrays, width=8, slack=1024)
        return {**res, "rows": arrays.result()[1], "trace_rows": ctx.trace_rows_last(),
                **stage_results(ctx, n_events, len(self.indices), int(arrays.offsets[-1])),
                **hypotheses_result(ctx, n_events, len(self.indices)), **reaction_result(ctx, self._reaction, n_events)}

    # ---------------------------------------------------------------- track estimates of the trace rows
    def configure_estimates(self, estimates=None, **parameters) -> None:
        """The track estimates of the trace rows (include/attpc_engine.h): a ``detector.estimate.EstimateSettings`` or
        its keywords (beam_region_radius, min_points) turn them on -- ``run_trace_rows`` and ``run_estimates`` then
        return one record per (event, position of ``indices``) under ``estimates``: circle, B rho, slope of z against
        the path, vertex and dE/dx of every simulated nucleus, made on the device from its trace rows; the field is the
        config's --, neither turns them off (the default).  The writers do not store the records."""
        configure_estimates(self.ctx, _settings(EstimateSettings, estimates, parameters), self.config)

    def configure_thinning(self, thinning=None, **parameters) -> None:
        """Thinning in front of the track estimates (include/attpc_engine.h, "thinned track points"): a
        ``detector.thinning.ThinSettings`` or its keyword (z_step in mm, default 5) turns it on -- the estimates of
        ``run_trace_rows`` / ``run_estimates`` are then made of one charge-weighted centroid per z bin of every track,
        not of its raw rows, and ``min_points`` counts those points --, neither turns it off (the default).  Without
        the estimates it does nothing."""
        configure_thinning(self.ctx, _settings(ThinSettings, thinning, parameters))

    def configure_circle_fit(self, circle=None, **parameters) -> None:
        """The geometric circle fit behind the track estimates (include/attpc_engine.h, "geometric circle fit"): a
        ``detector.circle.CircleFitSettings`` or its keywords (max_evaluations, tolerance in units of 1/16 mm) turn it
        on -- centre, radius, vertex and B rho of the estimates of ``run_trace_rows`` / ``run_estimates`` then come from
        the Kasa circle refined by a least-squares fit of the geometric distances, ``reserved`` carries the evaluations
        made --, neither turns it off (the default).  Without the estimates it does nothing."""
        configure_circle(self.ctx, _settings(CircleFitSettings, circle, parameters))

    def configure_helix_slope(self, settings=None, **parameters) -> None:
        """The helix slope behind the circle of the track estimates (include/attpc_engine.h, "helix slope"): a
        ``detector.helix.HelixSlopeSettings`` or its keyword (regressor) turns it on -- slope, vz and B rho of the
        estimates of ``run_trace_rows`` / ``run_estimates`` then come from the regression of z against the turning
        angle of the segment's points about the centre of the record's circle, and ``detector.helix.STATUS_BITS["NO_HELIX"]`` marks
        a record in which it could not run --, neither turns it off (the default).  Without the estimates it does
        nothing."""
        configure_helix(self.ctx, _settings(HelixSlopeSettings, settings, parameters))

    def configure_track_fit(self, settings=None, **parameters) -> None:
        """The track fit behind the track estimates (include/attpc_engine.h, "track fit"): a
        ``detector.fit.TrackFitSettings`` or its keywords (time_step, max_steps, max_evaluations, tolerance_momentum,
        tolerance_position) turn it on -- ``run_trace_rows`` and ``run_estimates`` then return one record per (event,
        position) under ``fits`` (``detector.fit.FIT_DTYPE``): momentum over mass and vertex of the trial track through
        the gas that fits the track's points best, started from its estimate record --, neither turns it off (the
        default).  Without the estimates it does nothing.  The writers do not store the records."""
        configure_track_fit(self.ctx, _settings(TrackFitSettings, settings, parameters))

    def configure_clustering(self, settings=None, **parameters) -> None:
        """The clustering of the trace rows (include/attpc_engine.h, "clustering"): a
        ``detector.clustering.ClusterSettings`` or its keywords (eps_xy, eps_z, min_samples, min_cluster_size, max_rows,
        match) turn it on -- every chunk of ``run_trace_rows`` / ``run_estimates`` is clustered on the device behind the
        drift correction, and the thinning, the estimates and the track fit match the cluster labels in place of the
        truth labels; the results carry ``clusters`` = (events [n] ``CLUSTER_EVENT_DTYPE``, records [n, 8]
        ``CLUSTER_DTYPE``) and, where the rows are fetched, ``cluster_labels``; ``labels`` stay the truth labels --,
        neither turns it off (the default).  DBSCAN with definite ties, not Spyral's HDBSCAN sequence.  The writers do not
        store the records."""
        configure_clustering(self.ctx, _settings(ClusterSettings, settings, parameters))

    def configure_cluster_join(self, settings=None, **parameters) -> None:
        """The cluster joining behind the clustering (include/attpc_engine.h, "cluster joining"): a
        ``detector.joining.JoinSettings`` or its keywords (overlap_ratio, min_radius, radius_ratio, max_clusters) turn it
        on -- with the clustering configured too, the clusters of an event whose circles in the pad plane overlap are
        joined before they are ranked and labelled, so the pieces of a broken track carry one label into the thinning,
        the estimates and the track fit; the results of ``run_trace_rows`` / ``run_estimates`` carry ``joins`` = (events
        [n] ``JOIN_EVENT_DTYPE``, records [n, 8] ``JOIN_DTYPE``), and ``clusters`` describe the joined clusters --,
        neither turns it off (the default).  Without the clustering it does nothing.  Spyral's joining in structure, with
        definite ties and one round only; not compared against Spyral.  The writers do not store the records."""
        configure_cluster_join(self.ctx, _settings(JoinSettings, settings, parameters))

    def configure_pid(self, gates=None, mode: str = "any") -> None:
        """The particle identification between the track estimates and the track fit (include/attpc_engine.h, "particle
        identification"): a ``detector.pid.PidSettings``, or ``gates`` (a sequence or a dict by position of
        ``detector.pid.Gate``, None = no gate) with ``mode`` ("any" or "own"), turns it on -- every (event, slot) of
        ``run_trace_rows`` / ``run_estimates`` is then assigned the lowest free position whose polygon gate holds its
        estimate record's (B rho, dE/dx), the track fit uses that position's species and skips the slots without one
        (``detector.pid.FIT_NO_PID``), and the results carry ``pid`` [n, n_sim] (``detector.pid.PID_DTYPE``) --, None
        turns it off (the default).  Without the estimates it does nothing.  ``detector.pid.Gate.from_band`` makes gates
        from a calibration run.  The writers, ``run_simulation`` and ``run_fused`` do not take it and do not store the
        records."""
        settings = gates if gates is None or isinstance(gates, PidSettings) else PidSettings(gates, mode)
        configure_pid(self.ctx, settings)

    def configure_reaction(self, settings=None, **keywords) -> None:
        """The reaction reconstruction behind the track estimates and the track fit (include/attpc_engine.h, "reaction
        reconstruction"): a ``detector.reaction.ReactionSettings``, or the keywords of
        ``ReactionSettings.from_pipeline`` for this engine's pipeline and indices (track, source, ex_range, ex_bins,
        theta_bins), turns it on -- ``run_trace_rows`` and ``run_estimates`` then carry ``reaction`` [n]
        (``detector.reaction.REACTION_DTYPE``: excitation energy and centre-of-mass angle from the observed track of
        position ``track``, and from the truth) and ``spectra`` (a ``detector.reaction.ReactionSpectra``), and
        ``run_spectra`` returns the spectra alone --, neither turns it off (the default).  Without its source (the
        estimates, and for source "fit" the track fit) it does nothing.  ``run_fused``, ``run_simulation``,
        ``simulate_batch_trace_rows`` and the writers do not take it."""
        if settings is None and keywords:
            settings = ReactionSettings.from_pipeline(self.pipeline, indices=self.indices, **keywords)
        elif settings is not None and keywords:
            raise TypeError("give a ReactionSettings or the keywords of ReactionSettings.from_pipeline, not both")
        if isinstance(settings, ReactionSettings):
            settings.check_indices(self.indices)
        configure_reaction(self.ctx, settings)
        self._reaction = settings

    def run_spectra(self, n_events: int, seed: int = 0, first_event: int = 0) -> dict:
        """``run_trace_rows(fetch=False)`` for the spectra of the reaction reconstruction alone: ``spectra`` (a
        ``detector.reaction.ReactionSpectra``, 8 bytes per cell whatever the number of events) and the cloud's
        ``stats``; the estimate, fit, pid, reaction and cluster records of the call stay on the device (the library's
        option ``reaction_spectra_only``), so nothing that grows with ``n_events`` crosses the link.  The spectra of disjoint id ranges add (``ReactionSpectra.__add__``).  Raises if
        the reaction reconstruction or its source is not configured."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        self._apply_reaction()
        self._apply_hypotheses()
        if not source_on(self.ctx, self._reaction):
            raise RuntimeError("run_spectra needs the reaction reconstruction and its source: call configure_reaction, "
                               "configure_estimates and (for source 'fit') configure_track_fit first")
        self._trace_rows_defaults()
        ctx, stats, out = self.ctx, _abi.RunStats(), _abi.CloudOut()
        ctx.check(ctx.lib.attpc_set_option(ctx.handle, b"reaction_spectra_only", 1), "attpc_set_option")
        try:  # (no stage record of the call is copied to the host: only the spectra cross the link)
            ctx.check(ctx.lib.attpc_sim_run_trace_rows(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                                       None, None, None, out, stats), "attpc_sim_run_trace_rows")
        finally:
            ctx.check(ctx.lib.attpc_set_option(ctx.handle, b"reaction_spectra_only", 0), "attpc_set_option")
        return {"stats": stats.as_dict(), **reaction_result(ctx, self._reaction, n_events, records=False)}

    def _apply_reaction(self) -> None:
        """This engine's reaction reconstruction on the context (another engine of the same context, or a file-driven
        entry point, may have replaced or removed it since ``configure_reaction``); no call if it is what the context
        holds."""
        configure_reaction(self.ctx, self._reaction)

    def configure_fit_hypotheses(self, settings=None, **parameters) -> None:
        """The fit hypotheses behind the track fit (include/attpc_engine.h, "fit hypotheses"): a
        ``detector.hypothesis.HypothesisSettings`` or its keyword (candidates: a bit mask or a sequence of positions,
        default all) turns them on -- with the estimates and the track fit on, every slot of ``run_trace_rows`` /
        ``run_estimates`` is then fitted once per candidate species of the layout and takes the free position of the
        lowest objective ``f``; the results carry ``hypotheses`` [n, n_sim] (``detector.hypothesis.HYPOTHESIS_DTYPE``),
        ``fits`` are the chosen species' records, and the reaction reconstruction reads this stage's positions; with the
        particle identification on, its gates only narrow the candidates --, neither turns them off (the default).
        ``simulate_batch*``, ``run_fused``, ``run_simulation`` and the writers do not take it."""
        self._hypotheses = _settings(HypothesisSettings, settings, parameters)
        configure_fit_hypotheses(self.ctx, self._hypotheses)

    def _apply_hypotheses(self) -> None:
        """This engine's fit hypotheses on the context, as ``_apply_reaction``."""
        configure_fit_hypotheses(self.ctx, self._hypotheses)

    def run_estimates(self, n_events: int, seed: int = 0, first_event: int = 0) -> dict:
        """``run_trace_rows(fetch=False)`` for its track estimates: the rows are made, estimated and left on the device,
        128 bytes per track cross PCIe (``estimates`` [n, n_sim], ``detector.estimate.ESTIMATE_DTYPE``), beside the
        kinematics they estimate (``p4``, ``vertex``, ``status``; ``detector.estimate.truth_tracks``) and ``indices``,
        as ``run_summary`` returns them; ``trace_rows`` and ``stats`` as ``run_trace_rows``.  Raises if the estimates
        are not configured."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if self.ctx._tokens["estimates"] is None:
            raise RuntimeError("run_estimates needs the estimates: call configure_estimates first")
        self._trace_rows_defaults()
        self._apply_reaction()
        self._apply_hypotheses()
        ctx, stats, out = self.ctx, _abi.RunStats(), _abi.CloudOut()
        p4 = np.empty((n_events, self.n_rows, 4), dtype=np.float64)
        vertex = np.empty((n_events, 3), dtype=np.float64)
        status = np.empty(n_events, dtype=np.int32)
        ctx.check(ctx.lib.attpc_sim_run_trace_rows(ctx.handle, int(seed), int(first_event), int(n_events), self.layout,
                                                   _abi.dptr(p4), _abi.dptr(vertex), _abi.iptr(status, _abi.C.c_int32),
                                                   out, stats), "attpc_sim_run_trace_rows")
        return {"indices": list(self.indices), "vertex": vertex, "p4": p4, "status": status, "stats": stats.as_dict(),
                "trace_rows": ctx.trace_rows_last(), **stage_results(ctx, n_events, len(self.indices)),
                **hypotheses_result(ctx, n_events, len(self.indices)), **reaction_result(ctx, self._reaction, n_events)}


    # ---------------------------------------------------------------- event and track summaries of a resident run
    def configure_summary(self, config=None, min_electrons: int | None = None) -> None:
        """Upload the summary settings (include/attpc_engine.h): ``min_electrons`` -- a cloud row is kept iff its
        electrons reach it; default ``detector.summary.electrons_above_threshold(config)``: the row survives the ADC
        threshold as a Spyral row -- and the pad centres (the geometry of ``rho2_max``)."""
        from .detector.summary import configure_summary

        configure_summary(config or self.config, self.ctx, min_electrons)
        self._summary_configured = True

    def run_summary(self, n_events: int, seed: int = 0, first_event: int = 0) -> dict:
        """A device-resident run (``run(fetch=False)``: nothing of the clouds crosses PCIe) that reduces every chunk's
        cloud and track samples on the device, behind its scatter, to one record per event and one per (event,
        simulated nucleus) (``attpc_sim_run_summary``): ``events`` [n] and ``tracks`` [n, n_sim], numpy structured
        arrays (``_abi.EVENT_SUMMARY_DTYPE`` / ``_abi.TRACK_SUMMARY_DTYPE``; the fields are defined in
        include/attpc_engine.h), ``indices`` (the nucleus of every track position), the kinematics and the cloud's
        ``stats``.  Configures with the defaults if ``configure_summary`` was not called."""
        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if not self._summary_configured:
            self.configure_summary()
        ctx, stats = self.ctx, _abi.RunStats()
        p4 = np.empty((n_events, self.n_rows, 4), dtype=np.float64)
        vertex = np.empty((n_events, 3), dtype=np.float64)
        status = np.empty(n_events, dtype=np.int32)
        arrays = SummaryArrays(n_events, n_sim=len(self.indices))
        ctx.check(ctx.lib.attpc_sim_run_summary(ctx.handle, seed, first_event, n_events, self.layout, _abi.dptr(p4),
                                                _abi.dptr(vertex), _abi.iptr(status, _abi.C.c_int32), arrays.out, stats),
                  "attpc_sim_run_summary")
        return {"events": arrays.events, "tracks": arrays.tracks, "indices": list(self.indices), "vertex": vertex,
                "p4": p4, "status": status, "stats": stats.as_dict()}


    # ---------------------------------------------------------------- selected delivery
    def configure_selection(self, selection=None, **cuts) -> None:
        """Upload the selection of ``run_selected``: a ``detector.selection.Selection`` or its keyword cuts (n_kept,
        n_pads, tb_span, charge; tracks / track_mask, min_tracks, track_n_kept, track_n_pads, track_n_samples,
        track_rho2_max, track_end_tb, track_end_rho2; include/attpc_engine.h)."""
        from .detector.selection import configure_selection

        selection = configure_selection(self.ctx, selection, **cuts)
        selection.check_positions(len(self.indices))
        self._selection = selection

    def run_selected(self, n_events: int, seed: int = 0, first_event: int = 0, rows: str = "cloud", fetch: bool = True,
                     pinned: bool = False, capacity_per_event: int | None = None, reuse_buffers: bool = False) -> dict:
        """The delivered run ``run(fetch=True)`` (``rows="cloud"``) or ``run_spyral`` (``rows="spyral"``) of the events
        that pass the configured selection (``attpc_sim_run_selected``): every chunk is reduced to its summary records
        on the device, the predicate is evaluated there, and only the rows of the events that pass are put in event
        order, converted and copied.  Returns ``passed`` [n] bool, ``n_passed``, ``n_rows``, ``events`` [n] and
        ``tracks`` [n, n_sim] (the records of ALL events, as ``run_summary``), ``indices``, ``offsets`` [n+1] (a rejected
        event is an empty range), ``points`` [P,3] or ``rows`` [P',8], ``labels``, ``event_points`` [n] (cloud rows of
        every event before selection and threshold), the kinematics and the cloud's ``stats`` over all events.
        ``fetch=False``: no row arrays -- points / rows and labels are None, everything else is what the fetched call
        returns (what the selection would deliver).  ``pinned`` / ``reuse_buffers`` as in ``run``.  Configures the summary (and for Spyral rows the Spyral stage) with
        the defaults if they were not configured; raises if no selection was configured."""
        from .detector.selection import ROW_KINDS, selected_result

        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if rows not in ROW_KINDS:
            raise ValueError(f"rows must be one of {sorted(ROW_KINDS)}, got {rows!r}")
        if self._selection is None:
            raise RuntimeError("run_selected needs a selection: call configure_selection first")
        if not self._summary_configured:
            self.configure_summary()
        if rows == "spyral" and not self._spyral_configured:
            self.configure_spyral()
        # (the token of the context may have been replaced through another engine of the same context)
        self.configure_selection(self._selection)
        if capacity_per_event is None:
            capacity_per_event = 12288 if rows == "cloud" else 6144
        capacity = max(4096, int(capacity_per_event) * n_events) if fetch else 1
        arrays, res = self._deliver("attpc_sim_run_selected", n_events, seed, first_event, capacity, pinned and fetch,
                                    holder=SelectedArrays, width=ROW_KINDS[rows], n_sim=len(self.indices), rows=fetch,
                                    slack=4096, cache=self, reuse=reuse_buffers)
        return {**res, **selected_result(arrays, rows, res["stats"]), "indices": list(self.indices)}

    # ---------------------------------------------------------------- run maps
    def configure_maps(self, maps=None, **parameters) -> None:
        """The settings of ``run_maps``: a ``detector.maps.MapsSettings`` or its keywords (tracks: the positions of
        ``indices`` whose rows contribute, default all; other_labels; selected: only the events that pass the configured
        selection contribute; include/attpc_engine.h); neither: the defaults."""
        from .detector.maps import MapsSettings, configure_maps

        self._maps = configure_maps(self.ctx, _settings(MapsSettings, maps, parameters) or MapsSettings())

    def run_maps(self, n_events: int, seed: int = 0, first_event: int = 0) -> dict:
        """``run_summary`` that also accumulates, on the device and behind every chunk's summary, the maps of the run
        (``attpc_sim_run_maps``): ``maps`` (a ``detector.maps.RunMaps``: per pad the events that fired it and its charge,
        per time bucket the events, rows and charge, over the kept rows of the configured track positions; ``n_events``
        and ``n_hit``), ``passed`` [n] bool (the events that contributed: all without ``selected``), ``events`` [n] and
        ``tracks`` [n, n_sim] (the records of ALL events, as ``run_summary``), ``indices``, the kinematics and the cloud's
        ``stats``.  The maps of disjoint id ranges add (``RunMaps.__add__``): shards of a run combine that way.
        Configures the summary and the maps with the defaults if they were not configured; raises if the maps are of the
        selected events and no selection was configured."""
        from .detector.maps import RunMaps

        seed, first_event, n_events = _abi.check_id_range(seed, first_event, n_events)
        if self._maps is None:
            self.configure_maps()
        if self._maps.selected and self._selection is None:
            raise RuntimeError("maps of the selected events need a selection: call configure_selection first")
        if not self._summary_configured:
            self.configure_summary()
        # (the tokens of the context may have been replaced through another engine of the same context)
        if self._maps.selected:
            self.configure_selection(self._selection)
        self.configure_maps(self._maps)
        ctx, stats = self.ctx, _abi.RunStats()
        p4 = np.empty((n_events, self.n_rows, 4), dtype=np.float64)
        vertex = np.empty((n_events, 3), dtype=np.float64)
        status = np.empty(n_events, dtype=np.int32)
        arrays = SummaryArrays(n_events, n_sim=len(self.indices))
        passed, maps = np.zeros(n_events, dtype=np.uint8), RunMaps()
        out = maps.out()
        ctx.check(ctx.lib.attpc_sim_run_maps(ctx.handle, seed, first_event, n_events, self.layout, _abi.dptr(p4),
                                             _abi.dptr(vertex), _abi.iptr(status, _abi.C.c_int32), arrays.out,
                                             _abi.iptr(passed, _abi.C.c_uint8), out, stats), "attpc_sim_run_maps")
        return {"maps": maps.absorb(out), "passed": passed.astype(bool), "events": arrays.events, "tracks": arrays.tracks,
                "indices": list(self.indices), "vertex": vertex, "p4": p4, "status": status, "stats": stats.as_dict()}


def _settings(cls, given, parameters: dict, what: str = "keywords"):
    """What the configure methods of the stages take, a settings object or the keywords of its class, not both -> the
    object (None: neither)."""
    if given is not None and parameters:
        raise TypeError(f"give a {cls.__name__} or its {what}, not both")
    return cls(**parameters) if parameters else given


def run_fused(pipeline, config, writer, n_events: int, indices: list[int] | None = None, seed: int | None = None,
              batch_size: int = 65536, context: _abi.Context | None = None, selection=None, trigger=None,
              gain=None, common_mode=None, straggling=None, distortion=None, correction=None) -> None:
    """run_kinematics_pipeline + run_simulation + SpyralWriter without the kinematics file and with
    the response / threshold / row conversion / z-sort done on the GPU: per event with a non-empty
    cloud (before the threshold, as simulator.py:204-205 decides it -- an event whose rows all fall
    below the ADC threshold is still written, with 0 rows, and counts towards the file roll-over exactly
    as in run_simulation + SpyralWriter.write), in event order,
    ``writer.write_rows(rows, labels, event_number, presorted=True)``, then ``close()``.  A SpyralWriter with ``peaks``
    gets the peaks of the event's pad traces as its rows (``Engine.run_trace_rows``).  A writer that offers
    ``write_traces`` (TraceWriter) gets ``write_traces(pads, samples, labels, event_number)`` per such event instead,
    the traces made on the device (``Engine.run_traces``) with the writer's own trace settings.  ``selection``
    (``Engine.run_selected``; rows or plain clouds), ``trigger``, ``gain`` and ``common_mode``: as ``run_simulation`` takes them, with
    the same rules about the kinds of writer (``detector.simulator.plan_delivery``); event numbers stay the global
    ones, the file roll-over counts written events.  ``straggling`` (a ``detector.straggling.StragglingSettings``; None =
    off): the track straggling (``Engine.configure_straggling``), with any writer.  ``distortion`` (a
    ``detector.distortion.DistortionMap``; None = off): the drift distortion (``Engine.configure_distortion``), with any
    writer.  ``correction`` (a ``detector.correction.CorrectionSettings``; default: the writer's own, None = off): the
    drift correction of the trace rows, with a SpyralWriter with ``peaks``."""
    engine = Engine(pipeline, config, indices, context=context)
    engine.configure_straggling(straggling)
    engine.configure_distortion(distortion)
    seed = pipeline.seed if seed is None else int(seed)
    kind, emit, chain = plan_delivery(writer, config, selection, trigger, gain, plain_clouds=False, common_mode=common_mode,
                                      correction=correction)
    if selection is not None:
        engine.configure_selection(selection)
        if kind == "rows":
            engine.configure_spyral(config)

        def selected(start, stop):
            res = engine.run_selected(stop - start, seed=seed, first_event=start, rows="spyral" if kind == "rows" else "cloud")
            return selected_events(res, "rows" if kind == "rows" else "points")

        deliver_events(writer, n_events, batch_size, selected, emit)
        return
    if chain is None:
        engine.configure_spyral(config)
    else:
        engine._configure_chain(chain, rows=kind == "trace_rows")
    run = {"traces": engine.run_traces, "trace_rows": engine.run_trace_rows, "rows": engine.run_spyral}[kind]

    packed = kind == "traces" and writer_packed(writer)

    def batch(start, stop):
        res = run(stop - start, seed=seed, first_event=start, **({"packed": True} if packed else {}))
        if packed:
            arrays = (res["pads"], PackedRows(res["row_start"], res["packed"]))
        else:
            arrays = (res["pads"], res["samples"]) if kind == "traces" else (res["rows"],)
        return fired_events(res["offsets"], res["event_points"], res.get("trigger"), *arrays, res["labels"])

    deliver_events(writer, n_events, batch_size, batch, emit)
