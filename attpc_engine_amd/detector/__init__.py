"""Detector effects: same public names as the reference package (reference
``detector/__init__.py:13-21``) plus the batch entry points, device backed."""
from . import clustering as _clustering
from . import joining as _joining
from . import correction as _correction
from . import distortion as _distortion
from . import fit as _fit
from . import hypothesis as _hypothesis
from . import maps as _maps
from . import parameters as _parameters
from . import pid as _pid
from . import reaction as _reaction
from . import selection as _selection
from . import simulator as _simulator
from . import straggling as _straggling
from . import summary as _summary
from . import traces as _traces
from . import writer as _writer

_EXPORTS = {
    _parameters: ("Config", "DetectorParams", "ElectronicsParams", "PadParams"),
    _simulator: ("run_simulation", "simulate", "simulate_batch"),
    _traces: ("configure_traces", "simulate_batch_traces", "clouds_to_traces", "PeakSettings", "configure_trace_rows",
              "simulate_batch_trace_rows", "clouds_to_trace_rows", "BaselineSettings", "configure_baseline", "remove_baseline",
              "TriggerSettings", "configure_trigger", "traces_to_trigger", "TRIGGER_DTYPE",
              "GainSettings", "configure_gain", "clouds_to_gain", "polya_rel_variance", "normal_quantile_table",
              "CommonModeSettings", "configure_common_mode", "common_mode_values",
              "pack_traces", "pack_traces_host", "unpack_traces", "PackedRows", "TRACE_PACK_FORMAT"),
    _summary: ("SummarySettings", "configure_summary", "simulate_batch_summary", "clouds_to_summary",
               "electrons_above_threshold"),
    _selection: ("Selection", "configure_selection", "simulate_batch_selected", "clouds_to_selection"),
    _maps: ("MapsSettings", "RunMaps", "configure_maps", "simulate_batch_maps", "clouds_to_maps"),
    _straggling: ("StragglingSettings", "configure_straggling", "radiation_length", "electron_density"),
    _distortion: ("DistortionMap", "configure_distortion", "samples_to_distortion"),
    _correction: ("CorrectionSettings", "configure_correction", "rows_to_correction"),
    _fit: ("TrackFitSettings", "configure_track_fit", "rows_to_fit"),
    _clustering: ("ClusterSettings", "configure_clustering", "rows_to_clusters", "cluster_scores"),
    _joining: ("JoinSettings", "configure_cluster_join", "joins_last", "rows_to_joined_clusters"),
    _pid: ("Gate", "PidSettings", "configure_pid", "pid_last", "estimates_to_pid", "by_position", "PID_DTYPE"),
    _reaction: ("ReactionSettings", "ReactionSpectra", "configure_reaction", "reaction_last", "records_to_reaction",
                "REACTION_DTYPE"),
    _hypothesis: ("HypothesisSettings", "configure_fit_hypotheses", "hypotheses_last", "hypothesis_fits_last",
                  "rows_to_fit_hypotheses", "HYPOTHESIS_DTYPE"),
    _writer: ("SimulationWriter", "SpyralWriter", "TraceWriter", "read_traces"),
}
__all__ = []
for _module, _names in _EXPORTS.items():
    for _name in _names:
        globals()[_name] = getattr(_module, _name)
        __all__.append(_name)
del _module, _names, _name
