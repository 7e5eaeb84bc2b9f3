"""ctypes binding of the C ABI declared in ``include/attpc_engine.h``.

This is the *only* place the Python package touches native code.  There is no CPU
fallback: if ``libattpc_hip.so`` is missing or no HIP device is present every
engine call raises (``EngineUnavailable``) instead of silently computing on the host.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

MAX_STEPS = 8
MAX_ROWS = 4 + 2 * (MAX_STEPS - 1)
MAX_SPECIES = 16
MAX_SIM = 8
DEDX_EMIN = -30
DEDX_EMAX = 14
DEDX_SUB = 32
DEDX_NODES = (DEDX_EMAX - DEDX_EMIN) * DEDX_SUB + 1
NUM_TB = 512
NUM_PADS = 10240
MAX_NOISE_LEVELS = 512
READOUT_HIT, READOUT_PARTIAL, READOUT_FULL = 0, 1, 2
TIME_SAMPLES = 10001
LONG_STEPS = 5

EX_GAUSSIAN, EX_UNIFORM, EX_TABLE = 0, 1, 2
POLAR_UNIFORM, POLAR_ARBITRARY = 0, 1

ABI_VERSION = 3  # ATTPC_ABI_VERSION of include/attpc_engine.h this binding was written against

OK, E_INVALID, E_NODEVICE, E_HIP, E_CAPACITY, E_NOTCONFIGURED, E_DATALOSS = 0, 1, 2, 3, 4, 5, 6

_dp = C.POINTER(C.c_double)


class ExcitationDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("table_len", C.c_int32),
        ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double),
        ("table_x", _dp), ("table_cdf", _dp),
    ]


class PolarDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("table_len", C.c_int32),
        ("cos_min", C.c_double), ("cos_max", C.c_double), ("bin_width", C.c_double),
        ("angles", _dp), ("cdf", _dp),
    ]


class KinDesc(C.Structure):
    _fields_ = [
        ("n_steps", C.c_int32), ("sample_limit", C.c_int32),
        ("beam_energy", C.c_double),
        ("masses", C.c_double * MAX_ROWS),
        ("excitation", ExcitationDesc * MAX_STEPS),
        ("polar", PolarDesc * MAX_STEPS),
        ("has_target", C.c_int32), ("eloss_len", C.c_int32),
        ("rho_sigma", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
        ("eloss", _dp),
    ]


class SpeciesDesc(C.Structure):
    _fields_ = [("Z", C.c_int32), ("A", C.c_int32), ("mass", C.c_double), ("dedx", _dp)]


class DetDesc(C.Structure):
    _fields_ = [
        ("length", C.c_double), ("efield", C.c_double), ("bfield", C.c_double),
        ("density", C.c_double), ("diffusion", C.c_double), ("fano_factor", C.c_double),
        ("w_value", C.c_double),
        ("mpgd_gain", C.c_int64),
        ("micromegas_edge", C.c_int32), ("windows_edge", C.c_int32),
        ("pad_lut", C.POINTER(C.c_int16)),
        ("lut_n", C.c_int32), ("lut_lo", C.c_int32),
        ("n_species", C.c_int32), ("ode_substeps", C.c_int32),
        ("species", SpeciesDesc * MAX_SPECIES),
        ("longitudinal_diffusion", C.c_double),
        ("long_weights", C.c_double * 5),
        ("mc_diffusion", C.c_int32),
        ("reserved_ext", C.c_int32),
        ("path_step", C.c_double),
    ]


class EventLayout(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int32), ("n_sim", C.c_int32),
        ("indices", C.c_int32 * MAX_SIM),
        ("species_of_row", C.c_int32 * MAX_ROWS),
    ]


class CloudOut(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64),
        ("offsets", C.POINTER(C.c_int64)),
        ("points", _dp),
        ("labels", C.POINTER(C.c_int64)),
        ("event_points", C.POINTER(C.c_int64)),
    ]


class SpyralDesc(C.Structure):
    _fields_ = [
        ("response", _dp), ("pad_centers", _dp), ("pad_sizes", _dp),
        ("n_pads", C.c_int32), ("windows_edge", C.c_int32), ("micromegas_edge", C.c_int32),
        ("reserved", C.c_int32),
        ("length", C.c_double), ("adc_threshold", C.c_double),
    ]


class TraceDesc(C.Structure):
    _fields_ = [("response", _dp), ("adc_threshold", C.c_double), ("offset", C.c_int32), ("reserved", C.c_int32)]


class TraceNoiseDesc(C.Structure):
    _fields_ = [
        ("cdf", C.POINTER(C.c_uint32)), ("n_levels", C.c_int32), ("min_level", C.c_int32),
        ("pedestals", C.POINTER(C.c_int16)), ("stream", C.c_uint32), ("reserved", C.c_int32),
    ]


class TraceReadoutDesc(C.Structure):
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("channels", C.POINTER(C.c_uint8))]


class PeakDesc(C.Structure):
    _fields_ = [("separation", C.c_double), ("prominence", C.c_double), ("min_width", C.c_double),
                ("max_width", C.c_double), ("rel_height", C.c_double), ("threshold", C.c_double)]


class BaselineDesc(C.Structure):
    _fields_ = [("window_scale", C.c_double)]


class TriggerDesc(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("window", C.c_int32), ("group_multiplicity", C.c_int32),
                ("min_groups", C.c_int32), ("groups", C.POINTER(C.c_uint8)), ("gate", C.c_int32), ("reserved", C.c_int32)]


class TriggerRecord(C.Structure):
    _fields_ = [("fired", C.c_int32), ("sample", C.c_int32), ("groups", C.c_uint32), ("n_rows", C.c_int32),
                ("n_hit_pads", C.c_int32), ("peak_group_sum", C.c_int32), ("peak_sum", C.c_int32),
                ("peak_sample", C.c_int32)]


# the trigger record as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
TRIGGER_DTYPE = np.dtype([("fired", "<i4"), ("sample", "<i4"), ("groups", "<u4"), ("n_rows", "<i4"), ("n_hit_pads", "<i4"),
                          ("peak_group_sum", "<i4"), ("peak_sum", "<i4"), ("peak_sample", "<i4")], align=True)
assert TRIGGER_DTYPE.itemsize == C.sizeof(TriggerRecord) == 32
assert all(TRIGGER_DTYPE.fields[name][1] == getattr(TriggerRecord, name).offset for name, _ in TriggerRecord._fields_)
MAX_TRIGGER_GROUPS = 16


class EstimateDesc(C.Structure):
    _fields_ = [("beam_region_radius", C.c_double), ("magnetic_field", C.c_double), ("min_points", C.c_int32),
                ("reserved", C.c_int32)]


class TrackEstimate(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_used", C.c_int32), ("n_fit", C.c_int32), ("status", C.c_int32),
                ("direction", C.c_int32), ("reserved", C.c_int32), ("charge", C.c_int64), ("arc", C.c_int64),
                ("cx", C.c_double), ("cy", C.c_double), ("radius", C.c_double), ("vx", C.c_double), ("vy", C.c_double),
                ("vz", C.c_double), ("slope", C.c_double), ("x_mean", C.c_double), ("y_mean", C.c_double),
                ("dedx", C.c_double), ("brho", C.c_double)]


# the track estimate as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
ESTIMATE_DTYPE = np.dtype([(name, {C.c_int32: "<i4", C.c_int64: "<i8", C.c_double: "<f8"}[ctype])
                           for name, ctype in TrackEstimate._fields_], align=True)
assert ESTIMATE_DTYPE.itemsize == C.sizeof(TrackEstimate) == 128
assert all(ESTIMATE_DTYPE.fields[name][1] == getattr(TrackEstimate, name).offset for name, _ in TrackEstimate._fields_)
# ATTPC_EST_*: the bits of TrackEstimate.status
EST_EMPTY, EST_FEW, EST_RANGE, EST_CAPPED, EST_NO_CIRCLE, EST_ON_AXIS, EST_NO_SLOPE = 1, 2, 4, 8, 16, 32, 64
EST_MAX_FIT = 2048


class CircleDesc(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("max_evaluations", C.c_int32), ("reserved", C.c_int32)]


# the geometric circle fit behind the estimates: its status bit, the range of max_evaluations and the defaults
EST_NOT_CONVERGED = 128
CIRCLE_MIN_EVALUATIONS, CIRCLE_MAX_EVALUATIONS = 2, 64
CIRCLE_DEFAULT_EVALUATIONS, CIRCLE_DEFAULT_TOLERANCE = 32, 1.0 / 128.0


class HelixDesc(C.Structure):
    _fields_ = [("regressor", C.c_int32), ("reserved", C.c_int32)]


# the helix slope behind the circle of the estimates: its status bit and the regressors
EST_NO_HELIX = 256
HELIX_AUTO, HELIX_Z_ON_PATH, HELIX_PATH_ON_Z = 0, 1, 2


class FitDesc(C.Structure):
    _fields_ = [("time_step", C.c_double), ("tolerance_momentum", C.c_double), ("tolerance_position", C.c_double),
                ("max_steps", C.c_int32), ("max_evaluations", C.c_int32)]


class TrackFit(C.Structure):
    _fields_ = [("status", C.c_int32), ("evaluations", C.c_int32), ("n_points", C.c_int32), ("n_inside", C.c_int32),
                ("steps", C.c_int32), ("end", C.c_int32), ("f", C.c_double), ("lambda_", C.c_double), ("g", C.c_double * 3),
                ("vertex", C.c_double * 3), ("ke", C.c_double), ("brho", C.c_double), ("path", C.c_double),
                ("reserved", C.c_double * 2)]


# the track fit as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
FIT_DTYPE = np.dtype([("status", "<i4"), ("evaluations", "<i4"), ("n_points", "<i4"), ("n_inside", "<i4"), ("steps", "<i4"),
                      ("end", "<i4"), ("f", "<f8"), ("lambda", "<f8"), ("g", "<f8", (3,)), ("vertex", "<f8", (3,)),
                      ("ke", "<f8"), ("brho", "<f8"), ("path", "<f8"), ("reserved", "<f8", (2,))], align=True)
assert FIT_DTYPE.itemsize == C.sizeof(TrackFit) == 128 and C.sizeof(FitDesc) == 32
assert all(FIT_DTYPE.fields[name.rstrip("_")][1] == getattr(TrackFit, name).offset for name, _ in TrackFit._fields_)
# ATTPC_FIT_*: the bits of TrackFit.status, the ends of a trial, the limits and the defaults
FIT_EMPTY, FIT_FEW, FIT_CAPPED, FIT_NO_START, FIT_SINGULAR, FIT_STEP_CAP, FIT_NOT_CONVERGED = 1, 2, 8, 16, 32, 64, 128
FIT_END_STOPPED, FIT_END_LEFT, FIT_END_STEP_CAP, FIT_END_NOT_FINITE = 1, 2, 3, 4
FIT_MAX_POINTS, FIT_MAX_STEPS, FIT_MIN_EVALUATIONS, FIT_MAX_EVALUATIONS = 2048, 10000, 2, 32
FIT_DEFAULT_TIME_STEP, FIT_DEFAULT_EVALUATIONS = 1.0e-10, 12


class ClusterDesc(C.Structure):  # attpc_cluster_desc
    _fields_ = [("eps_xy", C.c_double), ("eps_z", C.c_double), ("min_samples", C.c_int32), ("min_cluster_size", C.c_int32),
                ("max_rows", C.c_int32), ("match", C.c_int32), ("reserved", C.c_int32 * 2)]


class ClusterEvent(C.Structure):  # attpc_cluster_event
    _fields_ = [("n_rows", C.c_int32), ("n_range", C.c_int32), ("n_core", C.c_int32), ("n_border", C.c_int32),
                ("n_noise", C.c_int32), ("n_clusters", C.c_int32), ("n_small", C.c_int32), ("n_split", C.c_int32),
                ("n_fake", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 2), ("truth_rows", C.c_uint16 * MAX_SIM)]


class ClusterRecord(C.Structure):  # attpc_cluster_record
    _fields_ = [("rows", C.c_int32), ("core_rows", C.c_int32), ("first_row", C.c_int32), ("majority", C.c_int32),
                ("majority_rows", C.c_int32), ("label", C.c_int32), ("z_min", C.c_int32), ("z_max", C.c_int32)]


# the cluster records as numpy structured dtypes: itemsize and field offsets are those of include/attpc_engine.h
CLUSTER_EVENT_DTYPE = np.dtype([("n_rows", "<i4"), ("n_range", "<i4"), ("n_core", "<i4"), ("n_border", "<i4"), ("n_noise", "<i4"),
                                ("n_clusters", "<i4"), ("n_small", "<i4"), ("n_split", "<i4"), ("n_fake", "<i4"), ("status", "<i4"),
                                ("reserved", "<i4", (2,)), ("truth_rows", "<u2", (MAX_SIM,))], align=True)
CLUSTER_DTYPE = np.dtype([("rows", "<i4"), ("core_rows", "<i4"), ("first_row", "<i4"), ("majority", "<i4"),
                          ("majority_rows", "<i4"), ("label", "<i4"), ("z_min", "<i4"), ("z_max", "<i4")], align=True)
assert C.sizeof(ClusterDesc) == 40 and CLUSTER_EVENT_DTYPE.itemsize == C.sizeof(ClusterEvent) == 64
assert CLUSTER_DTYPE.itemsize == C.sizeof(ClusterRecord) == 32
assert all(CLUSTER_EVENT_DTYPE.fields[name][1] == getattr(ClusterEvent, name).offset for name, _ in ClusterEvent._fields_)
# ATTPC_CLUSTER_*: the match modes, the bits of ClusterEvent.status, the limits and the default
CLUSTER_MATCH_TRUTH, CLUSTER_MATCH_RANK = 0, 1
CLUSTER_CAPPED, CLUSTER_INTERNAL = 1, 2
CLUSTER_DEFAULT_MAX_ROWS, CLUSTER_MAX_ROWS_LIMIT = 16384, 65535


class JoinDesc(C.Structure):  # attpc_join_desc
    _fields_ = [("overlap_ratio", C.c_double), ("min_radius", C.c_double), ("radius_ratio", C.c_double),
                ("max_clusters", C.c_int32), ("reserved", C.c_int32 * 3)]


class JoinEvent(C.Structure):  # attpc_join_event
    _fields_ = [("n_candidates", C.c_int32), ("n_circles", C.c_int32), ("n_taking_part", C.c_int32), ("n_pairs", C.c_int32),
                ("n_joined", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32 * 2)]


class JoinRecord(C.Structure):  # attpc_join_record
    _fields_ = [("parts", C.c_int32), ("first_row", C.c_int32), ("a", C.c_double), ("b", C.c_double), ("radius", C.c_double)]


# the join records as numpy structured dtypes: itemsize and field offsets are those of include/attpc_engine.h
JOIN_EVENT_DTYPE = np.dtype([("n_candidates", "<i4"), ("n_circles", "<i4"), ("n_taking_part", "<i4"), ("n_pairs", "<i4"),
                             ("n_joined", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))], align=True)
JOIN_DTYPE = np.dtype([("parts", "<i4"), ("first_row", "<i4"), ("a", "<f8"), ("b", "<f8"), ("radius", "<f8")], align=True)
assert C.sizeof(JoinDesc) == 40 and JOIN_EVENT_DTYPE.itemsize == C.sizeof(JoinEvent) == 32
assert JOIN_DTYPE.itemsize == C.sizeof(JoinRecord) == 32
assert all(JOIN_DTYPE.fields[name][1] == getattr(JoinRecord, name).offset for name, _ in JoinRecord._fields_)
# ATTPC_JOIN_*: the bits of JoinEvent.status and the limit of max_clusters
JOIN_CAPPED, JOIN_NOT_CLUSTERED = 1, 2
JOIN_MAX_CLUSTERS = 64

# ATTPC_PID_*: the modes, the limit of a gate's vertices and the bits of PidRecord.status; ATTPC_FIT_NO_PID
PID_ANY, PID_OWN = 0, 1
PID_MAX_VERTICES = 32
PID_NO_ESTIMATE, PID_NONE, PID_TAKEN, PID_AMBIGUOUS = 1, 2, 4, 8
FIT_NO_PID = 256


class PidDesc(C.Structure):  # attpc_pid_desc
    _fields_ = [("n_vertices", C.c_int32 * MAX_SIM), ("mode", C.c_int32), ("reserved", C.c_int32),
                ("vertices", C.c_double * 2 * PID_MAX_VERTICES * MAX_SIM)]


class PidRecord(C.Structure):  # attpc_pid_record
    _fields_ = [("position", C.c_int32), ("species", C.c_int32), ("held", C.c_int32), ("status", C.c_int32)]


# the pid records as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
PID_DTYPE = np.dtype([("position", "<i4"), ("species", "<i4"), ("held", "<i4"), ("status", "<i4")], align=True)
assert C.sizeof(PidDesc) == 4136 and PID_DTYPE.itemsize == C.sizeof(PidRecord) == 16
assert all(PID_DTYPE.fields[name][1] == getattr(PidRecord, name).offset for name, _ in PidRecord._fields_)

# ATTPC_REACTION_*: the sources, the bits of ReactionRecord.status and the limits of the bins and of the table
REACTION_FROM_FIT, REACTION_FROM_ESTIMATE = 0, 1
REACTION_NO_TRACK, REACTION_OUTSIDE_TARGET, REACTION_UNPHYSICAL, REACTION_NO_TRUTH = 1, 2, 4, 8
REACTION_MAX_EX, REACTION_MAX_THETA, REACTION_MAX_ELOSS = 256, 180, 65536


class ReactionDesc(C.Structure):  # attpc_reaction_desc
    _fields_ = [("masses", C.c_double * 4), ("beam_energy", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("ex_lo", C.c_double), ("ex_hi", C.c_double), ("ex_inv_width", C.c_double), ("theta_inv_width", C.c_double),
                ("eloss", C.POINTER(C.c_double)), ("eloss_len", C.c_int32), ("has_target", C.c_int32), ("charge", C.c_int32),
                ("track", C.c_int32), ("observed_row", C.c_int32), ("source", C.c_int32), ("n_ex", C.c_int32),
                ("n_theta", C.c_int32), ("reserved", C.c_int64)]


class ReactionRecord(C.Structure):  # attpc_reaction_record
    _fields_ = [("status", C.c_int32), ("slot", C.c_int32), ("beam_ke", C.c_double), ("ex", C.c_double),
                ("theta_cm", C.c_double), ("truth_beam_ke", C.c_double), ("truth_ex", C.c_double),
                ("truth_theta_cm", C.c_double), ("reserved", C.c_double)]


# the reaction records as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
REACTION_DTYPE = np.dtype([("status", "<i4"), ("slot", "<i4"), ("beam_ke", "<f8"), ("ex", "<f8"), ("theta_cm", "<f8"),
                           ("truth_beam_ke", "<f8"), ("truth_ex", "<f8"), ("truth_theta_cm", "<f8"), ("reserved", "<f8")],
                          align=True)
assert C.sizeof(ReactionDesc) == 136 and REACTION_DTYPE.itemsize == C.sizeof(ReactionRecord) == 64
assert all(REACTION_DTYPE.fields[name][1] == getattr(ReactionRecord, name).offset for name, _ in ReactionRecord._fields_)

# ATTPC_HYP_*: the bits of FitHypothesis.status
HYP_NO_CANDIDATE, HYP_NO_FIT, HYP_TAKEN, HYP_DISPLACED = 1, 2, 4, 8


class HypothesisDesc(C.Structure):  # attpc_hypothesis_desc
    _fields_ = [("candidates", C.c_int32), ("reserved", C.c_int32)]


class FitHypothesis(C.Structure):  # attpc_fit_hypothesis
    _fields_ = [("position", C.c_int32), ("species", C.c_int32), ("tried", C.c_int32), ("fitted", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32), ("f", C.c_double * MAX_SIM), ("f_next", C.c_double)]


# the hypothesis records as a numpy structured dtype: itemsize and field offsets are those of include/attpc_engine.h
HYPOTHESIS_DTYPE = np.dtype([("position", "<i4"), ("species", "<i4"), ("tried", "<i4"), ("fitted", "<i4"), ("status", "<i4"),
                             ("reserved", "<i4"), ("f", "<f8", (MAX_SIM,)), ("f_next", "<f8")], align=True)
assert C.sizeof(HypothesisDesc) == 8 and HYPOTHESIS_DTYPE.itemsize == C.sizeof(FitHypothesis) == 96
assert all(HYPOTHESIS_DTYPE.fields[name][1] == getattr(FitHypothesis, name).offset for name, _ in FitHypothesis._fields_)


class ThinDesc(C.Structure):
    _fields_ = [("z_step", C.c_double), ("reserved", C.c_int32), ("pad", C.c_int32)]


class ThinInfo(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_points", C.c_int32), ("n_dropped", C.c_int32), ("n_split", C.c_int32)]


# attpc_thin_info as a numpy structured dtype
THIN_INFO_DTYPE = np.dtype([(name, "<i4") for name, _ in ThinInfo._fields_], align=True)
assert THIN_INFO_DTYPE.itemsize == C.sizeof(ThinInfo) == 16
THIN_MAX_RUN = 4096


class TraceGainDesc(C.Structure):
    _fields_ = [("rel_variance", C.c_double), ("pad_gain", _dp), ("quantiles", _dp), ("stream", C.c_uint32),
                ("reserved", C.c_int32)]


GAIN_KNOTS = 4097


class TraceCommonDesc(C.Structure):
    _fields_ = [("groups", C.POINTER(C.c_uint8)), ("cdf", C.POINTER(C.c_uint32)), ("n_levels", C.c_int32),
                ("min_level", C.c_int32), ("stream", C.c_uint32), ("reserved", C.c_int32)]


class EventSummary(C.Structure):
    _fields_ = [("n_points", C.c_uint32), ("n_kept", C.c_uint32), ("n_pads", C.c_uint32), ("tb_min", C.c_int32),
                ("tb_max", C.c_int32), ("reserved", C.c_int32), ("charge", C.c_int64)]


class TrackSummary(C.Structure):
    _fields_ = [("n_points", C.c_uint32), ("n_kept", C.c_uint32), ("n_pads", C.c_uint32), ("tb_min", C.c_int32),
                ("tb_max", C.c_int32), ("reserved", C.c_int32), ("charge", C.c_int64), ("rho2_max", C.c_double),
                ("n_steps", C.c_int32), ("n_samples", C.c_int32), ("electrons", C.c_int64),
                ("end_x", C.c_double), ("end_y", C.c_double), ("end_tb", C.c_double)]


# the two records as numpy structured dtypes: itemsize and field offsets are those of include/attpc_engine.h
EVENT_SUMMARY_DTYPE = np.dtype([("n_points", "<u4"), ("n_kept", "<u4"), ("n_pads", "<u4"), ("tb_min", "<i4"),
                                ("tb_max", "<i4"), ("reserved", "<i4"), ("charge", "<i8")], align=True)
TRACK_SUMMARY_DTYPE = np.dtype([("n_points", "<u4"), ("n_kept", "<u4"), ("n_pads", "<u4"), ("tb_min", "<i4"),
                                ("tb_max", "<i4"), ("reserved", "<i4"), ("charge", "<i8"), ("rho2_max", "<f8"),
                                ("n_steps", "<i4"), ("n_samples", "<i4"), ("electrons", "<i8"),
                                ("end_x", "<f8"), ("end_y", "<f8"), ("end_tb", "<f8")], align=True)


class SummaryDesc(C.Structure):
    _fields_ = [("min_electrons", C.c_int64), ("pad_centers", _dp), ("n_pads", C.c_int32), ("reserved", C.c_int32)]


class SummaryOut(C.Structure):
    _fields_ = [("events", C.POINTER(EventSummary)), ("tracks", C.POINTER(TrackSummary))]


class SelectDesc(C.Structure):
    _fields_ = [("n_kept_lo", C.c_uint32), ("n_kept_hi", C.c_uint32), ("n_pads_lo", C.c_uint32), ("n_pads_hi", C.c_uint32),
                ("tb_span_lo", C.c_uint32), ("tb_span_hi", C.c_uint32), ("charge_lo", C.c_int64), ("charge_hi", C.c_int64),
                ("track_mask", C.c_uint32), ("min_tracks", C.c_uint32),
                ("track_n_kept_lo", C.c_uint32), ("track_n_kept_hi", C.c_uint32),
                ("track_n_pads_lo", C.c_uint32), ("track_n_pads_hi", C.c_uint32),
                ("track_n_samples_lo", C.c_uint32), ("track_n_samples_hi", C.c_uint32),
                ("track_rho2_max_lo", C.c_double), ("track_rho2_max_hi", C.c_double),
                ("track_end_tb_lo", C.c_double), ("track_end_tb_hi", C.c_double),
                ("track_end_rho2_lo", C.c_double), ("track_end_rho2_hi", C.c_double)]


SELECT_CLOUD, SELECT_SPYRAL = 0, 1


class SelectOut(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("capacity", C.c_int64),
                ("offsets", C.POINTER(C.c_int64)), ("points", _dp), ("labels", C.POINTER(C.c_int64)),
                ("event_points", C.POINTER(C.c_int64)), ("passed", C.POINTER(C.c_uint8)),
                ("events", C.POINTER(EventSummary)), ("tracks", C.POINTER(TrackSummary)),
                ("n_passed", C.c_int64), ("n_rows", C.c_int64)]


class MapsDesc(C.Structure):
    _fields_ = [("track_mask", C.c_uint32), ("selected", C.c_uint32)]


class MapsOut(C.Structure):
    _fields_ = [("pad_events", C.POINTER(C.c_uint64)), ("pad_charge", C.POINTER(C.c_int64)),
                ("tb_events", C.POINTER(C.c_uint64)), ("tb_rows", C.POINTER(C.c_uint64)),
                ("tb_charge", C.POINTER(C.c_int64)), ("n_events", C.c_uint64), ("n_hit", C.c_uint64)]


class TraceOut(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64),
        ("offsets", C.POINTER(C.c_int64)),
        ("pads", C.POINTER(C.c_int32)),
        ("samples", C.POINTER(C.c_int16)),
        ("labels", C.POINTER(C.c_int64)),
        ("event_points", C.POINTER(C.c_int64)),
        ("n_rows", C.c_int64),
        ("sample_checksum", C.c_uint64),
        ("pad_checksum", C.c_uint64),
    ]


class TracePackedOut(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64),
        ("offsets", C.POINTER(C.c_int64)),
        ("pads", C.POINTER(C.c_int32)),
        ("row_start", C.POINTER(C.c_int64)),
        ("bytes", C.POINTER(C.c_uint8)),
        ("byte_capacity", C.c_int64),
        ("labels", C.POINTER(C.c_int64)),
        ("event_points", C.POINTER(C.c_int64)),
        ("n_rows", C.c_int64),
        ("n_bytes", C.c_int64),
        ("sample_checksum", C.c_uint64),
        ("pad_checksum", C.c_uint64),
    ]


class StraggleDesc(C.Structure):  # attpc_straggle_desc
    _fields_ = [("angular_scale", C.c_double), ("energy_scale", C.c_double), ("radiation_length", C.c_double),
                ("electron_density", C.c_double), ("stream", C.c_uint32)]


class DistortDesc(C.Structure):  # attpc_distort_desc
    _fields_ = [("rho_step", C.c_double), ("tau_step", C.c_double), ("tb_origin", C.c_double),
                ("n_rho", C.c_int32), ("n_tau", C.c_int32),
                ("radial", _dp), ("azimuthal", _dp), ("time", _dp)]


class UndistortDesc(C.Structure):  # attpc_undistort_desc
    _fields_ = [("map", DistortDesc), ("windows_edge", C.c_int32), ("micromegas_edge", C.c_int32), ("length", C.c_double),
                ("iterations", C.c_int32), ("tolerance_xy", C.c_double), ("tolerance_tb", C.c_double)]


class UndistortInfo(C.Structure):  # attpc_undistort_info
    _fields_ = [("n_rows", C.c_int64), ("n_skipped", C.c_int64), ("n_unconverged", C.c_int64), ("n_moved", C.c_int64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


assert C.sizeof(UndistortDesc) == 96 and C.sizeof(UndistortInfo) == 32

TRACE_PACK_FORMAT = "for64-bitplane-v1"  # ATTPC_TRACE_PACK_FORMAT
TRACE_PACK_MAX_ROW_BYTES = 784


class RunStats(C.Structure):
    _fields_ = [
        ("n_events", C.c_uint64), ("n_points", C.c_uint64), ("n_track_samples", C.c_uint64),
        ("n_sample_limit", C.c_uint64), ("n_lds_overflow", C.c_uint64), ("n_failed", C.c_uint64),
        ("charge_checksum", C.c_uint64), ("key_checksum", C.c_uint64),
        ("ms_kinematics", C.c_double), ("ms_tracks", C.c_double), ("ms_scatter", C.c_double),
        ("launches_kinematics", C.c_uint32), ("launches_tracks", C.c_uint32),
        ("launches_scatter", C.c_uint32), ("n_inconsistent", C.c_uint32),
        ("n_lone_buckets", C.c_uint64), ("n_buffer_growths", C.c_uint64),
        ("n_tracks_capped", C.c_uint64), ("device_bytes", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


U64 = 1 << 64


def check_id_range(seed, first_event, n_events) -> tuple[int, int, int]:
    """``(seed, first_event, n_events)`` as the C ABI takes them (three u64), or ``ValueError``: ctypes would wrap a
    negative or too large value silently (``seed=-1`` -> 2^64 - 1).  Seeds are ``0 <= seed < 2^64``; the event ids
    ``first_event .. first_event + n_events - 1`` must lie in ``[0, 2^64)`` (include/attpc_engine.h)."""
    seed, first_event, n_events = int(seed), int(first_event), int(n_events)
    if not 0 <= seed < U64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    if not 0 <= first_event < U64:
        raise ValueError(f"first_event must be in [0, 2^64), got {first_event}")
    if n_events < 0:
        raise ValueError(f"n_events must be >= 0, got {n_events}")
    if first_event + n_events > U64:
        raise ValueError(f"event ids {first_event} .. {first_event} + {n_events} - 1 pass 2^64")
    return seed, first_event, n_events


class EngineUnavailable(RuntimeError):
    """The HIP library or a HIP device is missing -- there is no CPU fallback."""


class DataLossError(RuntimeError):
    """A run finished but part of an event's charge is missing from its cloud
    (``stats.n_failed`` / ``stats.n_inconsistent`` != 0, status ATTPC_E_DATALOSS)."""


def dptr(arr: np.ndarray | None):
    if arr is None:
        return None
    assert arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(_dp)


def iptr(arr: np.ndarray | None, ctype):
    if arr is None:
        return None
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.POINTER(ctype))


def library_path() -> Path:
    env = os.environ.get("ATTPC_HIP_LIBRARY")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent / "_lib" / "libattpc_hip.so"


# every symbol include/attpc_engine.h declares
EXPORTED_SYMBOLS = (
    "attpc_version", "attpc_device_count", "attpc_ctx_create", "attpc_ctx_destroy",
    "attpc_last_error", "attpc_set_chunk_events", "attpc_sync", "attpc_kin_configure",
    "attpc_kin_run", "attpc_kin_calculate", "attpc_decay_calculate", "attpc_det_configure", "attpc_det_run",
    "attpc_sim_run", "attpc_det_tracks", "attpc_spyral_rows", "attpc_spyral_configure", "attpc_sim_run_spyral",
    "attpc_set_option", "attpc_host_alloc", "attpc_host_free", "attpc_det_scatter", "attpc_unpack_rows",
    "attpc_unpack_spyral_rows", "attpc_det_run_spyral", "attpc_sim_hint_next", "attpc_unpack_rows8",
    "attpc_trace_configure", "attpc_sim_run_traces", "attpc_det_run_traces", "attpc_traces",
    "attpc_trace_configure_noise", "attpc_traces_at", "attpc_trace_configure_readout",
    "attpc_trace_configure_peaks", "attpc_sim_run_trace_rows", "attpc_det_run_trace_rows", "attpc_trace_rows_at",
    "attpc_trace_rows_last", "attpc_trace_configure_baseline", "attpc_trace_baseline",
    "attpc_trace_configure_trigger", "attpc_trigger_last", "attpc_trigger_rows",
    "attpc_trace_configure_gain", "attpc_gain_rows",
    "attpc_trace_configure_common_mode", "attpc_common_mode_rows",
    "attpc_sim_run_traces_packed", "attpc_det_run_traces_packed", "attpc_traces_packed_at", "attpc_trace_pack",
    "attpc_trace_pack_host", "attpc_trace_unpack",
    "attpc_summary_configure", "attpc_sim_run_summary", "attpc_det_run_summary", "attpc_cloud_summary",
    "attpc_select_configure", "attpc_sim_run_selected", "attpc_det_run_selected", "attpc_cloud_select",
    "attpc_maps_configure", "attpc_sim_run_maps", "attpc_det_run_maps", "attpc_cloud_maps",
    "attpc_trace_configure_estimates", "attpc_estimates_last", "attpc_rows_estimate",
    "attpc_trace_configure_thinning", "attpc_rows_thin",
    "attpc_det_configure_straggling",
    "attpc_trace_configure_circle", "attpc_rows_estimate_circle",
    "attpc_trace_configure_helix", "attpc_rows_estimate_helix",
    "attpc_det_configure_distortion", "attpc_samples_distort",
    "attpc_trace_configure_correction", "attpc_correction_last", "attpc_rows_undistort",
    "attpc_trace_configure_fit", "attpc_fits_last", "attpc_rows_fit",
    "attpc_trace_configure_clustering", "attpc_clusters_last", "attpc_cluster_labels_last", "attpc_rows_cluster",
    "attpc_trace_configure_cluster_join", "attpc_joins_last", "attpc_rows_cluster_join",
    "attpc_trace_configure_pid", "attpc_pid_last", "attpc_estimates_pid", "attpc_rows_fit_pid",
    "attpc_reaction_configure", "attpc_reaction_last", "attpc_reaction_spectra_last", "attpc_reaction_records",
    "attpc_trace_configure_hypotheses", "attpc_hypotheses_last", "attpc_hypothesis_fits_last", "attpc_rows_fit_hypotheses",
)

# The entry points added under ABI version 3 (additive), group by group in the order they were added:
# group -> {symbol: argtypes}.  Another build of that version named by ATTPC_HIP_LIBRARY -- the yardstick of
# tools/trace_rows_rate.py -- may lack whole groups: it loads, and a call of a missing entry point is the AttributeError
# ctypes raises.  The package's own library must have every symbol.
_ctxp, _i16p, _i32p, _i64p, _u8p = C.c_void_p, C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
_ids = [_ctxp, C.c_uint64, C.c_uint64, C.c_uint64]  # (seed, first event, events)
_rows_in = [_ctxp, C.c_int64, _i64p, _dp, _i64p]  # (events, offsets, rows, labels of host rows in CSR form)
_sim_head = _ids + [C.POINTER(EventLayout), _dp, _dp, _i32p]  # ... then the output struct and the statistics
_det_head = _ids + [C.POINTER(EventLayout), _dp, _dp]
_at_head = [_ctxp, C.c_uint64, C.c_uint64, C.c_int64, _i64p, _dp, _i64p]


def _run(head, out):
    return head + [C.POINTER(out), C.POINTER(RunStats)]


SYMBOL_GROUPS = {
    "trace_rows": {
        "attpc_trace_configure_peaks": [_ctxp, C.POINTER(PeakDesc)],
        "attpc_sim_run_trace_rows": _run(_sim_head, CloudOut),
        "attpc_det_run_trace_rows": _run(_det_head, CloudOut),
        "attpc_trace_rows_at": _at_head + [C.POINTER(CloudOut)],
        "attpc_trace_rows_last": [_ctxp, _i64p, C.POINTER(C.c_uint64)],
    },
    "summary": {
        "attpc_summary_configure": [_ctxp, C.POINTER(SummaryDesc)],
        "attpc_sim_run_summary": _run(_sim_head, SummaryOut),
        "attpc_det_run_summary": _run(_det_head, SummaryOut),
        "attpc_cloud_summary": _rows_in + [C.POINTER(EventLayout), C.POINTER(SummaryOut)],
    },
    "select": {
        "attpc_select_configure": [_ctxp, C.POINTER(SelectDesc)],
        "attpc_sim_run_selected": _run(_sim_head, SelectOut),
        "attpc_det_run_selected": _run(_det_head, SelectOut),
        "attpc_cloud_select": _rows_in + [C.POINTER(EventLayout), C.POINTER(SummaryOut), _u8p],
    },
    "baseline": {
        "attpc_trace_configure_baseline": [_ctxp, C.POINTER(BaselineDesc)],
        "attpc_trace_baseline": [_ctxp, C.c_int64, _i16p, C.c_double, _i16p, _dp],
    },
    "trigger": {
        "attpc_trace_configure_trigger": [_ctxp, C.POINTER(TriggerDesc)],
        "attpc_trigger_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(TriggerRecord)],
        "attpc_trigger_rows": [_ctxp, C.c_int64, _i64p, _i32p, _i16p, _i16p, C.POINTER(TriggerDesc), C.POINTER(TriggerRecord)],
    },
    "gain": {
        "attpc_trace_configure_gain": [_ctxp, C.POINTER(TraceGainDesc)],
        "attpc_gain_rows": [_ctxp, C.c_uint64, C.c_uint64, C.c_int64, _i64p, _dp, _dp],
    },
    "common_mode": {
        "attpc_trace_configure_common_mode": [_ctxp, C.POINTER(TraceCommonDesc)],
        "attpc_common_mode_rows": [_ctxp, C.c_uint64, C.c_uint64, C.c_int64, _i16p],
    },
    "trace_pack": {
        "attpc_sim_run_traces_packed": _run(_sim_head, TracePackedOut),
        "attpc_det_run_traces_packed": _run(_det_head, TracePackedOut),
        "attpc_traces_packed_at": _at_head + [C.POINTER(TracePackedOut)],
        "attpc_trace_pack": [_ctxp, C.c_int64, _i16p, _i64p, _u8p, C.c_int64, _i64p],
        "attpc_trace_pack_host": [C.c_int64, _i16p, _i64p, _u8p, C.c_int64, _i64p],
        "attpc_trace_unpack": [_u8p, C.c_int64, _i64p, C.c_int64, _i16p, C.c_int32],
    },
    "maps": {
        "attpc_maps_configure": [_ctxp, C.POINTER(MapsDesc)],
        "attpc_sim_run_maps": _sim_head + [C.POINTER(SummaryOut), _u8p, C.POINTER(MapsOut), C.POINTER(RunStats)],
        "attpc_det_run_maps": _det_head + [C.POINTER(SummaryOut), _u8p, C.POINTER(MapsOut), C.POINTER(RunStats)],
        "attpc_cloud_maps": _rows_in + [C.POINTER(EventLayout), C.POINTER(SummaryOut), _u8p, C.POINTER(MapsOut)],
    },
    "estimates": {
        "attpc_trace_configure_estimates": [_ctxp, C.POINTER(EstimateDesc)],
        "attpc_estimates_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(TrackEstimate)],
        "attpc_rows_estimate": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(TrackEstimate)],
    },
    "thinning": {
        "attpc_trace_configure_thinning": [_ctxp, C.POINTER(ThinDesc)],
        "attpc_rows_thin": _rows_in + [C.POINTER(EventLayout), C.POINTER(ThinDesc), C.c_int64, _i64p, _dp, _i64p,
                                       C.POINTER(ThinInfo), _i64p],
    },
    "straggling": {"attpc_det_configure_straggling": [_ctxp, C.POINTER(StraggleDesc)]},
    "circle": {
        "attpc_trace_configure_circle": [_ctxp, C.POINTER(CircleDesc)],
        "attpc_rows_estimate_circle": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(CircleDesc),
                                                  C.POINTER(TrackEstimate)],
    },
    "helix": {
        "attpc_trace_configure_helix": [_ctxp, C.POINTER(HelixDesc)],
        "attpc_rows_estimate_helix": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(CircleDesc),
                                                 C.POINTER(HelixDesc), C.POINTER(TrackEstimate)],
    },
    "distortion": {
        "attpc_det_configure_distortion": [_ctxp, C.POINTER(DistortDesc)],
        "attpc_samples_distort": [_ctxp, C.c_int64, _dp, C.POINTER(DistortDesc), _dp],
    },
    "correction": {
        "attpc_trace_configure_correction": [_ctxp, C.POINTER(UndistortDesc)],
        "attpc_correction_last": [_ctxp, C.POINTER(UndistortInfo)],
        "attpc_rows_undistort": _rows_in + [C.POINTER(UndistortDesc), _dp, _i64p, _i64p, C.POINTER(UndistortInfo)],
    },
    "fit": {
        "attpc_trace_configure_fit": [_ctxp, C.POINTER(FitDesc)],
        "attpc_fits_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(TrackFit)],
        "attpc_rows_fit": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(TrackEstimate), _dp,
                                      C.POINTER(FitDesc), C.POINTER(TrackFit)],
    },
    "clustering": {
        "attpc_trace_configure_clustering": [_ctxp, C.POINTER(ClusterDesc)],
        "attpc_clusters_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(ClusterEvent), C.POINTER(ClusterRecord)],
        "attpc_cluster_labels_last": [_ctxp, C.c_int64, C.c_int64, _i64p],
        "attpc_rows_cluster": _rows_in + [C.POINTER(EventLayout), C.POINTER(ClusterDesc), _i64p, C.POINTER(ClusterEvent),
                                          C.POINTER(ClusterRecord)],
    },
    "cluster_join": {
        "attpc_trace_configure_cluster_join": [_ctxp, C.POINTER(JoinDesc)],
        "attpc_joins_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(JoinEvent), C.POINTER(JoinRecord)],
        "attpc_rows_cluster_join": _rows_in + [C.POINTER(EventLayout), C.POINTER(ClusterDesc), C.POINTER(JoinDesc), _i64p,
                                               C.POINTER(ClusterEvent), C.POINTER(ClusterRecord), C.POINTER(JoinEvent),
                                               C.POINTER(JoinRecord)],
    },
    "pid": {
        "attpc_trace_configure_pid": [_ctxp, C.POINTER(PidDesc)],
        "attpc_pid_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(PidRecord)],
        "attpc_estimates_pid": [_ctxp, C.c_int64, C.c_int32, C.POINTER(TrackEstimate), C.POINTER(PidDesc), C.POINTER(PidRecord)],
        "attpc_rows_fit_pid": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(TrackEstimate), _dp,
                                          C.POINTER(FitDesc), C.POINTER(PidRecord), C.POINTER(TrackFit)],
    },
    "reaction": {
        "attpc_reaction_configure": [_ctxp, C.POINTER(ReactionDesc)],
        "attpc_reaction_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(ReactionRecord)],
        "attpc_reaction_spectra_last": [_ctxp, C.c_int64, C.POINTER(C.c_uint64)],
        "attpc_reaction_records": [_ctxp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ReactionDesc), C.POINTER(TrackFit),
                                   C.POINTER(TrackEstimate), C.POINTER(PidRecord), _dp, _dp, _i32p,
                                   C.POINTER(ReactionRecord), C.c_int64, C.POINTER(C.c_uint64)],
    },
    "hypotheses": {
        "attpc_trace_configure_hypotheses": [_ctxp, C.POINTER(HypothesisDesc)],
        "attpc_hypotheses_last": [_ctxp, C.c_int64, C.c_int64, C.POINTER(FitHypothesis)],
        "attpc_hypothesis_fits_last": [_ctxp, C.c_int64, C.c_int64, _i32p, C.POINTER(TrackFit)],
        "attpc_rows_fit_hypotheses": _rows_in + [C.POINTER(EventLayout), C.POINTER(EstimateDesc), C.POINTER(TrackEstimate), _dp,
                                                 C.POINTER(FitDesc), C.POINTER(HypothesisDesc), C.POINTER(PidRecord),
                                                 C.POINTER(FitHypothesis), C.POINTER(TrackFit), C.POINTER(TrackFit), _i32p, _i32p],
    },
}
(TRACE_ROW_SYMBOLS, SUMMARY_SYMBOLS, SELECT_SYMBOLS, BASELINE_SYMBOLS, TRIGGER_SYMBOLS, GAIN_SYMBOLS, COMMON_SYMBOLS,
 TRACE_PACK_SYMBOLS, MAPS_SYMBOLS, ESTIMATE_SYMBOLS, THIN_SYMBOLS, STRAGGLE_SYMBOLS, CIRCLE_SYMBOLS, HELIX_SYMBOLS,
 DISTORT_SYMBOLS, UNDISTORT_SYMBOLS, FIT_SYMBOLS, CLUSTER_SYMBOLS, JOIN_SYMBOLS, PID_SYMBOLS,
 REACTION_SYMBOLS, HYPOTHESIS_SYMBOLS) = (
     tuple(group) for group in SYMBOL_GROUPS.values())

_lib = None


def load_library() -> C.CDLL:
    """Load libattpc_hip.so and declare prototypes (no device is touched here)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise EngineUnavailable(
            f"HIP engine library not found at {path}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "attpc_engine_amd has no CPU fallback."
        )
    lib = C.CDLL(str(path))
    ctxp = C.c_void_p
    lib.attpc_version.restype = C.c_int32
    if lib.attpc_version() != ABI_VERSION:
        raise EngineUnavailable(
            f"{path} implements ABI version {lib.attpc_version()}, this package needs {ABI_VERSION}: rebuild it "
            "(`python -c 'import __graft_entry__ as g; g.build(force=True)'`)")
    lib.attpc_device_count.restype = C.c_int32
    lib.attpc_ctx_create.argtypes = [C.c_int32, C.POINTER(ctxp)]
    lib.attpc_ctx_destroy.argtypes = [ctxp]
    lib.attpc_last_error.argtypes = [ctxp]
    lib.attpc_last_error.restype = C.c_char_p
    lib.attpc_set_chunk_events.argtypes = [ctxp, C.c_int32]
    lib.attpc_sync.argtypes = [ctxp]
    lib.attpc_kin_configure.argtypes = [ctxp, C.POINTER(KinDesc)]
    lib.attpc_kin_run.argtypes = [
        ctxp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, C.POINTER(C.c_int32),
        C.POINTER(C.c_uint32),
    ]
    lib.attpc_kin_calculate.argtypes = [
        ctxp, C.c_uint64, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32),
    ]
    lib.attpc_decay_calculate.argtypes = [
        ctxp, C.c_uint64, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32),
    ]
    lib.attpc_det_configure.argtypes = [ctxp, C.POINTER(DetDesc)]
    lib.attpc_det_run.argtypes = _run(_det_head, CloudOut)
    lib.attpc_sim_run.argtypes = _run(_sim_head, CloudOut)
    lib.attpc_sim_run_spyral.argtypes = lib.attpc_sim_run.argtypes
    lib.attpc_det_run_spyral.argtypes = lib.attpc_det_run.argtypes
    lib.attpc_sim_hint_next.argtypes = [ctxp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(EventLayout)]
    lib.attpc_spyral_configure.argtypes = [ctxp, C.POINTER(SpyralDesc)]
    lib.attpc_trace_configure.argtypes = [ctxp, C.POINTER(TraceDesc)]
    lib.attpc_sim_run_traces.argtypes = _run(_sim_head, TraceOut)
    lib.attpc_det_run_traces.argtypes = _run(_det_head, TraceOut)
    lib.attpc_traces.argtypes = [ctxp, C.c_int64, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64), C.POINTER(TraceOut)]
    lib.attpc_trace_configure_noise.argtypes = [ctxp, C.POINTER(TraceNoiseDesc)]
    lib.attpc_traces_at.argtypes = _at_head + [C.POINTER(TraceOut)]
    lib.attpc_trace_configure_readout.argtypes = [ctxp, C.POINTER(TraceReadoutDesc)]
    absent = set()  # the symbols of the groups a library named by ATTPC_HIP_LIBRARY lacks altogether
    for group in SYMBOL_GROUPS.values():
        if os.environ.get("ATTPC_HIP_LIBRARY") and not any(hasattr(lib, name) for name in group):
            absent.update(group)
            continue
        for name, argtypes in group.items():
            getattr(lib, name).argtypes = argtypes
    lib.attpc_det_tracks.argtypes = [
        ctxp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(EventLayout), _dp, _dp, C.c_int64,
        _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
    ]
    lib.attpc_det_scatter.argtypes = [
        ctxp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(EventLayout), _dp, C.POINTER(C.c_int32),
        C.POINTER(CloudOut), C.POINTER(RunStats),
    ]
    lib.attpc_set_option.argtypes = [ctxp, C.c_char_p, C.c_int64]
    lib.attpc_host_alloc.argtypes = [ctxp, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.attpc_host_free.argtypes = [ctxp, C.c_void_p]
    lib.attpc_unpack_rows.argtypes = [C.c_void_p, C.c_int64, _dp, C.POINTER(C.c_int64), C.c_int32]
    lib.attpc_unpack_rows8.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.c_uint64, C.c_uint64, _dp,
                                       C.POINTER(C.c_int64), C.c_int32]
    lib.attpc_unpack_spyral_rows.argtypes = [C.c_void_p, C.c_int64, _dp, _dp, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                             C.c_double, _dp, C.POINTER(C.c_int64), C.c_int32]
    lib.attpc_spyral_rows.argtypes = [
        ctxp, C.c_int64, _dp, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_double, _dp,
    ]
    for name in EXPORTED_SYMBOLS:
        if name in absent:
            continue
        fn = getattr(lib, name)
        if fn.restype is C.c_int:  # default -> int32 status
            fn.restype = C.c_int32
    _lib = lib
    return lib


CONFIGURE_SLOTS = ("det", "spyral", "trace", "trace_noise", "trace_common", "trace_readout", "trace_gain", "peaks", "baseline", "trigger", "summary",
                   "select", "maps", "estimates", "thinning", "straggling", "circle", "helix", "distortion", "correction", "fit", "clustering", "cluster_join", "pid",
                   "reaction", "hypotheses")


class Context:
    """One engine context == one HIP device (single-threaded, like the reference objects)."""

    def __init__(self, device: int | None = None):
        self.lib = load_library()
        if device is None:
            device = int(os.environ.get("ATTPC_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        handle = C.c_void_p()
        status = self.lib.attpc_ctx_create(int(device), C.byref(handle))
        if status != OK:
            raise EngineUnavailable(
                f"attpc_ctx_create(device={device}) failed with status {status} "
                "(no HIP device?). attpc_engine_amd has no CPU fallback."
            )
        self.handle = handle
        self.device = device
        self._keepalive: list = []  # host arrays referenced by descriptors during configure
        # what the device holds, as far as this shim uploaded it: a content token per configure slot (None = unknown),
        self._tokens: dict = dict.fromkeys(CONFIGURE_SLOTS)
        self._kin_owner: int | None = None  # id() of the KinematicsPipeline whose tables attpc_kin_configure got,
        self._trace_readout_rows = 0  # and the rows every event keeps in a full trace readout (|S|, else 0)

    def configure(self, slot: str, token, call: str, desc) -> None:
        """``lib.<call>(handle, desc)`` unless ``slot`` already holds the content ``token`` (a context that was never
        configured holds None, which is also the token of "off" for the noise and the readout)."""
        if self._tokens[slot] == token:
            return
        self.check(getattr(self.lib, call)(self.handle, desc), call)
        self._tokens[slot] = token

    def forget(self, slot: str) -> None:
        """Drop the token of ``slot``: for whoever configures through the C ABI directly, after which the token no
        longer describes the device.  KeyError for a name that is not one of CONFIGURE_SLOTS."""
        if slot not in self._tokens:
            raise KeyError(slot)
        self._tokens[slot] = None

    def check(self, status: int, what: str) -> None:
        if status != OK:
            msg = self.lib.attpc_last_error(self.handle)
            text = msg.decode() if msg else ""
            if status == E_CAPACITY:
                raise BufferError(f"{what}: output capacity too small ({text})")
            if status == E_INVALID:
                raise ValueError(f"{what}: {text}")
            if status == E_DATALOSS:
                raise DataLossError(f"{what}: {text}")
            raise RuntimeError(f"{what} failed with status {status}: {text}")

    def trace_rows_last(self) -> dict:
        """Rows and row checksum of this context's last trace-row call (``attpc_trace_rows_last``)."""
        n_rows, checksum = C.c_int64(), C.c_uint64()
        self.check(self.lib.attpc_trace_rows_last(self.handle, C.byref(n_rows), C.byref(checksum)), "attpc_trace_rows_last")
        return {"n_rows": int(n_rows.value), "row_checksum": int(checksum.value)}

    def correction_last(self) -> dict:
        """The counts of the drift correction in this context's last trace-row call (``attpc_correction_last``);
        RuntimeError if the stage was off for it."""
        info = UndistortInfo()
        self.check(self.lib.attpc_correction_last(self.handle, C.byref(info)), "attpc_correction_last")
        return info.as_dict()

    def trigger_last(self, n_events: int) -> np.ndarray:
        """The trigger records [n_events] (``TRIGGER_DTYPE``) of this context's last trace or trace-row call
        (``attpc_trigger_last``); RuntimeError if no trigger was configured for it."""
        records = np.empty(int(n_events), dtype=TRIGGER_DTYPE)
        self.check(self.lib.attpc_trigger_last(self.handle, 0, len(records), iptr(records, TriggerRecord)), "attpc_trigger_last")
        return records

    def estimates_last(self, n_events: int, n_sim: int) -> np.ndarray:
        """The track estimates [n_events, n_sim] (``ESTIMATE_DTYPE``) of this context's last trace-row call
        (``attpc_estimates_last``); RuntimeError if the stage was off for it."""
        records = np.empty((int(n_events), int(n_sim)), dtype=ESTIMATE_DTYPE)
        self.check(self.lib.attpc_estimates_last(self.handle, 0, len(records), iptr(records, TrackEstimate)),
                   "attpc_estimates_last")
        return records

    def set_option(self, name: str, value: int) -> None:
        """Tuning / test switches of the context (``attpc_set_option``)."""
        self.check(self.lib.attpc_set_option(self.handle, name.encode(), int(value)), f"attpc_set_option({name})")

    def pinned_empty(self, shape, dtype=np.float64) -> np.ndarray:
        """Uninitialised numpy array in page-locked host memory (``attpc_host_alloc``): device-to-host
        copies into it run at the PCIe rate.  The memory is returned when the array (and every view of
        it) is garbage collected, or with the context."""
        import weakref

        dtype = np.dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n_bytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        ptr = C.c_void_p()
        self.check(self.lib.attpc_host_alloc(self.handle, max(1, n_bytes), C.byref(ptr)), "attpc_host_alloc")
        raw = (C.c_char * max(1, n_bytes)).from_address(ptr.value)
        arr = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        lib, handle_ref, address = self.lib, weakref.ref(self), ptr.value

        def release():
            ctx = handle_ref()
            if ctx is not None and getattr(ctx, "handle", None):
                lib.attpc_host_free(ctx.handle, C.c_void_p(address))

        weakref.finalize(raw, release)
        return arr

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.attpc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx
