"""Digitised GET pad traces on the device (EXTENSION: the reference stops at point clouds, its user guide's "Why Point
clouds").  The contract -- integer time bucket of every row, f64 sum of q * R in ascending t without fused multiply-add,
4095 clip of the summed signal, rint half to even, strict ADC threshold on the pad's largest sample, label of the pad's
largest charge -- is written out in include/attpc_engine.h; ``tests/trace_reference.py`` restates it in numpy.

``simulate_batch_traces`` is ``simulate_batch`` with the traces made on the device behind the scatter
(``attpc_det_run_traces``); ``clouds_to_traces`` turns any host cloud into traces (``attpc_traces_at``).

Electronic noise and per-pad pedestals are opt-in (``noise_sigma`` or ``noise_table``, ``pedestals``, ``noise_stream``):
every sample gets its pad's pedestal and one draw from a discrete noise table, a pure function of (seed, global event id,
pad, sample), and the threshold is taken above the pedestal (include/attpc_engine.h; ``tests/trace_noise_reference.py``
restates it).  ``gaussian_noise_table`` builds the table of a discretised Gaussian.

The readout of noise-only pads is opt-in too (``readout="partial"`` or ``"full"``, ``readout_pads``): in partial readout
(zero suppression) every pad of the readout set whose noise crosses the threshold is read out as well, with label -1;
in full readout every pad of the set is (include/attpc_engine.h; ``tests/readout_reference.py`` restates it).
``expected_noise_pads`` gives the mean number of noise-only pads a partial readout keeps per event.

Trace rows are the step after the traces, still on the device (``PeakSettings``, ``simulate_batch_trace_rows``,
``clouds_to_trace_rows``): the peaks of every kept pad trace above its pedestal -- separation, prominence, width and
amplitude threshold as in the first phase of Spyral -- as Spyral rows of eight columns in ascending z
(include/attpc_engine.h; ``tests/peaks_reference.py`` restates it).  Every trace setting above composes with them.

The Fourier baseline is opt-in on top of them (``BaselineSettings``, ``baseline=`` beside ``peaks=``): instead of being
handed every pad's true pedestal, the peak stage gets Spyral's own estimate of the baseline -- a low-pass filter of the
trace with its peaks masked out, which takes part of a wide pulse for baseline -- made on the device
(include/attpc_engine.h; ``tests/baseline_reference.py`` restates it).  ``remove_baseline`` is that stage alone on any
host rows.

The multiplicity trigger is opt-in beside all of them (``TriggerSettings``, ``trigger=``): would the GET electronics
have triggered on the event, and when -- a discriminator per pad, the multiplicity of every trigger group summed over a
sliding window, a number of groups required --, evaluated on the device on the kept traces; one 32-byte record per
event comes back (``TRIGGER_DTYPE``; include/attpc_engine.h; ``tests/trigger_reference.py`` restates it).
``traces_to_trigger`` is that stage alone on any host rows.

The micromegas gain is opt-in in front of all of them (``GainSettings``, ``gain=``): the avalanche statistics of the
amplification (a Polya single-electron gain of relative variance f = 1 / (1 + theta), so that a bucket of q electrons
has a relative amplitude spread of sqrt(f / q)) and a per-pad gain map, applied on the device to every cloud row's
charge before the trace kernels read it -- a pure function of (seed, global event id, pad, time bucket, charge)
(include/attpc_engine.h; ``tests/gain_reference.py`` restates it).  ``clouds_to_gain`` is that stage alone on any host
cloud.

Common-mode noise is opt-in beside the pad noise (``CommonModeSettings``, ``common_mode=``): one further table-driven
draw per (event, group, sample), added to every pad of the group before the clamp -- the coherent part of the GET
noise, which lifts a whole chip or board over a threshold in the same sample.  The pad -> group map is the caller's
(include/attpc_engine.h; ``tests/common_mode_reference.py`` restates it).  ``common_mode_values`` is that stage alone.

Every stage is a settings class with its context slot (``slot``), its C call (``call``), ``token()`` -- its content,
None when the stage changes nothing -- and ``desc()``, the call's descriptor; ``detector.stage.configure_stage`` applies
any of them.  ``TraceChain`` is one whole trace configuration, validated once: the entry points build it from their
keywords, the writers hold one, the runs configure it in the order of ``STAGES`` and collect their results with
``stage_results``.  Adding a trace stage: its own module (the settings class, its configure and result functions, its
host-row operator), one row of ``STAGES`` here, one group of ``_abi.SYMBOL_GROUPS`` (with its slot in
``_abi.CONFIGURE_SLOTS`` and its descriptor structs), and its own functions in csrc/abi.hip and include/attpc_engine.h.
Its keyword is then spelt out where it is public API: in the signatures of ``TraceChain``, ``configure_trace_rows`` and
``simulate_batch_trace_rows``, each of which hands it on by name, and in ``REPLACE_FIELDS``; ``Engine`` has a documented
``configure_*`` method per stage.  tests/test_trace_chain_cpu.py holds every row of ``STAGES`` to these places.
"""
from __future__ import annotations

import collections
import copy
import math
import statistics

import numpy as np

from .. import _abi
from ..outputs import PackedTraceArrays, RowArrays, TraceArrays, call_with_capacity  # noqa: F401 (TraceArrays stays importable from here)
from .circle import CircleFitSettings, circle_result, configure_circle
from .clustering import ClusterSettings, clustering_result, configure_clustering
from .correction import CorrectionSettings, configure_correction, correction_result
from .estimate import EstimateSettings, configure_estimates, estimates_result
from .fit import TrackFitSettings, configure_track_fit, fit_result
from .helix import HelixSlopeSettings, configure_helix, helix_result
from .joining import JoinSettings, configure_cluster_join, join_result
from .parameters import Config
from .pid import PidSettings, configure_pid, pid_result
from .stage import checked, configure_stage  # noqa: F401 (configure_stage stays importable from here)
from .thinning import ThinSettings, configure_thinning, thinning_result


def trace_settings(config: Config, response=None, threshold=None, offset: int = 0):
    """(response [512] f64, threshold, offset) with the defaults filled in: get_response(config) and
    ``ElectronicsParams.adc_threshold``."""
    from .response import get_response

    response = np.ascontiguousarray(get_response(config) if response is None else response, dtype=np.float64)
    if response.shape != (_abi.NUM_TB,):
        raise ValueError(f"response must have {_abi.NUM_TB} samples, got shape {response.shape}")
    threshold = float(config.elec_params.adc_threshold if threshold is None else threshold)
    return response, threshold, int(offset)


def gaussian_noise_table(sigma: float) -> tuple[np.ndarray, int]:
    """Noise table (cdf [2L] u32, min_level = -L) of rint(sigma * z), z standard normal, on the levels -L .. L with
    L = ceil(8 sigma); the tails beyond are folded into the end levels.  The cdf entry below level m + 1 is
    2^32 P(sigma z < m + 0.5), the lower half from ``math.erfc`` and the upper half its mirror image, so the level masses
    are exactly symmetric (each end level keeps at least 2^-32).  ``sigma = 0``: no noise (an empty cdf, min_level 0).
    ValueError for a negative or non-finite sigma and for L > 255 (more than ATTPC_MAX_NOISE_LEVELS levels)."""
    sigma = float(sigma)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError(f"noise sigma must be finite and >= 0, got {sigma}")
    if sigma == 0.0:
        return np.zeros(0, dtype=np.uint32), 0
    half = math.ceil(8.0 * sigma)
    if 2 * half + 1 > _abi.MAX_NOISE_LEVELS:
        raise ValueError(f"noise sigma {sigma} needs {2 * half + 1} levels, at most {_abi.MAX_NOISE_LEVELS}")
    scale = sigma * math.sqrt(2.0)
    lower = [max(1, round(0.5 * math.erfc((half - k - 0.5) / scale) * 2.0 ** 32)) for k in range(half)]
    cdf = lower + [(1 << 32) - c for c in reversed(lower)]
    return np.array(cdf, dtype=np.uint32), -half


def _noise_table(what: str, sigma, table):
    """(cdf u32, min_level, n_levels, sigma) of a noise table given as the Gaussian of ``sigma`` or as ``table`` =
    (cdf, min_level), under the rules of ``NoiseSettings`` (``what`` names the table in the messages)."""
    if table is not None and float(sigma) != 0.0:
        raise ValueError(f"give the {what} sigma or its table, not both")
    if table is None:
        cdf, min_level = gaussian_noise_table(sigma)
        sigma = float(sigma)
    else:
        cdf, min_level = table
        sigma = math.nan
    cdf = np.asarray(cdf)
    if cdf.ndim != 1 or (cdf.size and (cdf.dtype.kind not in "iu" or cdf.min() < 0 or cdf.max() >= 1 << 32)):
        raise ValueError(f"the {what} cdf must be a 1-D array of integers in [0, 2^32)")
    if cdf.size + 1 > _abi.MAX_NOISE_LEVELS:
        raise ValueError(f"a {what} table of {cdf.size + 1} levels: at most {_abi.MAX_NOISE_LEVELS}")
    cdf = np.ascontiguousarray(cdf, dtype=np.uint32)
    if np.any(np.diff(cdf.astype(np.int64)) < 0):
        raise ValueError(f"the {what} cdf decreases")
    if int(min_level) != min_level or not -4095 <= int(min_level) <= 4095:
        raise ValueError(f"{what} min_level must be an integer in -4095 .. 4095, got {min_level}")
    n_levels = cdf.size + 1 if (cdf.size or int(min_level)) else 0
    return cdf, int(min_level), n_levels, (sigma if n_levels else 0.0)


class NoiseSettings:
    """The validated noise of a trace configuration: cdf [n_levels - 1] u32, min_level, n_levels (0 = no noise draw),
    pedestals [ATTPC_NUM_PADS] i16 or None, stream, sigma (NaN for a custom table, 0 without noise)."""

    slot, call = "trace_noise", "attpc_trace_configure_noise"

    def __init__(self, noise_sigma: float = 0.0, noise_table=None, pedestals=None, noise_stream: int = 0):
        self.cdf, self.min_level, self.n_levels, self.sigma = _noise_table("noise", noise_sigma, noise_table)
        if pedestals is not None:
            ped = np.broadcast_to(np.asarray(pedestals), (_abi.NUM_PADS,))
            if ped.dtype.kind not in "iu" or ped.min() < 0 or ped.max() > 4095:
                raise ValueError(f"pedestals must be {_abi.NUM_PADS} integers in 0 .. 4095")
            pedestals = np.ascontiguousarray(ped, dtype=np.int16)
        self.pedestals = pedestals
        if int(noise_stream) != noise_stream or not 0 <= int(noise_stream) < 1 << 31:
            raise ValueError(f"noise_stream must be an integer in [0, 2^31), got {noise_stream}")
        self.stream = int(noise_stream)

    @property
    def on(self) -> bool:
        """Anything added to the noiseless samples."""
        return self.n_levels > 0 or self.pedestals is not None

    def token(self):
        if not self.on:
            return None
        return (self.cdf.tobytes(), self.min_level, self.n_levels, None if self.pedestals is None else
                self.pedestals.tobytes(), self.stream)

    def desc(self) -> _abi.TraceNoiseDesc:
        """(the descriptor points into ``self.cdf`` and ``self.pedestals``: keep the settings alive over the call)"""
        return _abi.TraceNoiseDesc(_abi.iptr(self.cdf, _abi.C.c_uint32), self.n_levels, self.min_level,
                                   _abi.iptr(self.pedestals, _abi.C.c_int16), self.stream, 0)


def configure_noise(ctx: _abi.Context, noise: NoiseSettings) -> None:
    """``attpc_trace_configure_noise`` unless this ctx already holds the same noise (decided on its content)."""
    configure_stage(ctx, NoiseSettings, noise)


class CommonModeSettings:
    """The validated common-mode noise of the traces (``attpc_trace_common_desc``, include/attpc_engine.h): the table of
    its own as ``sigma`` (``gaussian_noise_table``) or ``table`` = (cdf, min_level) under the rules of the pad noise's,
    ``groups`` ([ATTPC_NUM_PADS] uint8: below 255 the pad's group -- its chip or board; the map is the caller's --,
    255 = the pad has no common-mode term; None = every pad in group 0) and ``stream`` in [0, 2^29) (another
    realisation).  ``cdf``, ``min_level``, ``n_levels`` (0 = off) and ``n_groups`` (1 + the highest group) are the
    results."""

    slot, call = "trace_common", "attpc_trace_configure_common_mode"

    def __init__(self, sigma: float = 0.0, table=None, groups=None, stream: int = 0):
        self.cdf, self.min_level, self.n_levels, self.sigma = _noise_table("common-mode", sigma, table)
        if groups is not None:
            g = np.asarray(groups)
            if g.shape != (_abi.NUM_PADS,) or g.dtype != np.uint8:
                raise ValueError(f"common-mode groups must be {_abi.NUM_PADS} uint8, got {g.dtype} {g.shape}")
            groups = np.ascontiguousarray(g)
        self.groups = groups
        if isinstance(stream, (bool, np.bool_)) or int(stream) != stream or not 0 <= int(stream) < 1 << 29:
            raise ValueError(f"common-mode stream must be an integer in [0, 2^29), got {stream!r}")
        self.stream = int(stream)

    @property
    def n_groups(self) -> int:
        """1 + the highest group of the map (0: no pad has a group)."""
        if self.groups is None:
            return 1
        used = self.groups[self.groups != 255]
        return int(used.max()) + 1 if used.size else 0

    @property
    def on(self) -> bool:
        """Anything added to a sample."""
        return self.n_levels > 0 and self.n_groups > 0

    def level_masses(self):
        """(levels, their probabilities) of the table; the one level 0 when the stage is off."""
        return _level_masses(self.cdf, self.min_level) if self.on else (np.zeros(1, dtype=np.int64), np.ones(1))

    def token(self):
        if not self.on:
            return None
        return (self.cdf.tobytes(), self.min_level, self.n_levels, None if self.groups is None else self.groups.tobytes(),
                self.stream)

    def desc(self) -> _abi.TraceCommonDesc:
        """(the descriptor points into ``self.groups`` and ``self.cdf``: keep the settings alive over the call)"""
        return _abi.TraceCommonDesc(_abi.iptr(self.groups, _abi.C.c_uint8), _abi.iptr(self.cdf, _abi.C.c_uint32),
                                    self.n_levels, self.min_level, self.stream, 0)


def configure_common_mode(ctx: _abi.Context, common_mode: CommonModeSettings | None) -> None:
    """``attpc_trace_configure_common_mode`` unless this ctx already holds the same setting (``None``, or one without
    effect: off)."""
    configure_stage(ctx, CommonModeSettings, checked(CommonModeSettings, common_mode, "common_mode"))


def common_mode_values(n_events: int, common_mode: CommonModeSettings, seed: int = 0, first_event: int = 0,
                       ctx: _abi.Context | None = None) -> np.ndarray:
    """The common-mode stage alone (``attpc_common_mode_rows``; the kernel of the fused path, no other configuration
    needed): c_g[j] of the global events ``first_event`` .. as [n_events, n_groups, 512] int16.  ``common_mode`` is
    configured first; one that is off gives zeros."""
    if not isinstance(common_mode, CommonModeSettings):
        raise TypeError("common_mode must be a CommonModeSettings")
    seed, first_event, n = _abi.check_id_range(seed, first_event, int(n_events))
    ctx = ctx or _abi.default_context()
    configure_common_mode(ctx, common_mode)
    out = np.zeros((n, common_mode.n_groups, _abi.NUM_TB), dtype=np.int16)
    if common_mode.on and n:
        ctx.check(ctx.lib.attpc_common_mode_rows(ctx.handle, seed, first_event, n, _abi.iptr(out, _abi.C.c_int16)),
                  "attpc_common_mode_rows")
    return out


def _level_masses(cdf, min_level: int):
    """(levels [n], probabilities [n]) of a noise table: level min_level + i has 2^-32 (cdf[i] - cdf[i - 1]), with
    cdf[-1] = 0 and cdf[n - 1] = 2^32."""
    edges = np.concatenate(([0], np.asarray(cdf, dtype=np.int64), [1 << 32]))
    return int(min_level) + np.arange(len(edges) - 1, dtype=np.int64), np.diff(edges) / 2.0 ** 32


READOUT_MODES = {"hit": _abi.READOUT_HIT, "partial": _abi.READOUT_PARTIAL, "full": _abi.READOUT_FULL}


def readout_mask(readout_pads=None) -> np.ndarray:
    """The readout set as a uint8 mask [ATTPC_NUM_PADS]: ``None`` = every pad not in BEAM_PADS (the reference drops
    their charge, transporter.py:164, 237), a boolean mask of ATTPC_NUM_PADS entries, or unique pad ids."""
    from .beam_pads import BEAM_PADS_ARRAY

    if readout_pads is None:
        mask = np.ones(_abi.NUM_PADS, dtype=np.uint8)
        mask[BEAM_PADS_ARRAY] = 0
        return mask
    pads = np.asarray(readout_pads)
    if pads.dtype == np.bool_:
        if pads.shape != (_abi.NUM_PADS,):
            raise ValueError(f"a readout_pads mask needs {_abi.NUM_PADS} entries, got shape {pads.shape}")
        return pads.astype(np.uint8)
    if pads.ndim != 1 or (pads.size and pads.dtype.kind not in "iu"):
        raise ValueError("readout_pads must be a boolean mask or a 1-D array of pad ids")
    if pads.size and (pads.min() < 0 or pads.max() >= _abi.NUM_PADS):
        raise ValueError(f"readout_pads ids must lie in 0 .. {_abi.NUM_PADS - 1}")
    if np.unique(pads).size != pads.size:
        raise ValueError("readout_pads ids repeat")
    mask = np.zeros(_abi.NUM_PADS, dtype=np.uint8)
    mask[pads.astype(np.int64)] = 1
    return mask


class ReadoutSettings:
    """The validated readout of a trace configuration: ``name`` ("hit", "partial", "full"), ``mode``
    (ATTPC_READOUT_*), ``channels`` uint8 [ATTPC_NUM_PADS] (the readout set S, ignored in hit mode)."""

    slot, call = "trace_readout", "attpc_trace_configure_readout"

    def __init__(self, readout: str = "hit", readout_pads=None):
        if readout not in READOUT_MODES:
            raise ValueError(f"readout must be one of {sorted(READOUT_MODES)}, got {readout!r}")
        self.name = readout
        self.mode = READOUT_MODES[readout]
        self.channels = np.ascontiguousarray(readout_mask(readout_pads))

    @property
    def pads(self) -> np.ndarray:
        """The pad ids of S, ascending."""
        return np.flatnonzero(self.channels).astype(np.int32)

    def rows_per_event(self) -> int:
        """Kept rows of every event when known in advance: |S| in full readout, else 0."""
        return int(self.channels.sum()) if self.mode == _abi.READOUT_FULL else 0

    def token(self):
        return None if self.mode == _abi.READOUT_HIT else (self.mode, self.channels.tobytes())

    def desc(self) -> _abi.TraceReadoutDesc:
        """(the descriptor points into ``self.channels``: keep the settings alive over the call)"""
        return _abi.TraceReadoutDesc(self.mode, 0, _abi.iptr(self.channels, _abi.C.c_uint8))


def configure_readout(ctx: _abi.Context, readout: ReadoutSettings) -> None:
    """``attpc_trace_configure_readout`` unless this ctx already holds the same readout (decided on its content)."""
    configure_stage(ctx, ReadoutSettings, readout)
    ctx._trace_readout_rows = readout.rows_per_event()


def readout_cutoff(cdf, min_level: int, threshold: float):
    """The cutoff of the readout's decision rule (include/attpc_engine.h) -> ("always" | "never" | "draw", cut): with
    c = floor(thr) + 1 - min_level, max_j n_j > thr always (c <= 0), never (c > n_levels - 1; no table: the one level
    0) or iff some u_j >= cut = cdf[c - 1]."""
    cdf = np.asarray(cdf, dtype=np.uint32)
    n_levels = cdf.size + 1 if (cdf.size or min_level) else 1
    thr = min(max(float(threshold), -16384.0), 16384.0)
    c = math.floor(thr) + 1 - int(min_level)
    if c <= 0:
        return "always", 0
    if c > n_levels - 1:
        return "never", 0
    return "draw", int(cdf[c - 1])


def expected_noise_pads(noise_table, threshold: float, readout_pads=None, pedestals=None, common_mode=None) -> float:
    """The mean number of noise-only pads a partial readout keeps per event: sum over the pads p of the readout set of
    1 - (1 - q_p)^512, q_p the exact probability 2^-32 (2^32 - cut) that one draw reaches the cutoff of the decision
    rule, with its pedestal terms (a pad with 4095 - ped_p <= thr is never kept, one with -ped_p > thr always).
    ``noise_table``: (cdf, min_level), or None for no noise; ``readout_pads`` and ``pedestals`` as configure_traces
    takes them.  ``common_mode`` (a ``CommonModeSettings``; None = off): for a pad with a group the per-sample probability
    is P(n + c > thr), from the convolution of the two tables' level masses; the pad's probability is still
    1 - (1 - q)^512, its 512 sums being independent, and the mean over the pads is still their sum.  The pads of a group
    share their common-mode draws and are correlated, so the number of kept pads does not have the binomial variance."""
    cdf, min_level = (np.zeros(0, dtype=np.uint32), 0) if noise_table is None else noise_table
    noise = NoiseSettings(noise_table=(cdf, min_level), pedestals=pedestals)
    mask = readout_mask(readout_pads).astype(bool)
    ped = np.zeros(_abi.NUM_PADS, dtype=np.int64) if noise.pedestals is None else noise.pedestals.astype(np.int64)
    thr = float(threshold)
    kind, cut = readout_cutoff(noise.cdf, noise.min_level, thr)
    if kind == "draw":
        q = (2.0 ** 32 - cut) / 2.0 ** 32
        p_draw = -math.expm1(_abi.NUM_TB * math.log1p(-q)) if q < 1.0 else 1.0
    else:
        p_draw = 1.0 if kind == "always" else 0.0
    p_draw = np.full(_abi.NUM_PADS, p_draw)
    if checked(CommonModeSettings, common_mode, "common_mode") is not None and common_mode.on:
        levels, mass = _level_masses(noise.cdf, noise.min_level) if noise.n_levels else (np.zeros(1, dtype=np.int64), np.ones(1))
        c_levels, c_mass = common_mode.level_masses()
        over = (levels[:, None] + c_levels[None, :]) > thr
        q = min(float((mass[:, None] * c_mass[None, :])[over].sum()), 1.0)
        grouped = np.ones(_abi.NUM_PADS, dtype=bool) if common_mode.groups is None else common_mode.groups != 255
        p_draw[grouped] = -math.expm1(_abi.NUM_TB * math.log1p(-q)) if q < 1.0 else 1.0
    p = np.where(4095 - ped > thr, np.where(-ped > thr, 1.0, p_draw), 0.0)
    return float(p[mask].sum())


TRACE_KWARGS = ("response", "threshold", "offset", "noise_sigma", "noise_table", "pedestals", "noise_stream", "readout",
                "readout_pads")


def configure_traces(config: Config, ctx: _abi.Context, response=None, threshold=None, offset: int = 0,
                     noise_sigma: float = 0.0, noise_table=None, pedestals=None, noise_stream: int = 0,
                     readout: str = "hit", readout_pads=None) -> None:
    """Upload the response, ADC threshold and sample offset of the traces, and their noise (off by default), unless this
    ctx already holds the same ones (decided on their content, as configure_spyral).  ``noise_table``: (cdf, min_level)
    instead of the Gaussian of ``noise_sigma``; ``pedestals``: [ATTPC_NUM_PADS] (or one value for every pad) in
    0 .. 4095; ``noise_stream`` in [0, 2^31) draws another noise realisation.  ``readout``: "hit" (default: only pads
    with cloud rows), "partial" (noise-only pads of ``readout_pads`` that cross the threshold too) or "full" (every pad
    of ``readout_pads``); ``readout_pads``: None = every pad not in BEAM_PADS, a boolean mask [ATTPC_NUM_PADS] or
    unique pad ids.  Everything is validated before the first call to the library; the trigger, the gain and the
    common-mode noise stay as the ctx holds them."""
    chain = TraceChain(config, response, threshold, offset, NoiseSettings(noise_sigma, noise_table, pedestals, noise_stream),
                       ReadoutSettings(readout, readout_pads))
    chain.configure(ctx, keep=("trigger", "gain", "common_mode"))


def validate_trace_kwargs(config: Config, trace_kwargs: dict, gain=None) -> None:
    """The trace settings a caller passes on as keywords (``configure_traces``'s, TRACE_KWARGS), checked before any
    library call: TypeError for a name configure_traces does not take, ValueError for a value it would refuse.
    ``gain``: the ``GainSettings`` that goes with them (or None), TypeError for anything else."""
    checked(GainSettings, gain, "gain")
    TraceChain.from_kwargs(config, **trace_kwargs)


def simulate_batch_traces(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config,
                          seed: int, indices: list[int], first_event: int = 0, ctx: _abi.Context | None = None,
                          response=None, threshold=None, offset: int = 0, capacity_per_event: int = 1024,
                          noise_sigma: float = 0.0, noise_table=None, pedestals=None, noise_stream: int = 0,
                          readout: str = "hit", readout_pads=None, trigger: TriggerSettings | None = None,
                          gain: GainSettings | None = None, common_mode: CommonModeSettings | None = None,
                          packed: bool = False, straggling=None, distortion=None):
    """simulate() + the pad traces of every event, on the device (``attpc_det_run_traces``; the noise keyed on
    ``seed`` and the global event ids; ``readout`` / ``readout_pads`` as configure_traces) ->
    (offsets [n+1], pads [R] i32, samples [R,512] i16, labels [R] i64, event_points [n] = cloud rows of every event
    before the suppression, stats dict: the cloud's run statistics plus ``n_rows`` / ``sample_checksum`` /
    ``pad_checksum`` of the traces, and with ``trigger`` (a ``TriggerSettings``; None = off) its records [n] under
    ``"trigger"``).  ``gain`` (a ``GainSettings``; None = off): the micromegas gain of every cloud row's charge, keyed on
    ``seed`` and the global event ids like the noise.  ``common_mode`` (a ``CommonModeSettings``; None = off): the
    common-mode noise of every pad with a group, keyed the same way.  ``packed=True``
    (``attpc_det_run_traces_packed``): (offsets, pads, row_start [R+1] i64, packed uint8, labels, event_points, stats
    with ``n_bytes``) -- the rows as packed records, ``unpack_traces`` gives the samples back.  ``straggling`` (a
    ``detector.straggling.StragglingSettings``; None = off): multiple scattering and energy-loss straggling of the tracks.
    ``distortion`` (a ``detector.distortion.DistortionMap``; None = off): the drift distortion of the track samples."""
    chain = TraceChain(config, response, threshold, offset, NoiseSettings(noise_sigma, noise_table, pedestals, noise_stream),
                       ReadoutSettings(readout, readout_pads), gain, trigger=trigger, common_mode=common_mode)
    return chain.run_batch(False, momenta, vertices, proton_numbers, mass_numbers, seed, indices, first_event, ctx,
                           capacity_per_event, packed, straggling=straggling, distortion=distortion)


def _host_cloud(offsets, points, labels, seed, first_event):
    """A host cloud in CSR form as the C ABI takes it, checked: (offsets i64, points [P,3] f64, labels i64 or None,
    seed, first_event, n events)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(offsets) - 1
    if n < 0:
        raise ValueError("offsets needs n_events + 1 entries")
    seed, first_event, _ = _abi.check_id_range(seed, first_event, n)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
    if (labels is not None and len(points) != len(labels)) or (n and offsets[-1] > len(points)):
        raise ValueError(f"points{'' if labels is None else ' / labels'} do not hold the rows the offsets name")
    return offsets, points, labels, seed, first_event, n


def clouds_to_traces(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, ctx: _abi.Context, seed: int = 0,
                     first_event: int = 0, packed: bool = False):
    """Pad traces of any host cloud in CSR form (``attpc_traces_at``; ``ctx`` configured with ``configure_traces``):
    offsets [n+1], points [P,3] (pad, time bucket, electrons), labels [P] ->
    (offsets [n+1], pads [R] i32, samples [R,512] i16, labels [R] i64, {n_rows, sample_checksum, pad_checksum}; when
    the ctx holds a trigger (``configure_trigger``) its records [n] too, under ``"trigger"``).
    Event i of the call is the global event ``first_event + i``: its noise is keyed on (seed, first_event + i), and the
    pad checksum counts events from ``first_event``.  ``packed=True`` (``attpc_traces_packed_at``): (offsets, pads,
    row_start [R+1] i64, packed uint8, labels, sums with ``n_bytes``)."""
    offsets, points, labels, seed, first_event, n = _host_cloud(offsets, points, labels, seed, first_event)
    packed = _packed_flag(packed)
    name = "attpc_traces_packed_at" if packed else "attpc_traces_at"

    def call(out):
        return getattr(ctx.lib, name)(ctx.handle, seed, first_event, n, _abi.iptr(offsets, _abi.C.c_int64),
                                      _abi.dptr(points), _abi.iptr(labels, _abi.C.c_int64), out)

    rows = int(offsets[-1] - offsets[0]) if n else 0
    rows = max(16, rows, ctx._trace_readout_rows * n)  # full readout: |S| rows per event
    how = dict(holder=PackedTraceArrays, byte_capacity=PACKED_BYTES_PER_ROW * rows) if packed else {}
    arrays = call_with_capacity(ctx, n, rows, call, name, **how)
    return (*arrays.result(), {**arrays.sums(), **trigger_result(ctx, n)})


# ---- packed pad traces (include/attpc_engine.h, "packed pad traces") ----
TRACE_PACK_FORMAT = _abi.TRACE_PACK_FORMAT
PACKED_BYTES_PER_ROW = 512  # the byte capacity a packed call first tries, per row of its row capacity (a row: 16 .. 784)


def _packed_flag(packed) -> bool:
    if not isinstance(packed, (bool, np.bool_)):
        raise TypeError(f"packed must be a bool, got {packed!r}")
    return bool(packed)


class PackedRows:
    """``row_start`` / ``packed`` of a packed call as one row-indexed sequence: ``rows[lo:hi]`` is the same for rows
    lo .. hi - 1 (views, nothing is copied or decoded) -- what an event loop slices beside pads and labels."""

    def __init__(self, row_start, packed):
        self.row_start, self.packed = row_start, packed

    def __len__(self) -> int:
        return len(self.row_start) - 1

    def __getitem__(self, rows: slice) -> "PackedRows":
        lo, hi, step = rows.indices(len(self))
        if step != 1:
            raise IndexError("PackedRows takes slices of step 1")
        return PackedRows(self.row_start[lo:max(hi, lo) + 1], self.packed)

    def samples(self, n_threads: int = 0) -> np.ndarray:
        return unpack_traces(self.row_start, self.packed, n_threads=n_threads)


def _sample_rows(samples) -> np.ndarray:
    samples = np.asarray(samples)
    if samples.dtype.kind not in "iu":
        raise TypeError(f"samples must be integers, got {samples.dtype}")
    if samples.ndim != 2 or samples.shape[1] != _abi.NUM_TB:
        raise ValueError(f"samples must be [R, {_abi.NUM_TB}], got {samples.shape}")
    if samples.size and (samples.min() < 0 or samples.max() > 4095):
        raise ValueError("samples must lie in 0 .. 4095")
    return np.ascontiguousarray(samples, dtype=np.int16)


def _pack(samples, call, check):
    samples = _sample_rows(samples)
    n = len(samples)
    row_start = np.zeros(n + 1, dtype=np.int64)
    n_bytes = _abi.C.c_int64()
    i16, i64, u8 = _abi.C.c_int16, _abi.C.c_int64, _abi.C.c_uint8
    packed = np.empty(max(8, n * _abi.TRACE_PACK_MAX_ROW_BYTES), dtype=np.uint8)  # (the most the rows can take: one call)
    check(call(n, _abi.iptr(samples, i16), _abi.iptr(row_start, i64), _abi.iptr(packed, u8), len(packed), _abi.C.byref(n_bytes)))
    return row_start, packed[:int(n_bytes.value)].copy()


def pack_traces(samples, ctx: _abi.Context | None = None):
    """The pack stage alone, on the device (``attpc_trace_pack``: the two kernels of the packed runs): samples [R,512]
    integers in 0 .. 4095 (ValueError otherwise) -> (row_start [R+1] i64, packed uint8)."""
    ctx = ctx or _abi.default_context()
    return _pack(samples, lambda *a: ctx.lib.attpc_trace_pack(ctx.handle, *a), lambda status: ctx.check(status, "attpc_trace_pack"))


def _check_host(what: str):
    def check(status):
        if status != _abi.OK:
            raise ValueError(f"{what}: refused (status {status}): malformed records, offsets or samples")
    return check


def pack_traces_host(samples):
    """The same encoder on the host (``attpc_trace_pack_host``: no context, no GPU) -> (row_start, packed)."""
    return _pack(samples, _abi.load_library().attpc_trace_pack_host, _check_host("attpc_trace_pack_host"))


def unpack_traces(row_start, packed, rows=None, n_threads: int = 0) -> np.ndarray:
    """Packed records -> samples [R,512] int16, on the host (``attpc_trace_unpack``; ``n_threads`` 0 = automatic).
    ``rows``: a slice (step 1) or an index array of the rows to decode -- one event of a run is
    ``slice(offsets[e], offsets[e + 1])`` -- default all.  ValueError for records the decoder refuses."""
    row_start = np.ascontiguousarray(row_start, dtype=np.int64)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if row_start.ndim != 1 or len(row_start) < 1:
        raise ValueError("row_start needs R + 1 entries")
    n_all = len(row_start) - 1
    if rows is None:
        rows = slice(0, n_all)
    if isinstance(rows, slice):
        lo, hi, step = rows.indices(n_all)
        if step != 1:
            rows = np.arange(lo, hi, step)
        else:
            starts = row_start[lo:max(hi, lo) + 1]
    if not isinstance(rows, slice):
        index = np.asarray(rows)
        if index.dtype == bool:
            index = np.flatnonzero(index)
        index = np.where(index < 0, index + n_all, index).astype(np.int64).reshape(-1)
        if index.size and (index.min() < 0 or index.max() >= n_all):
            raise IndexError("rows out of range")
        # the named records side by side in a byte array of their own
        begin, size = row_start[index], row_start[index + 1] - row_start[index]
        if (size < 0).any() or (begin < 0).any() or (index.size and (begin + size).max() > len(packed)):
            raise ValueError("attpc_trace_unpack: offsets outside the packed bytes")
        starts = np.zeros(len(index) + 1, dtype=np.int64)
        np.cumsum(size, out=starts[1:])
        gather = np.repeat(begin - starts[:-1], size) + np.arange(int(starts[-1]))
        packed = np.ascontiguousarray(packed[gather])
    starts = np.ascontiguousarray(starts)
    out = np.empty((len(starts) - 1, _abi.NUM_TB), dtype=np.int16)
    lib = _abi.load_library()
    status = lib.attpc_trace_unpack(_abi.iptr(packed, _abi.C.c_uint8), len(packed), _abi.iptr(starts, _abi.C.c_int64), len(out),
                                    _abi.iptr(out, _abi.C.c_int16), int(n_threads))
    _check_host("attpc_trace_unpack")(status)
    return out


class PeakSettings:
    """The validated peak parameters of the trace rows (``attpc_peak_desc``, include/attpc_engine.h): ``separation``
    (>= 1 samples between kept peaks), ``prominence`` (>= 0), ``min_width`` <= ``max_width`` (>= 0, samples at
    ``rel_height`` in (0, 1] of the prominence) and the amplitude ``threshold`` above the pedestal.  The defaults are
    this project's (they fit its GET response: a lone arrival is one peak 15.5 samples wide)."""

    slot, call = "peaks", "attpc_trace_configure_peaks"

    def __init__(self, separation: float = 50.0, prominence: float = 20.0, min_width: float = 1.0,
                 max_width: float = 50.0, rel_height: float = 0.95, threshold: float = 40.0):
        values = [float(v) for v in (separation, prominence, min_width, max_width, rel_height, threshold)]
        self.separation, self.prominence, self.min_width, self.max_width, self.rel_height, self.threshold = values
        if not self.separation >= 1.0:
            raise ValueError(f"peak separation must be >= 1, got {separation}")
        if not self.prominence >= 0.0:
            raise ValueError(f"peak prominence must be >= 0, got {prominence}")
        if not 0.0 <= self.min_width <= self.max_width:
            raise ValueError(f"peak widths must be 0 <= min_width <= max_width, got {min_width}, {max_width}")
        if not 0.0 < self.rel_height <= 1.0:
            raise ValueError(f"peak rel_height must be in (0, 1], got {rel_height}")
        if math.isnan(self.threshold):
            raise ValueError("peak threshold is NaN")

    def token(self):
        return (self.separation, self.prominence, self.min_width, self.max_width, self.rel_height, self.threshold)

    def desc(self) -> _abi.PeakDesc:
        return _abi.PeakDesc(*self.token())


def configure_peaks(ctx: _abi.Context, peaks: PeakSettings | None) -> None:
    """``attpc_trace_configure_peaks`` unless this ctx already holds the same parameters (``None``: the stage off)."""
    configure_stage(ctx, PeakSettings, peaks)


class BaselineSettings:
    """The validated Fourier baseline of the trace rows (``attpc_baseline_desc``, include/attpc_engine.h):
    ``window_scale`` (finite, > 0), Spyral's ``GetParameters.baseline_window_scale`` and its default."""

    slot, call = "baseline", "attpc_trace_configure_baseline"

    def __init__(self, window_scale: float = 20.0):
        self.window_scale = float(window_scale)
        if not (math.isfinite(self.window_scale) and self.window_scale > 0.0):
            raise ValueError(f"baseline window_scale must be finite and > 0, got {window_scale}")

    def token(self):
        return (self.window_scale,)

    def desc(self) -> _abi.BaselineDesc:
        return _abi.BaselineDesc(*self.token())


def configure_baseline(ctx: _abi.Context, baseline: BaselineSettings | None) -> None:
    """``attpc_trace_configure_baseline`` unless this ctx already holds the same setting (``None``: the stage off)."""
    configure_stage(ctx, BaselineSettings, baseline)


def remove_baseline(traces, window_scale: float = 20.0, ctx: _abi.Context | None = None, return_baseline: bool = False):
    """The Fourier baseline stage alone on any host rows (``attpc_trace_baseline``; the kernel of the fused path, no
    other configuration needed): traces [R,512] integers in 0 .. 4095 -> y [R,512] i16, and with ``return_baseline``
    (y, baseline [R,512] f64)."""
    window_scale = BaselineSettings(window_scale).window_scale
    traces = np.asarray(traces)
    if traces.ndim != 2 or traces.shape[1] != _abi.NUM_TB or traces.dtype.kind not in "iu":
        raise ValueError(f"traces must be integers of shape [rows, {_abi.NUM_TB}], got {traces.dtype} {traces.shape}")
    if traces.size and (traces.min() < 0 or traces.max() > 4095):
        raise ValueError("trace samples must lie in 0 .. 4095")
    samples = np.ascontiguousarray(traces, dtype=np.int16)
    ctx = ctx or _abi.default_context()
    y = np.empty_like(samples)
    baseline = np.empty(samples.shape, dtype=np.float64) if return_baseline else None
    i16 = _abi.C.c_int16
    ctx.check(ctx.lib.attpc_trace_baseline(ctx.handle, len(samples), _abi.iptr(samples, i16), window_scale,
                                           _abi.iptr(y, i16), _abi.dptr(baseline)), "attpc_trace_baseline")
    return (y, baseline) if return_baseline else y


TRIGGER_DTYPE = _abi.TRIGGER_DTYPE


class TriggerSettings:
    """The validated multiplicity trigger of the traces (``attpc_trigger_desc``, include/attpc_engine.h): ``threshold``
    (integer in 0 .. 4095, the discriminator level above the pedestal), ``window`` (1 .. 512 samples),
    ``group_multiplicity`` (>= 1: the windowed sum a group must reach), ``min_groups`` (1 .. 16 groups that must assert
    together), ``groups`` ([ATTPC_NUM_PADS] integers: below 16 the pad's trigger group -- its CoBo; the map is the
    caller's --, 255 = the pad takes no part; None = every pad in group 0) and ``gate`` (trace rows only: an event that
    did not fire gets no rows)."""

    slot, call = "trigger", "attpc_trace_configure_trigger"

    def __init__(self, threshold, window: int = 64, group_multiplicity: int = 1, min_groups: int = 1, groups=None,
                 gate: bool = False):
        def integer(name, value, lo, hi):
            if isinstance(value, (bool, np.bool_)) or int(value) != value or not lo <= int(value) <= hi:
                raise ValueError(f"trigger {name} must be an integer in {lo} .. {hi}, got {value!r}")
            return int(value)

        self.threshold = integer("threshold", threshold, 0, 4095)
        self.window = integer("window", window, 1, _abi.NUM_TB)
        self.group_multiplicity = integer("group_multiplicity", group_multiplicity, 1, 2 ** 31 - 1)
        self.min_groups = integer("min_groups", min_groups, 1, _abi.MAX_TRIGGER_GROUPS)
        if groups is not None:
            g = np.asarray(groups)
            if g.shape != (_abi.NUM_PADS,) or g.dtype.kind not in "iu":
                raise ValueError(f"trigger groups must be {_abi.NUM_PADS} integers, got {g.dtype} {g.shape}")
            if np.any(((g < 0) | (g >= _abi.MAX_TRIGGER_GROUPS)) & (g != 255)):
                raise ValueError(f"a trigger group must lie in 0 .. {_abi.MAX_TRIGGER_GROUPS - 1} or be 255 (no part)")
            groups = np.ascontiguousarray(g, dtype=np.uint8)
        self.groups = groups
        if not isinstance(gate, (bool, np.bool_)) and gate not in (0, 1):
            raise ValueError(f"trigger gate must be a bool, got {gate!r}")
        self.gate = bool(gate)

    def gated(self, gate: bool = True) -> "TriggerSettings":
        """The same trigger with ``gate`` set."""
        return TriggerSettings(self.threshold, self.window, self.group_multiplicity, self.min_groups, self.groups, gate)

    def token(self):
        return (self.threshold, self.window, self.group_multiplicity, self.min_groups,
                None if self.groups is None else self.groups.tobytes(), self.gate)

    def desc(self) -> _abi.TriggerDesc:
        """(the descriptor points into ``self.groups``: keep the settings alive over the call)"""
        return _abi.TriggerDesc(self.threshold, self.window, self.group_multiplicity, self.min_groups,
                                _abi.iptr(self.groups, _abi.C.c_uint8), int(self.gate), 0)


def configure_trigger(ctx: _abi.Context, trigger: TriggerSettings | None) -> None:
    """``attpc_trace_configure_trigger`` unless this ctx already holds the same setting (``None``: the stage off)."""
    configure_stage(ctx, TriggerSettings, trigger)


def trigger_result(ctx: _abi.Context, n_events: int, n_sim: int = 0, n_rows=None) -> dict:
    """``{"trigger": records [n_events]}`` of ctx's last trace or trace-row call if the ctx holds a trigger, else {}."""
    return {"trigger": ctx.trigger_last(n_events)} if ctx._tokens["trigger"] is not None else {}


def traces_to_trigger(offsets, pads, samples, trigger: TriggerSettings, pedestals=None, ctx: _abi.Context | None = None):
    """The trigger stage alone on any host rows in CSR form (``attpc_trigger_rows``; the kernel of the fused path, no
    other configuration needed): offsets [n+1], pads [R] in 0 .. 10239, samples [R,512] integers in 0 .. 4095,
    ``pedestals`` [ATTPC_NUM_PADS] (or one value for every pad) in 0 .. 4095 or None -> records [n]
    (``TRIGGER_DTYPE``)."""
    if not isinstance(trigger, TriggerSettings):
        raise TypeError("trigger must be a TriggerSettings")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    if offsets.ndim != 1 or n < 0:
        raise ValueError("offsets needs n_events + 1 entries")
    pads, samples = np.asarray(pads), np.asarray(samples)
    if pads.ndim != 1 or (pads.size and pads.dtype.kind not in "iu"):
        raise ValueError("pads must be a 1-D array of integers")
    if samples.shape != (len(pads), _abi.NUM_TB) or (samples.size and samples.dtype.kind not in "iu"):
        raise ValueError(f"samples must be integers of shape [{len(pads)}, {_abi.NUM_TB}], got {samples.dtype} {samples.shape}")
    if n and (offsets[0] < 0 or np.any(np.diff(offsets) < 0) or offsets[-1] > len(pads)):
        raise ValueError("offsets must not decrease and must lie within the rows given")
    if pads.size and (pads.min() < 0 or pads.max() >= _abi.NUM_PADS):
        raise ValueError(f"pads must lie in 0 .. {_abi.NUM_PADS - 1}")
    if samples.size and (samples.min() < 0 or samples.max() > 4095):
        raise ValueError("trace samples must lie in 0 .. 4095")
    pads = np.ascontiguousarray(pads, dtype=np.int32)
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    pedestals = NoiseSettings(pedestals=pedestals).pedestals
    ctx = ctx or _abi.default_context()
    records = np.empty(n, dtype=TRIGGER_DTYPE)
    i16 = _abi.C.c_int16
    ctx.check(ctx.lib.attpc_trigger_rows(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.iptr(pads, _abi.C.c_int32),
                                         _abi.iptr(samples, i16), _abi.iptr(pedestals, i16), trigger.desc(),
                                         _abi.iptr(records, _abi.TriggerRecord)), "attpc_trigger_rows")
    return records


def polya_rel_variance(theta: float) -> float:
    """The relative variance f = 1 / (1 + theta) of a Polya-distributed single-electron gain, theta >= 0 (theta = 0:
    the exponential gain of a parallel-plate avalanche, f = 1)."""
    theta = float(theta)
    if not (theta >= 0.0 and math.isfinite(theta)):
        raise ValueError(f"the Polya parameter theta must be finite and >= 0, got {theta}")
    return 1.0 / (1.0 + theta)


_quantile_table = None


def normal_quantile_table() -> np.ndarray:
    """The quantile table [ATTPC_GAIN_KNOTS] of the gain's standardised fluctuation: Phi^-1((i + 0.5) / 4097) for
    i = 0 .. 4096 (``statistics.NormalDist``), divided by the standard deviation of the piecewise-linear law the table
    defines -- a uniformly chosen interval, a uniform position in it: mean 0 by symmetry, variance
    mean((a^2 + a b + b^2) / 3) over the intervals [a, b], 0.99663 unscaled -- so that law has unit variance."""
    global _quantile_table
    if _quantile_table is None:
        inv = statistics.NormalDist().inv_cdf
        z = np.array([inv((i + 0.5) / _abi.GAIN_KNOTS) for i in range(_abi.GAIN_KNOTS)], dtype=np.float64)
        z = 0.5 * (z - z[::-1])  # exactly antisymmetric
        a, b = z[:-1], z[1:]
        variance = math.fsum((a * a + a * b + b * b) / 3.0) / (_abi.GAIN_KNOTS - 1)
        _quantile_table = z / math.sqrt(variance)
        _quantile_table.setflags(write=False)
    return _quantile_table


class GainSettings:
    """The validated micromegas gain of the traces (``attpc_trace_gain_desc``, include/attpc_engine.h): exactly one of
    ``rel_variance`` (f in [0, 1]) and ``theta`` (the Polya parameter, f = 1 / (1 + theta)) -- neither, with a
    ``pad_gain``, means f = 0: pad gains only --, ``pad_gain`` ([ATTPC_NUM_PADS] finite factors >= 0, or one value for
    every pad; None = 1.0 everywhere), ``stream`` in [0, 2^30) (another realisation on the same physics).  The
    fluctuation is drawn through ``normal_quantile_table()``."""

    slot, call = "trace_gain", "attpc_trace_configure_gain"

    def __init__(self, rel_variance=None, theta=None, pad_gain=None, stream: int = 0):
        if rel_variance is not None and theta is not None:
            raise ValueError("give rel_variance or theta, not both")
        if rel_variance is None and theta is None and pad_gain is None:
            raise ValueError("a gain needs rel_variance, theta or pad_gain")
        if theta is not None:
            rel_variance = polya_rel_variance(theta)
        self.rel_variance = 0.0 if rel_variance is None else float(rel_variance)
        if not 0.0 <= self.rel_variance <= 1.0:
            raise ValueError(f"gain rel_variance must be in [0, 1], got {rel_variance}")
        if pad_gain is not None:
            g = np.asarray(pad_gain, dtype=np.float64)
            if g.ndim > 1 or (g.ndim == 1 and g.shape != (_abi.NUM_PADS,)):
                raise ValueError(f"pad_gain must be {_abi.NUM_PADS} factors (or one for every pad), got shape {g.shape}")
            g = np.broadcast_to(g, (_abi.NUM_PADS,))
            if not np.all(np.isfinite(g) & (g >= 0.0)):
                raise ValueError("pad gains must be finite and >= 0")
            pad_gain = np.ascontiguousarray(g)
        self.pad_gain = pad_gain
        if isinstance(stream, (bool, np.bool_)) or int(stream) != stream or not 0 <= int(stream) < 1 << 30:
            raise ValueError(f"gain stream must be an integer in [0, 2^30), got {stream!r}")
        self.stream = int(stream)
        self.quantiles = normal_quantile_table() if self.rel_variance > 0.0 else None

    @property
    def on(self) -> bool:
        """Anything that changes a charge."""
        return self.rel_variance > 0.0 or self.pad_gain is not None

    def token(self):
        if not self.on:
            return None
        return (self.rel_variance, None if self.pad_gain is None else self.pad_gain.tobytes(), self.stream)

    def desc(self) -> _abi.TraceGainDesc:
        """(the descriptor points into ``self.pad_gain`` and the quantile table: keep the settings alive over the call)"""
        return _abi.TraceGainDesc(self.rel_variance, _abi.dptr(self.pad_gain), _abi.dptr(self.quantiles), self.stream, 0)


def configure_gain(ctx: _abi.Context, gain: GainSettings | None) -> None:
    """``attpc_trace_configure_gain`` unless this ctx already holds the same gain (``None``, or one without effect: off)."""
    configure_stage(ctx, GainSettings, checked(GainSettings, gain, "gain"))


def clouds_to_gain(offsets: np.ndarray, points: np.ndarray, ctx: _abi.Context, seed: int = 0, first_event: int = 0,
                   gain: GainSettings | None = None) -> np.ndarray:
    """The gain stage alone on any host cloud in CSR form (``attpc_gain_rows``; the kernel of the fused path):
    offsets [n+1], points [P,3] (pad, time bucket, electrons) -> the gained charge of every row [P] f64 (rows outside
    the offsets' range keep 0).  ``gain``: configured first (None: the stage off, the charges come back as they are).
    Event i of the call is the global event ``first_event + i``."""
    offsets, points, _, seed, first_event, n = _host_cloud(offsets, points, None, seed, first_event)
    configure_gain(ctx, gain)
    gained = np.zeros(len(points), dtype=np.float64)
    ctx.check(ctx.lib.attpc_gain_rows(ctx.handle, seed, first_event, n, _abi.iptr(offsets, _abi.C.c_int64),
                                      _abi.dptr(points), _abi.dptr(gained)), "attpc_gain_rows")
    return gained


# One row per stage of the chain, in the order the chain configures them: ``field`` (the field of ``TraceChain`` and the
# keyword of the entry points), ``settings`` (its class: ``slot`` and ``call``), ``configure`` (ctx, settings -- and,
# with ``config``, the chain's config), ``result`` (ctx, n_events, n_sim, n_rows -> what the stage adds to the result of
# a run, or None), ``keep`` (the name of ``TraceChain.configure``'s ``keep`` that leaves the stage as the ctx holds it),
# ``rows`` (a stage of the trace rows only), ``default`` (what None means, if not "off"), ``replace`` (a field that
# ``TraceChain.replace`` takes).
Stage = collections.namedtuple("Stage", "field settings configure result keep rows default config replace",
                               defaults=(None, None, False, None, False, True))
STAGES = (
    Stage("noise", NoiseSettings, configure_noise, default=NoiseSettings, replace=False),
    Stage("common_mode", CommonModeSettings, configure_common_mode, keep="common_mode"),
    Stage("readout", ReadoutSettings, configure_readout, default=ReadoutSettings, replace=False),
    Stage("peaks", PeakSettings, configure_peaks, rows=True, default=PeakSettings),
    Stage("baseline", BaselineSettings, configure_baseline, rows=True),
    Stage("trigger", TriggerSettings, configure_trigger, trigger_result, keep="trigger"),
    Stage("gain", GainSettings, configure_gain, keep="gain"),
    Stage("correction", CorrectionSettings, configure_correction, correction_result, "correction", True, config=True),
    Stage("clustering", ClusterSettings, configure_clustering, clustering_result, "clustering", True),
    Stage("join", JoinSettings, configure_cluster_join, join_result, "clustering", True),
    Stage("estimates", EstimateSettings, configure_estimates, estimates_result, "estimates", True, config=True),
    Stage("thinning", ThinSettings, configure_thinning, thinning_result, "estimates", True),
    Stage("circle", CircleFitSettings, configure_circle, circle_result, "estimates", True),
    Stage("helix", HelixSlopeSettings, configure_helix, helix_result, "estimates", True),
    Stage("fit", TrackFitSettings, configure_track_fit, fit_result, "estimates", True),
    Stage("pid", PidSettings, configure_pid, pid_result, "estimates", True),
)


def stage_results(ctx: _abi.Context, n_events: int, n_sim: int, n_rows: int | None = None) -> dict:
    """What the stages the ctx holds add to the result of its last trace-row call of ``n_events`` events and ``n_sim``
    track positions, each under its own keys (``trigger``, ``correction``, ``clusters``, ``joins``, ``estimates``,
    ``thinning``, ``circle``, ``slope``, ``fits``, ``pid``); with ``n_rows`` (the rows the call fetched) the
    ``cluster_labels`` of those rows too."""
    results = {}
    for stage in STAGES:
        if stage.result is not None:
            results.update(stage.result(ctx, n_events, n_sim, n_rows))
    return results


class TraceChain:
    """One trace configuration, validated here, before any library call: ``config``, the ``response`` [512] f64,
    ``threshold`` and ``offset`` with their defaults filled in (``trace_settings``), the ``noise`` (a ``NoiseSettings``;
    None = off) and the ``readout`` (a ``ReadoutSettings``; None = hit pads), and the stages that are None when off:
    ``gain``, ``peaks`` (trace rows; None = ``PeakSettings()``), ``baseline``, ``trigger``, ``common_mode``,
    ``estimates`` (trace rows: a ``detector.estimate.EstimateSettings``), ``thinning`` (the rows in front of the
    estimates: a ``detector.thinning.ThinSettings``), ``circle`` (the geometric circle fit behind them: a
    ``detector.circle.CircleFitSettings``), ``helix`` (the helix slope behind the circle: a
    ``detector.helix.HelixSlopeSettings``) and ``correction`` (trace rows: the drift correction of the rows, in front
    of the thinning, the estimates and the delivery: a ``detector.correction.CorrectionSettings``), ``fit`` (the
    track fit behind the estimates: a ``detector.fit.TrackFitSettings``) and ``clustering`` (trace rows: the cluster
    labels the thinning, the estimates and the fit match in place of the truth labels: a
    ``detector.clustering.ClusterSettings``) with ``join`` (the cluster joining between the clustering's size cut and
    its ranking: a ``detector.joining.JoinSettings``; it does nothing without the clustering) and ``pid`` (the particle
    identification between the estimates and the track fit: a ``detector.pid.PidSettings``; it does nothing without
    the estimates).  TypeError for a stage that is not of the class its row of ``STAGES`` names."""

    def __init__(self, config: Config, response=None, threshold=None, offset: int = 0, noise=None, readout=None,
                 gain=None, peaks=None, baseline=None, trigger=None, common_mode=None, estimates=None,
                 thinning=None, circle=None, helix=None, correction=None, fit=None, clustering=None, join=None,
                 pid=None):
        given = dict(noise=noise, readout=readout, gain=gain, peaks=peaks, baseline=baseline, trigger=trigger,
                     common_mode=common_mode, estimates=estimates, thinning=thinning, circle=circle, helix=helix,
                     correction=correction, fit=fit, clustering=clustering, join=join, pid=pid)
        self.config, self._given = config, (response, threshold)
        self.response, self.threshold, self.offset = trace_settings(config, response, threshold, offset)
        for stage in STAGES:
            setattr(self, stage.field, checked(stage.settings, given[stage.field], stage.field))
        self.noise, self.readout = self.noise or NoiseSettings(), self.readout or ReadoutSettings()

    @classmethod
    def from_kwargs(cls, config: Config, **trace_kwargs) -> "TraceChain":
        """The chain of the trace settings a caller passes on as keywords (TRACE_KWARGS, as ``configure_traces``
        describes them): TypeError for any other name, ValueError for a value that is refused."""
        unknown = set(trace_kwargs) - set(TRACE_KWARGS)
        if unknown:
            raise TypeError(f"unexpected trace settings {sorted(unknown)}: configure_traces takes {list(TRACE_KWARGS)}")
        get = trace_kwargs.get
        return cls(config, get("response"), get("threshold"), get("offset", 0),
                   NoiseSettings(get("noise_sigma", 0.0), get("noise_table"), get("pedestals"), get("noise_stream", 0)),
                   ReadoutSettings(get("readout", "hit"), get("readout_pads")))

    def replace(self, **fields) -> "TraceChain":
        """The same chain with the given fields (``REPLACE_FIELDS``: config and the stages the entry points take as
        keywords; TypeError for any other) replaced.  A new ``config`` fills in again the response and the threshold
        the chain was built without."""
        unknown = set(fields) - set(REPLACE_FIELDS)
        if unknown:
            raise TypeError(f"TraceChain.replace takes {', '.join(REPLACE_FIELDS[:-1])} and {REPLACE_FIELDS[-1]}, "
                            f"not {sorted(unknown)}")
        chain = copy.copy(self)
        vars(chain).update(fields)
        if "config" in fields:
            chain.response, chain.threshold, _ = trace_settings(chain.config, *self._given, self.offset)
        for stage in STAGES:
            checked(stage.settings, getattr(chain, stage.field), stage.field)
        return chain

    def configure(self, ctx: _abi.Context, rows: bool = False, keep=(), but=()) -> None:
        """Every configure call of the chain, each skipped when the ctx already holds the same content: the trace, then
        the stages in the order of ``STAGES`` -- noise, common-mode noise, readout; with ``rows`` (trace rows) the
        geometry of the rows (``configure_spyral``), peaks and baseline; trigger; gain; with ``rows`` the drift
        correction of the rows, the clustering and the cluster joining, the track estimates, the thinning, the circle
        fit, the helix slope, the track fit and the particle identification.  A stage that is off is turned off,
        whatever an earlier use of the ctx left -- except those of "trigger", "gain", "common_mode", "estimates" (the
        thinning, the circle fit, the helix slope, the track fit and the particle identification with them),
        "correction" and "clustering" (the cluster joining with it) that ``keep`` names, which stay as the ctx holds
        them, unless ``but`` names the stage's own field."""
        from .simulator import configure_spyral

        ctx.configure("trace", (self.response.tobytes(), self.threshold, self.offset), "attpc_trace_configure",
                      _abi.TraceDesc(_abi.dptr(self.response), self.threshold, self.offset, 0))
        for stage in STAGES:
            if (stage.rows and not rows) or (stage.keep in keep and stage.field not in but):
                continue
            if stage.field == "peaks":  # the first stage of the rows: their geometry goes in front of it
                configure_spyral(self.config, ctx)
            settings = getattr(self, stage.field)
            if settings is None and stage.default is not None:
                settings = stage.default()
            stage.configure(ctx, settings, *((self.config,) if stage.config else ()))

    def run_batch(self, rows: bool, momenta, vertices, proton_numbers, mass_numbers, seed, indices, first_event: int = 0,
                  ctx: _abi.Context | None = None, capacity_per_event: int | None = None, packed: bool = False,
                  straggling=None, distortion=None):
        """simulate() + this chain on the device for n events: what ``simulate_batch_trace_rows`` (``rows``) or
        ``simulate_batch_traces`` returns (``capacity_per_event``: None = the default of that entry point; ``packed``:
        the traces as packed records, ``attpc_det_run_traces_packed``; ``straggling``: the track straggling, a
        ``detector.straggling.StragglingSettings`` or None = off; ``distortion``: the drift distortion, a
        ``detector.distortion.DistortionMap`` or None = off)."""
        from .simulator import run_batch

        ctx = ctx or _abi.default_context()
        packed = _packed_flag(packed)
        if packed and rows:
            raise ValueError("packed applies to traces, not to trace rows")

        def configure(c):
            self.configure(c, rows)
            return 0 if rows else c._trace_readout_rows  # traces in full readout: |S| rows per event

        per_event = (2048 if rows else 1024) if capacity_per_event is None else capacity_per_event
        how = dict(holder=RowArrays, width=8, slack=1024) if rows else {}
        if packed:
            how = dict(holder=PackedTraceArrays, byte_capacity=PACKED_BYTES_PER_ROW * max(1024, int(per_event) * len(momenta)))
        arrays, stats = run_batch("attpc_det_run_trace_rows" if rows else "attpc_det_run_traces_packed" if packed
                                  else "attpc_det_run_traces", momenta, vertices,
                                  proton_numbers, mass_numbers, self.config, seed, indices, first_event, ctx,
                                  per_event, configure, straggling=straggling, distortion=distortion, **how)
        n_events = len(arrays.offsets) - 1
        if rows:
            extra = stage_results(ctx, n_events, len(indices), int(arrays.offsets[-1]))
        else:
            extra = trigger_result(ctx, n_events)
        sums = ctx.trace_rows_last() if rows else arrays.sums()
        return (*arrays.result(), arrays.event_points, {**stats.as_dict(), **sums, **extra})


# the fields ``TraceChain.replace`` takes, in the order ``TraceChain`` takes them (and its TypeError names them)
REPLACE_FIELDS = ("config", "gain", "peaks", "baseline", "trigger", "common_mode", "estimates", "thinning", "circle", "helix",
                  "correction", "fit", "clustering", "join", "pid")


def _checked_join(join):  # (tests import this name and the next)
    return checked(JoinSettings, join, "join")


def _checked_pid(pid):
    return checked(PidSettings, pid, "pid")


def configure_trace_rows(config: Config, ctx: _abi.Context, peaks: PeakSettings | None = None,
                         baseline: BaselineSettings | None = None, gain: GainSettings | None = None,
                         common_mode: CommonModeSettings | None = None, thinning=None, circle=None, helix=None,
                         correction=None, clustering=None, join=None, pid=None, **trace_kwargs) -> None:
    """Everything a trace-row call needs beside the detector: the trace settings (``configure_traces(**trace_kwargs)``),
    the geometry of the rows (``configure_spyral``), the peak parameters (default ``PeakSettings()``), the Fourier
    baseline (default None: off, the peaks stand on the configured pedestals), the micromegas gain and the common-mode
    noise (default None: off).  The trigger, the track estimates, the thinning, the circle fit and the helix slope stay
    as the ctx holds them; a ``thinning`` (a ``detector.thinning.ThinSettings``), a ``circle`` (a
    ``detector.circle.CircleFitSettings``) or a ``helix`` (a ``detector.helix.HelixSlopeSettings``) is configured, None
    leaves what the ctx holds; so do ``correction`` (the drift correction of the rows, a
    ``detector.correction.CorrectionSettings``) and ``clustering`` (the cluster labels in place of the truth labels, a
    ``detector.clustering.ClusterSettings``) and ``join`` (the cluster joining behind it, a
    ``detector.joining.JoinSettings``) and ``pid`` (the particle identification behind the estimates, a
    ``detector.pid.PidSettings``)."""
    stages = dict(peaks=peaks, baseline=baseline, gain=gain, common_mode=common_mode, thinning=thinning, circle=circle,
                  helix=helix, correction=correction, clustering=clustering, join=join, pid=pid)
    chain = TraceChain.from_kwargs(config, **trace_kwargs).replace(**stages)
    chain.configure(ctx, rows=True, keep=("trigger", "estimates", "correction", "clustering"),
                    but=[field for field, settings in stages.items() if settings is not None])


def simulate_batch_trace_rows(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config,
                              seed: int, indices: list[int], first_event: int = 0, ctx: _abi.Context | None = None,
                              peaks: PeakSettings | None = None, capacity_per_event: int = 2048,
                              baseline: BaselineSettings | None = None, trigger: TriggerSettings | None = None,
                              gain: GainSettings | None = None, common_mode: CommonModeSettings | None = None,
                              estimates=None, thinning=None, straggling=None, circle=None, helix=None,
                              distortion=None, correction=None, fit=None, clustering=None, join=None, pid=None,
                              **trace_kwargs):
    """simulate() + the pad traces of every event + their peaks as Spyral rows, all on the device
    (``attpc_det_run_trace_rows``; ``trace_kwargs`` as configure_traces takes them, ``baseline`` as configure_trace_rows) ->
    (offsets [n+1], rows [P,8] in ascending z per event, labels [P], event_points [n] = cloud rows of every event
    before any suppression, stats dict: the cloud's run statistics with ``n_points`` = the rows, plus ``n_rows`` /
    ``row_checksum``, and with ``trigger`` (a ``TriggerSettings``; None = off; its ``gate`` leaves the events that did
    not fire without rows) its records [n] under ``"trigger"``, and with ``estimates`` (a
    ``detector.estimate.EstimateSettings``; None = off) the track estimates [n, len(indices)] under ``"estimates"`` --
    with ``thinning`` (a ``detector.thinning.ThinSettings``; None = off) those of the thinned points, and its z step
    under ``"thinning"``; with ``circle`` (a ``detector.circle.CircleFitSettings``; None = off) their circles refined by
    the geometric fit, and ``"circle": "geometric"``; with ``helix`` (a ``detector.helix.HelixSlopeSettings``; None =
    off) their slope, vz and B rho from the helix, and ``"slope": "helix"``).
    ``gain``, ``common_mode``, ``straggling`` and ``distortion`` as simulate_batch_traces takes them.  With
    ``correction`` (a ``detector.correction.CorrectionSettings``; None = off) the rows and labels are the drift-corrected
    ones, per event in ascending corrected z, the estimates are made of them, and the stage's counts come under
    ``"correction"``.  With ``fit`` (a ``detector.fit.TrackFitSettings``; None = off) and ``estimates`` the track fits
    [n, len(indices)] come under ``"fits"``.  With ``clustering`` (a ``detector.clustering.ClusterSettings``; None = off)
    the thinning, the estimates and the fit match the cluster labels in place of the truth labels; the labels returned
    stay the truth labels, the cluster labels [P] come under ``"cluster_labels"`` and the event and cluster records
    under ``"clusters"``.  With ``join`` (a ``detector.joining.JoinSettings``; None = off) beside it, clusters whose
    circles overlap are joined before they are ranked and labelled, and the join events and records come under
    ``"joins"``.  With ``pid`` (a ``detector.pid.PidSettings``; None = off) beside the estimates, every (event, slot)
    is assigned a position by the gates on its estimate record's dE/dx against B rho, the fit uses that position's
    species, and the records [n, len(indices)] come under ``"pid"``."""
    chain = TraceChain.from_kwargs(config, **trace_kwargs).replace(
        peaks=peaks, baseline=baseline, trigger=trigger, gain=gain, common_mode=common_mode, estimates=estimates,
        thinning=thinning, circle=circle, helix=helix, correction=correction, fit=fit, clustering=clustering, join=join, pid=pid)
    return chain.run_batch(True, momenta, vertices, proton_numbers, mass_numbers, seed, indices, first_event, ctx,
                           capacity_per_event, straggling=straggling, distortion=distortion)


def clouds_to_trace_rows(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, ctx: _abi.Context, seed: int = 0,
                         first_event: int = 0):
    """Trace rows of any host cloud in CSR form (``attpc_trace_rows_at``; ``ctx`` configured with
    ``configure_trace_rows``): offsets [n+1], points [P,3] (pad, time bucket, electrons), labels [P] ->
    (offsets [n+1], rows [R,8], labels [R], {n_rows, row_checksum; when the ctx holds a trigger its records [n] too,
    under ``"trigger"``}).  Event i of the call is the global event ``first_event + i`` (noise, centroid jitter and
    checksum)."""
    offsets, points, labels, seed, first_event, n = _host_cloud(offsets, points, labels, seed, first_event)
    needed = _abi.RunStats()  # (the host-cloud call has no statistics: its rows come from attpc_trace_rows_last)

    def call(out):
        status = ctx.lib.attpc_trace_rows_at(ctx.handle, seed, first_event, n, _abi.iptr(offsets, _abi.C.c_int64),
                                             _abi.dptr(points), _abi.iptr(labels, _abi.C.c_int64), out)
        if status in (_abi.OK, _abi.E_CAPACITY):
            needed.n_points = ctx.trace_rows_last()["n_rows"]
        return status

    rows = int(offsets[-1] - offsets[0]) if n else 0
    arrays = call_with_capacity(ctx, n, max(16, rows, 4 * ctx._trace_readout_rows * n), call, "attpc_trace_rows_at", needed,
                                holder=RowArrays, width=8, slack=16)
    extra = trigger_result(ctx, n)
    return (*arrays.result(), {**ctx.trace_rows_last(), **extra})
