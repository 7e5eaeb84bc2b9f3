"""The runs and responses tests/test_gpu_spyral_edges.py drives through the fused Spyral path, shared with
tests/test_spyral_cpu.py, which checks on the CPU oracle's clouds of the same runs that they mean what they say."""
from __future__ import annotations

import copy

import numpy as np

from attpc_engine_amd import workloads
from tests.spyral_reference import NUM_TB, bipolar_response

SEED = 11
GAINS = (175000, 100_000_000, 100_000_000_000)  # the default; most kept rows partly clipped; the suite's own 1e11
LOW_GAIN = 1000  # amplitudes of 40 .. 50 ADC counts at the most and rows of zero charge: the threshold decides
SWEEP = ("be10dp", 20, 6)       # workload, first event, events: the gain sweep
# The other responses.  The clipped sum of the bipolar response changes sign near q = 3.9e10; between 3.87e10 and 3.91e10
# the reference's own f64 sum is more than 1e-13 (up to 3e-12) from the exact sum, and a relative tolerance means
# nothing.  At a gain of 1e11 most events hold a few such charges; events 0 .. 5 hold none (event 5 is empty).
RESPONSES = ("be10dp", 0, 6)
THRESHOLDS = ("be10dp", 0, 8)   # at LOW_GAIN; events 4 .. 6 keep nothing at the median of the events' maxima
CROWDED = ("b10chain", 10, 2)   # the oracle's clouds of events 10, 11 hold 68 and 43 rows in their fullest sort bin


def responses(config) -> dict:
    """name -> response [512]: the default, one with negative lobes, a flat one (k is 0 or 512) and a single sample
    (integral == amplitude)."""
    from attpc_engine_amd.detector.response import get_response

    default = np.ascontiguousarray(get_response(config), dtype=np.float64)
    single = np.zeros(NUM_TB)
    single[37] = default.max()
    return {"default": default, "bipolar": bipolar_response(), "flat": np.full(NUM_TB, default.max()), "single": single}


def with_settings(config, gain=None, threshold=None):
    """A copy of ``config`` with another gain and / or ADC threshold."""
    config = copy.copy(config)
    config.det_params = copy.copy(config.det_params)
    config.elec_params = copy.copy(config.elec_params)
    if gain is not None:
        config.det_params.mpgd_gain = gain
    if threshold is not None:
        config.elec_params.adc_threshold = threshold
    return config


def builder(name: str, gain):
    """A workload builder (tests.helpers.Inputs takes one) with ``gain`` as the detector's gain."""
    def build(**kw):
        pipeline, config, indices = workloads.WORKLOADS[name](**kw)
        config.det_params.mpgd_gain = gain
        return pipeline, config, indices
    return build


def sort_bins(tb: np.ndarray) -> np.ndarray:
    """The bin of the device's counting sort: (time bucket, sixteenth of the jitter)."""
    whole = np.floor(tb)
    return whole.astype(np.int64) * 16 + np.floor((tb - whole) * 16.0).astype(np.int64)
