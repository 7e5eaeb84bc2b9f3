"""The launches of the track-straggling tests, defined once: tests/test_straggling_cpu.py checks on the reference alone
that no track of them ends within a rounding difference of a terminal event, tests/test_gpu_straggling.py runs them on
the device against the same references (tests/straggle_reference.py)."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd.detector.straggling import electron_density, radiation_length
from tests import straggle_reference as sr
from tests import track_cases as tc

# 130 events of be10dp, both nuclei: 260 tracks, more than four waves -- lanes refill and batches of ids cross
SEED, FIRST, EVENTS = 21, 1000, 130
# name -> ((angular_scale, energy_scale), what differs in the detector description)
PASSES = {
    "angular": ((1.0, 0.0), {}),
    "energy": ((0.0, 1.0), {}),
    "both": ((1.0, 1.0), {}),
    "substeps2": ((1.0, 1.0), {"ode_substeps": 2}),
    "path_step": ((1.0, 1.0), {"path_step": 1.0e-3}),
}
# a track whose reference comes this close to a terminal event at some step may end one step apart on the device
MIN_MARGIN = 1.0e-9

# the clamp: an 11Be of 1 MeV whose energy fluctuation is fifty times Bohr's -- a kick takes it below KE_LIMIT long
# before it would have ranged out
CLAMP_SEED, CLAMP_EVENT, CLAMP_ENERGY_SCALE = 5, 0, 50.0


def settings_of(inp, scales, stream: int = 0) -> sr.Settings:
    """The reference settings of ``scales`` on the gas of ``inp`` (the values the Python layer works out)."""
    gas = inp.config.det_params.gas_target
    return sr.Settings(scales[0], scales[1], radiation_length(gas), electron_density(gas), stream)


_CACHE: dict = {}


def pass_inputs(name: str):
    from tests.helpers import Inputs
    key = ("inputs", name)
    if key not in _CACHE:
        _CACHE[key] = Inputs("be10dp", **PASSES[name][1])
    return _CACHE[key]


def pass_references(orc, name: str):
    """(inp, settings, p4, vertex, references of the 260 tracks) of a pass, computed once per process."""
    if name not in _CACHE:
        inp = pass_inputs(name)
        settings = settings_of(inp, PASSES[name][0])
        vertex, p4, status, _ = orc.kin_batch(inp.kin, SEED, FIRST, EVENTS, threads=8)
        assert (status == 0).all()
        _CACHE[name] = (inp, settings, p4, vertex, sr.reference_tracks(orc, inp, p4, vertex, SEED, FIRST, settings))
    return _CACHE[name]


def clamp_event():
    """(inp, p4 [1, 4, 4], vertex [1, 3]) of the clamp case: the 11Be at 1 MeV, the proton an ordinary short track."""
    inp = pass_inputs("both")
    p4 = np.zeros((1, 4, 4))
    p4[0, tc.ROW["be11"]] = tc.momentum(tc.MASS["be11"], 1.0, 0.3, 1.0)
    p4[0, tc.ROW["p"]] = tc.momentum(tc.MASS["p"], 0.3, 0.4, 1.0)
    return inp, p4, np.array([[0.001, 0.002, 0.3]])
