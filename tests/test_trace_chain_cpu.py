"""``TraceChain`` against its parts, without a device: per context slot the chain uploads the content (token) and the
descriptor scalars of the individually constructed settings classes -- all stages off, each alone, all on --, and
``from_kwargs`` refuses what the settings classes and ``validate_trace_kwargs`` refuse, with the same exception type.
The library is the recording stand-in of tests/test_run_layer_cpu.py."""
import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from attpc_engine_amd.detector.traces import (
    BaselineSettings, GainSettings, NoiseSettings, PeakSettings, ReadoutSettings, TraceChain, TriggerSettings,
    configure_stage, gaussian_noise_table, trace_settings)
from tests.test_run_layer_cpu import RecordingContext

STAGES = {  # chain field -> (settings class, how from_kwargs or replace gets it, the settings built on their own)
    "noise": (NoiseSettings, {"noise_sigma": 2.0, "pedestals": 300, "noise_stream": 3}, NoiseSettings(2.0, None, 300, 3)),
    "readout": (ReadoutSettings, {"readout": "full", "readout_pads": [3, 5, 8]}, ReadoutSettings("full", [3, 5, 8])),
    "gain": (GainSettings, None, GainSettings(theta=1.0, pad_gain=1.25, stream=7)),
    "peaks": (PeakSettings, None, PeakSettings(prominence=30.0, threshold=35.0)),
    "baseline": (BaselineSettings, None, BaselineSettings(25.0)),
    "trigger": (TriggerSettings, None, TriggerSettings(25, window=50, group_multiplicity=4, gate=True)),
}
CASES = {"all_off": (), **{name: (name,) for name in STAGES}, "all_on": tuple(STAGES)}


@pytest.fixture(scope="module")
def config():
    return workloads.o16aa()[1]


def _chain(config, on):
    kw = {k: v for name in on if STAGES[name][1] for k, v in STAGES[name][1].items()}
    return TraceChain.from_kwargs(config, **kw).replace(**{name: STAGES[name][2] for name in on if not STAGES[name][1]})


def _uploads(ctx):
    """{slot: (token, descriptor scalars or None)} of what ``ctx`` was configured with."""
    calls = {name: desc for name, desc in ctx.lib.configure_descs}
    return {cls.slot: (ctx._tokens[cls.slot], calls.get(cls.call)) for cls, _, _ in STAGES.values()}


@pytest.mark.parametrize("case", CASES)
def test_chain_uploads_what_its_parts_upload(config, case):
    on = CASES[case]
    chain, parts = RecordingContext(), RecordingContext()
    _chain(config, on).configure(chain, rows=True)
    for name, (cls, _, settings) in STAGES.items():
        default = PeakSettings() if name == "peaks" else None  # (trace rows always have peaks)
        configure_stage(parts, cls, settings if name in on else default)
    assert _uploads(chain) == _uploads(parts)
    for name, (cls, _, settings) in STAGES.items():
        token, desc = _uploads(chain)[cls.slot]
        if name in on:
            assert token == settings.token() and desc is not None
        elif name != "peaks":
            assert token is None and desc is None  # off: never uploaded to a new context
    # the fixed part, and the call order
    response, threshold, offset = trace_settings(config)
    assert chain._tokens["trace"] == (response.tobytes(), threshold, offset) and chain._trace_readout_rows == (
        3 if "readout" in on else 0)
    order = ["trace_configure", "trace_configure_noise", "trace_configure_readout", "spyral_configure", "trace_configure_peaks",
             "trace_configure_baseline", "trace_configure_trigger", "trace_configure_gain"]
    assert chain.lib.names() == [n for n in order if n in chain.lib.names()] and chain.lib.names()[0] == "trace_configure"


def test_chain_holds_the_settings_it_was_given(config):
    chain = _chain(config, tuple(STAGES))
    for name in ("gain", "peaks", "baseline", "trigger"):
        assert getattr(chain, name) is STAGES[name][2]
    assert chain.noise.token() == STAGES["noise"][2].token() and chain.readout.token() == STAGES["readout"][2].token()
    plain = TraceChain(config)
    assert plain.noise.token() is None and plain.readout.token() is None and plain.threshold == config.elec_params.adc_threshold
    assert (plain.gain, plain.peaks, plain.baseline, plain.trigger) == (None, None, None, None) and plain.offset == 0
    # keep: the trigger and the gain of the context are left alone
    ctx = RecordingContext()
    chain.configure(ctx, rows=True)
    ctx.lib.calls.clear()
    plain.configure(ctx, rows=True, keep=("trigger", "gain"))
    assert "trace_configure_trigger" not in ctx.lib.names() and "trace_configure_gain" not in ctx.lib.names()
    assert ctx._tokens["trigger"] == STAGES["trigger"][2].token() and ctx._tokens["baseline"] is None


def test_from_kwargs_refuses_an_unknown_keyword(config):
    for kw in ({"noise": 1.0}, {"gain": GainSettings(theta=1.0)}, {"peaks": PeakSettings()}, {"trigger": None}):
        with pytest.raises(TypeError, match="unexpected trace settings"):
            TraceChain.from_kwargs(config, **kw)


# the bad values of tests/test_trace_noise_cpu.py and tests/test_readout_cpu.py (ValueError each, there and here)
_CDF, _LO = gaussian_noise_table(2.0)
BAD_KWARGS = [
    {"noise_sigma": 32.0}, {"noise_sigma": -1.0}, {"noise_sigma": float("nan")}, {"noise_sigma": float("inf")},
    {"pedestals": np.full(10240, -1)}, {"pedestals": np.full(10240, 4096)}, {"pedestals": np.zeros(5)},
    {"pedestals": np.full(10240, 1.5)}, {"noise_table": (_CDF[::-1], _LO)},
    {"noise_table": (np.arange(512, dtype=np.uint32), 0)}, {"noise_table": (_CDF, 4096)},
    {"noise_table": (np.array([-1, 3]), 0)}, {"noise_stream": 1 << 31}, {"noise_stream": -1},
    {"noise_sigma": 1.0, "noise_table": (_CDF, _LO)},
    {"readout": "zero"}, {"readout": 1}, {"readout": "partial", "readout_pads": [0, 10240]},
    {"readout": "full", "readout_pads": [-1]}, {"readout": "full", "readout_pads": [3, 4, 3]},
    {"readout": "partial", "readout_pads": np.ones(10239, dtype=bool)},
    {"readout": "partial", "readout_pads": np.ones((2, 10240), dtype=bool)},
    {"readout": "partial", "readout_pads": [1.5, 2.0]}, {"readout_pads": [5, 5]}, {"readout": "full", "readout_pads": [1, 1]},
    {"response": np.ones(100)},  # (tests/test_traces_cpu.py: the response has 512 samples)
]


@pytest.mark.parametrize("kw", BAD_KWARGS, ids=[f"{i}-{'-'.join(kw)}" for i, kw in enumerate(BAD_KWARGS)])
def test_from_kwargs_refuses_the_bad_values_of_noise_and_readout(config, kw):
    with pytest.raises(ValueError):
        TraceChain.from_kwargs(config, **kw)


def test_chain_refuses_a_gain_that_is_no_gain_settings(config):
    # (tests/test_gain_cpu.py.  The bad values of the gain, peak, baseline and trigger settings never reach a chain:
    #  it takes those stages as objects their own classes have validated -- tests/test_gain_cpu.py, test_peaks_cpu.py,
    #  test_baseline_cpu.py and test_trigger_cpu.py -- and from_kwargs refuses their names, above)
    for bad in (0.5, {"theta": 1.0}, "on"):
        with pytest.raises(TypeError, match="gain must be a GainSettings or None"):
            TraceChain(config, gain=bad)
        with pytest.raises(TypeError, match="gain must be a GainSettings or None"):
            TraceChain.from_kwargs(config).replace(gain=bad)


def test_replace_takes_its_fields_only_and_a_config_fills_the_defaults_in_again(config):
    import copy
    import dataclasses

    chain = TraceChain.from_kwargs(config, noise_sigma=2.0)
    for bad in ({"triger": None}, {"noise": NoiseSettings()}, {"threshold": 3.0}):
        with pytest.raises(TypeError, match="TraceChain.replace takes"):
            chain.replace(**bad)
    other = copy.copy(config)
    other.elec_params = dataclasses.replace(config.elec_params, adc_threshold=config.elec_params.adc_threshold + 7)
    moved = chain.replace(config=other)
    assert moved.config is other and moved.threshold == other.elec_params.adc_threshold != chain.threshold
    assert moved.response.tobytes() == trace_settings(other)[0].tobytes() and moved.noise is chain.noise
    # a response and a threshold that were given stay as given
    given = TraceChain(config, np.arange(512.0), 12.0, 3).replace(config=other, trigger=STAGES["trigger"][2])
    assert (given.threshold, given.offset) == (12.0, 3) and given.response.tobytes() == np.arange(512.0).tobytes()
    assert given.trigger is STAGES["trigger"][2] and chain.config is config
