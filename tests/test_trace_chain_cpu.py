"""``TraceChain`` against its parts, without a device: per context slot the chain uploads the content (token) and the
descriptor scalars of the individually constructed settings classes -- all stages off, each alone, all on --, and
``from_kwargs`` refuses what the settings classes and ``validate_trace_kwargs`` refuse, with the same exception type.
Then the chain as a whole: the order of its configure calls with every stage on and with every stage turned off again,
what each ``keep`` group leaves alone, what ``configure_trace_rows`` uploads when it is given every optional stage, and
the keys every trace-row entry point returns with all stages on and with none.
The library is the recording stand-in of tests/test_run_layer_cpu.py."""
import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.clustering import ClusterSettings
from attpc_engine_amd.detector.correction import CorrectionSettings
from attpc_engine_amd.detector.estimate import EstimateSettings
from attpc_engine_amd.detector.fit import TrackFitSettings
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.joining import JoinSettings
from attpc_engine_amd.detector.pid import Gate, PidSettings
from attpc_engine_amd.detector.thinning import ThinSettings
from attpc_engine_amd.detector.traces import (
    BaselineSettings, CommonModeSettings, GainSettings, NoiseSettings, PeakSettings, ReadoutSettings, TraceChain,
    TriggerSettings, configure_stage, configure_trace_rows, gaussian_noise_table, simulate_batch_trace_rows, trace_settings)
from attpc_engine_amd.engine import Engine
from tests import distortion_cases as dc
from tests.test_run_layer_cpu import RecordingContext, _kinematics

STAGES = {  # chain field -> (settings class, how from_kwargs or replace gets it, the settings built on their own)
    "noise": (NoiseSettings, {"noise_sigma": 2.0, "pedestals": 300, "noise_stream": 3}, NoiseSettings(2.0, None, 300, 3)),
    "readout": (ReadoutSettings, {"readout": "full", "readout_pads": [3, 5, 8]}, ReadoutSettings("full", [3, 5, 8])),
    "gain": (GainSettings, None, GainSettings(theta=1.0, pad_gain=1.25, stream=7)),
    "peaks": (PeakSettings, None, PeakSettings(prominence=30.0, threshold=35.0)),
    "baseline": (BaselineSettings, None, BaselineSettings(25.0)),
    "trigger": (TriggerSettings, None, TriggerSettings(25, window=50, group_multiplicity=4, gate=True)),
    "common_mode": (CommonModeSettings, None, CommonModeSettings(1.5, stream=5)),
    "correction": (CorrectionSettings, None, CorrectionSettings(dc.named_map(), iterations=7)),
    "clustering": (ClusterSettings, None, ClusterSettings(eps_xy=15.0, min_samples=4, match="rank")),
    "join": (JoinSettings, None, JoinSettings(overlap_ratio=0.25, max_clusters=16)),
    "estimates": (EstimateSettings, None, EstimateSettings(30.0, min_points=20)),
    "thinning": (ThinSettings, None, ThinSettings(10.0)),
    "circle": (CircleFitSettings, None, CircleFitSettings(max_evaluations=12)),
    "helix": (HelixSlopeSettings, None, HelixSlopeSettings("path_on_z")),
    "fit": (TrackFitSettings, None, TrackFitSettings(max_steps=500, max_evaluations=8)),
    "pid": (PidSettings, None, PidSettings([Gate.rectangle((0.1, 2.0), (1.0, 50.0)), None, [(0, 0), (1, 0), (1, 1)]], "own")),
}
# every configure call of ``TraceChain.configure(rows=True)``, in its order
ORDER = ["trace_configure", "trace_configure_noise", "trace_configure_common_mode", "trace_configure_readout",
         "spyral_configure", "trace_configure_peaks", "trace_configure_baseline", "trace_configure_trigger",
         "trace_configure_gain", "trace_configure_correction", "trace_configure_clustering", "trace_configure_cluster_join",
         "trace_configure_estimates", "trace_configure_thinning", "trace_configure_circle", "trace_configure_helix",
         "trace_configure_fit", "trace_configure_pid"]
# the stages each name of ``keep`` leaves as the context holds them
KEEP = {"trigger": ("trigger",), "gain": ("gain",), "common_mode": ("common_mode",), "correction": ("correction",),
        "clustering": ("clustering", "join"), "estimates": ("estimates", "thinning", "circle", "helix", "fit", "pid")}
CASES = {"all_off": (), **{name: (name,) for name in STAGES}, "all_on": tuple(STAGES)}


@pytest.fixture(scope="module")
def config():
    return workloads.o16aa()[1]


def _chain(config, on):
    kw = {k: v for name in on if STAGES[name][1] for k, v in STAGES[name][1].items()}
    return TraceChain.from_kwargs(config, **kw).replace(**{name: STAGES[name][2] for name in on if not STAGES[name][1]})


def _token(config, name):
    """The content of stage ``name`` of STAGES as the chain uploads it: the estimates in the field of the config, the
    correction in its drift."""
    settings = STAGES[name][2]
    if name == "correction":
        return settings.token(config)
    return (settings.for_field(config.det_params.bfield) if name == "estimates" else settings).token()


def _configure_alone(ctx, config, name, on=True):
    """Stage ``name`` of STAGES on its own through ``configure_stage`` (``on`` False: turned off; the peaks: their
    default, trace rows always have peaks).  The correction's token and descriptor need the config, which
    ``configure_stage`` does not pass: it goes through ``Context.configure``, as ``configure_stage`` does."""
    cls, _, settings = STAGES[name]
    if not on:
        configure_stage(ctx, cls, PeakSettings() if name == "peaks" else None)
    elif name == "correction":
        ctx.configure(cls.slot, settings.token(config), cls.call, settings.desc(config))
    else:
        configure_stage(ctx, cls, settings.for_field(config.det_params.bfield) if name == "estimates" else settings)


def _uploads(ctx):
    """{slot: (token, descriptor scalars or None)} of what ``ctx`` was configured with."""
    calls = {name: desc for name, desc in ctx.lib.configure_descs}
    return {cls.slot: (ctx._tokens[cls.slot], calls.get(cls.call)) for cls, _, _ in STAGES.values()}


@pytest.mark.parametrize("case", CASES)
def test_chain_uploads_what_its_parts_upload(config, case):
    on = CASES[case]
    chain, parts = RecordingContext(), RecordingContext()
    _chain(config, on).configure(chain, rows=True)
    for name in STAGES:
        _configure_alone(parts, config, name, name in on)
    assert _uploads(chain) == _uploads(parts)
    for name, (cls, _, settings) in STAGES.items():
        token, desc = _uploads(chain)[cls.slot]
        if name in on:
            assert token == _token(config, name) and desc is not None
        elif name != "peaks":
            assert token is None and desc is None  # off: never uploaded to a new context
    # the fixed part, and the call order
    response, threshold, offset = trace_settings(config)
    assert chain._tokens["trace"] == (response.tobytes(), threshold, offset) and chain._trace_readout_rows == (
        3 if "readout" in on else 0)
    assert chain.lib.names() == [n for n in ORDER if n in chain.lib.names()] and chain.lib.names()[0] == "trace_configure"


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


def test_every_row_of_the_stage_table_is_wired_in(config):
    """What ``detector.traces`` promises of a row of ``STAGES``: the chain has the field and ``replace`` takes it, the
    context has the slot, the library exports the call, and the trace-row entry point takes the keyword."""
    import inspect

    from attpc_engine_amd.detector import traces

    keywords = inspect.signature(simulate_batch_trace_rows).parameters
    chain = TraceChain(config)
    assert {stage.field for stage in traces.STAGES} == set(STAGES)  # (so the tests above cover every row)
    for stage in traces.STAGES:
        assert hasattr(chain, stage.field) and stage.field in inspect.signature(TraceChain).parameters
        assert stage.settings.slot in _abi.CONFIGURE_SLOTS and stage.settings.call in _abi.EXPORTED_SYMBOLS
        assert any(stage.settings.call in group for group in _abi.SYMBOL_GROUPS.values()) or stage.field in ("noise", "readout")
        if stage.replace:
            assert getattr(chain.replace(**{stage.field: STAGES[stage.field][2]}), stage.field) is STAGES[stage.field][2]
            assert stage.field in keywords and stage.field in traces.REPLACE_FIELDS
        else:  # the noise and the readout come as the keywords of TRACE_KWARGS
            with pytest.raises(TypeError, match="TraceChain.replace takes"):
                chain.replace(**{stage.field: STAGES[stage.field][2]})
    replaceable = {stage.field for stage in traces.STAGES if stage.replace}
    assert list(traces.REPLACE_FIELDS) == ["config"] + [name for name in inspect.signature(TraceChain).parameters
                                                        if name in replaceable]
    # the configure order of the table is the one written out above
    assert [stage.settings.call[len("attpc_"):] for stage in traces.STAGES] == [
        name for name in ORDER if name not in ("trace_configure", "spyral_configure")]


def _descs(ctx):
    """{call without ``attpc_``: scalar fields of its descriptor, or None} of the configure calls ``ctx`` recorded, each
    made once."""
    descs = {name[len("attpc_"):]: desc for name, desc in ctx.lib.configure_descs}
    assert len(descs) == len(ctx.lib.configure_descs)
    return descs


def _all_on(config):
    """(a context the chain with every stage of STAGES on has configured, what every stage uploads on its own)"""
    ctx, parts = RecordingContext(), RecordingContext()
    _chain(config, tuple(STAGES)).configure(ctx, rows=True)
    for name in STAGES:
        _configure_alone(parts, config, name)
    return ctx, _descs(parts)


def test_configure_makes_every_call_in_one_order_and_turns_every_stage_off_again(config):
    ctx, alone = _all_on(config)
    assert ctx.lib.names() == ORDER
    descs = _descs(ctx)
    assert {name: descs[name] for name in alone} == alone and all(desc is not None for desc in descs.values())
    assert all(ctx._tokens[STAGES[name][0].slot] == _token(config, name) for name in STAGES)
    # the plain chain on that context: every stage is turned off in the same order; the response and the geometry are
    # the same and are not uploaded again, the peaks go back to their defaults
    ctx.lib.calls.clear()
    ctx.lib.configure_descs.clear()
    TraceChain(config).configure(ctx, rows=True)
    assert ctx.lib.names() == [name for name in ORDER if name not in ("trace_configure", "spyral_configure")]
    descs = _descs(ctx)
    assert descs.pop("trace_configure_peaks") == {f: getattr(PeakSettings().desc(), f) for f, _ in _abi.PeakDesc._fields_}
    assert set(descs.values()) == {None}
    assert all(ctx._tokens[cls.slot] is None for name, (cls, _, _) in STAGES.items() if name != "peaks")
    # traces, not rows: neither the geometry nor a stage of the rows is touched
    fresh = RecordingContext()
    _chain(config, tuple(STAGES)).configure(fresh)
    assert fresh.lib.names() == ["trace_configure", "trace_configure_noise", "trace_configure_common_mode",
                                 "trace_configure_readout", "trace_configure_trigger", "trace_configure_gain"]


@pytest.mark.parametrize("group", KEEP)
def test_keep_leaves_its_stages_as_the_context_holds_them(config, group):
    ctx, _ = _all_on(config)
    ctx.lib.calls.clear()
    TraceChain(config).configure(ctx, rows=True, keep=(group,))
    kept = [STAGES[name][0] for name in KEEP[group]]
    off = [name for name in ORDER if name not in ("trace_configure", "spyral_configure")]
    assert ctx.lib.names() == [name for name in off if "attpc_" + name not in [cls.call for cls in kept]]
    for name, (cls, _, _) in STAGES.items():
        if name in KEEP[group]:
            assert ctx._tokens[cls.slot] == _token(config, name)
        elif name != "peaks":
            assert ctx._tokens[cls.slot] is None


def test_configure_trace_rows_uploads_every_stage_it_is_given(config):
    taken = ("noise", "readout", "gain", "peaks", "baseline", "common_mode", "correction", "clustering", "join", "thinning",
             "circle", "helix", "pid")
    left = ("trigger", "estimates", "fit")  # these stay as the context holds them
    _, alone = _all_on(config)
    ctx = RecordingContext()
    for name in left:
        _configure_alone(ctx, config, name)
    ctx.lib.calls.clear()
    ctx.lib.configure_descs.clear()
    configure_trace_rows(config, ctx, **STAGES["noise"][1], **STAGES["readout"][1],
                         **{name: STAGES[name][2] for name in taken[2:]})
    # (compared as a set of calls, each made once, with its descriptor: not as an order)
    descs = _descs(ctx)
    assert sorted(ctx.lib.names()) == sorted(["trace_configure", "spyral_configure"] + [STAGES[name][0].call[len("attpc_"):]
                                                                                      for name in taken])
    assert {name: desc for name, desc in descs.items() if name in alone} == {
        STAGES[name][0].call[len("attpc_"):]: alone[STAGES[name][0].call[len("attpc_"):]] for name in taken}
    assert all(ctx._tokens[STAGES[name][0].slot] == _token(config, name) for name in taken + left)
    # given nothing, it turns off what it owns and leaves the reconstruction stages and the trigger alone
    ctx.lib.calls.clear()
    configure_trace_rows(config, ctx)
    assert sorted(ctx.lib.names()) == sorted(STAGES[name][0].call[len("attpc_"):] for name in taken[:6])
    kept = ("correction", "clustering", "join", "thinning", "circle", "helix", "pid") + left
    assert all(ctx._tokens[STAGES[name][0].slot] == _token(config, name) for name in kept)


# the keys of a trace-row result beside the stages', and what every stage adds when it is on
STAGE_KEYS = {"trigger", "estimates", "thinning", "circle", "slope", "correction", "fits", "clusters", "joins", "pid"}
FETCHED = {"vertex", "p4", "status", "offsets", "labels", "event_points", "stats", "rows", "trace_rows"}
RESIDENT = {"stats", "trace_rows"}
ESTIMATES = {"estimates", "indices", "vertex", "p4", "status", "stats", "trace_rows"}


@pytest.mark.parametrize("on", [True, False], ids=["all_on", "all_off"])
def test_trace_row_results_carry_the_keys_of_the_stages_that_are_on(config, on):
    pipeline, _, indices = workloads.o16aa()
    engine = Engine(pipeline, config, indices, context=RecordingContext())
    chain = _chain(config, tuple(STAGES) if on else ())
    engine._configure_chain(chain, rows=True)
    extra = STAGE_KEYS if on else set()
    n, n_sim = 5, len(indices)
    fetched = engine.run_trace_rows(n, seed=2, first_event=1)
    assert set(fetched) == FETCHED | extra | ({"cluster_labels"} if on else set())
    resident = engine.run_trace_rows(n, seed=2, first_event=1, fetch=False)
    assert set(resident) == RESIDENT | extra
    if not on:
        with pytest.raises(RuntimeError, match="run_estimates needs the estimates"):
            engine.run_estimates(n)
        engine.configure_estimates(STAGES["estimates"][2])
    estimated = engine.run_estimates(n, seed=2, first_event=1)
    assert set(estimated) == ESTIMATES | extra
    momenta, vertices, z, a = _kinematics(workloads.o16aa(), n)
    ctx = RecordingContext()
    batch = simulate_batch_trace_rows(momenta, vertices, z, a, config, 2, indices, first_event=1, ctx=ctx,
                                      **{name: STAGES[name][2] for name in (STAGES if on else ()) if not STAGES[name][1]},
                                      **(dict(STAGES["noise"][1], **STAGES["readout"][1]) if on else {}))
    assert len(batch) == 5
    assert set(batch[4]) == set(_abi.RunStats().as_dict()) | {"n_rows", "row_checksum"} | extra | (
        {"cluster_labels"} if on else set())
    if on:
        rows = int(fetched["offsets"][-1])
        for res in (fetched, resident, estimated, batch[4]):
            assert res["estimates"].shape == res["fits"].shape == res["pid"].shape == (n, n_sim)
            assert (res["thinning"], res["circle"], res["slope"]) == (10.0, "geometric", "helix")
            assert res["trigger"].shape == (n,) and set(res["correction"]) == {"n_rows", "n_skipped", "n_unconverged", "n_moved"}
            assert [part.shape for part in res["clusters"]] == [part.shape for part in res["joins"]] == [(n,), (n, _abi.MAX_SIM)]
        assert fetched["cluster_labels"].shape == batch[4]["cluster_labels"].shape == (rows,)
        assert (estimated["estimates"].dtype, estimated["fits"].dtype, estimated["pid"].dtype) == (
            _abi.ESTIMATE_DTYPE, _abi.FIT_DTYPE, _abi.PID_DTYPE)
