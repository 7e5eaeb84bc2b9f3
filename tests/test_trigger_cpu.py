"""The multiplicity trigger of the pad traces without a device: the numpy restatement (tests/trigger_reference.py)
against a brute-force loop straight from the contract's definitions, the edges of the definitions one by one, the
validation of ``TriggerSettings``, the record's layout, and the host side of the triggered writers with the library
replaced by the recording stand-in of tests/test_run_layer_cpu.py."""
import ctypes as C
import sys
import warnings

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.traces import TRIGGER_DTYPE, TriggerSettings, traces_to_trigger
from tests import trigger_reference as ref
from tests.test_run_layer_cpu import POINTS, RecordingContext, RecordingLibrary

NUM_TB = _abi.NUM_TB


def _rows(*runs, n_rows=None, level=100):
    """Rows of zeros with ``level`` on the samples lo .. hi of (row, lo, hi)."""
    n_rows = 1 + max(r for r, _, _ in runs) if n_rows is None else n_rows
    x = np.zeros((n_rows, NUM_TB), dtype=np.int16)
    for r, lo, hi in runs:
        x[r, lo:hi + 1] = level
    return x


def _one(pads, samples, trigger, pedestals=None):
    fast = ref.event_record(pads, samples, trigger, pedestals)
    assert fast == ref.event_record_brute(pads, samples, trigger, pedestals)
    return dict(zip(ref.FIELDS, fast))


def test_restatement_equals_brute_force_on_random_rows():
    rng = np.random.default_rng(11)
    groups = rng.integers(0, 10, size=_abi.NUM_PADS).astype(np.uint8)
    groups[rng.random(_abi.NUM_PADS) < 0.1] = 255
    pedestals = rng.integers(200, 401, size=_abi.NUM_PADS)
    fired = []
    for case, (window, mg, min_groups) in enumerate([(1, 1, 1), (20, 15, 2), (512, 60, 1), (50, 4, 3)]):
        for n_rows in (1, 3, 6):
            pads, samples = ref.pulse_rows(rng, n_rows, pedestals)
            trigger = ref.Params(25, window, mg, min_groups, groups)
            fired.append(_one(pads, samples, trigger, pedestals)["fired"])
            _one(pads, samples, ref.Params(25, window, mg, min_groups, None), None)
    assert 0 in fired and 1 in fired


def test_windows():
    x = _rows((0, 10, 12))  # hits at 10, 11, 12
    pads = np.array([5])
    assert _one(pads, x, ref.Params(50, 1, 1))["sample"] == 10
    assert _one(pads, x, ref.Params(50, 1, 2))["fired"] == 0           # W = 1 never sums two samples
    rec = _one(pads, x, ref.Params(50, 512, 3))
    assert (rec["fired"], rec["sample"], rec["peak_group_sum"]) == (1, 12, 3)
    rec = _one(pads, x, ref.Params(50, 100, 3))                        # W larger than the first hit's sample
    assert (rec["sample"], rec["peak_sample"]) == (12, 12)
    rec = _one(pads, x, ref.Params(50, 2, 3))                          # the window drops the first hit again
    assert (rec["fired"], rec["peak_group_sum"], rec["peak_sample"]) == (0, 2, 11)
    tail = _rows((0, 0, 0), (0, 511, 511))
    rec = _one(pads, tail, ref.Params(50, 511, 2))                     # 0 and 511 never share a window of 511
    assert rec["fired"] == 0 and _one(pads, tail, ref.Params(50, 512, 2))["sample"] == 511


def test_threshold_is_strict_and_above_the_pedestal():
    x = _rows((0, 40, 40), level=130)
    pads = np.array([7])
    ped = np.zeros(_abi.NUM_PADS, dtype=np.int64)
    ped[7] = 30
    assert _one(pads, x, ref.Params(100, 1, 1), ped)["fired"] == 0     # y == threshold is not a hit
    assert _one(pads, x, ref.Params(99, 1, 1), ped)["sample"] == 40
    assert _one(pads, x, ref.Params(100, 1, 1), None)["sample"] == 40  # without the pedestal y = 130


def test_multiplicity_reached_exactly_and_one_short():
    x = _rows((0, 100, 101), (1, 101, 102), (2, 300, 300))
    pads = np.array([1, 2, 3])
    rec = _one(pads, x, ref.Params(50, 4, 4))
    assert (rec["fired"], rec["sample"], rec["peak_group_sum"], rec["n_hit_pads"], rec["n_rows"]) == (1, 102, 4, 3, 3)
    assert _one(pads, x, ref.Params(50, 4, 5))["fired"] == 0


def test_min_groups_and_excluded_pads():
    groups = np.full(_abi.NUM_PADS, 255, dtype=np.uint8)
    groups[[0, 1, 2, 3]] = [0, 4, 15, 4]
    x = _rows((0, 50, 60), (1, 55, 70), (2, 65, 80), (3, 200, 210), (4, 0, 511))
    pads = np.array([0, 1, 2, 3, 9])  # pad 9 takes no part
    rec = _one(pads, x, ref.Params(50, 1, 1, 1, groups))
    assert (rec["sample"], rec["groups"], rec["n_rows"], rec["n_hit_pads"]) == (50, 1 | 1 << 4 | 1 << 15, 5, 4)
    assert _one(pads, x, ref.Params(50, 1, 1, 3, groups))["fired"] == 0        # never three groups in one sample
    rec = _one(pads, x, ref.Params(50, 16, 1, 3, groups))
    assert (rec["fired"], rec["sample"]) == (1, 65)                            # 0 until 75, 4 until 85, 15 from 65
    assert _one(pads, x, ref.Params(50, 1, 1, 2, groups))["sample"] == 55
    only_excluded = _one(np.array([9]), x[4:], ref.Params(50, 1, 1, 1, groups))
    assert only_excluded == dict(zip(ref.FIELDS, (0, -1, 0, 1, 0, 0, 0, -1)))


def test_first_index_on_ties():
    x = _rows((0, 20, 20), (1, 20, 20), (0, 90, 90), (1, 90, 90))
    rec = _one(np.array([3, 4]), x, ref.Params(50, 1, 2))
    assert (rec["sample"], rec["peak_sample"], rec["peak_sum"]) == (20, 20, 2)
    flat = _rows((0, 0, 511))
    rec = _one(np.array([3]), flat, ref.Params(50, 8, 8))
    assert (rec["sample"], rec["peak_sample"], rec["peak_sum"]) == (7, 7, 8)


def test_empty_event_and_csr():
    x = _rows((0, 5, 9), (1, 7, 9))
    got = ref.records([0, 0, 2, 2], np.array([1, 2]), x, ref.Params(50, 4, 1))
    assert got.dtype == TRIGGER_DTYPE and got.tolist() == [(0, -1, 0, 0, 0, 0, 0, -1), (1, 5, 1, 2, 2, 7, 7, 9),
                                                           (0, -1, 0, 0, 0, 0, 0, -1)]


@pytest.mark.parametrize("kw", [
    {"threshold": -1}, {"threshold": 4096}, {"threshold": 10.5}, {"threshold": True}, {"window": 0}, {"window": 513},
    {"group_multiplicity": 0}, {"min_groups": 0}, {"min_groups": 17}, {"groups": np.zeros(5, dtype=np.uint8)},
    {"groups": np.full(_abi.NUM_PADS, 16)}, {"groups": np.full(_abi.NUM_PADS, -1)}, {"groups": np.zeros(_abi.NUM_PADS)},
    {"gate": 2}])
def test_trigger_settings_refuse(kw):
    with pytest.raises(ValueError):
        TriggerSettings(**{"threshold": 25, **kw})


def test_trigger_settings_token_and_desc():
    groups = np.arange(_abi.NUM_PADS) % 16
    groups[3] = 255
    t = TriggerSettings(25, window=50, group_multiplicity=4, min_groups=3, groups=groups)
    d = t.desc()
    assert (d.threshold, d.window, d.group_multiplicity, d.min_groups, d.gate, d.reserved) == (25, 50, 4, 3, 0, 0)
    assert [d.groups[i] for i in (0, 3, 17)] == [0, 255, 1] and t.groups.dtype == np.uint8
    assert t.token() != t.gated().token() and t.gated().desc().gate == 1 and t.gated(False).token() == t.token()
    assert TriggerSettings(25).token() == TriggerSettings(25, 64, 1, 1, None, False).token()
    assert not TriggerSettings(25).desc().groups
    ctx = RecordingContext()
    with pytest.raises(TypeError):
        traces_to_trigger([0], np.zeros(0, dtype=np.int32), np.zeros((0, NUM_TB), dtype=np.int16), None, ctx=ctx)
    for bad in ({"pads": np.array([_abi.NUM_PADS])}, {"samples": np.full((1, NUM_TB), 4096)}, {"offsets": [0, 2]},
                {"pedestals": 5000}):
        args = {"offsets": [0, 1], "pads": np.array([0]), "samples": np.zeros((1, NUM_TB), dtype=np.int16), "pedestals": None, **bad}
        with pytest.raises(ValueError):
            traces_to_trigger(args["offsets"], args["pads"], args["samples"], t, args["pedestals"], ctx=ctx)
    assert ctx.lib.calls == []  # everything is refused before the library is called


def test_record_layout_and_sources():
    import __graft_entry__ as entry

    assert "trigger.hip" in entry.HIP_SOURCES
    assert TRIGGER_DTYPE.itemsize == 32 == C.sizeof(_abi.TriggerRecord)
    assert TRIGGER_DTYPE.names == ref.FIELDS == tuple(name for name, _ in _abi.TriggerRecord._fields_)
    assert [TRIGGER_DTYPE.fields[f][1] for f in ref.FIELDS] == list(range(0, 32, 4))
    assert TRIGGER_DTYPE["groups"] == np.uint32 and all(TRIGGER_DTYPE[f] == np.int32 for f in ref.FIELDS if f != "groups")
    assert set(_abi.TRIGGER_SYMBOLS) <= set(_abi.EXPORTED_SYMBOLS) and "trigger" in _abi.CONFIGURE_SLOTS
    header = (entry.ROOT / "include" / "attpc_engine.h").read_text()
    assert "#define ATTPC_MAX_TRIGGER_GROUPS 16" in header and _abi.MAX_TRIGGER_GROUPS == 16
    script = (entry.ROOT / "tools" / "build_variant.sh").read_text()
    assert "trigger.hip" in script and "baseline.hip" in script


# ---------------------------------------------------------------- the triggered writers, the library replaced ----
def _fires(event):
    return event % 3 != 1


class TriggerLibrary(RecordingLibrary):
    """The recording library with a trigger: the records of the last run call fire on the global events ``_fires``
    names; the descriptors of the configure calls are kept."""

    def __init__(self):
        super().__init__()
        self.first, self.descs = 0, []

    def _call(self, name, args):
        if name.endswith("_run_traces") or name.endswith("_run_trace_rows"):
            self.first = args[2]
        if name == "attpc_trace_configure_trigger":
            self.descs.append(None if args[1] is None else (args[1].threshold, args[1].gate))
        status = super()._call(name, args)
        if name == "attpc_trigger_last":
            _, first, count, out = args
            for i in range(count):
                out[first + i].fired = int(_fires(self.first + first + i))
        return status


@pytest.fixture
def no_h5py(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)


class TraceSink:
    def __init__(self):
        self.events, self.closed = [], 0

    def write_traces(self, pads, samples, labels, event):
        self.events.append((event, len(pads)))

    def close(self):
        self.closed += 1


def test_run_fused_with_a_trigger(tmp_path, no_h5py):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import PeakSettings, SpyralWriter
    from attpc_engine_amd.engine import Engine, run_fused

    pipeline, config, indices = workloads.o16aa()
    ctx = RecordingContext(TriggerLibrary())
    lib = ctx.lib
    trigger = TriggerSettings(25, window=50, group_multiplicity=4)
    sink = TraceSink()
    sink.response, sink.threshold, sink.offset = None, None, 0
    sink.noise_kwargs = sink.readout_kwargs = dict
    run_fused(pipeline, config, sink, 10, indices, seed=8, batch_size=4, context=ctx, trigger=trigger)
    assert [c[1] for c in lib.of("sim_run_traces")] == [(8, 0, 4), (8, 4, 4), (8, 8, 2)]
    assert [c[1] for c in lib.of("trigger_last")] == [(0, 4), (0, 4), (0, 2)] and lib.descs == [(25, 0)]
    # exactly the fired events with a cloud, under their own numbers (ROWS / POINTS of the stand-in: id % 4)
    written = [i for i in range(10) if _fires(i) and POINTS[i % 4]]
    assert written == [2, 3, 5, 6, 9] and [e for e, _ in sink.events] == written and sink.closed == 1
    assert [n for _, n in sink.events] == [1, 2, 0, 1, 0]
    # without a trigger: every event with a cloud, no records asked for, a trigger the context held is turned off
    lib.calls.clear()
    plain = TraceSink()
    plain.response, plain.threshold, plain.offset, plain.noise_kwargs, plain.readout_kwargs = None, None, 0, dict, dict
    run_fused(pipeline, config, plain, 10, indices, seed=8, batch_size=4, context=ctx)
    assert [e for e, _ in plain.events] == [i for i in range(10) if POINTS[i % 4]]
    assert not lib.of("trigger_last") and lib.descs == [(25, 0), None]
    # trace rows: the gate is set for the device
    lib.calls.clear()
    run_fused(pipeline, config, SpyralWriter(tmp_path, config, peaks=PeakSettings(), npz_fallback=True), 4, indices, seed=8,
              context=ctx, trigger=trigger)
    assert lib.descs[-1] == (25, 1) and len(lib.of("sim_run_trace_rows")) == 1 and len(lib.of("trigger_last")) == 1
    # a writer of Spyral rows or clouds
    lib.calls.clear()
    with pytest.raises(ValueError, match="a trigger delivers traces or trace rows"):
        run_fused(pipeline, config, SpyralWriter(tmp_path, config), 4, indices, context=ctx, trigger=trigger)
    assert not [n for n in lib.names() if "run" in n]
    # the engine's own calls
    engine = Engine(pipeline, config, indices, context=ctx)
    with pytest.raises(RuntimeError, match="configure_trigger"):
        (engine.configure_trigger(), engine.run_trigger(4))
    engine.configure_trigger(threshold=30, window=8)
    lib.calls.clear()
    res = engine.run_trigger(5, seed=1, first_event=3)
    assert lib.names() == ["sim_run_traces", "trigger_last"] and lib.calls[0][2] == 0  # nothing fetched
    assert res["trigger"]["fired"].tolist() == [int(_fires(3 + i)) for i in range(5)] and "pads" not in res
    with pytest.raises(TypeError):
        engine.configure_trigger(trigger, threshold=3)
    engine.configure_trigger()
    assert "trigger" not in engine.run_traces(2, fetch=False)


def test_run_simulation_with_a_trigger(tmp_path, monkeypatch, capsys, no_h5py):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import SpyralWriter, run_simulation
    from attpc_engine_amd.io import KinematicsFileWriter

    pipeline, config, indices = workloads.o16aa()
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    path = tmp_path / "kin.npz"
    w = KinematicsFileWriter(path, 10, z, a, chunk_size=4)
    rng = np.random.default_rng(1)
    w.write_batch(0, rng.normal(size=(10, 3)), rng.normal(size=(10, len(z), 4)))
    w.close()
    ctx = RecordingContext(TriggerLibrary())
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    sink = TraceSink()
    sink.response, sink.threshold, sink.offset, sink.noise_kwargs, sink.readout_kwargs = None, None, 0, dict, dict
    sink.get_directory_name = lambda: tmp_path
    run_simulation(config, path, sink, indices, batch_size=4, seed=5, trigger=TriggerSettings(25))
    assert [e for e, _ in sink.events] == [2, 3, 5, 6, 9] and sink.closed == 1
    with pytest.raises(ValueError, match="a trigger delivers traces or trace rows"):
        run_simulation(config, path, SpyralWriter(tmp_path, config), indices, seed=5, trigger=TriggerSettings(25))
    capsys.readouterr()
