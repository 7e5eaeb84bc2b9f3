"""Characterisation of the Python run layer above the C ABI: which library calls every entry point makes, with which
scalar arguments, output capacities and NULL pointers, what the capacity retry of each mode passes, which configure
calls the content tokens skip, and which events each kind of writer receives.

Nothing here needs the library or a device: the package is driven through a ``Context`` whose ``lib`` is a recording
stand-in.  Every ``lib.attpc_*`` call is recorded as ``(name, scalar arguments, capacity, NULL pointers)``; the run
calls fill offsets, rows and counters from two small tables keyed on the global event id, and can answer
ATTPC_E_CAPACITY on the first try.  The scalar fields of every configure call's descriptor are kept beside them
(``configure_descs``), and the trigger records of a run fire on the odd global event ids.
"""
import ctypes as C
import sys
import warnings

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from attpc_engine_amd.detector import SpyralWriter, TraceWriter
from attpc_engine_amd.detector.simulator import (
    configure_detector, configure_spyral, run_simulation, simulate, simulate_batch, simulate_batch_spyral)
from attpc_engine_amd.detector.traces import (
    BaselineSettings, GainSettings, PeakSettings, TriggerSettings, clouds_to_gain, clouds_to_trace_rows, clouds_to_traces,
    configure_trace_rows, configure_traces, configure_trigger, simulate_batch_trace_rows, simulate_batch_traces)
from attpc_engine_amd.detector.writer import convert_to_spyral
from attpc_engine_amd.engine import Engine, run_fused
from attpc_engine_amd.io import KinematicsFileWriter

# kept rows and cloud rows before the threshold of the global event g: ROWS[g % 4], POINTS[g % 4].  Events 0, 4, 8 are
# empty; events 1, 5, 9 have a cloud but keep no row (written by the Spyral and trace paths, skipped by plain write)
ROWS = (0, 0, 1, 2)
POINTS = (0, 5, 6, 7)
WIDTH = {"attpc_sim_run": 3, "attpc_det_run": 3, "attpc_sim_run_spyral": 8, "attpc_det_run_spyral": 8,
         "attpc_sim_run_traces": 0, "attpc_det_run_traces": 0, "attpc_traces_at": 0, "attpc_sim_run_trace_rows": 8,
         "attpc_det_run_trace_rows": 8, "attpc_trace_rows_at": 8}


class RecordingLibrary:
    """Stands in for libattpc_hip.so.  ``calls``: one ``(name, scalars, capacity, nulls)`` per call -- the int / float
    arguments after the context handle, the capacity of the output struct (None without one), and the positions of
    the NULL arguments plus the names of the NULL pointers of the output struct.  ``refuse[name] = rows``: the next
    call of ``name`` whose capacity is below ``rows`` reports that many needed rows and ATTPC_E_CAPACITY.
    ``configure_descs``: one ``(name, scalar fields of the descriptor or None)`` per configure call.  The trace-row
    calls leave their rows and ``33 + first event`` for ``attpc_trace_rows_last``; ``attpc_trigger_last`` fills records
    that fired on the odd global event ids of the last run call."""

    def __init__(self):
        self.calls = []
        self.refuse = {}
        self.configure_descs = []
        self.first = 0  # the first global event id of the last run call
        self.last_rows = (0, 0)  # (n_rows, row_checksum) of the last trace-row call

    def __getattr__(self, name):
        if not name.startswith("attpc_"):
            raise AttributeError(name)

        def call(*args):
            return self._call(name, args)

        return call

    def names(self):
        return [name[len("attpc_"):] for name, *_ in self.calls]

    def of(self, name):
        return [c for c in self.calls if c[0] == "attpc_" + name]

    def stage_descs(self):
        """``configure_descs`` of the trace stages: without the kinematics, the detector and the Spyral geometry."""
        return [(name[len("attpc_trace_"):], desc) for name, desc in self.configure_descs if name.startswith("attpc_trace_")]

    def _call(self, name, args):
        if name == "attpc_last_error":
            return b"recorded"
        args = args[1:]  # (the context handle)
        out = next((a for a in args if isinstance(a, (_abi.CloudOut, _abi.TraceOut))), None)
        nulls = [i for i, a in enumerate(args) if a is None]
        if out is not None:
            nulls += [field for field, ctype in out._fields_ if issubclass(ctype, C._Pointer) and not getattr(out, field)]
        scalars = tuple(a for a in args if isinstance(a, (int, float)))
        self.calls.append((name, scalars, None if out is None else int(out.capacity), tuple(nulls)))
        if name.endswith("configure") or "_configure_" in name:
            desc = args[0]
            self.configure_descs.append((name, None if desc is None else {
                field: getattr(desc, field) for field, _ in desc._fields_ if isinstance(getattr(desc, field), (int, float))}))
        if name in WIDTH:
            return self._run(name, args, out)
        if name == "attpc_trace_rows_last":  # (byref(n_rows), byref(checksum))
            args[0]._obj.value, args[1]._obj.value = self.last_rows
        if name == "attpc_trigger_last":  # (first, count, records)
            for i in range(args[1]):
                args[2][args[0] + i].fired = (self.first + args[0] + i) % 2
        if name == "attpc_spyral_rows":  # (n, points, response, centers, sizes, n_pads, window, mm, length, rows)
            for i in range(args[0] * 8):
                args[9][i] = 100.0 + i
        return _abi.OK

    def _run(self, name, args, out):
        _, first, n = args[:3]
        stats = next((a for a in args if isinstance(a, _abi.RunStats)), None)
        rows = [ROWS[(first + i) % 4] for i in range(n)]
        need = max(self.refuse.pop(name, 0), sum(rows))
        self.first = first
        if name.endswith("trace_rows") or name == "attpc_trace_rows_at":
            self.last_rows = (sum(rows), 33 + first)
        if stats is not None:
            stats.n_events = n
            stats.n_points = sum(POINTS[(first + i) % 4] for i in range(n))
        if isinstance(out, _abi.TraceOut):
            out.n_rows, out.sample_checksum, out.pad_checksum = sum(rows), 11 + first, 22 + first
        if out is None or not out.offsets:
            return _abi.OK
        if need > out.capacity:
            if isinstance(out, _abi.TraceOut):
                out.n_rows = need
            elif stats is not None:
                stats.n_points = need
            self.last_rows = (need, self.last_rows[1])  # (the host-cloud trace rows report their need there)
            return _abi.E_CAPACITY
        width, row = WIDTH[name], 0
        for i in range(n):
            out.offsets[i] = row
            if out.event_points:
                out.event_points[i] = POINTS[(first + i) % 4]
            for _ in range(rows[i]):
                out.labels[row] = first + i
                if width:
                    for c in range(width):
                        out.points[row * width + c] = 10.0 * (first + i) + c
                else:
                    out.pads[row] = first + i
                    for k in range(_abi.NUM_TB):
                        out.samples[row * _abi.NUM_TB + k] = row
                row += 1
        out.offsets[n] = row
        return _abi.OK


class RecordingContext(_abi.Context):
    """A Context over a RecordingLibrary: ``lib``, ``handle`` and ``check`` are the real ones, ``pinned_empty`` hands
    out ordinary arrays and counts them."""

    def __init__(self, lib=None):
        saved, _abi._lib = _abi._lib, lib or RecordingLibrary()
        try:
            super().__init__(0)
        finally:
            _abi._lib = saved
        self.lib.calls.clear()
        self.pinned = 0

    def pinned_empty(self, shape, dtype=np.float64):
        self.pinned += 1
        return np.empty(shape, dtype=dtype)


def forget(ctx, slot):
    """Forget what the shim believes the context holds in ``slot`` (as after a configure through the C ABI)."""
    ctx.forget(slot)


@pytest.fixture(scope="module")
def workload():
    return workloads.o16aa()


@pytest.fixture(scope="module")
def engine(workload):
    pipeline, config, indices = workload
    return Engine(pipeline, config, indices, context=RecordingContext())


@pytest.fixture
def ctx():
    return RecordingContext()


@pytest.fixture
def no_h5py(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)


def _kinematics(workload, n):
    pipeline, _, _ = workload
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    rng = np.random.default_rng(1)
    return rng.normal(size=(n, len(z), 4)), rng.normal(size=(n, 3)), z, a


def test_engine_construction_configures_unconditionally(workload):
    pipeline, config, indices = workload
    ctx = RecordingContext()
    keys = [(2, 4), (6, 12)]
    configure_detector(config, keys, ctx)
    configure_detector(config, keys, ctx)
    assert ctx.lib.names() == ["det_configure"]
    Engine(pipeline, config, indices, context=ctx, chunk_events=64)
    Engine(pipeline, config, indices, context=ctx)
    assert ctx.lib.names() == ["det_configure", "kin_configure", "det_configure", "set_chunk_events", "kin_configure",
                               "det_configure"]
    assert ctx.lib.of("set_chunk_events")[0][1] == (64,)
    # the engine's own attpc_det_configure leaves the shim without a token: the next configure_detector uploads again
    ctx.lib.calls.clear()
    configure_detector(config, keys, ctx)
    configure_detector(config, keys, ctx)
    assert ctx.lib.names() == ["det_configure"]
    forget(ctx, "det")
    configure_detector(config, keys, ctx)
    assert ctx.lib.names() == ["det_configure", "det_configure"]


def test_engine_run(engine):
    lib = engine.ctx.lib
    lib.calls.clear()
    res = engine.run(6, seed=9, first_event=3)
    assert sorted(res) == ["stats"] and res["stats"]["n_points"] == 7 + 0 + 5 + 6 + 7 + 0
    assert lib.calls == [("attpc_sim_run", (9, 3, 6), None, (4, 5, 6, 7))]
    lib.calls.clear()
    res = engine.run(6, seed=9, first_event=3, fetch=True)
    assert lib.calls == [("attpc_sim_run", (9, 3, 6), 6 * 12288, ())]
    assert sorted(res) == ["event_points", "labels", "offsets", "p4", "points", "stats", "status", "vertex"]
    assert res["p4"].shape == (6, 6, 4) and res["vertex"].shape == (6, 3) and res["status"].dtype == np.int32
    np.testing.assert_array_equal(res["offsets"], [0, 2, 2, 2, 3, 5, 5])
    np.testing.assert_array_equal(res["event_points"], [7, 0, 5, 6, 7, 0])
    np.testing.assert_array_equal(res["labels"], [3, 3, 6, 7, 7])
    np.testing.assert_array_equal(res["points"][:, 0], [30, 30, 60, 70, 70])
    assert res["points"].shape == (5, 3) and engine.ctx.pinned == 0
    lib.calls.clear()
    engine.run(2, fetch=True, capacity_per_event=10)
    assert lib.calls == [("attpc_sim_run", (0, 0, 2), 4096, ())]
    with pytest.raises(ValueError):
        engine.run(1, seed=-1)
    engine.hint_next(5, seed=2, first_event=7)
    assert lib.calls[1:] == [("attpc_sim_hint_next", (2, 7, 5), None, ())]


def test_engine_run_retry_and_buffers(engine):
    ctx, lib = engine.ctx, engine.ctx.lib
    lib.calls.clear()
    lib.refuse["attpc_sim_run"] = 70000
    res = engine.run(4, capacity_per_event=10, fetch=True)
    assert [c[2] for c in lib.calls] == [4096, 74096] and lib.names() == ["sim_run", "sim_run"]
    assert res["points"].base.shape == (74096, 3)
    # reuse_buffers: the same arrays on the next call of the same shape, fresh ones after _out_cache = None
    engine._out_cache = None
    a = engine.run(4, fetch=True, reuse_buffers=True)
    b = engine.run(4, fetch=True, reuse_buffers=True)
    assert a["offsets"] is b["offsets"] and a["points"].base is b["points"].base and a["labels"].base is b["labels"].base
    assert a["event_points"] is b["event_points"] and a["p4"] is not b["p4"]
    engine._out_cache = None
    c = engine.run(4, fetch=True, reuse_buffers=True)
    assert c["offsets"] is not a["offsets"] and c["points"].base is not a["points"].base
    d = engine.run(5, fetch=True, reuse_buffers=True)  # another shape: other arrays
    assert d["points"].base is not c["points"].base
    e = engine.run(5, fetch=True)  # without reuse: fresh arrays, and nothing kept
    assert e["points"].base is not d["points"].base and engine._out_cache is None
    before = ctx.pinned
    engine.run(4, fetch=True, pinned=True)
    assert ctx.pinned == before + 2  # rows and labels; offsets and event_points are ordinary arrays
    engine.run_spyral(4, pinned=True, reuse_buffers=True)
    engine.run_spyral(4, pinned=True, reuse_buffers=True)
    assert ctx.pinned == before + 4
    engine._out_cache = None


def test_engine_run_spyral(workload):
    pipeline, config, indices = workload
    engine = Engine(pipeline, config, indices, context=RecordingContext())
    lib = engine.ctx.lib
    lib.calls.clear()
    res = engine.run_spyral(6, seed=9, first_event=3)
    assert lib.calls == [("attpc_spyral_configure", (), None, ()), ("attpc_sim_run_spyral", (9, 3, 6), 6 * 6144, ())]
    assert sorted(res) == ["event_points", "labels", "offsets", "p4", "rows", "stats", "status", "vertex"]
    assert res["rows"].shape == (5, 8)
    np.testing.assert_array_equal(res["rows"][:, 7], [37, 37, 67, 77, 77])
    np.testing.assert_array_equal(res["event_points"], [7, 0, 5, 6, 7, 0])
    lib.calls.clear()
    lib.refuse["attpc_sim_run_spyral"] = 70000
    engine.run_spyral(4, capacity_per_event=10)
    assert lib.calls == [("attpc_sim_run_spyral", (0, 0, 4), 4096, ()), ("attpc_sim_run_spyral", (0, 0, 4), 74096, ())]
    lib.calls.clear()
    engine.configure_spyral()  # the same content: no call
    config.elec_params.adc_threshold = 41
    try:
        engine.configure_spyral()
        engine.configure_spyral(config)
    finally:
        config.elec_params.adc_threshold = 40
    assert lib.names() == ["spyral_configure"]


def test_engine_run_traces(workload):
    pipeline, config, indices = workload
    engine = Engine(pipeline, config, indices, context=RecordingContext())
    ctx, lib = engine.ctx, engine.ctx.lib
    lib.calls.clear()
    res = engine.run_traces(6, seed=9, first_event=3)
    assert lib.calls == [("attpc_trace_configure", (), None, ()), ("attpc_sim_run_traces", (9, 3, 6), 6 * 1024, ())]
    assert sorted(res) == ["event_points", "labels", "offsets", "p4", "pads", "samples", "stats", "status", "trace",
                           "vertex"]
    assert res["trace"] == {"n_rows": 5, "sample_checksum": 14, "pad_checksum": 25}
    assert res["samples"].shape == (5, 512) and res["samples"].dtype == np.int16 and res["pads"].dtype == np.int32
    np.testing.assert_array_equal(res["pads"], [3, 3, 6, 7, 7])
    np.testing.assert_array_equal(res["samples"][:, 5], [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(res["offsets"], [0, 2, 2, 2, 3, 5, 5])
    lib.calls.clear()
    res = engine.run_traces(6, seed=9, first_event=3, fetch=False)
    assert lib.calls == [("attpc_sim_run_traces", (9, 3, 6), 0,
                          (4, 5, 6, "offsets", "pads", "samples", "labels", "event_points"))]
    assert sorted(res) == ["stats", "trace"] and res["trace"] == {"n_rows": 5, "sample_checksum": 14, "pad_checksum": 25}
    lib.calls.clear()
    lib.refuse["attpc_sim_run_traces"] = 70000
    engine.run_traces(4, capacity_per_event=10, pinned=True)
    assert [c[2] for c in lib.calls] == [1024, 70000] and lib.names() == ["sim_run_traces"] * 2
    assert ctx.pinned == 6  # pads, samples and labels of both tries
    # trace, noise and readout each configure once per content
    lib.calls.clear()
    engine.configure_traces()
    engine.configure_traces(noise_sigma=2.0)
    engine.configure_traces(noise_sigma=2.0)
    engine.configure_traces(noise_sigma=2.0, noise_stream=1)
    engine.configure_traces(noise_sigma=2.0, noise_stream=1, threshold=20.0)
    engine.configure_traces(threshold=20.0, readout="full", readout_pads=np.arange(2000))
    assert lib.names() == ["trace_configure_noise", "trace_configure_noise", "trace_configure", "trace_configure_noise",
                           "trace_configure_readout"]
    assert [c[3] for c in lib.calls] == [(), (), (), (0,), ()]  # noise off is a NULL descriptor
    lib.calls.clear()
    engine.run_traces(4, capacity_per_event=10)  # full readout: |S| rows per event
    assert lib.calls == [("attpc_sim_run_traces", (0, 0, 4), 8000, ())]
    engine.configure_traces(threshold=20.0, readout="partial", readout_pads=np.arange(2000))
    engine.run_traces(4, capacity_per_event=10)
    engine.configure_traces(threshold=20.0)
    assert lib.calls[1:] == [("attpc_trace_configure_readout", (), None, ()),
                             ("attpc_sim_run_traces", (0, 0, 4), 1024, ()),
                             ("attpc_trace_configure_readout", (), None, (0,))]
    for slot in ("trace", "trace_noise", "trace_readout"):
        forget(ctx, slot)
    lib.calls.clear()
    engine.configure_traces(threshold=20.0)  # noise and readout off are what a context holds when nothing is known
    assert lib.names() == ["trace_configure"]


def test_simulate_batches(workload, ctx, monkeypatch):
    _, config, indices = workload
    momenta, vertices, z, a = _kinematics(workload, 6)
    lib = ctx.lib
    offsets, points, labels, stats = simulate_batch(momenta, vertices, z, a, config, 9, indices, first_event=3, ctx=ctx)
    assert lib.calls == [("attpc_det_configure", (), None, ()),
                         ("attpc_det_run", (9, 3, 6), 6 * 16384, ("event_points",))]
    np.testing.assert_array_equal(offsets, [0, 2, 2, 2, 3, 5, 5])
    np.testing.assert_array_equal(labels, [3, 3, 6, 7, 7])
    assert points.shape == (5, 3) and stats["n_points"] == 25 and stats["n_events"] == 6
    lib.calls.clear()
    out = simulate_batch_spyral(momenta, vertices, z, a, config, 9, indices, first_event=3, ctx=ctx)
    assert lib.calls == [("attpc_spyral_configure", (), None, ()), ("attpc_det_run_spyral", (9, 3, 6), 6 * 8192, ())]
    assert len(out) == 5 and out[1].shape == (5, 8) and isinstance(out[4], dict)
    np.testing.assert_array_equal(out[3], [7, 0, 5, 6, 7, 0])
    lib.calls.clear()
    out = simulate_batch_traces(momenta, vertices, z, a, config, 9, indices, first_event=3, ctx=ctx)
    assert lib.calls == [("attpc_trace_configure", (), None, ()), ("attpc_det_run_traces", (9, 3, 6), 6 * 1024, ())]
    assert len(out) == 6 and out[2].shape == (5, 512) and out[5]["n_rows"] == 5 and out[5]["n_points"] == 25
    np.testing.assert_array_equal(out[1], [3, 3, 6, 7, 7])
    np.testing.assert_array_equal(out[4], [7, 0, 5, 6, 7, 0])
    # the retry of each mode
    lib.calls.clear()
    for name in ("attpc_det_run", "attpc_det_run_spyral", "attpc_det_run_traces"):
        lib.refuse[name] = 70000
    simulate_batch(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, capacity_per_event=10)
    simulate_batch_spyral(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, capacity_per_event=10)
    simulate_batch_traces(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, capacity_per_event=10)
    assert [(c[0], c[2]) for c in lib.calls] == [
        ("attpc_det_run", 1024), ("attpc_det_run", 71024), ("attpc_det_run_spyral", 1024),
        ("attpc_det_run_spyral", 71024), ("attpc_det_run_traces", 1024), ("attpc_det_run_traces", 70000)]
    # a changed detector parameter, response or readout configures again; the full readout sizes the first try
    lib.calls.clear()
    config.det_params.diffusion += 0.01
    try:
        simulate_batch(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx)
    finally:
        config.det_params.diffusion -= 0.01
    simulate_batch_spyral(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, response=np.ones(512))
    simulate_batch_traces(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, readout="full",
                          readout_pads=np.arange(3000), noise_sigma=1.0)
    assert lib.names() == ["det_configure", "det_run", "det_configure", "spyral_configure", "det_run_spyral",
                           "trace_configure_noise", "trace_configure_readout", "det_run_traces"]
    assert lib.calls[-1][2] == 6000
    with pytest.raises(ValueError):  # validated before the first library call
        lib.calls.clear()
        simulate_batch_traces(momenta, vertices, z, a, config, 9, indices, ctx=ctx, readout="full", readout_pads=[1, 1])
    assert lib.calls == []
    # clouds_to_traces: capacity from the cloud's rows, or |S| per event in full readout
    lib.calls.clear()
    cloud = np.zeros((40, 3))
    res = clouds_to_traces(np.array([0, 10, 40]), cloud, np.zeros(40, dtype=np.int64), ctx, seed=4, first_event=2)
    assert lib.calls == [("attpc_traces_at", (4, 2, 2), 6000, ())] and len(res) == 5 and res[4]["n_rows"] == 3
    configure_traces(config, ctx)
    lib.calls.clear()
    lib.refuse["attpc_traces_at"] = 70000
    clouds_to_traces(np.array([0, 10, 40]), cloud, np.zeros(40, dtype=np.int64), ctx)
    assert [(c[0], c[1], c[2]) for c in lib.calls] == [("attpc_traces_at", (0, 0, 2), 40),
                                                        ("attpc_traces_at", (0, 0, 2), 70000)]
    # simulate(): one event through the default context
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    lib.calls.clear()
    points, labels = simulate(momenta[0], vertices[0], z, a, config, np.random.default_rng(3), indices)
    seed = int(np.random.default_rng(3).integers(0, 1 << 63))
    assert lib.calls == [("attpc_det_run", (seed, 0, 1), 16384, ("event_points",))] and points.shape == (0, 3)


def test_configure_functions(workload, ctx):
    _, config, _ = workload
    lib = ctx.lib
    configure_spyral(config, ctx)
    configure_spyral(config, ctx)
    configure_spyral(config, ctx, response=np.ones(512))
    configure_traces(config, ctx)
    configure_traces(config, ctx)
    configure_traces(config, ctx, offset=3)
    configure_traces(config, ctx, offset=3, pedestals=100)
    configure_traces(config, ctx, offset=3, pedestals=100, readout="partial")
    configure_traces(config, ctx, offset=3, pedestals=100, readout="partial")
    assert lib.names() == ["spyral_configure", "spyral_configure", "trace_configure", "trace_configure",
                           "trace_configure_noise", "trace_configure_readout"]
    forget(ctx, "spyral")
    forget(ctx, "trace_readout")
    lib.calls.clear()
    configure_spyral(config, ctx, response=np.ones(512))
    configure_traces(config, ctx, offset=3, pedestals=100, readout="partial")
    assert lib.names() == ["spyral_configure", "trace_configure_readout"]
    rows = convert_to_spyral(np.zeros((2, 3)), 560, 10, 1.0, np.ones(512), config.pad_centers, config.pad_sizes, ctx)
    assert lib.calls[-1] == ("attpc_spyral_rows", (2, len(config.pad_sizes), 560, 10, 1.0), None, ())
    assert rows.shape == (2, 8) and rows[1, 7] == 115.0


class PlainWriter:
    def __init__(self, directory):
        self.directory, self.events, self.closed = directory, [], 0

    def write(self, data, labels, config, event_number):
        self.events.append((event_number, data.shape, list(labels)))

    def get_directory_name(self):
        return self.directory

    def close(self):
        self.closed += 1


def _files(directory):
    """{file name: {dataset or attribute name: array}} of the .npz run files of a directory."""
    return {p.name: dict(np.load(p)) for p in sorted(directory.glob("run_*.npz"))}


def _events(content, prefix):
    return [int(k[len(prefix):]) for k in content if k.startswith(prefix) and "@" not in k]


def _kinematics_file(workload, tmp_path, n):
    momenta, vertices, z, a = _kinematics(workload, n)
    writer = KinematicsFileWriter(tmp_path / "kin.npz", n, z, a, chunk_size=4)
    writer.write_batch(0, vertices, momenta)
    writer.close()
    return tmp_path / "kin.npz"


def test_run_simulation(workload, ctx, tmp_path, monkeypatch, no_h5py, capsys):
    _, config, indices = workload
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    lib = ctx.lib
    path = _kinematics_file(workload, tmp_path, 10)
    run_seed = int(np.random.default_rng(5).integers(0, 1 << 63))
    batches = [(run_seed, 0, 4), (run_seed, 4, 4), (run_seed, 8, 2)]

    plain = PlainWriter(tmp_path)
    run_simulation(config, path, plain, indices, batch_size=4, seed=5)
    assert lib.names() == ["det_configure", "det_run", "det_run", "det_run"]
    assert [c[1] for c in lib.of("det_run")] == batches
    assert [c[2] for c in lib.of("det_run")] == [4 * 16384, 4 * 16384, 2 * 16384]
    # plain write: the events whose cloud has rows
    assert plain.events == [(2, (1, 3), [2]), (3, (2, 3), [3, 3]), (6, (1, 3), [6]), (7, (2, 3), [7, 7])]
    assert plain.closed == 1

    lib.calls.clear()
    (tmp_path / "spyral").mkdir()
    run_simulation(config, path, SpyralWriter(tmp_path / "spyral", config, max_events_per_file=3), indices,
                   batch_size=4, seed=5)
    assert lib.names() == ["spyral_configure", "det_run_spyral", "det_run_spyral", "det_run_spyral"]
    assert [c[1] for c in lib.of("det_run_spyral")] == batches
    assert [c[2] for c in lib.of("det_run_spyral")] == [4 * 8192, 4 * 8192, 2 * 8192]
    files = _files(tmp_path / "spyral")
    # presorted rows: every event with a cloud before the threshold, also the ones that keep no row
    assert [_events(f, "cloud/cloud_") for f in files.values()] == [[1, 2, 3], [5, 6, 7], [9]]
    assert [(int(f["cloud@min_event"]), int(f["cloud@max_event"])) for f in files.values()] == [(0, 3), (5, 7), (9, 9)]
    assert files["run_0000.npz"]["cloud/cloud_1"].shape == (0, 8)
    np.testing.assert_array_equal(files["run_0001.npz"]["cloud/cloud_7"][:, 0], [70, 70])
    np.testing.assert_array_equal(files["run_0001.npz"]["cloud/labels_7"], [7, 7])
    assert int(files["run_0001.npz"]["cloud/cloud_7@orig_run"]) == 1

    lib.calls.clear()
    (tmp_path / "trace").mkdir()
    run_simulation(config, path, TraceWriter(tmp_path / "trace", config, max_events_per_file=3, noise_sigma=1.5,
                                             readout="partial", threshold=25.0), indices, batch_size=4, seed=5)
    assert lib.names() == ["trace_configure", "trace_configure_noise", "trace_configure_readout", "det_run_traces",
                           "det_run_traces", "det_run_traces"]
    assert [c[1] for c in lib.of("det_run_traces")] == batches
    assert [c[2] for c in lib.of("det_run_traces")] == [4 * 1024, 4 * 1024, 2 * 1024]
    files = _files(tmp_path / "trace")
    assert [_events(f, "trace/trace_") for f in files.values()] == [[1, 2, 3], [5, 6, 7], [9]]
    assert [(int(f["trace@min_event"]), int(f["trace@max_event"])) for f in files.values()] == [(0, 3), (5, 7), (9, 9)]
    assert all(str(f["trace@readout"]) == "partial" and "trace/noise_cdf" in f for f in files.values())
    assert files["run_0002.npz"]["trace/trace_9"].shape == (0, 512)
    np.testing.assert_array_equal(files["run_0001.npz"]["trace/pads_7"], [7, 7])
    assert "Done." in capsys.readouterr().out


def test_writers_write_one_event(workload, ctx, tmp_path, monkeypatch, no_h5py):
    _, config, _ = workload
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    lib = ctx.lib
    spyral = SpyralWriter(tmp_path, config, max_events_per_file=1, first_run_number=4)
    assert spyral.get_directory_name() == tmp_path
    spyral.write(np.zeros((3, 3)), np.array([5, 6, 7]), config, 12)
    spyral.write(np.zeros((2, 3)), np.array([8, 9]), config, 15)
    spyral.close()
    assert lib.names() == ["spyral_rows", "spyral_rows"]
    files = _files(tmp_path)
    assert list(files) == ["run_0004.npz", "run_0005.npz"]
    assert _events(files["run_0004.npz"], "cloud/cloud_") == [12] and _events(files["run_0005.npz"], "cloud/cloud_") == [15]
    assert (int(files["run_0005.npz"]["cloud@min_event"]), int(files["run_0005.npz"]["cloud@max_event"])) == (15, 15)
    np.testing.assert_array_equal(files["run_0004.npz"]["cloud/labels_12"], [5, 6, 7])
    lib.calls.clear()
    (tmp_path / "t").mkdir()
    trace = TraceWriter(tmp_path / "t", config, max_events_per_file=2, noise_seed=77)
    for event in (2, 3, 6):
        trace.write(np.zeros((4, 3)), np.zeros(4, dtype=np.int64), config, event)
    trace.close()
    assert lib.names() == ["trace_configure", "traces_at", "traces_at", "traces_at"]
    assert [c[1:3] for c in lib.of("traces_at")] == [((77, 2, 1), 16), ((77, 3, 1), 16), ((77, 6, 1), 16)]
    files = _files(tmp_path / "t")
    assert [_events(f, "trace/trace_") for f in files.values()] == [[2, 3], [6]]
    assert files["run_0000.npz"]["trace/trace_3"].shape == (2, 512) and "trace@readout" not in files["run_0000.npz"]


def test_run_fused(workload, ctx, tmp_path, no_h5py):
    pipeline, config, indices = workload
    lib = ctx.lib
    (tmp_path / "spyral").mkdir()
    (tmp_path / "trace").mkdir()
    run_fused(pipeline, config, SpyralWriter(tmp_path / "spyral", config, max_events_per_file=3), 10, indices, seed=8,
              batch_size=4, context=ctx)
    assert lib.names() == ["kin_configure", "det_configure", "spyral_configure"] + ["sim_run_spyral"] * 3
    assert [c[1:] for c in lib.of("sim_run_spyral")] == [((8, 0, 4), 4 * 6144, ()), ((8, 4, 4), 4 * 6144, ()),
                                                         ((8, 8, 2), 2 * 6144, ())]
    files = _files(tmp_path / "spyral")
    assert [_events(f, "cloud/cloud_") for f in files.values()] == [[1, 2, 3], [5, 6, 7], [9]]
    assert [(int(f["cloud@min_event"]), int(f["cloud@max_event"])) for f in files.values()] == [(0, 3), (5, 7), (9, 9)]
    np.testing.assert_array_equal(files["run_0001.npz"]["cloud/cloud_6"][0], np.arange(60.0, 68.0))

    def trace_writer(name, **kw):
        (tmp_path / name).mkdir(exist_ok=True)
        return TraceWriter(tmp_path / name, config, max_events_per_file=3, **kw)

    lib.calls.clear()
    run_fused(pipeline, config, trace_writer("trace"), 10, indices, batch_size=4, context=ctx)
    assert lib.names() == ["kin_configure", "det_configure", "trace_configure"] + ["sim_run_traces"] * 3
    assert [c[1:] for c in lib.of("sim_run_traces")] == [((pipeline.seed, 0, 4), 4096, ()), ((pipeline.seed, 4, 4), 4096, ()),
                                                         ((pipeline.seed, 8, 2), 2048, ())]
    files = _files(tmp_path / "trace")
    assert [_events(f, "trace/trace_") for f in files.values()] == [[1, 2, 3], [5, 6, 7], [9]]
    assert [(int(f["trace@min_event"]), int(f["trace@max_event"])) for f in files.values()] == [(0, 3), (5, 7), (9, 9)]
    np.testing.assert_array_equal(files["run_0000.npz"]["trace/labels_3"], [3, 3])
    # the same trace content is already on the context: no attpc_trace_configure; other noise: only that
    lib.calls.clear()
    run_fused(pipeline, config, trace_writer("trace2"), 10, indices, batch_size=4, context=ctx)
    run_fused(pipeline, config, trace_writer("trace3", noise_sigma=1.0), 2, indices, context=ctx)
    assert lib.names() == ["kin_configure", "det_configure"] + ["sim_run_traces"] * 3 + [
        "kin_configure", "det_configure", "trace_configure_noise", "sim_run_traces"]


# ---------------------------------------------------------------- the trace stages through both run entry points ----
TRIGGER = TriggerSettings(25, window=50, group_multiplicity=4)
GAIN = GainSettings(theta=1.0, stream=4)
GAIN_DESC = {"rel_variance": 0.5, "stream": 4, "reserved": 0}
PEAK_DESC = {"separation": 50.0, "prominence": 30.0, "min_width": 1.0, "max_width": 50.0, "rel_height": 0.95,
             "threshold": 40.0}
WITH_CLOUD = [1, 2, 3, 5, 6, 7, 9]  # POINTS[g % 4] != 0
FIRED_WITH_CLOUD = [1, 3, 5, 7, 9]  # ... and the stand-in's trigger fired: g odd
# the order of the last two configure calls of a trace-row run, per entry point (TraceChain.configure: one order)
ROWS_TAIL = {"fused": ("trigger", "gain"), "simulation": ("trigger", "gain")}


def _trigger_desc(gate):
    return {"threshold": 25, "window": 50, "group_multiplicity": 4, "min_groups": 1, "gate": gate, "reserved": 0}


class Runner:
    """10 events in batches of 4 through ``run_fused`` or ``run_simulation`` on one recording context."""

    batches = [(0, 4), (4, 4), (8, 2)]

    def __init__(self, entry, workload, ctx, tmp_path, monkeypatch):
        self.entry, self.workload, self.ctx, self.tmp_path, self.n_dirs = entry, workload, ctx, tmp_path, 0
        self.prefix = "sim_run" if entry == "fused" else "det_run"
        if entry == "simulation":
            monkeypatch.setattr(_abi, "_default_ctx", ctx)
            self.path = _kinematics_file(workload, tmp_path, 10)
            self.seed = int(np.random.default_rng(5).integers(0, 1 << 63))
        else:
            self.seed = 8

    def directory(self):
        self.n_dirs += 1
        path = self.tmp_path / f"out{self.n_dirs}"
        path.mkdir()
        return path

    def run(self, writer, **kw):
        """-> the names of the calls the run made, without the engine's own unconditional ones."""
        pipeline, config, indices = self.workload
        self.ctx.lib.calls.clear()
        self.ctx.lib.configure_descs.clear()
        if self.entry == "fused":
            run_fused(pipeline, config, writer, 10, indices, seed=self.seed, batch_size=4, context=self.ctx, **kw)
            names = self.ctx.lib.names()
            assert names[:2] == ["kin_configure", "det_configure"]
            return names[2:]
        run_simulation(config, self.path, writer, indices, batch_size=4, seed=5, **kw)
        return self.ctx.lib.names()

    def run_calls(self, mode):
        return [c[1:] for c in self.ctx.lib.of(f"{self.prefix}_{mode}")]

    def expected_runs(self, capacity_per_event):
        return [((self.seed, first, n), n * capacity_per_event, ()) for first, n in self.batches]


@pytest.fixture(params=["fused", "simulation"])
def runner(request, workload, ctx, tmp_path, monkeypatch, no_h5py, capsys):
    return Runner(request.param, workload, ctx, tmp_path, monkeypatch)


def _written(directory, prefix):
    return sorted(e for f in _files(directory).values() for e in _events(f, prefix))


@pytest.mark.parametrize("triggered", [True, False])
def test_trace_writer_with_every_stage(runner, triggered):
    _, config, _ = runner.workload
    lib = runner.ctx.lib
    kw = {"trigger": TRIGGER} if triggered else {}

    def writer(**settings):
        return TraceWriter(runner.directory(), config, noise_sigma=1.5, readout="partial", **settings)

    first = writer(gain=GAIN)
    names = runner.run(first, **kw)
    det = [] if runner.entry == "fused" else ["det_configure"]
    configure = ["trace_configure", "trace_configure_noise", "trace_configure_readout"] + (
        ["trace_configure_trigger"] if triggered else []) + ["trace_configure_gain"]
    per_batch = [f"{runner.prefix}_traces"] + (["trigger_last"] if triggered else [])
    assert names == det + configure + per_batch * 3
    assert runner.run_calls("traces") == runner.expected_runs(1024)
    if triggered:
        assert [c[1] for c in lib.of("trigger_last")] == [(0, 4), (0, 4), (0, 2)]
    assert lib.stage_descs() == [
        ("configure", {"adc_threshold": float(config.elec_params.adc_threshold), "offset": 0, "reserved": 0}),
        ("configure_noise", {"n_levels": 25, "min_level": -12, "stream": 0, "reserved": 0}),
        ("configure_readout", {"mode": _abi.READOUT_PARTIAL, "reserved": 0})] + (
        [("configure_trigger", _trigger_desc(0))] if triggered else []) + [("configure_gain", GAIN_DESC)]
    assert _written(first.get_directory_name(), "trace/trace_") == (FIRED_WITH_CLOUD if triggered else WITH_CLOUD)
    # the same settings on the same context: nothing is configured again
    assert runner.run(writer(gain=GAIN), **kw) == per_batch * 3 and lib.stage_descs() == []
    # no trigger and no gain after a run with them: both are turned off
    off = runner.run(writer())
    assert off == (["trace_configure_trigger"] if triggered else []) + ["trace_configure_gain"] + [f"{runner.prefix}_traces"] * 3
    assert all(desc is None for _, desc in lib.stage_descs()) and len(lib.stage_descs()) == 1 + triggered


@pytest.mark.parametrize("triggered", [True, False])
def test_spyral_writer_with_peaks_and_every_stage(runner, triggered):
    _, config, _ = runner.workload
    lib = runner.ctx.lib
    kw = {"trigger": TRIGGER} if triggered else {}
    tail = [stage for stage in ROWS_TAIL[runner.entry] if triggered or stage != "trigger"]

    def writer(**settings):
        return SpyralWriter(runner.directory(), config, peaks=PeakSettings(prominence=30.0), baseline=BaselineSettings(25.0),
                            pedestals=100, **settings)

    first = writer(gain=GAIN)
    names = runner.run(first, **kw)
    det = [] if runner.entry == "fused" else ["det_configure"]
    configure = ["trace_configure", "trace_configure_noise", "spyral_configure", "trace_configure_peaks",
                 "trace_configure_baseline"] + [f"trace_configure_{stage}" for stage in tail]
    last = ["trigger_last"] if triggered else []
    # (the engine asks for the rows' sums before the records, the batch entry point after them)
    per_batch = [f"{runner.prefix}_trace_rows"] + (["trace_rows_last"] + last if runner.entry == "fused" else
                                                    last + ["trace_rows_last"])
    assert names == det + configure + per_batch * 3
    assert runner.run_calls("trace_rows") == runner.expected_runs(2048)
    stage_desc = {"trigger": ("configure_trigger", _trigger_desc(1)), "gain": ("configure_gain", GAIN_DESC)}
    assert lib.stage_descs() == [
        ("configure", {"adc_threshold": float(config.elec_params.adc_threshold), "offset": 0, "reserved": 0}),
        ("configure_noise", {"n_levels": 0, "min_level": 0, "stream": 0, "reserved": 0}),
        ("configure_peaks", PEAK_DESC), ("configure_baseline", {"window_scale": 25.0})] + [stage_desc[s] for s in tail]
    assert _written(first.get_directory_name(), "cloud/cloud_") == (FIRED_WITH_CLOUD if triggered else WITH_CLOUD)
    assert runner.run(writer(gain=GAIN), **kw) == per_batch * 3 and lib.stage_descs() == []
    off = runner.run(writer())
    assert off[:len(tail)] == [f"trace_configure_{stage}" for stage in tail] and "trigger_last" not in off
    assert lib.stage_descs() == [(f"configure_{stage}", None) for stage in tail]


def test_a_run_uses_its_own_config_not_the_writers(runner):
    """A writer built with another Config than the run's: the detector, the geometry of the rows and every default a
    SpyralWriter(peaks=...) left unset are the run's; a TraceWriter's response and threshold are its own, resolved when
    it was built."""
    import copy
    import dataclasses

    _, config, _ = runner.workload
    other = copy.copy(config)
    other.elec_params = dataclasses.replace(config.elec_params, adc_threshold=config.elec_params.adc_threshold + 7)
    other.det_params = dataclasses.replace(config.det_params, length=2.0 * config.det_params.length)
    threshold, length = float(config.elec_params.adc_threshold), float(config.det_params.length)

    def configured(writer):
        runner.run(writer, trigger=TRIGGER)
        descs = runner.ctx.lib.configure_descs
        return {name[len("attpc_"):]: desc for name, desc in descs}, [name for name, _ in descs].count("attpc_det_configure")

    descs, n_det = configured(TraceWriter(runner.directory(), other, gain=GAIN))
    assert n_det == 1 and descs["det_configure"]["length"] == length
    assert descs["trace_configure"] == {"adc_threshold": threshold + 7, "offset": 0, "reserved": 0}
    assert descs["trace_configure_trigger"] == _trigger_desc(0) and descs["trace_configure_gain"] == GAIN_DESC
    descs, n_det = configured(SpyralWriter(runner.directory(), other, peaks=PeakSettings(prominence=30.0), gain=GAIN))
    assert n_det == (1 if runner.entry == "fused" else 0) and descs.get("det_configure", {"length": length})["length"] == length
    assert descs["trace_configure"] == {"adc_threshold": threshold, "offset": 0, "reserved": 0}
    assert (descs["spyral_configure"]["length"], descs["spyral_configure"]["adc_threshold"]) == (length, threshold)
    assert descs["trace_configure_peaks"] == PEAK_DESC and descs["trace_configure_trigger"] == _trigger_desc(1)
    # a threshold the writer was given stays the writer's
    descs, _ = configured(SpyralWriter(runner.directory(), other, peaks=PeakSettings(), threshold=12.0))
    assert descs["trace_configure"]["adc_threshold"] == 12.0 and "spyral_configure" not in descs  # (the same geometry)


def test_spyral_writer_write_uses_the_config_of_the_call(workload, ctx, tmp_path, monkeypatch, no_h5py):
    import copy
    import dataclasses

    _, config, _ = workload
    other = copy.copy(config)
    other.elec_params = dataclasses.replace(config.elec_params, adc_threshold=config.elec_params.adc_threshold + 7)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    writer = SpyralWriter(tmp_path, other, peaks=PeakSettings())
    writer.write(np.array([[5.0, 100.0, 900.0]]), np.array([1]), config, 2)
    descs = {name[len("attpc_"):]: desc for name, desc in ctx.lib.configure_descs}
    threshold = float(config.elec_params.adc_threshold)
    assert descs["trace_configure"]["adc_threshold"] == threshold and descs["spyral_configure"]["adc_threshold"] == threshold


def test_writer_kinds_are_checked_before_any_run(runner):
    from attpc_engine_amd.detector.selection import Selection

    _, config, _ = runner.workload
    cases = [
        (TraceWriter(runner.directory(), config), {"selection": Selection(n_kept=(1, None))},
         "a selection delivers Spyral rows or clouds: trace writers are not supported"),
        (SpyralWriter(runner.directory(), config, peaks=PeakSettings()), {"selection": Selection(n_kept=(1, None))},
         "a selection delivers Spyral rows or clouds: trace writers are not supported"),
        (SpyralWriter(runner.directory(), config), {"trigger": TRIGGER},
         "a trigger delivers traces or trace rows: writers of Spyral rows or clouds are not supported"),
        (SpyralWriter(runner.directory(), config), {"gain": GAIN},
         "a gain acts on traces or trace rows: writers of Spyral rows or clouds are not supported"),
        (PlainWriter(runner.directory()), {"gain": GAIN},
         "a gain acts on traces or trace rows: writers of Spyral rows or clouds are not supported"),
    ]
    for writer, kw, message in cases:
        with pytest.raises(ValueError) as error:
            runner.run(writer, **kw)
        assert str(error.value) == message
        # (the engine of run_fused is built first: its two unconditional calls, and nothing after them)
        assert [n for n in runner.ctx.lib.names() if n not in ("kin_configure", "det_configure")] == []
    if runner.entry == "fused":
        with pytest.raises(AttributeError, match="run_fused needs a writer that offers write_rows or write_traces"):
            runner.run(PlainWriter(runner.directory()))


def test_simulate_batch_trace_rows(workload, ctx):
    _, config, indices = workload
    momenta, vertices, z, a = _kinematics(workload, 6)
    lib = ctx.lib
    settings = dict(peaks=PeakSettings(prominence=30.0), baseline=BaselineSettings(25.0), gain=GAIN, pedestals=100,
                    readout="partial")
    out = simulate_batch_trace_rows(momenta, vertices, z, a, config, 9, indices, first_event=3, ctx=ctx, trigger=TRIGGER,
                                    **settings)
    tail = [f"trace_configure_{stage}" for stage in ROWS_TAIL["simulation"]]
    assert lib.names() == ["det_configure", "trace_configure", "trace_configure_noise", "trace_configure_readout",
                           "spyral_configure", "trace_configure_peaks", "trace_configure_baseline"] + tail + [
                               "det_run_trace_rows", "trigger_last", "trace_rows_last"]
    assert lib.of("det_run_trace_rows") == [("attpc_det_run_trace_rows", (9, 3, 6), 6 * 2048, ())]
    assert dict(lib.stage_descs())["configure_trigger"] == _trigger_desc(0)  # (the caller's own gate)
    assert dict(lib.stage_descs())["configure_gain"] == GAIN_DESC and dict(lib.stage_descs())["configure_peaks"] == PEAK_DESC
    offsets, rows, labels, event_points, stats = out
    np.testing.assert_array_equal(offsets, [0, 2, 2, 2, 3, 5, 5])
    np.testing.assert_array_equal(event_points, [7, 0, 5, 6, 7, 0])
    np.testing.assert_array_equal(rows[:, 7], [37, 37, 67, 77, 77])
    np.testing.assert_array_equal(labels, [3, 3, 6, 7, 7])
    assert stats["n_rows"] == 5 and stats["row_checksum"] == 36 and stats["n_points"] == 25
    assert stats["trigger"]["fired"].tolist() == [1, 0, 1, 0, 1, 0] and list(stats)[-3:] == ["n_rows", "row_checksum", "trigger"]
    # the same settings: no configure call; the retry; without trigger and gain: both turned off, no records
    lib.calls.clear()
    lib.refuse["attpc_det_run_trace_rows"] = 70000
    simulate_batch_trace_rows(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, trigger=TRIGGER,
                              capacity_per_event=10, **settings)
    assert [(c[0], c[2]) for c in lib.calls] == [
        ("attpc_det_run_trace_rows", 1024), ("attpc_det_run_trace_rows", 71024), ("attpc_trigger_last", None),
        ("attpc_trace_rows_last", None)]
    lib.calls.clear()
    lib.configure_descs.clear()
    del settings["gain"]
    out = simulate_batch_trace_rows(momenta[:2], vertices[:2], z, a, config, 9, indices, ctx=ctx, **settings)
    assert lib.names() == tail + ["det_run_trace_rows", "trace_rows_last"] and "trigger" not in out[4]
    assert sorted(lib.stage_descs()) == [("configure_gain", None), ("configure_trigger", None)]
    with pytest.raises(TypeError):  # validated before the first library call
        lib.calls.clear()
        simulate_batch_trace_rows(momenta, vertices, z, a, config, 9, indices, ctx=ctx, noise=1.0)
    with pytest.raises(ValueError):
        simulate_batch_trace_rows(momenta, vertices, z, a, config, 9, indices, ctx=ctx, readout_pads=[1, 1])
    assert lib.calls == []


def test_clouds_to_trace_rows_and_gain(workload, ctx):
    _, config, _ = workload
    lib = ctx.lib
    cloud, labels = np.zeros((40, 3)), np.zeros(40, dtype=np.int64)
    configure_trace_rows(config, ctx, PeakSettings(prominence=30.0), BaselineSettings(25.0), GAIN, pedestals=100)
    assert lib.names() == ["trace_configure", "trace_configure_noise", "spyral_configure", "trace_configure_peaks",
                           "trace_configure_baseline", "trace_configure_gain"]
    assert lib.stage_descs()[2:] == [("configure_peaks", PEAK_DESC), ("configure_baseline", {"window_scale": 25.0}),
                                     ("configure_gain", GAIN_DESC)]
    lib.calls.clear()
    res = clouds_to_trace_rows(np.array([0, 10, 40]), cloud, labels, ctx, seed=4, first_event=2)
    assert lib.calls == [("attpc_trace_rows_at", (4, 2, 2), 40, ()), ("attpc_trace_rows_last", (), None, ()),
                         ("attpc_trace_rows_last", (), None, ())]
    assert len(res) == 4 and res[1].shape == (3, 8) and res[3] == {"n_rows": 3, "row_checksum": 35}
    np.testing.assert_array_equal(res[0], [0, 1, 3])
    # with a trigger on the context its records come too; the retry asks for the rows the call left
    configure_trigger(ctx, TRIGGER.gated())
    lib.calls.clear()
    lib.refuse["attpc_trace_rows_at"] = 70000
    res = clouds_to_trace_rows(np.array([0, 10, 40]), cloud, labels, ctx, seed=4, first_event=2)
    assert [(c[0], c[2]) for c in lib.calls] == [
        ("attpc_trace_rows_at", 40), ("attpc_trace_rows_last", None), ("attpc_trace_rows_at", 70016),
        ("attpc_trace_rows_last", None), ("attpc_trigger_last", None), ("attpc_trace_rows_last", None)]
    assert res[3]["trigger"]["fired"].tolist() == [0, 1] and list(res[3]) == ["n_rows", "row_checksum", "trigger"]
    # full readout: four rows per pad of the readout set and event on the first try
    configure_trace_rows(config, ctx, readout="full", readout_pads=np.arange(100))
    lib.calls.clear()
    clouds_to_trace_rows(np.array([0, 10, 40]), cloud, labels, ctx)
    assert lib.calls[0] == ("attpc_trace_rows_at", (0, 0, 2), 800, ())
    for bad in (lambda: clouds_to_trace_rows(np.array([0, 41]), cloud, labels, ctx),
                lambda: clouds_to_trace_rows(np.array([0, 40]), cloud, labels[:-1], ctx),
                lambda: clouds_to_trace_rows(np.array([0, 40]), cloud, labels, ctx, seed=-1),
                lambda: clouds_to_gain(np.array([0, 41]), cloud, ctx),
                lambda: clouds_to_gain(np.array([0, 40]), cloud, ctx, first_event=-1)):
        lib.calls.clear()
        with pytest.raises(ValueError):
            bad()
        assert lib.calls == []
    # clouds_to_gain configures its gain first (None: off) and has no capacity
    lib.configure_descs.clear()
    gained = clouds_to_gain(np.array([0, 10, 40]), cloud, ctx, seed=4, first_event=2, gain=GAIN)
    assert lib.calls == [("attpc_trace_configure_gain", (), None, ()), ("attpc_gain_rows", (4, 2, 2), None, ())]
    assert gained.shape == (40,) and lib.stage_descs() == [("configure_gain", GAIN_DESC)]
    clouds_to_gain(np.array([0, 10, 40]), cloud, ctx)
    assert lib.names()[2:] == ["trace_configure_gain", "gain_rows"] and lib.calls[2][3] == (0,)
