"""The micromegas gain of the pad traces without a device: the quality of the contract's approximation on a
deterministic grid of uniforms, its edge cases computed by hand, the quantile table, the validation of ``GainSettings``,
the header's declarations against their ctypes mirrors, and the Python layer through the recording stand-in library of
tests/test_run_layer_cpu.py."""
import ctypes as C
import math
import re
import subprocess
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.traces import (GainSettings, clouds_to_gain, configure_gain, configure_trace_rows,
                                              normal_quantile_table, polya_rel_variance, validate_trace_kwargs)
from tests import gain_reference as ref
from tests.test_run_layer_cpu import POINTS, RecordingContext, RecordingLibrary
from tests.trace_noise_reference import philox4x32_10

ROOT = Path(__file__).resolve().parents[1]
Z = normal_quantile_table()
GRID = np.arange(1 << 20, dtype=np.uint64) << np.uint64(12)  # u = k 2^12: every (interval, position / 256) once
CASES = [(f, q) for f in (1.0, 0.5, 0.25) for q in (1, 2, 3, 5, 10, 30, 100, 1000)]


# ---------------------------------------------------------------- the quantile table ----
def test_quantile_table_is_the_scaled_normal_inverse_cdf():
    import statistics

    assert Z.shape == (_abi.GAIN_KNOTS,) == (ref.KNOTS,) and Z.dtype == np.float64 and not Z.flags.writeable
    assert np.all(np.isfinite(Z)) and np.all(np.diff(Z) > 0) and np.array_equal(Z, -Z[::-1]) and Z[2048] == 0.0
    inv = statistics.NormalDist().inv_cdf
    raw = np.array([inv((i + 0.5) / 4097) for i in range(4097)])
    a, b = raw[:-1], raw[1:]
    variance = math.fsum((a * a + a * b + b * b) / 3.0) / 4096  # of the piecewise-linear law of the unscaled table
    assert abs(variance - 0.99663) < 1e-5
    np.testing.assert_allclose(Z, raw / math.sqrt(variance), rtol=1e-14, atol=1e-16)
    # the law the table defines, on the grid (whose positions inside an interval are k / 256): mean 0, variance 1
    i = (GRID >> np.uint64(20)).astype(np.int64)
    w = (GRID & np.uint64(0xFFFFF)).astype(np.float64) * 2.0 ** -20
    law = Z[i] + (Z[i + 1] - Z[i]) * w
    assert abs(law.mean()) < 1e-5 and abs(law.var() - 1.0) < 1e-4


# ---------------------------------------------------------------- quality of the approximation ----
@pytest.fixture(scope="module")
def moments():
    """(mean / q, variance / (q f), P(x = 0)) of q' over the grid, per case."""
    out = {}
    for f, q in CASES:
        qp = ref.Gain(f, Z).fluctuate(GRID, np.full(GRID.shape, float(q)))
        out[f, q] = (qp.mean() / q, qp.var() / (q * f), float(np.mean(qp == 0.0)))
    return out


def test_mean_and_variance_of_the_gained_charge(moments):
    for (f, q), (mean, var, _) in moments.items():
        print(f"f = {f}, q = {q}: mean ratio {mean:.5f}, variance ratio {var:.5f}")
    for (f, q), (mean, var, _) in moments.items():
        assert 0.997 <= mean <= 1.001, (f, q, mean)
        assert 0.98 <= var <= 1.01, (f, q, var)


def test_the_clamp_is_reached_at_one_electron_of_unit_variance_only(moments):
    for (f, q), (_, _, clamped) in moments.items():
        if (f, q) == (1.0, 1):
            assert 1e-3 < clamped < 1e-2, clamped  # x = 0 needs z < -8 / 3: P = 3.8e-3 for a normal z
        else:
            assert clamped == 0.0, (f, q, clamped)


# ---------------------------------------------------------------- edge cases, by hand ----
def _by_hand(u, q, f, g=1.0):
    """The contract in plain Python floats (IEEE f64, one rounding per operation)."""
    if q == 0.0:
        return 0.0
    if f == 0.0:
        return q * g
    i, w = u >> 20, float(u & 0xFFFFF) * 2.0 ** -20
    z0, z1 = float(Z[i]), float(Z[i + 1])
    z = z0 + (z1 - z0) * w
    r = (f / 9.0) / q
    s = math.sqrt(r)
    x = max((1.0 - r) + z * s, 0.0)
    return ((q * x) * x) * x * g


def test_edge_cases():
    gain = ref.Gain(1.0, Z)
    assert gain.fluctuate(np.array([12345], dtype=np.uint64), np.array([0.0]))[0] == 0.0             # q = 0
    q = np.array([0.0, 1.0, 7.0, 1e7, 123.456])
    pad_gain = np.linspace(0.5, 1.5, ref.NUM_PADS)
    pads = np.array([0, 1, 5000, 10239, 77])
    assert np.array_equal(ref.Gain(0.0, None, pad_gain).rows(3, 4, pads, pads % 512, q), q * pad_gain[pads])  # f = 0
    assert np.array_equal(ref.Gain(0.0).rows(3, 4, pads, pads % 512, q), q)
    # u = 0 at f = 1, q = 1: z = Z[0] = -3.67, x = 8/9 - 3.67 / 3 < 0 -> the clamp
    assert Z[0] < -8.0 / 3.0 and gain.fluctuate(np.array([0], dtype=np.uint64), np.array([1.0]))[0] == 0.0
    assert _by_hand(0, 1.0, 1.0) == 0.0
    # u = 2^32 - 1: the last interval at w = 1 - 2^-20
    top = 0xFFFFFFFF
    for f, qq in ((1.0, 1.0), (0.3, 5.0), (1.0, 1e5)):
        got = ref.Gain(f, Z).fluctuate(np.array([top], dtype=np.uint64), np.array([qq]))[0]
        assert got == _by_hand(top, qq, f) and got > qq
    z_top = float(Z[4095]) + (float(Z[4096]) - float(Z[4095])) * ((2 ** 20 - 1) * 2.0 ** -20)
    assert Z[4095] < z_top < Z[4096]
    # a few uniforms across the table against the plain-Python contract
    rng = np.random.default_rng(5)
    for u in rng.integers(0, 1 << 32, size=200).tolist():
        for f, qq in ((1.0, 1.0), (0.25, 3.0), (0.5, 1000.0)):
            assert ref.Gain(f, Z).fluctuate(np.array([u], dtype=np.uint64), np.array([qq]))[0] == _by_hand(u, qq, f)
    # pad_gain = 0 silences a pad, whatever the draw
    silent = np.ones(ref.NUM_PADS)
    silent[9] = 0.0
    out = ref.Gain(1.0, Z, silent).rows(1, 2, np.array([8, 9, 10]), np.array([3, 3, 3]), np.array([50.0, 50.0, 50.0]))
    assert out[1] == 0.0 and out[0] > 0.0 and out[2] > 0.0


def test_counter_of_a_row():
    """Pads 0 and 10239, time buckets 0 and 511, an event id past 2^32, a seed with its high word set, a stream."""
    seed, event, stream = 0xDEADBEEF12345678, (1 << 32) + 5, 77
    gain = ref.Gain(1.0, Z, stream=stream)
    pads, ts = np.array([0, 0, 10239, 10239]), np.array([0, 511, 0, 511])
    u = gain.uniforms(seed, event, pads, ts)
    index = [0, 511, 10239 * 512, 10239 * 512 + 511]
    assert index[-1] == 5242879 < 1 << 23
    for k in range(4):
        want = philox4x32_10(5, 1, index[k], 0x40000000 | stream, 0x12345678, 0xDEADBEEF)[0]
        assert int(u[k]) == int(want)
    assert len(set(u.tolist())) == 4
    # the domain: bit 30, apart from the noise's bit 31 and from every small domain; another stream, another draw
    assert ref.DOMAIN_TRACE_GAIN == 1 << 30
    assert int(ref.Gain(1.0, Z).uniforms(seed, event, pads, ts)[0]) != int(u[0])
    common = (ROOT / "attpc_engine_amd" / "csrc" / "common.hpp").read_text()
    assert re.search(r"DOMAIN_TRACE_GAIN = 0x40000000u;", common)
    q = np.array([1.0, 10.0, 1e3, 1e5])
    rows = gain.rows(seed, event, pads, ts, q)
    assert [rows[k] == _by_hand(int(u[k]), float(q[k]), 1.0) for k in range(4)] == [True] * 4
    # the cloud form: event i of the call is the global event first_event + i
    points = np.stack([pads.astype(float), ts + 0.75, q], axis=1)
    both = gain.cloud([0, 0, 2, 4], points, seed, event - 1)
    assert np.array_equal(both[:2], rows[:2]) and np.array_equal(both[2:], gain.rows(seed, event + 1, pads[2:], ts[2:], q[2:]))


def test_label_rule_keeps_the_clouds_charge():
    """Two rows of one pad, q = 100 and 101, whose gained charges swap order: the label stays that of 101."""
    gain = ref.Gain(1.0, Z)
    seed = next(s for s in range(200) if np.diff(gain.rows(s, 0, [7, 7], [100, 130], [100.0, 101.0]))[0] < 0)
    points = np.array([[7, 100.2, 100.0], [7, 130.9, 101.0]])
    response = np.zeros(512)
    response[:20] = 0.5
    from tests.trace_reference import traces

    offsets, cloud_labels = np.array([0, 2]), np.array([1, 2])
    off, pads, samples, labels, _ = ref.traces_with_gain(offsets, points, cloud_labels, gain, seed, 0,
                                                         lambda pts: traces(offsets, pts, cloud_labels, response, -1.0, 0))
    assert labels.tolist() == traces(offsets, points, cloud_labels, response, -1.0, 0)[3].tolist()
    assert pads.tolist() == [7] and labels.tolist() == [2] and off.tolist() == [0, 1]
    q2 = gain.rows(seed, 0, [7, 7], [100, 130], [100.0, 101.0])
    assert samples[0, 100] == np.rint(q2[0] * 0.5) and samples[0, 130] == np.rint(q2[1] * 0.5) and q2[0] > q2[1]


# ---------------------------------------------------------------- settings ----
def test_theta_and_rel_variance():
    assert polya_rel_variance(0.0) == 1.0 and polya_rel_variance(1.0) == 0.5 and polya_rel_variance(3.0) == 0.25
    assert GainSettings(theta=1.0).rel_variance == GainSettings(rel_variance=0.5).rel_variance == 0.5
    assert GainSettings(theta=1.0).token() == GainSettings(rel_variance=0.5).token()
    only_map = GainSettings(pad_gain=np.full(_abi.NUM_PADS, 1.25))
    assert only_map.rel_variance == 0.0 and only_map.on and only_map.quantiles is None
    assert not GainSettings(rel_variance=0.0).on and GainSettings(rel_variance=0.0).token() is None
    assert GainSettings(rel_variance=1.0, pad_gain=2.0).pad_gain.shape == (_abi.NUM_PADS,)
    assert GainSettings(rel_variance=0.3, stream=5).token() != GainSettings(rel_variance=0.3).token()


@pytest.mark.parametrize("kw", [
    {}, {"rel_variance": 0.5, "theta": 1.0}, {"rel_variance": -0.1}, {"rel_variance": 1.5}, {"rel_variance": math.nan},
    {"theta": -1.0}, {"theta": math.inf}, {"rel_variance": 0.5, "pad_gain": np.full(_abi.NUM_PADS, -1.0)},
    {"rel_variance": 0.5, "pad_gain": np.full(_abi.NUM_PADS, math.inf)}, {"rel_variance": 0.5, "pad_gain": np.ones(7)},
    {"pad_gain": np.full(_abi.NUM_PADS, math.nan)}, {"rel_variance": 0.5, "stream": 1 << 30},
    {"rel_variance": 0.5, "stream": -1}, {"rel_variance": 0.5, "stream": 1.5}])
def test_gain_settings_refuse(kw):
    with pytest.raises(ValueError):
        GainSettings(**kw)


def test_descriptor_layout_and_sources():
    import __graft_entry__ as entry

    assert "gain.hip" in entry.HIP_SOURCES
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    assert "micromegas gain of the traces" in header and "#define ATTPC_GAIN_KNOTS 4097" in header
    for name in _abi.GAIN_SYMBOLS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert "trace_gain" in _abi.CONFIGURE_SLOTS
    fields = [f for f, _ in _abi.TraceGainDesc._fields_]
    args = ", ".join(["sizeof(attpc_trace_gain_desc)"] + [f"offsetof(attpc_trace_gain_desc, {f})" for f in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n printf("'
           + " ".join(["%zu"] * (1 + len(fields))) + f'\\n", {args});\n return 0; }}\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_abi.TraceGainDesc)] + [getattr(_abi.TraceGainDesc, f).offset for f in fields]
    design = (ROOT / "DESIGN.md").read_text()
    assert "0x40000000" in design and "4.4f" in design


def test_library_exports_the_entry_points_and_the_kernel_is_clean():
    import __graft_entry__ as entry
    from tests.isa_tools import disassemble

    entry.build()
    lib = _abi.load_library()
    for name in _abi.GAIN_SYMBOLS:
        assert hasattr(lib, name), name
    functions = disassemble(entry.LIB)
    kernels = [insns for name, insns in functions.items() if "gain_kernel" in name]
    assert len(kernels) == 1
    text = [t for _, t in kernels[0]]
    assert not [t for t in text if t.startswith("scratch_")]          # no spill
    assert any(t.startswith("v_div_fixup_f64") for t in text)         # the f64 division of the contract
    assert any(t.startswith("ds_read") for t in text)                 # the quantile table is read from LDS


# ---------------------------------------------------------------- the Python layer, the library replaced ----
class GainLibrary(RecordingLibrary):
    """The recording library that keeps what every attpc_trace_configure_gain call was given: None, or (rel_variance,
    stream, reserved, pad gains of pads 0 / 3 or None, quantiles 0 / 2048 / 4096 or None)."""

    def __init__(self):
        super().__init__()
        self.descs = []

    def _call(self, name, args):
        if name == "attpc_trace_configure_gain":
            d = args[1]
            self.descs.append(None if d is None else (
                d.rel_variance, d.stream, d.reserved, (d.pad_gain[0], d.pad_gain[3]) if d.pad_gain else None,
                (d.quantiles[0], d.quantiles[2048], d.quantiles[4096]) if d.quantiles else None))
        if name == "attpc_gain_rows":
            _, seed, first, n, offsets, points, gained = args
            for r in range(offsets[n]):
                gained[r] = 2.0 * points[3 * r + 2]
        return super()._call(name, args)


@pytest.fixture
def ctx():
    return RecordingContext(GainLibrary())


def test_configure_gain_descriptor_and_off(ctx):
    pad_gain = np.ones(_abi.NUM_PADS)
    pad_gain[3] = 0.0
    configure_gain(ctx, GainSettings(theta=1.0, pad_gain=pad_gain, stream=9))
    assert ctx.lib.descs == [(0.5, 9, 0, (1.0, 0.0), (Z[0], 0.0, Z[4096]))]
    configure_gain(ctx, GainSettings(rel_variance=0.5, pad_gain=pad_gain, stream=9))  # the same content: skipped
    assert len(ctx.lib.descs) == 1
    configure_gain(ctx, GainSettings(pad_gain=pad_gain))  # f = 0: no table is handed over
    assert ctx.lib.descs[-1] == (0.0, 0, 0, (1.0, 0.0), None)
    configure_gain(ctx, None)  # off restores NULL
    assert ctx.lib.descs[-1] is None and len(ctx.lib.descs) == 3
    configure_gain(ctx, None)
    configure_gain(ctx, GainSettings(rel_variance=0.0))  # changes nothing: off as well, and already off
    assert len(ctx.lib.descs) == 3 and ctx.lib.names() == ["trace_configure_gain"] * 3
    with pytest.raises(TypeError):
        configure_gain(ctx, 0.5)
    # a context that never had a gain is not called to turn it off
    fresh = RecordingContext(GainLibrary())
    configure_gain(fresh, None)
    assert fresh.lib.calls == []


def test_clouds_to_gain_through_the_stand_in(ctx):
    points = np.array([[1, 2.5, 10.0], [2, 3.5, 20.0], [3, 4.5, 30.0]])
    out = clouds_to_gain([0, 1, 3], points, ctx, seed=5, first_event=1 << 33, gain=GainSettings(rel_variance=1.0))
    assert ctx.lib.names() == ["trace_configure_gain", "gain_rows"] and ctx.lib.of("gain_rows")[0][1] == (5, 1 << 33, 2)
    assert out.tolist() == [20.0, 40.0, 60.0] and out.dtype == np.float64
    with pytest.raises(ValueError):
        clouds_to_gain([0, 4], points, ctx)
    with pytest.raises(ValueError):
        clouds_to_gain([0, 3], points, ctx, seed=-1)


def test_engine_and_row_configuration(ctx):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.o16aa()
    engine = Engine(pipeline, config, indices, context=ctx)
    ctx.lib.calls.clear()
    engine.configure_gain(theta=0.0, stream=2)
    assert ctx.lib.descs[-1][:3] == (1.0, 2, 0) and ctx.lib.names() == ["trace_configure_gain"]
    engine.run_traces(2, fetch=False)  # configuring the traces leaves the gain alone
    assert ctx.lib.names().count("trace_configure_gain") == 1 and len(ctx.lib.descs) == 1
    with pytest.raises(TypeError):
        engine.configure_gain(GainSettings(theta=0.0), theta=1.0)
    engine.configure_gain()
    assert ctx.lib.descs[-1] is None
    # the rows' configuration takes the gain beside the baseline
    configure_trace_rows(config, ctx, gain=GainSettings(rel_variance=0.25))
    assert ctx.lib.descs[-1][0] == 0.25
    configure_trace_rows(config, ctx)
    assert ctx.lib.descs[-1] is None
    validate_trace_kwargs(config, {"noise_sigma": 2.0}, GainSettings(theta=1.0))
    with pytest.raises(TypeError):
        validate_trace_kwargs(config, {}, gain=0.5)
    with pytest.raises(TypeError):
        validate_trace_kwargs(config, {"gain": GainSettings(theta=1.0)})  # not a keyword of configure_traces


class TraceSink:
    def __init__(self, tmp_path):
        self.events, self.closed = [], 0
        self.response, self.threshold, self.offset, self.noise_kwargs, self.readout_kwargs = None, None, 0, dict, dict
        self.get_directory_name = lambda: tmp_path

    def write_traces(self, pads, samples, labels, event):
        self.events.append(event)

    def close(self):
        self.closed += 1


@pytest.fixture
def no_h5py(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)


def test_writers_and_runs_take_a_gain(ctx, tmp_path, monkeypatch, no_h5py, capsys):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import PeakSettings, SpyralWriter, TraceWriter, run_simulation
    from attpc_engine_amd.engine import run_fused
    from attpc_engine_amd.io import KinematicsFileWriter

    pipeline, config, indices = workloads.o16aa()
    gain = GainSettings(theta=1.0, pad_gain=1.1, stream=4)
    with_cloud = [i for i in range(6) if POINTS[i % 4]]
    # run_fused: the gain given, the writer's own, none (whatever the context held is turned off)
    sink = TraceSink(tmp_path)
    run_fused(pipeline, config, sink, 6, indices, seed=8, batch_size=4, context=ctx, gain=gain)
    assert ctx.lib.descs[-1][:2] == (0.5, 4) and sink.events == with_cloud and sink.closed == 1
    sink.gain = GainSettings(rel_variance=0.25)
    run_fused(pipeline, config, sink, 2, indices, seed=8, context=ctx)
    assert ctx.lib.descs[-1][0] == 0.25
    del sink.gain
    run_fused(pipeline, config, sink, 2, indices, seed=8, context=ctx)
    assert ctx.lib.descs[-1] is None
    (tmp_path / "a").mkdir()
    rows_writer = SpyralWriter(tmp_path / "a", config, peaks=PeakSettings(), gain=gain)
    assert rows_writer.gain is gain
    run_fused(pipeline, config, rows_writer, 2, indices, seed=8, context=ctx)
    assert ctx.lib.descs[-1][:2] == (0.5, 4) and len(ctx.lib.of("sim_run_trace_rows")) == 1
    with pytest.raises(ValueError, match="a gain acts on traces or trace rows"):
        run_fused(pipeline, config, SpyralWriter(tmp_path, config), 2, indices, context=ctx, gain=gain)
    with pytest.raises(TypeError, match="only with peaks"):
        SpyralWriter(tmp_path, config, gain=gain)
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, peaks=PeakSettings(), gain=0.5)
    with pytest.raises(TypeError):
        TraceWriter(tmp_path, config, gain=0.5)
    # a trace writer records its gain in every file and configures it for write()
    (tmp_path / "b").mkdir()
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    writer = TraceWriter(tmp_path / "b", config, gain=gain)
    writer.write(np.array([[5.0, 10.5, 100.0]]), np.array([1]), config, 3)
    assert ctx.lib.descs[-1][:2] == (0.5, 4) and ctx.lib.names()[-1] == "traces_at"
    writer.close()
    content = np.load(tmp_path / "b" / "run_0000.npz")
    assert content["trace@gain_rel_variance"] == 0.5 and content["trace@gain_stream"] == 4
    assert content["trace/pad_gain"].shape == (_abi.NUM_PADS,) and content["trace/pad_gain"][0] == 1.1
    # run_simulation: through the batch entry points
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    path = tmp_path / "kin.npz"
    w = KinematicsFileWriter(path, 6, z, a, chunk_size=4)
    rng = np.random.default_rng(1)
    w.write_batch(0, rng.normal(size=(6, 3)), rng.normal(size=(6, len(z), 4)))
    w.close()
    sink = TraceSink(tmp_path)
    run_simulation(config, path, sink, indices, batch_size=4, seed=5, gain=GainSettings(rel_variance=0.75))
    assert ctx.lib.descs[-1][0] == 0.75 and sink.events == with_cloud
    run_simulation(config, path, sink, indices, batch_size=4, seed=5)
    assert ctx.lib.descs[-1] is None
    with pytest.raises(ValueError, match="a gain acts on traces or trace rows"):
        run_simulation(config, path, SpyralWriter(tmp_path, config), indices, seed=5, gain=gain)
