"""The common-mode noise of the pad traces without a device (include/attpc_engine.h, "common-mode noise of the
traces"): the numpy restatement against a per-sample loop written from the contract's text and against cases worked out
by hand, the settings' validation, the descriptor's layout and the symbols, ``expected_noise_pads`` with a common-mode
table against an enumeration over all level pairs, and the Python layer (``TraceChain``, the writers) over the recording
library of tests/test_run_layer_cpu.py."""
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

from attpc_engine_amd import _abi, workloads
from attpc_engine_amd.detector.traces import (
    CommonModeSettings, NoiseSettings, TraceChain, configure_common_mode, configure_trace_rows, expected_noise_pads,
    gaussian_noise_table)
from tests import common_mode_reference as cmr
from tests.test_run_layer_cpu import RecordingContext, RecordingLibrary
from tests.trace_noise_reference import Noise, philox4x32_10
from tests.trace_noise_reference import traces as noise_traces

ROOT = Path(__file__).resolve().parents[1]
NUM_PADS, NUM_TB = _abi.NUM_PADS, _abi.NUM_TB


# ---------------------------------------------------------------- the reference itself ----
def test_reference_values_equal_a_loop_over_the_contracts_text():
    cdf, min_level = gaussian_noise_table(3.0)
    seed, stream = (5 << 32) | 77, 9
    groups = [0, 2, 254]
    for event in (3, (7 << 32) | 1):
        got = cmr.values(seed, event, groups, (cdf, min_level), stream)
        assert got.shape == (3, NUM_TB)
        for i, g in enumerate(groups):
            for j in range(NUM_TB):
                out = philox4x32_10(event & 0xFFFFFFFF, event >> 32, g * 128 + 2 * (j % 64) + j // 256, 0x20000000 | stream,
                                    seed & 0xFFFFFFFF, seed >> 32)
                u = int(out[(j // 64) % 4])
                assert got[i, j] == min_level + sum(1 for c in cdf if int(c) <= u), (event, g, j)
    # another stream, another group, another event: other numbers
    base = cmr.values(seed, 3, [0], (cdf, min_level), stream)
    for other in (cmr.values(seed, 3, [0], (cdf, min_level), stream + 1), cmr.values(seed, 3, [1], (cdf, min_level), stream),
                  cmr.values(seed, 4, [0], (cdf, min_level), stream), cmr.values(seed + 1, 3, [0], (cdf, min_level), stream)):
        assert (other != base).mean() > 0.5


RESPONSE = np.zeros(NUM_TB)
RESPONSE[:3] = [1.0, 0.5, 0.25]


def _cloud():
    # pads 0 (group 0), 7 (group 254), 10239 (group 255), 9 (group 0): one event
    points = np.array([[0, 10.2, 100.0], [0, 300.0, 40.0], [7, 20.0, 50.0], [10239, 511.0, 30.0], [9, 0.0, 5000.0]])
    labels = np.array([1, 2, 3, 4, 5])
    groups = np.zeros(NUM_PADS, dtype=np.uint8)
    groups[7] = 254
    groups[10239] = 255
    return [0, 5], points, labels, groups


def test_one_level_table_by_hand():
    offsets, points, labels, groups = _cloud()
    cdf, lo = gaussian_noise_table(1.0)
    for pedestal in (0, 300, 4095):
        ped = np.full(NUM_PADS, pedestal)
        for noise in (Noise(cdf, lo, pedestals=ped), Noise(pedestals=ped)):
            for level in (3, -3):
                common = cmr.CommonMode((np.zeros(0, dtype=np.uint32), level), groups)
                assert common.n_groups == 255 and (common.all_values(1, 2) == level).all()
                _, pads0, samples0, labels0, _ = noise_traces(offsets, points, labels, RESPONSE, -1.0, 0, noise, seed=4, first_event=6)
                # thr = -1 keeps every hit pad with and without the term, so the rows can be compared one to one
                _, pads1, samples1, labels1, sums = cmr.traces(offsets, points, labels, RESPONSE, -1.0, 0, noise, common, seed=4,
                                                               first_event=6)
                assert pads0.tolist() == pads1.tolist() == [0, 7, 9, 10239] and labels0.tolist() == labels1.tolist() == [1, 3, 5, 4]
                s = np.zeros((4, NUM_TB), dtype=np.int64)  # the noiseless samples, by hand
                s[0, 10:13] = [100, 50, 25]
                s[0, 300:303] = [40, 20, 10]
                s[1, 20:23] = [50, 25, 12]  # rint(12.5) = 12, half to even
                s[2, 0:3] = [4095, 2500, 1250]
                s[3, 511] = 30
                n = noise.values(4, 6, [0, 7, 9, 10239])
                expect = np.clip(s + pedestal + n + np.array([level, level, level, 0])[:, None], 0, 4095)
                assert np.array_equal(samples1, expect)
                assert np.array_equal(samples1[3], samples0[3])  # group 255: unchanged
                grouped = np.clip(samples0[:3].astype(np.int64) + level, 0, 4095)
                if pedestal == 300:  # no clamp in the way (|n| <= 8): the pad-noise traces plus the level
                    inner = (s[:3] + pedestal + n[:3] + level >= 0) & (s[:3] + pedestal + n[:3] <= 4095)
                    assert np.array_equal(samples1[:3][inner], grouped[inner]) and inner.mean() > 0.99
                if pedestal == 4095 and level == 3:
                    assert samples1[:3].max() == 4095 and (samples1[:3] == 4095).mean() > 0.9  # clamps high
                if pedestal == 0 and level == -3:
                    assert samples1[:3].min() == 0 and (samples1[:3] == 0).mean() > 0.9  # clamps at 0
                assert sums["n_rows"] == 4
                assert sums["sample_checksum"] == int((samples1.astype(np.int64) @ np.arange(1, 513)).sum()) % (1 << 64)


def test_reference_threshold_is_taken_on_the_sum():
    # one pad, one row of 10 electrons: s = 10 at sample 5; thr = 11; a level of +3 lifts it over, -3 does not
    groups = np.zeros(NUM_PADS, dtype=np.uint8)
    groups[1] = 255
    for pad, level, kept in ((0, 3, True), (0, -3, False), (1, 3, False), (0, 1, False), (0, 2, True)):
        common = cmr.CommonMode((np.zeros(0, dtype=np.uint32), level), groups)
        _, pads, _, _, _ = cmr.traces([0, 1], np.array([[pad, 5.0, 10.0]]), np.array([1]), RESPONSE, 11.0, 0, None, common)
        assert (len(pads) == 1) == kept, (pad, level)
    # partial readout: a noise-only pad with a group is kept iff the level is above thr; full keeps all of S
    channels = np.zeros(NUM_PADS, dtype=bool)
    channels[[0, 1, 2]] = True
    common = cmr.CommonMode((np.zeros(0, dtype=np.uint32), 3), groups)
    off, pads, samples, labels, _ = cmr.traces([0, 0, 1], np.array([[1, 5.0, 10.0]]), np.array([9]), RESPONSE, 2.0, 0, None,
                                               common, mode=cmr.PARTIAL, channels=channels)
    assert off.tolist() == [0, 2, 5] and pads.tolist() == [0, 2, 0, 1, 2] and labels.tolist() == [-1, -1, -1, 9, -1]
    assert (samples[0] == 3).all() and samples[3].max() == 10
    off, pads, _, _, _ = cmr.traces([0, 0], np.zeros((0, 3)), np.zeros(0), RESPONSE, 3.0, 0, None, common, mode=cmr.PARTIAL,
                                    channels=channels)
    assert len(pads) == 0
    off, pads, _, _, _ = cmr.traces([0, 0], np.zeros((0, 3)), np.zeros(0), RESPONSE, 3.0, 0, None, common, mode=cmr.FULL,
                                    channels=channels)
    assert pads.tolist() == [0, 1, 2]


# ---------------------------------------------------------------- settings ----
_CDF, _LO = gaussian_noise_table(2.0)
_GROUPS = np.zeros(NUM_PADS, dtype=np.uint8)


@pytest.mark.parametrize("kw", [
    {"table": (_CDF[::-1], _LO)},                                   # a decreasing cdf
    {"table": (np.arange(512, dtype=np.uint32), 0)},                # 513 levels
    {"table": (_CDF, 4096)}, {"table": (_CDF, -4096)}, {"table": (_CDF, 0.5)},  # min_level out of range
    {"table": (np.array([-1, 3]), 0)}, {"table": (np.array([0, 1 << 32]), 0)}, {"table": (np.array([0.5, 1.5]), 0)},
    {"table": (np.zeros((2, 2), dtype=np.uint32), 0)},
    {"sigma": 2.0, "stream": 1 << 29}, {"sigma": 2.0, "stream": -1}, {"sigma": 2.0, "stream": 1.5},  # the stream
    {"sigma": 2.0, "groups": np.zeros(NUM_PADS - 1, dtype=np.uint8)},  # the groups: shape
    {"sigma": 2.0, "groups": np.zeros((2, NUM_PADS), dtype=np.uint8)},
    {"sigma": 2.0, "groups": np.zeros(NUM_PADS, dtype=np.int32)},      # ... and dtype
    {"sigma": 2.0, "groups": np.zeros(NUM_PADS, dtype=np.float64)},
    {"sigma": 2.0, "groups": 3},
    {"sigma": 1.0, "table": (_CDF, _LO)},                            # both
    {"sigma": -1.0}, {"sigma": math.nan}, {"sigma": 32.0},
])
def test_settings_refuse(kw):
    with pytest.raises(ValueError):
        CommonModeSettings(**kw)


def test_settings_content():
    cm = CommonModeSettings(sigma=2.0, groups=_GROUPS, stream=5)
    noise = NoiseSettings(2.0)
    assert np.array_equal(cm.cdf, noise.cdf) and cm.min_level == noise.min_level and cm.n_levels == noise.n_levels == 33
    assert cm.n_groups == 1 and cm.on and cm.sigma == 2.0 and cm.stream == 5
    assert (cm.slot, cm.call) == ("trace_common", "attpc_trace_configure_common_mode")
    d = cm.desc()
    assert (d.n_levels, d.min_level, d.stream, d.reserved) == (33, -16, 5, 0) and d.cdf[0] == cm.cdf[0] and d.groups[7] == 0
    assert CommonModeSettings(sigma=2.0).desc().groups is None or not CommonModeSettings(sigma=2.0).desc().groups
    groups = np.full(NUM_PADS, 255, dtype=np.uint8)
    assert CommonModeSettings(sigma=2.0, groups=groups).n_groups == 0 and CommonModeSettings(sigma=2.0, groups=groups).token() is None
    groups[5] = 254
    assert CommonModeSettings(sigma=2.0, groups=groups).n_groups == 255
    assert CommonModeSettings().token() is None and not CommonModeSettings().on and CommonModeSettings().n_levels == 0
    one = CommonModeSettings(table=(np.zeros(0, dtype=np.uint32), 3))
    assert one.n_levels == 1 and one.on and math.isnan(one.sigma)
    assert cm.token() != CommonModeSettings(sigma=2.0, groups=_GROUPS, stream=6).token()
    assert cm.token() != CommonModeSettings(sigma=2.0, stream=5).token()  # (NULL groups is another content)
    assert cm.token() == CommonModeSettings(table=(cm.cdf, cm.min_level), groups=_GROUPS.copy(), stream=5).token()


def test_descriptor_layout_symbols_and_documents():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    assert "common-mode noise of the traces" in header and "0x20000000 | stream" in header
    for name in ("attpc_trace_configure_common_mode", "attpc_common_mode_rows"):
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert set(_abi.COMMON_SYMBOLS) == {"attpc_trace_configure_common_mode", "attpc_common_mode_rows"}
    assert "trace_common" in _abi.CONFIGURE_SLOTS
    fields = [f for f, _ in _abi.TraceCommonDesc._fields_]
    args = ", ".join(["sizeof(attpc_trace_common_desc)"] + [f"offsetof(attpc_trace_common_desc, {f})" for f in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n printf("'
           + " ".join(["%zu"] * (1 + len(fields))) + f'\\n", {args});\n return 0; }}\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_abi.TraceCommonDesc)] + [getattr(_abi.TraceCommonDesc, f).offset for f in fields]
    common = (ROOT / "attpc_engine_amd" / "csrc" / "common.hpp").read_text()
    assert "DOMAIN_TRACE_COMMON = 0x20000000u" in common
    design = (ROOT / "DESIGN.md").read_text()
    assert "0x20000000" in design and "4.4g" in design


def test_library_exports_the_entry_points_and_the_kernels_are_clean():
    import __graft_entry__ as entry
    from tests.isa_tools import disassemble

    entry.build()
    lib = _abi.load_library()
    for name in _abi.COMMON_SYMBOLS:
        assert hasattr(lib, name), name
    functions = disassemble(entry.LIB)
    kernels = {name: [t for _, t in insns] for name, insns in functions.items() if "common_mode_kernel" in name}
    assert len(kernels) == 1
    # the new instantiations of the sample-producing kernels exist (CM = true is their last template argument) ...
    for needle in ("trace_count_kernelILb1ELb0ELb1E", "trace_count_kernelILb1ELb1ELb1E", "trace_write_kernelILb1ELb1E",
                   "trace_scan_kernelILb1E", "trace_noise_write_kernelILb1E"):
        found = [name for name in functions if needle in name]
        assert len(found) == 1, needle
        kernels[found[0]] = [t for _, t in functions[found[0]]]
    for name, text in kernels.items():
        assert not [t for t in text if t.startswith("scratch_")], name  # ... and none of them spills
        if "common_mode_kernel" in name:
            assert any(t.startswith("global_store_dwordx4") for t in text), name  # 16 B per lane
        else:
            assert any(t.startswith("global_load_dwordx4") for t in text), name  # the group's values: 16 B per lane


# ---------------------------------------------------------------- expected_noise_pads ----
def _enumerated(pad_table, common_table, thr, ped, grouped):
    """P(pad kept) by enumeration over all level pairs, from the decision rule's text."""
    if 4095 - ped <= thr:
        return 0.0
    if -ped > thr:
        return 1.0
    (pc, pl), (cc, cl) = pad_table, common_table
    pad_mass = np.diff(np.concatenate(([0], pc.astype(np.int64), [1 << 32])))
    com_mass = np.diff(np.concatenate(([0], cc.astype(np.int64), [1 << 32]))) if grouped else np.array([1 << 32])
    cl = cl if grouped else 0
    q = 0
    for i, a in enumerate(pad_mass):
        for k, b in enumerate(com_mass):
            if pl + i + cl + k > thr:
                q += int(a) * int(b)
    q = q / 2.0 ** 64  # (q is an exact integer up to here)
    return -math.expm1(512 * math.log1p(-q)) if q < 1.0 else 1.0


def test_expected_noise_pads_with_a_common_mode_table():
    # pad levels -3 .. 3 (7), common-mode levels -2 .. 2 (5): the sums reach 5
    pad = (np.array([1 << 20, 1 << 26, 1 << 30, 3 << 30, (1 << 32) - (1 << 26), (1 << 32) - (1 << 20)], dtype=np.uint32), -3)
    com = (np.array([1 << 22, 1 << 31, 3 << 30, (1 << 32) - (1 << 21)], dtype=np.uint32), -2)
    groups = np.zeros(NUM_PADS, dtype=np.uint8)
    groups[40] = 255
    groups[41:44] = [1, 2, 254]
    ped = np.full(NUM_PADS, 10, dtype=np.int64)
    ped[41] = 0       # -ped > thr for thr < 0: always
    ped[42] = 4095    # 4095 - ped <= thr for thr >= 0: never
    ped[43] = 4092    # 4095 - ped = 3: never for thr >= 3
    readout = np.array([40, 41, 42, 43, 44, 45])
    cm = CommonModeSettings(table=com, groups=groups)
    seen = set()
    for thr in (-1.0, 0.0, 2.5, 3.0, 4.0, 5.0, 40.0):
        want = 0.0
        for p in readout:
            term = _enumerated(pad, com, thr, int(ped[p]), groups[p] != 255)
            seen.add("always" if term == 1.0 else "never" if term == 0.0 else "draw")
            want += term
        got = expected_noise_pads(pad, thr, readout, ped, common_mode=cm)
        assert got == pytest.approx(want, rel=1e-12, abs=1e-300), thr
        # without the stage, and with a stage that is off, the value is the one of before
        assert expected_noise_pads(pad, thr, readout, ped, common_mode=CommonModeSettings()) == expected_noise_pads(pad, thr, readout, ped)
    assert seen == {"always", "never", "draw"}
    # thr = 4: the pad table alone never crosses (levels end at 3); pads with a group can (3 + 2 = 5), pad 40 cannot
    alone = expected_noise_pads(pad, 4.0, readout, ped)
    assert alone == 0.0 and expected_noise_pads(pad, 4.0, [40], ped, common_mode=cm) == 0.0
    assert expected_noise_pads(pad, 4.0, [44], ped, common_mode=cm) > 0.0
    # no pad table at all: the common-mode table alone decides
    only = expected_noise_pads(None, 1.0, [44, 45], None, common_mode=cm)
    q = (1 << 21) / 2.0 ** 32  # P(c = 2)
    assert only == pytest.approx(2 * (1.0 - (1.0 - q) ** 512), rel=1e-12)
    with pytest.raises(TypeError):
        expected_noise_pads(pad, 1.0, common_mode=3.0)


# ---------------------------------------------------------------- the Python layer, the library replaced ----
class CommonLibrary(RecordingLibrary):
    """The recording library that keeps what every attpc_trace_configure_common_mode call was given: None, or
    (n_levels, min_level, stream, reserved, first cdf entry or None, groups of pads 0 / 7 or None)."""

    def __init__(self):
        super().__init__()
        self.descs = []

    def _call(self, name, args):
        if name == "attpc_trace_configure_common_mode":
            d = args[1]
            self.descs.append(None if d is None else (
                d.n_levels, d.min_level, d.stream, d.reserved, d.cdf[0] if d.cdf else None,
                (d.groups[0], d.groups[7]) if d.groups else None))
        if name == "attpc_common_mode_rows":
            _, seed, first, n, out = args
            out[0] = 7
        return super()._call(name, args)


@pytest.fixture
def ctx():
    return RecordingContext(CommonLibrary())


@pytest.fixture(scope="module")
def config():
    return workloads.o16aa()[1]


def _settings(stream=3):
    groups = np.zeros(NUM_PADS, dtype=np.uint8)
    groups[7] = 4
    return CommonModeSettings(sigma=2.0, groups=groups, stream=stream)


def test_chain_holds_replaces_and_configures_the_stage(config, ctx):
    cm = _settings()
    assert TraceChain(config).common_mode is None
    chain = TraceChain(config, common_mode=cm)
    assert chain.common_mode is cm
    assert TraceChain(config).replace(common_mode=cm).common_mode is cm and chain.replace(common_mode=None).common_mode is None
    for bad in (2.0, {"sigma": 2.0}, "on"):
        with pytest.raises(TypeError, match="common_mode must be a CommonModeSettings or None"):
            TraceChain(config, common_mode=bad)
        with pytest.raises(TypeError, match="common_mode must be a CommonModeSettings or None"):
            chain.replace(common_mode=bad)
    # stage off on a fresh context: no call
    TraceChain(config).configure(ctx, rows=True)
    assert "trace_configure_common_mode" not in ctx.lib.names() and ctx.lib.descs == [] and ctx._tokens["trace_common"] is None
    # stage on: the call comes directly after the noise (noise on, so that its call is made too)
    fresh = RecordingContext(CommonLibrary())
    TraceChain.from_kwargs(config, noise_sigma=1.0).replace(common_mode=cm).configure(fresh, rows=True)
    names = fresh.lib.names()
    at = names.index("trace_configure_noise")
    assert names[at + 1] == "trace_configure_common_mode"
    assert names.count("trace_configure_common_mode") == 1
    assert fresh.lib.descs == [(33, -16, 3, 0, int(cm.cdf[0]), (0, 4))] and fresh._tokens["trace_common"] == cm.token()
    # the same content again: skipped; another stream: called; off again: NULL
    TraceChain(config, common_mode=_settings()).configure(fresh)
    assert len(fresh.lib.descs) == 1
    TraceChain(config, common_mode=_settings(4)).configure(fresh)
    assert fresh.lib.descs[-1][2] == 4
    TraceChain(config).configure(fresh, keep=("common_mode",))  # kept as the context holds it
    assert len(fresh.lib.descs) == 2 and fresh._tokens["trace_common"] == _settings(4).token()
    TraceChain(config).configure(fresh)
    assert fresh.lib.descs[-1] is None and len(fresh.lib.descs) == 3
    configure_common_mode(fresh, CommonModeSettings())  # without effect: off as well, and already off
    assert len(fresh.lib.descs) == 3
    with pytest.raises(TypeError):
        configure_common_mode(fresh, 2.0)


def test_engine_rows_configuration_and_values(config, ctx):
    from attpc_engine_amd.detector.traces import common_mode_values
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.o16aa()
    engine = Engine(pipeline, config, indices, context=ctx)
    ctx.lib.calls.clear()
    engine.configure_common_mode(sigma=2.0, stream=2)
    assert ctx.lib.descs[-1][:4] == (33, -16, 2, 0) and ctx.lib.descs[-1][5] is None
    assert ctx.lib.names() == ["trace_configure_common_mode"]
    engine.run_traces(2, fetch=False)  # configuring the traces leaves the stage alone
    assert ctx.lib.names().count("trace_configure_common_mode") == 1
    with pytest.raises(TypeError):
        engine.configure_common_mode(_settings(), sigma=1.0)
    engine.configure_common_mode()
    assert ctx.lib.descs[-1] is None
    configure_trace_rows(config, ctx, common_mode=_settings())
    assert ctx.lib.descs[-1][:4] == (33, -16, 3, 0)
    configure_trace_rows(config, ctx)
    assert ctx.lib.descs[-1] is None
    # the stage alone
    ctx.lib.calls.clear()
    out = common_mode_values(2, _settings(), seed=5, first_event=1 << 33, ctx=ctx)
    assert ctx.lib.names() == ["trace_configure_common_mode", "common_mode_rows"]
    assert ctx.lib.of("common_mode_rows")[0][1] == (5, 1 << 33, 2)
    assert out.shape == (2, 5, NUM_TB) and out.dtype == np.int16 and out[0, 0, 0] == 7
    assert common_mode_values(3, CommonModeSettings(), ctx=ctx).shape == (3, 1, NUM_TB)
    with pytest.raises(TypeError):
        common_mode_values(2, None, ctx=ctx)
    with pytest.raises(ValueError):
        common_mode_values(2, _settings(), seed=-1, ctx=ctx)


class TraceSink:
    def __init__(self, tmp_path):
        self.events, self.closed = [], 0
        self.response, self.threshold, self.offset = None, None, 0
        self.get_directory_name = lambda: tmp_path

    def write_traces(self, pads, samples, labels, event):
        self.events.append(event)

    def close(self):
        self.closed += 1


def test_writers_and_runs_take_the_stage(ctx, tmp_path, monkeypatch):
    from attpc_engine_amd.detector import PeakSettings, SpyralWriter, TraceWriter, run_simulation
    from attpc_engine_amd.engine import run_fused
    from attpc_engine_amd.io import KinematicsFileWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    pipeline, config, indices = workloads.o16aa()
    cm = _settings()
    sink = TraceSink(tmp_path)
    run_fused(pipeline, config, sink, 3, indices, seed=8, context=ctx, common_mode=cm)
    assert ctx.lib.descs[-1][:4] == (33, -16, 3, 0) and sink.closed == 1
    sink.common_mode = _settings(6)  # the writer's own
    run_fused(pipeline, config, sink, 2, indices, seed=8, context=ctx)
    assert ctx.lib.descs[-1][2] == 6
    del sink.common_mode
    run_fused(pipeline, config, sink, 2, indices, seed=8, context=ctx)  # none: whatever the context held is turned off
    assert ctx.lib.descs[-1] is None
    (tmp_path / "a").mkdir()
    rows_writer = SpyralWriter(tmp_path / "a", config, peaks=PeakSettings(), common_mode=cm)
    assert rows_writer.common_mode is cm and rows_writer.chain.common_mode is cm
    run_fused(pipeline, config, rows_writer, 2, indices, seed=8, context=ctx)
    assert ctx.lib.descs[-1][:4] == (33, -16, 3, 0) and len(ctx.lib.of("sim_run_trace_rows")) == 1
    with pytest.raises(ValueError, match="common-mode noise acts on traces or trace rows"):
        run_fused(pipeline, config, SpyralWriter(tmp_path, config), 2, indices, context=ctx, common_mode=cm)
    with pytest.raises(TypeError, match="only with peaks"):
        SpyralWriter(tmp_path, config, common_mode=cm)
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, peaks=PeakSettings(), common_mode=2.0)
    with pytest.raises(TypeError):
        TraceWriter(tmp_path, config, common_mode=2.0)
    # a trace writer records the stage in every file when it is set, and only then, and configures it for write()
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    for name, setting in (("b", cm), ("c", None), ("d", CommonModeSettings())):
        (tmp_path / name).mkdir()
        writer = TraceWriter(tmp_path / name, config, common_mode=setting)
        writer.write(np.array([[5.0, 10.5, 100.0]]), np.array([1]), config, 3)
        assert ctx.lib.names()[-1] == "traces_at"
        assert ctx.lib.descs[-1] is None if setting is not cm else ctx.lib.descs[-1][:4] == (33, -16, 3, 0)
        writer.close()
        content = np.load(tmp_path / name / "run_0000.npz")
        recorded = sorted(k for k in content.files if "common_mode" in k)
        if setting is cm:
            assert recorded == ["trace/common_mode_cdf", "trace/common_mode_groups", "trace@common_mode_min_level",
                                "trace@common_mode_sigma", "trace@common_mode_stream"]
            assert content["trace@common_mode_stream"] == 3 and content["trace@common_mode_sigma"] == 2.0
            assert content["trace@common_mode_min_level"] == -16 and np.array_equal(content["trace/common_mode_cdf"], cm.cdf)
            assert np.array_equal(content["trace/common_mode_groups"], cm.groups)
        else:
            assert recorded == []
    # run_simulation: through the batch entry points
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    path = tmp_path / "kin.npz"
    w = KinematicsFileWriter(path, 6, z, a, chunk_size=4)
    rng = np.random.default_rng(1)
    w.write_batch(0, rng.normal(size=(6, 3)), rng.normal(size=(6, len(z), 4)))
    w.close()
    sink = TraceSink(tmp_path)
    run_simulation(config, path, sink, indices, batch_size=4, seed=5, common_mode=_settings(9))
    assert ctx.lib.descs[-1][2] == 9
    run_simulation(config, path, sink, indices, batch_size=4, seed=5)
    assert ctx.lib.descs[-1] is None
    with pytest.raises(ValueError, match="common-mode noise acts on traces or trace rows"):
        run_simulation(config, path, SpyralWriter(tmp_path, config), indices, common_mode=cm)
