"""Trace rows, host side (no GPU): the numpy restatement of the contract (tests/peaks_reference.py) against scipy stage
by stage and, on tie-free inputs, against the one-call ``find_peaks``; its Philox2x32-7 against the CPU oracle's jitter;
the hand-made cases (tests/peaks_cases.py) asserted on the restatement, so that the GPU test cannot pass on inputs that
miss them; the validation of the parameters in Python; the generated code of the peak kernels (no fused multiply-add,
no scratch, no scalar stores, every barrier behind a wait); and the new exports in the header and the binding.

Why not one scipy call as the yardstick: on noisy integer traces two candidates of equal height within the separation
are the rule, and ``find_peaks(y, distance=...)`` then depends on numpy's unstable argsort of equal keys.  The
yardstick is scipy's public functions stage by stage with the tie made definite (a ramp of 2^-20 per candidate on the
integer heights: the later candidate wins).

scipy is required here (an ImportError fails the two tests, it does not skip them): they are the only checks of the
restatement against an independent implementation, and the GPU tests compare the device against the restatement alone."""
import ctypes as C
import math
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import peaks_cases
from tests.isa_tools import _LGKM_OPS, barriers_without_lds_wait, device_code_objects, disassemble_objects, llvm_tool
from tests.peaks_reference import (DOMAIN_JITTER, Geometry, Peaks, jitter_uniform, local_maxima, staged_peaks,
                                   trace_points, trace_rows)
from tests.trace_noise_reference import Noise
from tests.trace_noise_reference import traces as noisy_traces

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
SCALAR_MEMORY_WRITES = tuple(p for p in _LGKM_OPS if p.startswith("s_") and not p.startswith(
    ("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_sendmsg")))


def _synthetic_traces(n, seed):
    """Integer traces like the device's: 0 to 4 shaper-like pulses (single arrivals and tracks of up to 80 consecutive
    buckets), summed signal clipped at 4095, pedestal 0 / 300 / 4000, integer Gaussian noise of 0 / 1 / 5 counts,
    clipped to 0 .. 4095 -> y = trace - pedestal."""
    rng = np.random.default_rng(seed)
    t = np.arange(512.0)
    shape = np.exp(-3.0 * t / 7.0) * (t / 7.0) ** 3 * np.sin(t / 7.0)
    shape[shape < 0] = 0.0
    shape /= shape.max()
    for _ in range(n):
        s = np.zeros(512)
        for _ in range(int(rng.integers(0, 5))):
            t0, a, w = int(rng.integers(0, 510)), float(rng.choice([30, 100, 800, 3000, 9000])), int(rng.integers(1, 80))
            for q in range(w):
                if t0 + q < 512:
                    s[t0 + q:] += a / (1 if w < 4 else 3) * shape[:512 - t0 - q]
        s = np.rint(np.minimum(s, 4095.0))
        ped = int(rng.choice([0, 300, 4000]))
        noise = np.rint(rng.normal(0.0, float(rng.choice([0, 1, 5])), 512)) if rng.random() < 0.8 else np.zeros(512)
        yield (np.clip(s + ped + noise, 0, 4095) - ped).astype(np.int64)


def _scipy_staged(y, pk):
    from scipy.signal import find_peaks, peak_prominences, peak_widths

    y = y.astype(np.float64)
    cand = find_peaks(y)[0]
    if len(cand) == 0:
        return cand, []
    ramp = np.full(len(y), -1.0e9)
    ramp[cand] = y[cand] + np.arange(len(cand)) * 2.0 ** -20  # integer heights: the ramp only orders ties
    sel = find_peaks(ramp, distance=pk.separation)[0]
    prom, lb, rb = peak_prominences(y, sel)
    keep = prom >= pk.prominence
    sel, prom, lb, rb = sel[keep], prom[keep], lb[keep], rb[keep]
    width, _, lip, rip = peak_widths(y, sel, pk.rel_height, (prom, lb, rb))
    keep = (width >= pk.min_width) & (width <= pk.max_width)
    return cand, [(int(k), int(p), float(a), float(b)) for k, p, a, b in zip(sel[keep], prom[keep], lip[keep], rip[keep])]


@pytest.mark.parametrize("pk", [Peaks(), Peaks(separation=7.5, prominence=3.0, min_width=0.0, max_width=200.0,
                                               rel_height=0.5, threshold=0.0),
                                Peaks(separation=1.0, prominence=0.0, min_width=0.0, max_width=512.0, rel_height=1.0,
                                      threshold=-5000.0)], ids=["defaults", "loose", "everything"])
def test_restatement_equals_scipy_stage_by_stage(pk):
    n_points = n_ties = 0
    for y in _synthetic_traces(400, 11):
        cand, want = _scipy_staged(y, pk)
        np.testing.assert_array_equal(local_maxima(y), cand)
        got = staged_peaks(y, pk)
        assert got == want  # peaks, prominences, left_ip and right_ip: exactly
        n_points += len(got)
        heights = y[cand]
        n_ties += int(any(heights[i] == heights[j] and cand[j] - cand[i] < math.ceil(pk.separation)
                          for i in range(len(cand)) for j in range(i + 1, min(i + 12, len(cand)))))
    assert n_points > 300 and (pk.separation < 2 or n_ties > 100)  # ties within the separation are the rule


def test_restatement_equals_one_call_find_peaks_on_tie_free_inputs():
    from scipy import signal

    pk = Peaks()
    rng = np.random.default_rng(3)
    n_points = 0
    for y in _synthetic_traces(300, 12):
        y2 = y * 512 + rng.permutation(512)  # no two samples equal: no tie for argsort to break
        pk2 = pk._replace(prominence=pk.prominence * 512.0)
        sel, props = signal.find_peaks(y2.astype(np.float64), distance=pk2.separation, prominence=pk2.prominence,
                                       width=(pk2.min_width, pk2.max_width), rel_height=pk2.rel_height)
        want = [(int(k), int(p), float(a), float(b)) for k, p, a, b in
                zip(sel, props["prominences"], props["left_ips"], props["right_ips"])]
        assert staged_peaks(y2, pk2) == want
        n_points += len(want)
    assert n_points > 200


def test_philox2x32_7_is_the_oracles_jitter_generator():
    """With the key constant 0x100 the restatement's generator is the cloud's jitter, which the CPU oracle computes:
    0x300 is then the same function on another key word."""
    import __graft_entry__ as entry

    entry.build()
    from oracle import pyoracle as orc

    keys = np.array([0, 1, 77, (511 << 14) | 10239, (300 << 14) | 5, 0xFFFFFF], dtype=np.uint64)
    for seed, event in ((0, 0), (5, 100), (0xFEDCBA9876543210, (1 << 32) + 3), ((1 << 64) - 1, (1 << 40) - 1),
                        (0x1234567800000000, (1 << 64) - 2)):
        want = np.array([orc.jitter_uniform(seed, event, int(k)) for k in keys])
        np.testing.assert_array_equal(jitter_uniform(seed, event, keys, DOMAIN_JITTER), want)
        other = jitter_uniform(seed, event, keys)
        assert not np.array_equal(other, want) and ((0.0 <= other) & (other < 1.0)).all()
    assert jitter_uniform(5, 100, np.uint64(77)) == jitter_uniform(5, 100 + (1 << 40), np.uint64(77))  # 40 bits of the id
    assert jitter_uniform(5, 100, np.uint64(77)) != jitter_uniform(5, 101, np.uint64(77))


def test_division_by_an_integer_is_correctly_rounded(tmp_path):
    """div_by_int_rn (csrc/div_rn.hpp), the long division the peak kernels use for the contract's two quotients, against
    the host's IEEE division on 4e6 operands and the special values (tests/native/div_rn_check.cpp)."""
    exe = tmp_path / "div_rn_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "div_rn_check.cpp")], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0 and proc.stdout.strip().endswith("bad=0"), proc.stdout
    assert int(proc.stdout.split("n=")[1].split()[0]) > 4_000_000


def _hand_rows(seed=9, first=3):
    from attpc_engine_amd import workloads

    _, config, _ = workloads.o16aa()
    offsets, points, labels = peaks_cases.hand_cloud()
    ped = peaks_cases.pedestals()
    tr = noisy_traces(offsets, points, labels, peaks_cases.box_response(), peaks_cases.TRACE_THRESHOLD,
                      peaks_cases.TRACE_OFFSET, Noise(pedestals=ped), seed, first)
    geo = Geometry.of(config)
    return tr, trace_rows(tr[0], tr[1], tr[2], tr[3], Peaks(), geo, seed, first, ped), geo


def test_hand_cases_on_the_restatement():
    tr, (offsets, rows, labels, sums), geo = _hand_rows()
    cases = peaks_cases.hand_cases()
    assert len(offsets) == len(cases) + 1 and sums["n_rows"] == len(rows) == offsets[-1]
    checksum = 0
    for i, (name, points, case_labels, expected) in enumerate(cases):
        got = rows[offsets[i]:offsets[i + 1]]
        assert sorted((int(r[5]), int(r[6]), int(r[3])) for r in got) == sorted(expected), name
        assert (np.diff(got[:, 2]) >= 0).all() and (np.diff(got[:, 6]) <= 0).all(), name  # ascending z
        assert (labels[offsets[i]:offsets[i + 1]] == i % 7).all(), name
        for r in got:
            p, c = int(r[5]), r[6]
            assert r[0] == geo.pad_centers[p, 0] and r[1] == geo.pad_centers[p, 1] and r[7] == geo.pad_sizes[p]
            assert r[2] == (geo.windows_edge - c) / (geo.windows_edge - geo.micromegas_edge) * geo.length * 1000.0
            checksum += ((3 + i) << 23) + (p << 9) + int(c)
    assert sums["row_checksum"] == checksum % (1 << 64)
    by_name = {name: i for i, (name, *_rest) in enumerate(cases)}
    # the rows that have no point are there as traces: the stage, not the suppression, dropped them
    for name in ("prominence_below_limit_dropped", "width_above_max_dropped", "amplitude_at_threshold_dropped",
                 "all_zero_row"):
        i = by_name[name]
        assert tr[0][i + 1] - tr[0][i] == 1 and offsets[i + 1] == offsets[i], name
    zero = tr[2][tr[0][by_name["all_zero_row"]]]
    assert not zero.any()
    sat = tr[2][tr[0][by_name["saturated_flat_at_4095_minus_pedestal"]]]
    assert sat.max() == 4095 and (sat == 4095).sum() == 2 and sat.min() == 300
    # what each case is there for, on its own trace
    y = lambda name: tr[2][tr[0][by_name[name]]].astype(np.int64) - (300 if "saturated" in name else 0)
    assert local_maxima(y("flat_top_odd")).tolist() == [51] and local_maxima(y("flat_top_even")).tolist() == [52]
    assert local_maxima(y("lower_within_separation_dropped")).tolist() == [101, 131]
    assert local_maxima(y("equal_height_earlier_dropped")).tolist() == [101, 131]
    (k, amp, integral, prom, lip, rip), = trace_points(y("prominence_at_limit_kept"), Peaks())
    assert (k, amp, prom) == (102, 120, 20) and (lip, rip) == (100.0 + 1.0 / 20.0, 104.0 - 1.0 / 20.0)
    assert integral == 100 + 3 * 120  # samples 100 .. 103
    wide = staged_peaks(y("width_above_max_dropped"), Peaks(max_width=512.0))
    assert [p[0] for p in wide] == [341] and wide[0][3] - wide[0][2] > 80.0
    (k, amp, integral, prom, lip, rip), = trace_points(y("peak_at_sample_510"), Peaks())
    assert (k, amp, prom, integral) == (510, 150, 80, 80 + 80 + 150) and rip == 511.0 - 4.0 / 80.0
    assert trace_points(y("amplitude_at_threshold_dropped"), Peaks(threshold=39.0))[0][:2] == (51, 40)


def test_peak_settings_are_validated_in_python():
    from attpc_engine_amd.detector.traces import PeakSettings

    assert PeakSettings().token() == tuple(Peaks())
    for bad in ({"separation": 0.5}, {"separation": math.nan}, {"prominence": -1.0}, {"min_width": -0.1},
                {"min_width": 3.0, "max_width": 2.0}, {"max_width": math.nan}, {"rel_height": 0.0},
                {"rel_height": 1.5}, {"threshold": math.nan}):
        with pytest.raises(ValueError):
            PeakSettings(**bad)
    ok = PeakSettings(separation=1.0, prominence=0.0, min_width=0.0, max_width=0.0, rel_height=1.0, threshold=-10.0)
    desc = ok.desc()
    assert (desc.separation, desc.rel_height, desc.threshold) == (1.0, 1.0, -10.0)


def test_spyral_writer_takes_trace_settings_only_with_peaks(tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.detector.simulator import delivery_of
    from attpc_engine_amd.detector.traces import PeakSettings

    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    _, config, _ = workloads.be10dp()
    assert delivery_of(SpyralWriter(tmp_path, config), config)[0] == "rows"
    w = SpyralWriter(tmp_path, config, peaks=PeakSettings(), noise_sigma=5.0, pedestals=100, readout="partial")
    assert delivery_of(w, config)[0] == "trace_rows"
    assert w.trace_kwargs() == {"noise_sigma": 5.0, "pedestals": 100, "readout": "partial"}
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, noise_sigma=5.0)
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, peaks=PeakSettings(), sigma=5.0)
    with pytest.raises(ValueError):
        SpyralWriter(tmp_path, config, peaks=PeakSettings(), readout="everything")
    with pytest.raises(TypeError):
        SpyralWriter(tmp_path, config, 5000, 0, True, PeakSettings())  # keyword only


def _kernel_notes(code_object: Path) -> dict[str, str]:
    text = subprocess.run([str(llvm_tool("llvm-readelf")), "--notes", str(code_object)], capture_output=True, text=True,
                          check=True).stdout
    blocks = {}
    for block in text.split("\n  - .agpr_count:")[1:]:
        for line in block.splitlines():
            if line.strip().startswith(".name:"):
                blocks[line.split(":", 1)[1].strip()] = block
    return blocks


@pytest.mark.skipif(any(llvm_tool(t) is None for t in ("llvm-objdump", "llvm-objcopy", "llvm-readelf")),
                    reason="ROCm LLVM tools not installed")
def test_peak_kernels_round_every_product_use_no_scratch_and_wait_before_barriers():
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(LIB, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            notes.update(_kernel_notes(co))
    needles = ("peak_count_kernel", "peak_write_kernel", "peak_scan_blocks_kernel", "peak_scan_sums_kernel",
               "peak_scan_add_kernel", "peak_event_start_kernel", "peak_rows_kernel")
    kernels = {name: insns for name, insns in functions.items() if any(n in name for n in needles)}
    for needle in needles:
        assert any(needle in name for name in kernels), sorted(functions)
    for name, insns in kernels.items():
        ops = [text.split()[0] for _, text in insns if text]
        if "peak_count_kernel" in name or "peak_write_kernel" in name:
            assert "v_mul_f64" in ops and "v_add_f64" in ops, name  # prominence * rel_height, rounded on its own
        # (the contract's two quotients are long divisions on the mantissa: no hardware division expansion either)
        assert not [o for o in ops if o.startswith(("v_fma_f64", "v_div_fmas_f64"))], name
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert not [o for o in ops if o.startswith(SCALAR_MEMORY_WRITES)], name
        assert ".private_segment_fixed_size: 0" in notes[name], name
        assert not barriers_without_lds_wait(insns), name


def test_new_exports_are_declared_and_bound():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    new = ("attpc_trace_configure_peaks", "attpc_sim_run_trace_rows", "attpc_det_run_trace_rows", "attpc_trace_rows_at",
           "attpc_trace_rows_last")
    for name in new:
        assert re.search(rf"ATTPC_API\s+int32_t\s+{name}\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS
    assert "peaks" in _abi.CONFIGURE_SLOTS
    assert re.search(r"#define ATTPC_ABI_VERSION 3\b", header)
    assert [f for f, _ in _abi.PeakDesc._fields_] == ["separation", "prominence", "min_width", "max_width", "rel_height",
                                                      "threshold"]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "attpc_engine.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(attpc_peak_desc), offsetof(attpc_peak_desc, separation),
  offsetof(attpc_peak_desc, prominence), offsetof(attpc_peak_desc, min_width), offsetof(attpc_peak_desc, max_width),
  offsetof(attpc_peak_desc, rel_height), offsetof(attpc_peak_desc, threshold));
 return 0; }'''
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    assert out == [C.sizeof(_abi.PeakDesc)] + [getattr(_abi.PeakDesc, f).offset for f, _ in _abi.PeakDesc._fields_]
    import __graft_entry__ as entry

    entry.build()
    lib = _abi.load_library()
    for name in new:
        assert getattr(lib, name).restype is C.c_int32
