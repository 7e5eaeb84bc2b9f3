"""Digitised pad traces, host side (no GPU): the numpy restatement of the contract against the reference's own response
bits, TraceWriter's files through the npz fallback, the C layout of the trace structs against their ctypes mirrors, and
the generated code of the trace kernels (no fused multiply-add, no scratch, no scalar stores)."""
import ctypes as C
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests.isa_tools import _LGKM_OPS, device_code_objects, disassemble_objects, llvm_tool
from tests.trace_reference import event_traces, pad_trace, traces

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
# the scalar-memory classes of tests/isa_tools.py that write (stores, atomics, cache write-back / discard)
SCALAR_MEMORY_WRITES = tuple(p for p in _LGKM_OPS if p.startswith("s_") and not p.startswith(
    ("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_sendmsg")))


def test_one_row_is_the_shifted_clipped_response(golden_dir):
    """A one-row cloud gives rint(min(q R, 4095)) of the reference's response (tests/golden/response.npz), shifted to
    the row's time bucket; the jitter plays no part."""
    resp = np.load(golden_dir / "response.npz")["response"]
    for q, tau, offset in ((1.0, 0.0, 0), (37.0, 100.75, 0), (500.0, 511.5, 0), (3.0e4, 17.2, 0),
                           (12.0, 40.9, int(np.argmax(resp)))):
        t = int(np.floor(tau))
        pads, samples, labels = event_traces(np.array([[77.0, tau, q]]), np.array([5]), resp, -1.0, offset)
        expect = np.zeros(512)
        lo = max(t - offset, 0)
        k = np.arange(lo, 512) + offset - t
        keep = k < 512
        expect[lo:][keep] = q * resp[k[keep]]
        np.testing.assert_array_equal(samples[0], np.rint(np.minimum(expect, 4095.0)).astype(np.int16))
        assert list(pads) == [77] and list(labels) == [5]


def test_restatement_sums_in_ascending_time_and_clips_the_sum():
    resp = np.full(512, 1.0)
    resp[0] = 0.1
    tr = pad_trace(np.array([5, 2]), np.array([3000.0, 2000.0]), resp, 0)
    assert tr[1] == 0 and tr[2] == 200 and tr[4] == 2000 and tr[5] == 2300 and tr[6] == 4095  # pile-up saturates
    assert pad_trace(np.array([0]), np.array([2.5]), np.full(512, 1.0), 0)[0] == 2  # half to even
    _, pads, _, labels, sums = traces([0, 3], np.array([[1, 3.5, 9.0], [1, 7.2, 9.0], [2, 0.0, 1.0]]),
                                      np.array([4, 6, 8]), np.full(512, 1.0), 1.0, 0, first_event=3)
    assert list(pads) == [1] and list(labels) == [4]  # tie on q: the smaller t
    assert sums["pad_checksum"] == (3 << 14) + 1


def test_trace_writer_files_through_the_npz_fallback(tmp_path, monkeypatch):
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import TraceWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    _, config, _ = workloads.be10dp()
    with pytest.warns(RuntimeWarning, match="h5py is not installed"):
        w = TraceWriter(tmp_path, config, max_events_per_file=2, first_run_number=3)
    assert w.threshold == config.elec_params.adc_threshold and w.offset == 0 and w.response.shape == (512,)
    rng = np.random.default_rng(4)
    written = {}
    with pytest.warns(RuntimeWarning):
        for ev in (2, 5, 6):
            n = int(rng.integers(0, 4))
            rows = (np.sort(rng.choice(10240, n, replace=False)).astype(np.int32),
                    rng.integers(0, 4096, size=(n, 512)).astype(np.int16), rng.integers(0, 6, size=n))
            w.write_traces(*rows, ev)
            written[ev] = rows
        w.close()
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["run_0003.npz", "run_0004.npz"]
    f0, f1 = np.load(tmp_path / files[0]), np.load(tmp_path / files[1])
    assert sorted(k for k in f0.files if "@" not in k) == ["trace/labels_2", "trace/labels_5", "trace/pads_2",
                                                          "trace/pads_5", "trace/trace_2", "trace/trace_5"]
    assert sorted(k for k in f1.files if "@" not in k) == ["trace/labels_6", "trace/pads_6", "trace/trace_6"]
    assert (int(f0["trace@min_event"]), int(f0["trace@max_event"])) == (0, 5)
    assert (int(f1["trace@min_event"]), int(f1["trace@max_event"])) == (6, 6)
    for f, run, events in ((f0, 3, (2, 5)), (f1, 4, (6,))):
        for ev in events:
            pads, samples, labels = written[ev]
            assert f[f"trace/trace_{ev}"].dtype == np.int16 and f[f"trace/trace_{ev}"].shape == (len(pads), 512)
            assert f[f"trace/pads_{ev}"].dtype == np.int32 and f[f"trace/labels_{ev}"].dtype == np.int64
            np.testing.assert_array_equal(f[f"trace/trace_{ev}"], samples)
            np.testing.assert_array_equal(f[f"trace/pads_{ev}"], pads)
            np.testing.assert_array_equal(f[f"trace/labels_{ev}"], labels)
            assert int(f[f"trace/trace_{ev}@orig_run"]) == run and int(f[f"trace/trace_{ev}@orig_event"]) == ev


def test_trace_struct_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "attpc_engine.h"
int main(void){
 printf("%zu %zu %zu %zu %zu\n", sizeof(attpc_trace_desc), offsetof(attpc_trace_desc, response),
  offsetof(attpc_trace_desc, adc_threshold), offsetof(attpc_trace_desc, offset), offsetof(attpc_trace_desc, reserved));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(attpc_trace_out), offsetof(attpc_trace_out, capacity),
  offsetof(attpc_trace_out, offsets), offsetof(attpc_trace_out, pads), offsetof(attpc_trace_out, samples),
  offsetof(attpc_trace_out, labels), offsetof(attpc_trace_out, event_points), offsetof(attpc_trace_out, n_rows),
  offsetof(attpc_trace_out, sample_checksum), offsetof(attpc_trace_out, pad_checksum));
 printf("%d %d\n", ATTPC_NUM_PADS, ATTPC_ABI_VERSION);
 return 0; }'''
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    desc = [C.sizeof(_abi.TraceDesc)] + [getattr(_abi.TraceDesc, f).offset for f, _ in _abi.TraceDesc._fields_]
    tout = [C.sizeof(_abi.TraceOut)] + [getattr(_abi.TraceOut, f).offset for f, _ in _abi.TraceOut._fields_]
    assert out == desc + tout + [_abi.NUM_PADS, 3]


def _kernel_notes(code_object: Path) -> dict[str, str]:
    """{kernel symbol: its block of the code object's metadata note}."""
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
def test_trace_kernels_round_every_product_and_use_no_scratch():
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(LIB, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            notes.update(_kernel_notes(co))
    kernels = {name: insns for name, insns in functions.items() if "trace_count_kernel" in name or "trace_write_kernel" in name}
    assert any("trace_count_kernel" in n for n in kernels) and any("trace_write_kernel" in n for n in kernels), sorted(functions)
    for name, insns in kernels.items():
        ops = [text.split()[0] for _, text in insns if text]
        assert "v_mul_f64" in ops and "v_add_f64" in ops, name  # the products are there, rounded on their own
        assert not [o for o in ops if o.startswith("v_fma_f64")], name
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert not [o for o in ops if o.startswith(SCALAR_MEMORY_WRITES)], name
        meta = notes[name]
        assert ".private_segment_fixed_size: 0" in meta, name
