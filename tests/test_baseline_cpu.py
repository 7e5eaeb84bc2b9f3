"""The Fourier baseline of the trace rows without a GPU: the numpy restatement (tests/baseline_reference.py) against a
direct long-double DFT, its integer peak mask against numpy's float comparison, two rows whose result is known by
hand, the header and the binding, the validation of the Python layer, and the built kernel's private segment and LDS
size as its code object states them."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import baseline_reference as ref
from tests.isa_tools import device_code_objects, llvm_tool

ROOT = Path(__file__).resolve().parent.parent
NEW = ("attpc_trace_configure_baseline", "attpc_trace_baseline")


def _direct_baseline(b: np.ndarray, scale: float) -> np.ndarray:
    """Re(IDFT(DFT(b) F)) of the rows b [R,512] as O(N^2) sums in long double (angles reduced mod 512 first; pi from
    arctan in the wider type, numpy's constant being a double)."""
    n = np.arange(ref.NUM_TB)
    pi = 4 * np.arctan(np.longdouble(1))
    turn = (np.outer(n, n) % ref.NUM_TB).astype(np.longdouble) * (2 * pi / ref.NUM_TB)
    cos, sin = np.cos(turn), np.sin(turn)
    x = b.astype(np.longdouble).T
    re, im = cos @ x, -(sin @ x)
    w = np.where(n < ref.NUM_TB // 2, n, n - ref.NUM_TB).astype(np.longdouble) / np.longdouble(scale)
    f = np.where(w == 0, np.longdouble(1), np.sin(pi * w) / np.where(w == 0, np.longdouble(1), pi * w))[:, None]
    re, im = re * f, im * f
    return ((cos @ re - sin @ im) / ref.NUM_TB).T.astype(np.float64)


def test_restatement_against_a_direct_long_double_dft():
    x = ref.mixed_rows(40, seed=11)
    worst = 0.0
    for scale in (5.0, 20.0, 100.0):
        _, baseline, mask = ref.remove(x, scale)
        b = ref.replaced(ref.edge_fixed(x), mask)
        worst = max(worst, float(np.abs(baseline - _direct_baseline(b, scale)).max()))
    print(f"numpy.fft against the long-double DFT: max |difference| = {worst:.3e}")
    assert worst <= 1.0e-9


def test_integer_mask_against_the_float_comparison():
    x = ref.edge_fixed(ref.mixed_rows(2000, seed=23))
    mask = ref.peak_mask(x)
    xf = x.astype(np.float64)
    floating = xf - xf.mean(axis=1, keepdims=True) > 1.5 * xf.std(axis=1, keepdims=True)
    rows, cols = np.nonzero(mask != floating)
    # a difference is allowed only on a tie, 4 d^2 == 9 (512 Q - S^2), where the float comparison is a rounding away
    s, q = x.sum(axis=1), (x * x).sum(axis=1)
    ties = [(int(r), int(c)) for r, c in zip(rows, cols)
            if 4 * (512 * int(x[r, c]) - int(s[r])) ** 2 == 9 * (512 * int(q[r]) - int(s[r]) ** 2)]
    print(f"integer mask != float mask at {len(rows)} samples, ties among them: {ties}")
    assert len(ties) == len(rows), list(zip(rows.tolist(), cols.tolist()))
    assert mask.any() and not mask.all(axis=1).any()  # (the unmasked set is never empty)


def test_rows_known_by_hand():
    for level in (0, 300, 4095):
        y, baseline, mask = ref.remove(np.full((1, 512), level), 20.0)
        assert not mask.any() and not y.any(), level
        np.testing.assert_allclose(baseline, float(level), rtol=0, atol=1e-9)
    spike = np.zeros((1, 512), dtype=np.int64)
    spike[0, 200] = 4095
    y, baseline, mask = ref.remove(spike, 20.0)
    assert np.flatnonzero(mask[0]).tolist() == [200]
    assert y[0, 200] == 4095 and not np.delete(y[0], 200).any()  # b is all zero: so is the baseline
    # the edge fix is part of x: a spike at sample 0 is overwritten by sample 1 and gone from the result
    edge = np.zeros((1, 512), dtype=np.int64)
    edge[0, 0] = edge[0, 511] = 4095
    assert not ref.remove(edge, 20.0)[0].any()
    edge[0, 1] = 1000
    y = ref.remove(edge, 20.0)[0]
    assert y[0, 0] == y[0, 1] > 0


def test_new_exports_are_declared_and_bound():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in NEW:
        assert re.search(rf"ATTPC_API\s+int32_t\s+{name}\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS and name in _abi.BASELINE_SYMBOLS
    assert "baseline" in _abi.CONFIGURE_SLOTS
    assert re.search(r"#define ATTPC_ABI_VERSION 3\b", header) and _abi.ABI_VERSION == 3
    assert [f for f, _ in _abi.BaselineDesc._fields_] == ["window_scale"]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "attpc_engine.h"
int main(void){ printf("%zu %zu\n", sizeof(attpc_baseline_desc), offsetof(attpc_baseline_desc, window_scale)); return 0; }'''
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    assert out == [C.sizeof(_abi.BaselineDesc), _abi.BaselineDesc.window_scale.offset]
    import __graft_entry__ as entry

    assert "baseline.hip" in entry.HIP_SOURCES
    entry.build()
    lib = _abi.load_library()
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int32
    import attpc_engine_amd.detector as detector

    for name in ("BaselineSettings", "configure_baseline", "remove_baseline"):
        assert name in detector.__all__, name


def test_settings_are_validated():
    from attpc_engine_amd.detector.traces import BaselineSettings, remove_baseline

    assert BaselineSettings().window_scale == 20.0 and BaselineSettings(5).token() == (5.0,)
    assert BaselineSettings(7.5).desc().window_scale == 7.5
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            BaselineSettings(bad)
    # remove_baseline refuses what the library would before it asks for a device
    with pytest.raises(ValueError):
        remove_baseline(np.zeros((2, 512), dtype=np.int16), window_scale=0.0)
    with pytest.raises(ValueError):
        remove_baseline(np.zeros((2, 511), dtype=np.int16))
    with pytest.raises(ValueError):
        remove_baseline(np.full((1, 512), 4096, dtype=np.int16))
    with pytest.raises(ValueError):
        remove_baseline(np.zeros((1, 512)))  # not integers


def test_a_writer_takes_baseline_only_with_peaks(tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.detector.simulator import delivery_of
    from attpc_engine_amd.detector.traces import BaselineSettings, PeakSettings

    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    _, config, _ = workloads.be10dp()
    with pytest.raises(TypeError, match="only with peaks="):
        SpyralWriter(tmp_path, config, baseline=BaselineSettings())
    writer = SpyralWriter(tmp_path, config, peaks=PeakSettings(), baseline=BaselineSettings(30.0))
    assert writer.baseline.window_scale == 30.0 and delivery_of(writer, config)[0] == "trace_rows"
    assert SpyralWriter(tmp_path, config, peaks=PeakSettings()).baseline is None


@pytest.mark.skipif(any(llvm_tool(t) is None for t in ("llvm-objcopy", "llvm-readelf")),
                    reason="ROCm LLVM tools not installed")
def test_the_kernel_has_no_private_segment():
    """The code object's own notes: no scratch, at most 10 KiB of LDS."""
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(entry.LIB, Path(tmp))
        notes = "".join(subprocess.run([str(llvm_tool("llvm-readelf")), "--notes", str(co)], capture_output=True,
                                       text=True, check=True).stdout for co in objects)
    blocks = [b for b in notes.split("\n  - .agpr_count:")[1:] if re.search(r"\.name:\s+\S*baseline_kernel\S*\s", b)]
    assert len(blocks) == 1, len(blocks)
    assert ".private_segment_fixed_size: 0" in blocks[0], blocks[0]
    assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", blocks[0]).group(1)) <= 10240
