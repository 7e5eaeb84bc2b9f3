"""What the rows step of the scatter kernel (csrc/scatter.hip: mirror_weights / mirror_electrons, rows_round) takes
for granted, checked on the CPU: the 10 x 10 pixel weights are the same bit patterns under j <-> 9 - j and i <-> j, so
five products per mesh line give all ten pixel charges; the oracle's own pixels (numpy's pdf at the mesh positions,
not the constant table) show the same mirror; and the line number -> (entry, line) split the kernel does with a
24-bit multiply and a shift is the division it replaces."""
import ctypes as C

import numpy as np
import pytest

from attpc_engine_amd import GasTarget, nuclear_map, workloads
from attpc_engine_amd.detector.beam_pads import BEAM_PADS_ARRAY
from attpc_engine_amd.detector.luts import build_det_desc

MESH = 10


def kernel_weight_table():
    """scatter.hip: wtab[p] = (36/81) / (2 pi) * exp(-(2/9) (di^2 + dj^2)), di = p / 10 - 4.5, dj = p % 10 - 4.5."""
    p = np.arange(MESH * MESH)
    di, dj = (p // MESH).astype(np.float64) - 4.5, (p % MESH).astype(np.float64) - 4.5
    arg = -(2.0 / 9.0) * (di * di + dj * dj)
    return ((36.0 / 81.0) / (2.0 * np.pi) * np.exp(arg)).reshape(MESH, MESH), arg.reshape(MESH, MESH)


def test_weight_table_is_bit_symmetric():
    w, arg = kernel_weight_table()
    bits, arg_bits = w.view(np.uint64), arg.view(np.uint64)
    # the argument of exp is the same bit pattern for j and 9 - j (and for i <-> j): the squares of +-0.5 .. +-4.5 are
    # exact in binary and the sum is commutative
    d = np.arange(MESH, dtype=np.float64) - 4.5
    assert all(float(v * v).hex() == float((-v) * (-v)).hex() and (v * v * 4.0) == round(v * v * 4.0) for v in d)
    np.testing.assert_array_equal(arg_bits, arg_bits[:, ::-1])
    np.testing.assert_array_equal(arg_bits, arg_bits.T)
    np.testing.assert_array_equal(bits, bits[:, ::-1])
    np.testing.assert_array_equal(bits, bits[::-1, :])
    np.testing.assert_array_equal(bits, bits.T)
    # the centre pixels are the largest of every line (the kernel's one test for "fits u32" looks at pixel 4 == 5)
    assert (w.argmax(axis=1) == MESH // 2 - 1).all() and (w[:, MESH // 2 - 1] == w[:, MESH // 2]).all()
    # and the truncated products mirror for any electron count, because the factors do
    rng = np.random.default_rng(7)
    for n in np.concatenate([[1.0, 3_000_001.0, 123_457.0, 5_000_000_007.0], rng.integers(1, 1 << 40, 300).astype(np.float64)]):
        el = (w * n).astype(np.uint64)
        np.testing.assert_array_equal(el, el[:, ::-1])


def test_line_number_split_is_the_division():
    """rows_round: st = (row * 6554) >> 16 with a 24-bit multiply, i = row - 10 st, for every row a staging round can
    hold (STAGE x MESH = 3 200; the identity holds below 16 384, the bound the kernel asserts)."""
    row = np.arange(16384, dtype=np.uint32)
    assert (row * np.uint32(6554)).max() < (1 << 32) and row.max() < (1 << 24)
    st = (row * np.uint32(6554)) >> np.uint32(16)
    np.testing.assert_array_equal(st, row // MESH)
    np.testing.assert_array_equal(row - st * np.uint32(MESH), row % MESH)


@pytest.fixture(scope="module")
def one_pad_per_cell():
    """The default detector with a pad table of its own: every whole-mm cell of a 100 mm square around the centre is
    a pad by itself (none of them a beam pad), so the oracle's dictionary of one sample holds its 100 pixels one by
    one.  -> (descriptor, keepalive, pad id -> (cell x, cell y))"""
    gas = GasTarget([(1, 2, 2)], 300.0, nuclear_map)
    cfg = workloads.detector_config(gas, diffusion=2.77)  # 10x: mesh pitch 3.5 mm at time bucket 100
    desc, keep = build_det_desc(cfg, [nuclear_map.get_data(1, 1)], fold_beam=False)
    n, lo = int(desc.lut_n), int(desc.lut_lo)
    ids = np.setdiff1d(np.arange(16384), BEAM_PADS_ARRAY)[:100 * 100]
    lut = np.full((n, n), -1, dtype=np.int16)
    c0 = -50 - lo  # LUT index of the cell at -50 mm
    lut[c0:c0 + 100, c0:c0 + 100] = ids.reshape(100, 100).astype(np.int16)
    desc.pad_lut = lut.ctypes.data_as(C.POINTER(C.c_int16))
    cell_of = {int(pad): (k // 100, k % 100) for k, pad in enumerate(ids)}
    return desc, (keep, lut), cell_of


def test_oracle_pixels_of_a_sample_mirror(one_pad_per_cell):
    """transverse_transport of the oracle (pdf evaluated at the mesh positions, as the reference does) for a few
    hundred electron counts: the 10 x 10 pixel charges are equal under j <-> 9 - j in both directions, and within
    the project's 2 electrons of the kernel's table x n."""
    from oracle import pyoracle as orc

    desc, keep, cell_of = one_pad_per_cell
    w, _ = kernel_weight_table()
    rng = np.random.default_rng(11)
    counts = np.concatenate([[3_000_001, 123_457, 1, 99], rng.integers(1_000, 40_000_000, 300)]).astype(np.int64)
    worst = 0
    for k, n in enumerate(counts):
        x, y = 1e-3 * (rng.uniform(-8.0, 8.0, 2) if k else np.array([0.3, -0.7]))
        keys, charge, labels = orc.transport(desc, [(np.array([[x, y, 100.5]]), np.array([n], dtype=np.int64), 2)])
        assert len(keys) == MESH * MESH, len(keys)  # every pixel on a pad of its own
        cells = np.array([cell_of[orc.unpair(int(key))[1]] for key in keys])
        order = np.lexsort((cells[:, 1], cells[:, 0]))
        el = charge[order].reshape(MESH, MESH)
        np.testing.assert_array_equal(el, el[:, ::-1], err_msg=f"n = {n}")
        np.testing.assert_array_equal(el, el[::-1, :], err_msg=f"n = {n}")
        worst = max(worst, int(np.abs(el - (w * float(n)).astype(np.int64)).max()))
    print("largest |oracle pixel - table x n|:", worst)
    assert worst <= 2
