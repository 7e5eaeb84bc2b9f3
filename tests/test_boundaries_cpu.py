"""The oracle at the scatter's rounding edges: samples built by tests/boundary_cases.py to put one mesh line or slice
time within a few ulp of a whole-mm cell edge or a time-bucket edge, against the reference's own transport of the same
samples (tests/golden/boundary.npz).  Also shows that these cases have teeth: the fused-multiply-add rounding a
compiler contracts ``a * b + c`` into changes every mesh case, and an oracle built with contraction fails here.  CPU
only; the device side is tests/test_gpu_boundaries.py."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd.detector.luts import build_det_desc, longitudinal_weights
from oracle import pyoracle as orc
from tests import boundary_cases as bc
from tests.test_oracle_golden import _golden_det

ROOT = Path(__file__).resolve().parents[1]
MESH_GROUPS = ("mesh", "mesh10", "mesh_lone")      # class A, every sample changed by fused rounding
REF_GROUPS = MESH_GROUPS + ("lut_edge", "time", "far")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "boundary.npz")


def reference_sample(fx, group, i):
    o = fx[f"{group}_offsets"]
    s = slice(o[i], o[i + 1])
    return fx[f"{group}_keys"][s], fx[f"{group}_charge"][s], fx[f"{group}_labels"][s]


def _mismatch(got, want) -> str | None:
    keys, charge, labels = got
    r_keys, r_charge, r_labels = want
    if not np.array_equal(keys, r_keys):
        return "keys"
    if not np.array_equal(labels, r_labels):
        return "labels"
    if not np.array_equal(charge == 0, r_charge == 0):
        return "zero-charge pattern"
    if len(charge) and np.abs(charge - r_charge).max() > 2:
        return f"charge off by {int(np.abs(charge - r_charge).max())}"
    return None


def test_fixture_holds_the_promised_cases(fx):
    mesh = np.concatenate([fx[f"{g}_meta"] for g in MESH_GROUPS])
    assert len(mesh) >= 150
    for axis in (0, 1):
        on_axis = mesh[mesh[:, 0] == axis]
        assert set(on_axis[:, 1].tolist()) >= {0, 2, 4, 6, 7, 8, 9}, sorted(set(on_axis[:, 1].tolist()))
    xyt = np.concatenate([fx[f"{g}_xyt"] for g in MESH_GROUPS])
    u = np.where(mesh[:, 0] == 0, xyt[:, 0], xyt[:, 1])
    assert (u > 0).sum() >= 30 and (u < 0).sum() >= 30  # both signs of the coordinate on the edge
    assert (np.floor(fx["mesh_lone_xyt"][:, 2]) == 500).all()
    assert len(fx["slice_xyt"]) >= 30 and (fx["slice_meta"][:, 1] == 0).any()
    assert (fx["far_offsets"] == 0).all()  # far off the plane: no points in the reference either


@pytest.mark.parametrize("group", REF_GROUPS)
def test_oracle_vs_reference_at_decision_boundaries(fx, group):
    """Keys (insertion order) and labels exact, zero charges where the reference has them, charges within 2."""
    det, keep = _golden_det(None, diffusion=float(fx[f"{group}_diffusion"]))
    xyt, electrons = fx[f"{group}_xyt"], fx[f"{group}_electrons"]
    bad = []
    for i in range(len(xyt)):
        got = orc.transport(det, [(xyt[i][None], electrons[i:i + 1], bc.LABEL)])
        why = _mismatch(got, reference_sample(fx, group, i))
        if why:
            bad.append((i, why))
    assert not bad, f"{group}: {len(bad)} of {len(xyt)} samples differ from the reference, e.g. {bad[:5]}"


def test_negative_times_give_nothing_in_the_oracle():
    """t < 0 is undefined behaviour in the reference (deviation ii); the oracle and the device drop
    the sample -- also at t = -5e-324, where sigma_t^2 underflows to -0 instead of giving NaN."""
    det, keep = _golden_det(None)
    xyt, electrons = bc.time_edge_cases(negative=True)
    for row, el in zip(xyt, electrons):
        keys, _, _ = orc.transport(det, [(row[None], np.array([el]), bc.LABEL)])
        assert len(keys) == 0, row


@pytest.mark.parametrize("group", REF_GROUPS)
def test_numpy_order_emulation_reproduces_the_reference(fx, group):
    """The host emulation rounds as numpy does: it gives the reference's keys (and charges within 2), so the
    fused emulation below differs from the reference by its rounding alone."""
    det = bc.Detector(float(fx[f"{group}_diffusion"]))
    xyt, electrons = fx[f"{group}_xyt"], fx[f"{group}_electrons"]
    for i in range(len(xyt)):
        pts = bc.transport(det, *xyt[i], int(electrons[i]))
        got = (np.array(list(pts), dtype=np.int64), np.array([v[0] for v in pts.values()], dtype=np.int64),
               np.array([v[1] for v in pts.values()], dtype=np.int64))
        assert _mismatch(got, reference_sample(fx, group, i)) is None, (group, i)


@pytest.mark.parametrize("group", MESH_GROUPS)
def test_fused_rounding_changes_every_mesh_case(fx, group):
    """Teeth: one rounding per a * b + c (a contracted build) changes the key set of every class-A sample."""
    det = bc.Detector(float(fx[f"{group}_diffusion"]))
    xyt, electrons = fx[f"{group}_xyt"], fx[f"{group}_electrons"]
    for i in range(len(xyt)):
        ref_keys = set(reference_sample(fx, group, i)[0].tolist())
        assert set(bc.transport(det, *xyt[i], int(electrons[i]), fused=True)) != ref_keys, (group, i)


def _long_det(longitudinal_diffusion):
    from attpc_engine_amd import GasTarget, nuclear_map, workloads

    cfg = workloads.detector_config(GasTarget([(1, 2, 2)], 300.0, nuclear_map), diffusion=0.277)
    cfg.det_params.longitudinal_diffusion = longitudinal_diffusion
    return build_det_desc(cfg, [nuclear_map.get_data(1, 1)], fold_beam=False)


def test_slice_buckets_at_their_edges_oracle(fx):
    """Class B (longitudinal extension, no reference counterpart): the oracle's charge per time bucket is that of
    the slices numpy-order arithmetic puts there (weight x the sample's charge); fused arithmetic moves a slice to
    another bucket (or across t = 0 / 512) in every case."""
    det_l, keep = _long_det(bc.LONG_DIFFUSION)
    det_0, keep_0 = _long_det(0.0)
    emu = bc.Detector(0.277)
    w = longitudinal_weights()
    xyt, electrons = fx["slice_xyt"], fx["slice_electrons"]
    assert fx["slice_longitudinal_diffusion"] == bc.LONG_DIFFUSION
    for row, el in zip(xyt, electrons):
        keys, charge, _ = orc.transport(det_l, [(row[None], np.array([el]), bc.LABEL)])
        tb = np.array([orc.unpair(int(k))[0] for k in keys], dtype=np.int64)
        by_tb = {int(t): int(charge[tb == t].sum()) for t in np.unique(tb)}
        q = int(orc.transport(det_0, [(row[None], np.array([el]), bc.LABEL)])[1].sum())  # the sample, unsliced
        for fused in (False, True):
            share: dict = {}
            for sl, ts in enumerate(bc.slice_times(emu, row[2], fused)):
                if ts >= 0.0:
                    share[int(ts)] = share.get(int(ts), 0.0) + w[sl]
            ok = set(share) == set(by_tb) and all(abs(by_tb[t] - share[t] * q) <= 1e-4 * q for t in share)
            assert ok != fused, (row.tolist(), fused, by_tb, share)


def test_slice_cases_change_under_fused_rounding(fx):
    emu = bc.Detector(0.277)
    for t in fx["slice_xyt"][:, 2]:
        assert bc.slice_buckets(emu, t, False) != bc.slice_buckets(emu, t, True), t


@pytest.mark.timeout(300)
def test_contracted_oracle_fails_the_boundary_fixture(tmp_path):
    """Mutation: the oracle's source built with -ffp-contract=fast -mfma (every a * b + c one FMA) must fail
    test_oracle_vs_reference_at_decision_boundaries -- the cases catch a build that rounds like a contracted kernel."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    if "fma" not in Path("/proc/cpuinfo").read_text().split():
        pytest.skip("the CPU has no FMA instructions")
    lib = tmp_path / "libattpc_oracle_fma.so"
    made = subprocess.run([gcc, "-O2", "-fPIC", "-fopenmp", "-ffp-contract=fast", "-mfma", "-fno-fast-math", "-std=c11",
                           "-shared", "-o", str(lib), str(ROOT / "oracle" / "attpc_oracle.c"), "-lm"],
                          capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    objdump = shutil.which("objdump")
    if objdump is None:
        pytest.skip("objdump not available")
    asm = subprocess.run([objdump, "-d", str(lib)], capture_output=True, text=True).stdout
    if "vfmadd" not in asm and "vfmsub" not in asm and "vfnmadd" not in asm:
        pytest.skip("the contracted build holds no FMA instruction")
    env = dict(os.environ, ATTPC_ORACLE_LIBRARY=str(lib), OMP_NUM_THREADS="4")
    run = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_boundaries_cpu.py"), "-q",
                          "-p", "no:cacheprovider", "-k", "test_oracle_vs_reference_at_decision_boundaries"],
                         capture_output=True, text=True, env=env, cwd=str(ROOT))
    tail = run.stdout[-3000:] + run.stderr[-2000:]
    assert run.returncode == 1, tail  # tests ran and failed (not a collection error)
    assert "samples differ from the reference" in run.stdout, tail
    failed = [g for g in MESH_GROUPS if f"FAILED tests/test_boundaries_cpu.py::test_oracle_vs_reference_at_decision_boundaries[{g}]" in run.stdout]
    print("contracted oracle fails on", failed, run.stdout[-1500:])
    assert failed, tail


# the +-3.0 of c -+ 3 sigma and the line / slice indices above the inline constants (5.0 .. 8.0): literals an FMA of the
# mesh or slice arithmetic would carry
FUSED_LITERALS = ("0x40080000", "0xc0080000", "0x40140000", "0x40180000", "0x401c0000", "0x40200000")


def test_no_fused_mesh_or_slice_arithmetic_in_the_scatter_kernels():
    """The shipped library's scatter builds and lone kernel hold no v_fma_f64 / v_fmac_f64 on those literals (the
    parent library had 226: mul_add_rn, common.hpp)."""
    from tests.isa_tools import disassemble, llvm_tool

    if llvm_tool("llvm-objdump") is None or llvm_tool("llvm-objcopy") is None:
        pytest.skip("ROCm LLVM tools not installed")
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as entry

    entry.build()
    functions = disassemble(ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so")
    kernels = {n: i for n, i in functions.items() if "scatter_kernel" in n or "lone_bucket_kernel" in n}
    assert len(kernels) >= 8, sorted(functions)
    fused = {n: [t for _, t in insns if t.startswith(("v_fma_f64", "v_fmac_f64")) and any(c in t for c in FUSED_LITERALS)]
             for n, insns in kernels.items()}
    assert not any(fused.values()), {n: v[:3] for n, v in fused.items() if v}
