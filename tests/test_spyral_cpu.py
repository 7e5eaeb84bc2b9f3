"""The fused Spyral rows, host side (no GPU): the numpy restatement (tests/spyral_reference.py) against the rows the
reference's own code made (tests/golden/response.npz) and against the CPU oracle's convert_to_spyral from zero charge to
full saturation; the condition that gives the GPU test's tolerance its meaning (on the charges of the runs it drives, the
reference's sequential f64 sum is within 1e-13 of the exact sum, so 1e-12 against the exact sum asks no more than 1e-12
against the reference's loop); the closed form the kernels evaluate (csrc/spyral_integral.hpp) in a stand-alone program
against a long double sum; and the runs of tests/spyral_cases.py checked, on the oracle's clouds, to reach what the GPU
test needs of them."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import GasTarget, _abi, nuclear_map
from attpc_engine_amd.workloads import detector_config
from tests import spyral_cases as cases
from tests.helpers import Inputs
from tests.spyral_reference import (Geometry, clipped_count, convert, fused_rows, integral_exact, integral_sequential,
                                    z_mm)

ROOT = Path(__file__).resolve().parents[1]
OTHER_COLUMNS = [0, 1, 2, 3, 5, 6, 7]


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def config():
    return detector_config(GasTarget([(1, 2, 2)], 300.0, nuclear_map))


def _relative(got, want):
    """max |got - want| / |want|; a zero must be met exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0.0
    assert (got[zero] == 0.0).all()
    return float((np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])).max(initial=0.0))


def test_restatement_against_the_reference_rows(golden_dir, config):
    g = np.load(golden_dir / "response.npz")
    rows = convert(g["points"], g["response"], Geometry.of(config))
    np.testing.assert_allclose(rows[:, OTHER_COLUMNS], g["rows"][:, OTHER_COLUMNS], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rows[:, 4], g["rows"][:, 4], rtol=1e-12, atol=0)
    sequential = integral_sequential(g["response"], g["points"][:, 2])
    np.testing.assert_allclose(sequential, g["rows"][:, 4], rtol=1e-12, atol=0)
    k = clipped_count(g["response"], g["points"][:, 2])
    assert k.min() == 0 and k.max() > 0  # the reference's rows hold unclipped and clipped signals


def test_restatement_against_the_oracle_from_zero_charge_to_saturation(orc, config):
    """A hand-made cloud: charges 0, 1 and 600 log-spaced values up to 1e16 (whole numbers, as in a cloud), pads over the
    plane, time buckets over the window.  k runs from 0 to the largest value the response allows at 1e16."""
    geo = Geometry.of(config)
    response = cases.responses(config)["default"]
    rng = np.random.default_rng(5)
    q = np.concatenate([[0.0, 1.0], np.floor(10.0 ** np.linspace(0.0, 16.0, 600)), [1e16]])
    n = len(q)
    pts = np.ascontiguousarray(np.column_stack([rng.integers(0, len(geo.pad_sizes), n).astype(np.float64),
                                                rng.uniform(0.0, 512.0, n), q]))
    want = np.empty((n, 8))
    orc.lib().orc_convert_to_spyral(_abi.dptr(pts), n, geo.windows_edge, geo.micromegas_edge, geo.length,
                                    _abi.dptr(response), _abi.dptr(np.ascontiguousarray(geo.pad_centers)),
                                    _abi.dptr(np.ascontiguousarray(geo.pad_sizes)), _abi.dptr(want))
    rows = convert(pts, response, geo)
    np.testing.assert_array_equal(rows[:, OTHER_COLUMNS], want[:, OTHER_COLUMNS])  # (well inside the rtol of 1e-12)
    np.testing.assert_allclose(rows[:, 4], want[:, 4], rtol=1e-12, atol=0)
    np.testing.assert_allclose(integral_sequential(response, q), want[:, 4], rtol=1e-15, atol=0)  # the same loop
    k = clipped_count(response, q)
    largest = int((response * 1e16 > 4095.0).sum())  # (36 of the default response's 255 samples above zero)
    assert k[0] == 0 and k.max() == largest >= 30 and len(np.unique(k)) > largest // 2
    assert rows[0, 3] == 0.0 and rows[0, 4] == 0.0 and rows[-1, 3] == 4095.0


def test_restatement_threshold_and_order(config):
    """The restatement's own decisions on a cloud small enough to read: strict threshold, descending time bucket,
    equal time buckets in cloud order, event_points before the threshold, an event that keeps nothing."""
    geo = Geometry.of(config)
    response = cases.responses(config)["single"]  # amplitude = integral = r q
    r = float(response.max())
    q = [1e6, 2e6, 3e6, 2e6, 1e6, 5e6, 1e6]
    tb = [10.5, 300.25, 300.25, 20.0, 400.0, 7.0, 8.0]
    pts = np.column_stack([np.arange(7.0), tb, q])
    labels = np.arange(7) + 10
    out = fused_rows([0, 5, 5, 6, 7], pts, labels, response, geo, threshold=r * 1e6)
    np.testing.assert_array_equal(out.offsets, [0, 3, 3, 4, 4])
    np.testing.assert_array_equal(out.event_points, [5, 0, 1, 1])
    np.testing.assert_array_equal(out.labels, [11, 12, 13, 15])  # 300.25 twice: cloud order; then 20.0; event 2
    np.testing.assert_array_equal(out.rows[:, 3], out.rows[:, 4])
    np.testing.assert_array_equal(out.rows[:, 2], z_mm(np.array([300.25, 300.25, 20.0, 7.0]), geo))
    assert fused_rows([0, 7], pts, labels, response, geo, threshold=-1.0).offsets[-1] == 7


def _oracle_cloud(orc, run, gain):
    name, first, n = run
    inp = Inputs(cases.builder(name, gain))
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=cases.SEED, first=first, n=n, capacity=1 << 22, threads=8)
    return inp, ref["offsets"], ref["points"], ref["labels"]


def test_sequential_sum_within_1e13_of_the_exact_sum_on_the_charges_of_the_gpu_runs(orc, config):
    """Default and bipolar response, every charge of the oracle's clouds of the runs the GPU test drives (the device's
    charges are the oracle's to within two units of the gain's rounding; the GPU test repeats this on its own clouds,
    the two 50 k-row events of the crowded sort included, which are left out here for their time).  The bipolar response
    at a gain of 1e11 is close to the bound wherever one looks (8e-14 .. 2e-13 per event over ten seeds: its clipped sum
    changes sign at q = 3.9e10); tests/spyral_cases.py names events that keep it (9.2e-14)."""
    responses = cases.responses(config)
    worst = {}
    for run, gains, names in ((cases.SWEEP, cases.GAINS, ("default",)), (cases.RESPONSES, (cases.GAINS[0], cases.GAINS[2]), ("default", "bipolar")),
                              (cases.THRESHOLDS, (cases.LOW_GAIN,), ("default",))):
        for gain in gains:
            q = np.unique(_oracle_cloud(orc, run, gain)[2][:, 2])
            for name in names:
                err = _relative(integral_sequential(responses[name], q), integral_exact(responses[name], q))
                worst[name] = max(worst.get(name, 0.0), err)
    print("sequential f64 sum against the exact sum, worst relative error:", worst)
    assert worst["default"] <= 1e-13 and worst["bipolar"] <= 1e-13


def test_runs_of_the_gpu_test_reach_their_regimes_on_the_oracle(orc, config):
    """What tests/test_gpu_spyral_edges.py asserts of its own clouds, seen here on the oracle's clouds of the same runs,
    so that a change of a workload shows on this machine first."""
    response = cases.responses(config)["default"]
    # gain sweep: partly clipped rows with q >= 1e13 at 1e11, at least 10 values of k over the sweep
    ks = set()
    for gain in cases.GAINS:
        q = _oracle_cloud(orc, cases.SWEEP, gain)[2][:, 2]
        k = clipped_count(response, q)
        ks |= set(k.tolist())
        if gain == cases.GAINS[2]:
            assert ((q >= 1e13) & (k > 0) & (k < 512)).sum() >= 100
    assert len(ks) >= 10
    # thresholds: rows of zero charge, an event of 300 rows, events emptied between events that keep rows
    _, offsets, points, _ = _oracle_cloud(orc, cases.THRESHOLDS, cases.LOW_GAIN)
    amp = np.minimum(response.max() * points[:, 2], 4095.0)
    assert (points[:, 2] == 0.0).sum() > 0 and np.diff(offsets).max() >= 300
    top = np.array([amp[lo:hi].max(initial=0.0) for lo, hi in zip(offsets[:-1], offsets[1:])])
    kept = np.array([(amp[lo:hi] > np.median(top)).sum() for lo, hi in zip(offsets[:-1], offsets[1:])])
    filled = np.flatnonzero(kept > 0)
    assert (kept == 0).sum() >= 2 and len(filled) >= 2 and (kept[filled[0]:filled[-1]] == 0).any()
    # crowded sort: a (time bucket, sixteenth) bin of 32 rows in either event
    _, offsets, points, _ = _oracle_cloud(orc, cases.CROWDED, cases.GAINS[0])
    fullest = [int(np.bincount(cases.sort_bins(points[lo:hi, 1])).max()) for lo, hi in zip(offsets[:-1], offsets[1:])]
    print("fullest sort bin per event (oracle):", fullest, "rows", np.diff(offsets))
    assert min(fullest) >= 32


def test_closed_form_of_the_integral_against_a_long_double_sum(tmp_path, config):
    """csrc/spyral_integral.hpp, the tables and the evaluation the kernels use, in tests/native/spyral_integral_check.cpp
    on the four responses of tests/spyral_cases.py: worst relative error at most 1e-12 over 1e0 .. 1e16 and the charges
    either side of every sample's clip."""
    exe, data = tmp_path / "spyral_integral_check", tmp_path / "responses.f64"
    responses = cases.responses(config)
    np.stack([responses[name] for name in ("default", "bipolar", "flat", "single")]).astype("<f8").tofile(data)
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}", "-o", str(exe),
                    str(ROOT / "tests" / "native" / "spyral_integral_check.cpp")], check=True)
    proc = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    lines = [line for line in proc.stdout.splitlines() if line.startswith("response ")]
    assert len(lines) == 4
    for line in lines:
        assert int(line.split("n=")[1].split()[0]) > 1600 and float(line.split("worst=")[1].split()[0]) <= 1e-12, line


def test_engine_forwards_a_response_to_the_spyral_stage():
    from attpc_engine_amd import workloads
    from attpc_engine_amd.engine import Engine
    from tests.test_run_layer_cpu import RecordingContext

    pipeline, config, indices = workloads.be10dp()  # (its tables are built already: the runs above)
    engine = Engine(pipeline, config, indices, context=RecordingContext())
    lib = engine.ctx.lib
    lib.calls.clear()
    engine.configure_spyral()
    engine.configure_spyral(response=cases.responses(config)["default"])  # the default, spelled out: the same content
    engine.configure_spyral(response=cases.responses(config)["bipolar"])
    engine.configure_spyral(config, response=cases.responses(config)["bipolar"])
    engine.configure_spyral()
    assert lib.names() == ["spyral_configure"] * 3
