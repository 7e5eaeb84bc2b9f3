"""Electronic noise and pedestals of the pad traces, host side (no GPU): the numpy Philox against the CPU oracle and the
published known-answer vectors, the Gaussian noise table, the restatement of the contract on hand-computed cases and,
with noise off, against the noiseless restatement, the Python-side validation, and the C layout of
attpc_trace_noise_desc against its ctypes mirror."""
import ctypes as C
import math
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.traces import NoiseSettings, gaussian_noise_table
from tests import trace_reference
from tests.trace_noise_reference import Noise, level_masses, philox4x32_10, traces

ROOT = Path(__file__).resolve().parents[1]
ONES = 0xFFFFFFFF


def _philox(ctr, key):
    return [int(v) for v in philox4x32_10(*ctr, *key)]


def test_numpy_philox_matches_known_answers():
    """Random123 kat_vectors for philox4x32-10."""
    assert _philox([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert _philox([ONES] * 4, [ONES] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_numpy_philox_matches_the_oracle():
    from oracle import pyoracle as orc

    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(10000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(10000, 2), dtype=np.uint64)
    ctr[:50] = ONES  # all ones, high words included
    key[:50] = ONES
    ctr[50:100, 3] = 0x80000000 | rng.integers(0, 1 << 31, size=50, dtype=np.uint64)  # the noise domain
    got = np.stack(philox4x32_10(*ctr.T, *key.T), axis=1)
    for i in range(len(ctr)):
        assert list(got[i]) == list(orc.philox(ctr[i], key[i])), i


@pytest.mark.parametrize("sigma", [0.5, 1.0, 3.7, 12.0, 31.0])
def test_gaussian_noise_table(sigma):
    cdf, min_level = gaussian_noise_table(sigma)
    half = math.ceil(8 * sigma)
    assert cdf.dtype == np.uint32 and cdf.size == 2 * half and min_level == -half
    assert np.all(np.diff(cdf.astype(np.int64)) >= 0)
    p = level_masses(cdf, cdf.size + 1)
    np.testing.assert_array_equal(p, p[::-1])  # symmetric levels
    levels = np.arange(-half, half + 1, dtype=np.float64)
    assert abs(float(p @ levels)) < 1e-6
    # the exact discretised variance: masses of rint(sigma z) with the tails folded into the end levels
    phi = [0.5 * math.erfc(-(m + 0.5) / (sigma * math.sqrt(2.0))) for m in range(-half, half)]
    exact = np.diff(np.concatenate([[0.0], phi, [1.0]]))
    var = float(p @ levels ** 2)
    want = float(exact @ levels ** 2)
    assert abs(var - want) <= 1e-4 * want, (var, want)
    assert abs(want - (sigma ** 2 + 1 / 12)) < 0.02 * sigma ** 2 + 0.05  # (Sheppard: close to sigma^2 + 1/12)


def test_gaussian_noise_table_off_and_limits():
    cdf, min_level = gaussian_noise_table(0.0)
    assert cdf.size == 0 and min_level == 0
    assert NoiseSettings(0.0).n_levels == 0 and not NoiseSettings(0.0).on
    with pytest.raises(ValueError):
        gaussian_noise_table(32.0)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            gaussian_noise_table(bad)


def _hand_made():
    rng = np.random.default_rng(5)
    resp = np.zeros(512)
    resp[:40] = np.exp(-0.5 * ((np.arange(40) - 12) / 4.0) ** 2)
    rows = [[3.0, 10.5, 800.0], [3.0, 40.2, 300.0], [9.0, 100.0, 5000.0], [4000.0, 500.9, 60.0], [12.0, 7.0, 0.0]]
    points = np.array(rows)
    offsets = np.array([0, 3, 3, 5])
    labels = rng.integers(0, 5, size=len(points))
    return offsets, points, labels, resp


@pytest.mark.parametrize("threshold", [-1.0, 0.0, 40.0])
def test_noise_off_is_the_noiseless_restatement(threshold):
    offsets, points, labels, resp = _hand_made()
    want = trace_reference.traces(offsets, points, labels, resp, threshold, 0, first_event=9)
    got = traces(offsets, points, labels, resp, threshold, 0, Noise(), seed=123, first_event=9)
    for a, b in zip(got[:4], want[:4]):
        np.testing.assert_array_equal(a, b)
    assert got[4] == want[4]
    # an empty table with min_level 0 and pedestals all 0: the same numbers
    got = traces(offsets, points, labels, resp, threshold, 0, Noise((), 0, n_levels=1, pedestals=np.zeros(10240)),
                 seed=123, first_event=9)
    np.testing.assert_array_equal(got[2], want[2])


def test_hand_computed_clip_and_threshold_above_pedestal():
    resp = np.zeros(512)
    resp[0] = 1.0
    ped = np.zeros(10240, dtype=np.int16)
    ped[1], ped[2], ped[3] = 4090, 20, 50
    # a one-level table: n = min_level for every sample
    pts = np.array([[1.0, 5.0, 3.0], [2.0, 5.0, 10.0], [3.0, 5.0, 40.0]])
    off, pads, samples, _, _ = traces([0, 3], pts, np.array([1, 2, 3]), resp, 30.0, 0,
                                      Noise((), 2, pedestals=ped), seed=1)
    # pad 1: 4090 + 3 + 2 clips at 4095 at j = 5, elsewhere 4092; max - ped = 5 <= 30: dropped
    # pad 2: 20 + 10 + 2 = 32 at j = 5, max - ped = 12: dropped although 32 > 30
    # pad 3: 50 + 40 + 2 = 92, max - ped = 42 > 30: kept
    assert pads.tolist() == [3]
    assert samples[0, 5] == 92 and samples[0, 0] == 52
    off, pads, samples, _, _ = traces([0, 3], pts, np.array([1, 2, 3]), resp, -1.0, 0, Noise((), 2, pedestals=ped), seed=1)
    assert pads.tolist() == [1, 2, 3]
    assert samples[0, 5] == 4095 and samples[0, 0] == 4092 and samples[1, 5] == 32
    # the clip at 0: a negative noise level below a zero pedestal
    off, pads, samples, _, _ = traces([0, 1], pts[1:2], np.array([2]), resp, -1.0, 0, Noise((), -7), seed=1)
    assert samples[0, 5] == 3 and samples[0, 0] == 0 and samples[0].min() == 0


def test_table_lookup_is_searchsorted_right():
    noise = Noise(np.array([0, 10, 10, 1 << 31, ONES], dtype=np.uint32), -2)
    u = noise.uniforms(7, 3, [5, 6])
    n = noise.values(7, 3, [5, 6])
    want = -2 + (u >= 0).astype(int) + 2 * (u >= 10) + (u >= 1 << 31) + (u >= ONES)
    np.testing.assert_array_equal(n, want)
    # the draw of sample j: word (j // 64) % 4 of counter (e, pad * 128 + 2 (j % 64) + j // 256)
    for j in (0, 63, 64, 255, 256, 300, 511):
        out = philox4x32_10(3, 0, 5 * 128 + 2 * (j % 64) + j // 256, 0x80000000, 7, 0)
        assert int(u[0, j]) == int(out[(j // 64) % 4])


def test_python_validation():
    cdf, lo = gaussian_noise_table(2.0)
    for kw in ({"pedestals": np.full(10240, -1)}, {"pedestals": np.full(10240, 4096)}, {"pedestals": np.zeros(5)},
               {"pedestals": np.full(10240, 1.5)}, {"noise_table": (cdf[::-1], lo)},
               {"noise_table": (np.arange(512, dtype=np.uint32), 0)}, {"noise_table": (cdf, 4096)},
               {"noise_table": (np.array([-1, 3]), 0)}, {"noise_stream": 1 << 31}, {"noise_stream": -1},
               {"noise_sigma": 1.0, "noise_table": (cdf, lo)}):
        with pytest.raises(ValueError):
            NoiseSettings(**kw)
    ok = NoiseSettings(noise_table=(np.arange(511, dtype=np.uint32), -4095), pedestals=4095, noise_stream=(1 << 31) - 1)
    assert ok.n_levels == 512 and ok.pedestals.shape == (10240,) and ok.pedestals.dtype == np.int16
    assert math.isnan(ok.sigma)


def test_trace_writer_records_noise_only_when_set(tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import TraceWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    _, config, _ = workloads.be10dp()
    rows = (np.array([3], dtype=np.int32), np.full((1, 512), 7, dtype=np.int16), np.array([1]))
    plain, noisy = tmp_path / "plain", tmp_path / "noisy"
    plain.mkdir()
    noisy.mkdir()
    w = TraceWriter(plain, config)
    w.write_traces(*rows, 0)
    w.close()
    ped = np.arange(10240) % 100
    w = TraceWriter(noisy, config, noise_sigma=3.0, pedestals=ped, noise_stream=4, noise_seed=99)
    w.write_traces(*rows, 0)
    w.close()
    f0, f1 = np.load(plain / "run_0000.npz"), np.load(noisy / "run_0000.npz")
    assert not [k for k in f0.files if "noise" in k or "pedestal" in k]
    assert int(f1["trace@noise_stream"]) == 4 and float(f1["trace@noise_sigma"]) == 3.0
    cdf, lo = gaussian_noise_table(3.0)
    assert int(f1["trace@noise_min_level"]) == lo
    np.testing.assert_array_equal(f1["trace/noise_cdf"], cdf)
    np.testing.assert_array_equal(f1["trace/pedestals"], ped)
    assert w.noise_kwargs()["noise_stream"] == 4 and w.noise_seed == 99


def test_trace_noise_struct_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "attpc_engine.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(attpc_trace_noise_desc), offsetof(attpc_trace_noise_desc, cdf),
  offsetof(attpc_trace_noise_desc, n_levels), offsetof(attpc_trace_noise_desc, min_level),
  offsetof(attpc_trace_noise_desc, pedestals), offsetof(attpc_trace_noise_desc, stream),
  offsetof(attpc_trace_noise_desc, reserved));
 printf("%d\n", ATTPC_MAX_NOISE_LEVELS);
 return 0; }'''
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    desc = [C.sizeof(_abi.TraceNoiseDesc)] + [getattr(_abi.TraceNoiseDesc, f).offset for f, _ in _abi.TraceNoiseDesc._fields_]
    assert out == desc + [_abi.MAX_NOISE_LEVELS]
