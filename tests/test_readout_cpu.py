"""Readout of noise-only pads without a GPU: the decision rule the kernels use against the brute-force maximum of the
contract, ``expected_noise_pads`` against a Monte-Carlo of the numpy restatement (tests/readout_reference.py), the
restatement's own consistency, the Python-side validation, TraceWriter's records, and the C layout of
attpc_trace_readout_desc."""
import math
import subprocess
import tempfile
from pathlib import Path

import ctypes as C
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.beam_pads import BEAM_PADS
from attpc_engine_amd.detector.traces import (ReadoutSettings, configure_traces, expected_noise_pads,
                                              gaussian_noise_table, readout_cutoff, readout_mask)
from tests.readout_reference import FULL, PARTIAL, traces, uniforms, values
from tests.trace_noise_reference import Noise

ROOT = Path(__file__).resolve().parents[1]


def _rule(u, ped, thr, cdf, min_level):
    """The decision rule of include/attpc_engine.h for draws u [K, 512] of pads with pedestals ped [K]."""
    kind, cut = readout_cutoff(cdf, min_level, thr)
    crosses = {"always": np.ones(len(u), dtype=bool), "never": np.zeros(len(u), dtype=bool)}.get(kind)
    if crosses is None:
        crosses = (u >= cut).any(axis=1)
    return (4095 - ped > thr) & ((-ped > thr) | crosses)


def _brute(u, ped, thr, cdf, min_level):
    """max_j (trace_p[j] - ped_p) > thr with s_p = 0, trace = clip(ped + n, 0, 4095)."""
    n_levels = cdf.size + 1 if (cdf.size or min_level) else 0
    if n_levels == 0:
        n = np.zeros(u.shape, dtype=np.int64)
    else:
        n = min_level + np.searchsorted(cdf.astype(np.uint64), u.astype(np.uint64), side="right").astype(np.int64)
    trace = np.clip(ped[:, None] + n, 0, 4095)
    return (trace - ped[:, None]).max(axis=1) > thr


def _draws(rng, cdf, k):
    """u [k, 512]: uniform draws, plus rows that sit on, just below and just above every cdf entry and at the ends."""
    u = rng.integers(0, 1 << 32, size=(k, 512), dtype=np.uint64)
    edges = np.unique(np.concatenate([cdf.astype(np.int64) + d for d in (-1, 0, 1)] + [np.array([0, (1 << 32) - 1])]))
    edges = edges[(edges >= 0) & (edges < 1 << 32)]
    for i, v in enumerate(edges):  # one edge value in a row of low draws
        row = i % k
        u[row] = rng.integers(0, 1 << 20, size=512)
        u[row, i % 512] = v
    return u


TABLES = {
    "sigma5": gaussian_noise_table(5.0),
    "sigma1": gaussian_noise_table(1.0),
    "all_positive": (np.array([1 << 30, 1 << 31, 3 << 30], dtype=np.uint32), 3),   # c <= 0 for thr < 3
    "all_negative": (np.array([1 << 31], dtype=np.uint32), -9),                    # c > n_levels - 1 for thr >= -8
    "one_level": (np.zeros(0, dtype=np.uint32), 2),
    "none": (np.zeros(0, dtype=np.uint32), 0),
}


THRESHOLDS = [-1.0, 0.0, 0.5, 20.0, 40.0, 4094.5, 5000.0, -20.0, -4096.0, 2.0, 2.99]


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_decision_rule_equals_brute_force(table, thr):
    cdf, lo = TABLES[table]
    rng = np.random.default_rng(100 * sorted(TABLES).index(table) + THRESHOLDS.index(thr))  # the same draws every run
    k = 96
    u = _draws(rng, cdf, k)
    for ped0 in (0, 100, 4095, int(4095 - thr) if 0 <= thr <= 4095 else 7):
        ped = np.full(k, ped0, dtype=np.int64)
        ped[::7] = rng.integers(0, 4096, size=len(ped[::7]))
        np.testing.assert_array_equal(_rule(u, ped, thr, cdf, lo), _brute(u, ped, thr, cdf, lo),
                                      err_msg=f"{table} thr {thr} ped {ped0}")


def test_decision_rule_cutoff_kinds():
    cdf, lo = gaussian_noise_table(5.0)  # levels -40 .. 40
    assert readout_cutoff(cdf, lo, 40.0) == ("never", 0)  # the workloads' threshold can never fire a noise-only pad
    assert readout_cutoff(cdf, lo, 39.5) == ("draw", int(cdf[79]))
    assert readout_cutoff(cdf, lo, 20.0) == ("draw", int(cdf[60]))
    assert readout_cutoff(cdf, lo, -41.0)[0] == "always"
    assert readout_cutoff(cdf, lo, -40.5)[0] == "always"  # every level >= -40 > -40.5
    assert readout_cutoff(cdf, lo, -39.5) == ("draw", int(cdf[0]))
    none = np.zeros(0, dtype=np.uint32)
    assert readout_cutoff(none, 0, 0.0)[0] == "never" and readout_cutoff(none, 0, -0.5)[0] == "always"
    assert readout_cutoff(cdf, lo, math.inf)[0] == "never" and readout_cutoff(cdf, lo, -math.inf)[0] == "always"


def test_fast_uniforms_are_the_contract_draw():
    cdf, lo = gaussian_noise_table(3.0)
    noise = Noise(cdf, lo, stream=5)
    pads = np.array([0, 1, 77, 10239])
    for seed, event in ((0, 0), (0x9E3779B97F4A7C15, (1 << 32) + 3)):
        np.testing.assert_array_equal(uniforms(noise, seed, event, pads), noise.uniforms(seed, event, pads))
        np.testing.assert_array_equal(values(noise, seed, event, pads), noise.values(seed, event, pads))


def _expected_by_restatement(noise, thr, mask, n_events, seed):
    """Mean number of kept noise-only pads over n_events empty events of the restatement (partial readout)."""
    out = traces(np.zeros(n_events + 1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64),
                 np.zeros(512), thr, 0, noise, seed, 1000, PARTIAL, mask)
    assert (out[3] == -1).all()
    return out[4]["n_rows"] / n_events


def test_expected_noise_pads_matches_monte_carlo():
    cdf, lo = gaussian_noise_table(5.0)
    rng = np.random.default_rng(4)
    pads = rng.choice(_abi.NUM_PADS, 600, replace=False)
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[pads] = True
    ped = np.full(_abi.NUM_PADS, 100, dtype=np.int64)
    ped[pads[:40]] = 4095          # never kept
    ped[pads[40:60]] = 4095 - 17   # 4095 - ped = thr: never kept
    thr, n_events = 17.0, 12
    want = expected_noise_pads((cdf, lo), thr, pads, ped)
    q = (2.0 ** 32 - float(cdf[int(math.floor(thr)) + 1 - lo - 1])) / 2.0 ** 32
    assert want == pytest.approx(540 * (1 - (1 - q) ** 512), rel=1e-12)
    got = _expected_by_restatement(Noise(cdf, lo, pedestals=ped.astype(np.int16)), thr, mask, n_events, seed=11)
    sd = math.sqrt(want * (1 - want / 540) / n_events)
    assert abs(got - want) < 5 * sd, (got, want, sd)


def test_expected_noise_pads_closed_cases():
    cdf, lo = gaussian_noise_table(5.0)
    n_s = _abi.NUM_PADS - len(set(BEAM_PADS))
    assert expected_noise_pads((cdf, lo), 40.0) == 0.0
    assert expected_noise_pads(None, 0.0) == 0.0
    assert expected_noise_pads(None, -0.5) == n_s
    assert expected_noise_pads((cdf, lo), -41.0, [3, 4, 5]) == 3.0
    # 4095 - ped <= thr: never, even with a table that always crosses
    assert expected_noise_pads((cdf, lo), 20.0, [3], pedestals=4075) == 0.0
    # the issue's figure: sigma 5, thr 20, about 106 noise-only pads per event over the non-beam pads
    assert 100.0 < expected_noise_pads((cdf, lo), 20.0) < 112.0


def test_restatement_full_and_partial_agree_on_kept_pads():
    cdf, lo = gaussian_noise_table(6.0)
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[[1, 2, 3, 40, 41, 900, 10239]] = True
    noise = Noise(cdf, lo, pedestals=np.full(_abi.NUM_PADS, 4095 - 10, dtype=np.int16))
    pts = np.array([[2.0, 30.5, 500.0], [5.0, 40.0, 800.0], [900.0, 0.0, 0.0]])  # pad 5 is outside S
    off = np.array([0, 0, 3, 3])
    resp = np.zeros(512)
    resp[:20] = 1.0
    full = traces(off, pts, np.array([7, 8, 9]), resp, 5.0, 0, noise, 3, 50, FULL, mask)
    part = traces(off, pts, np.array([7, 8, 9]), resp, 5.0, 0, noise, 3, 50, PARTIAL, mask)
    np.testing.assert_array_equal(full[0], [0, 7, 14, 21])
    np.testing.assert_array_equal(full[1], np.tile(np.flatnonzero(mask), 3))
    assert 5 not in full[1]
    np.testing.assert_array_equal(full[3][7:14], [-1, 7, -1, -1, -1, 9, -1])  # event 1: rows on pads 2 and 900
    assert (full[3][:7] == -1).all() and (full[3][14:] == -1).all()
    # partial keeps a subset of the full rows with the same samples
    sel = np.isin(np.arange(21), [i for i in range(21) if (full[2][i].astype(np.int64) - (4095 - 10)).max() > 5.0])
    np.testing.assert_array_equal(part[1], full[1][sel])
    np.testing.assert_array_equal(part[2], full[2][sel])


def test_python_validation():
    for kw in ({"readout": "zero"}, {"readout": 1}, {"readout": "partial", "readout_pads": [0, 10240]},
               {"readout": "full", "readout_pads": [-1]}, {"readout": "full", "readout_pads": [3, 4, 3]},
               {"readout": "partial", "readout_pads": np.ones(10239, dtype=bool)},
               {"readout": "partial", "readout_pads": np.ones((2, 10240), dtype=bool)},
               {"readout": "partial", "readout_pads": [1.5, 2.0]}, {"readout_pads": [5, 5]}):
        with pytest.raises(ValueError):
            ReadoutSettings(**kw)

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"library touched: {name}")

    from attpc_engine_amd import workloads

    _, config, _ = workloads.be10dp()
    with pytest.raises(ValueError):  # validated before the first library call
        configure_traces(config, NoLibrary(), readout="full", readout_pads=[1, 1])
    default = readout_mask(None)
    assert default.sum() == _abi.NUM_PADS - len(set(BEAM_PADS)) and not default[BEAM_PADS].any()
    np.testing.assert_array_equal(readout_mask(np.flatnonzero(default)), default)
    np.testing.assert_array_equal(readout_mask(default.astype(bool)), default)
    ok = ReadoutSettings("full", [10239, 0])
    assert ok.rows_per_event() == 2 and list(ok.pads) == [0, 10239] and ok.token()[0] == _abi.READOUT_FULL
    assert ReadoutSettings("hit", [1]).token() is None and ReadoutSettings("partial").rows_per_event() == 0


def test_trace_writer_records_readout_only_off_hit(tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector import TraceWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)
    _, config, _ = workloads.be10dp()
    rows = (np.array([3], dtype=np.int32), np.full((1, 512), 7, dtype=np.int16), np.array([-1]))
    dirs = {name: tmp_path / name for name in ("plain", "hit", "partial", "full")}
    for d in dirs.values():
        d.mkdir()
    for name, kw in (("plain", {}), ("hit", {"readout": "hit", "readout_pads": [1, 2]}),
                     ("partial", {"readout": "partial"}), ("full", {"readout": "full", "readout_pads": [9, 3, 4]})):
        w = TraceWriter(dirs[name], config, **kw)
        w.write_traces(*rows, 0)
        w.close()
    plain, hit = (dirs[k] / "run_0000.npz" for k in ("plain", "hit"))
    assert plain.read_bytes() == hit.read_bytes()
    assert not [k for k in np.load(plain).files if "readout" in k]
    part, full = np.load(dirs["partial"] / "run_0000.npz"), np.load(dirs["full"] / "run_0000.npz")
    assert str(part["trace@readout"]) == "partial" and str(full["trace@readout"]) == "full"
    np.testing.assert_array_equal(part["trace/readout_pads"], np.flatnonzero(readout_mask(None)))
    np.testing.assert_array_equal(full["trace/readout_pads"], [3, 4, 9])
    w = TraceWriter(dirs["full"], config, readout="full", readout_pads=[9, 3, 4])
    assert w.readout_kwargs()["readout"] == "full" and w.readout_kwargs()["readout_pads"].sum() == 3
    w.close()


def test_trace_readout_struct_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "attpc_engine.h"
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(attpc_trace_readout_desc), offsetof(attpc_trace_readout_desc, mode),
  offsetof(attpc_trace_readout_desc, reserved), offsetof(attpc_trace_readout_desc, channels));
 printf("%d %d %d\n", ATTPC_READOUT_HIT, ATTPC_READOUT_PARTIAL, ATTPC_READOUT_FULL);
 return 0; }'''
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = [int(v) for v in subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True,
                                              check=True).stdout.split()]
    desc = [C.sizeof(_abi.TraceReadoutDesc)] + [getattr(_abi.TraceReadoutDesc, f).offset
                                                for f, _ in _abi.TraceReadoutDesc._fields_]
    assert out == desc + [_abi.READOUT_HIT, _abi.READOUT_PARTIAL, _abi.READOUT_FULL]
    assert "attpc_trace_configure_readout" in _abi.EXPORTED_SYMBOLS
