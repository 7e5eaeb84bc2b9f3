"""Electronic noise and pedestals of the pad traces on the device, bit for bit against the numpy restatement
(tests/trace_noise_reference.py): hand-made clouds through ``attpc_traces_at``, the fused and file-driven runs against the
restatement applied to the device's own clouds (event ids past 2^32, seeds with a high word), noise off = the noiseless
library, split / chunk / capacity invariance, seed and stream, the noise histogram against the table, and the cloud and
Spyral outputs unchanged beside noisy trace runs.  Needs a real MI355X: ``-m gpu``."""
import math

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import clouds_to_traces, configure_traces, gaussian_noise_table
from tests.helpers import ID_CASE_IDS, ID_CASES, Inputs, sort_cloud
from tests.test_gpu_traces import _assert_same, _csr, _engine, _hand_made_events
from tests.trace_noise_reference import Noise, level_masses
from tests.trace_noise_reference import traces as noisy_traces

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _pedestals(seed=3):
    ped = np.random.default_rng(seed).integers(0, 4096, size=_abi.NUM_PADS).astype(np.int16)
    return ped


def _noise(sigma, ped, stream=0):
    cdf, lo = gaussian_noise_table(sigma)
    return Noise(cdf, lo, pedestals=ped, stream=stream)


def _configure_noise_off_in_c(ctx):
    """attpc_trace_configure_noise(ctx, NULL) straight through the ABI (and forget the Python-side token)."""
    ctx.check(ctx.lib.attpc_trace_configure_noise(ctx.handle, None), "attpc_trace_configure_noise")
    ctx.forget("trace_noise")


@pytest.mark.parametrize("sigma", [1.0, 6.0])
@pytest.mark.parametrize("threshold", [-1.0, 0.0, 40.0], ids=["keep_all", "thr0", "thr40"])
def test_hand_made_clouds(ctx, sigma, threshold):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    ped = _pedestals(int(sigma))
    ped[[0, 5, 20, 21]] = 0
    ped[[7, 10, 10239, 30]] = 4095
    configure_traces(inp.config, ctx, resp, threshold, 0, noise_sigma=sigma, pedestals=ped, noise_stream=3)
    offsets, points, labels = _csr(_hand_made_events(resp))
    first = (1 << 32) - 3  # the events cross the low word
    got = clouds_to_traces(offsets, points, labels, ctx, seed=SEED_HI, first_event=first)
    ref = noisy_traces(offsets, points, labels, resp, threshold, 0, _noise(sigma, ped, 3), SEED_HI, first)
    _assert_same(got, ref)
    assert got[4]["n_rows"] > 0
    configure_traces(inp.config, ctx, resp, threshold, 0)


def _check_fused(inp, ctx, n, seed, first, sigma=5.0, stream=0, ped_seed=1):
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    ped = _pedestals(ped_seed)
    eng.configure_traces(inp.config, resp, thr, 0, noise_sigma=sigma, pedestals=ped, noise_stream=stream)
    cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
    res = eng.run_traces(n, seed=seed, first_event=first)
    got = (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"])
    ref = noisy_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, 0, _noise(sigma, ped, stream),
                       seed, first)
    _assert_same(got, ref)
    np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
    return eng, res, got


@pytest.mark.parametrize("name,n", [("o16aa", 16), ("be10dp", 24)])
def test_sim_and_det_run_traces_vs_restatement_of_own_cloud(ctx, name, n):
    from attpc_engine_amd.detector.traces import simulate_batch_traces

    inp = Inputs(name)
    seed, first = 21, 7
    eng, res, got = _check_fused(inp, ctx, n, seed, first)
    assert got[4]["n_rows"] > 0
    resp = get_response(inp.config)
    off, pads, samples, labels, raw, stats = simulate_batch_traces(
        res["p4"], res["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, first_event=first, ctx=ctx,
        response=resp, threshold=float(inp.config.elec_params.adc_threshold), offset=0, noise_sigma=5.0,
        pedestals=_pedestals(1))
    _assert_same((off, pads, samples, labels, {k: stats[k] for k in ("n_rows", "sample_checksum", "pad_checksum")}),
                 got)
    np.testing.assert_array_equal(raw, res["event_points"])


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_id_cases(ctx, case):
    _check_fused(Inputs("be10dp"), ctx, 8, seed=case.seed, first=case.first_event, sigma=3.0, stream=11)


def test_noise_off_is_the_noiseless_library(ctx):
    inp = Inputs("be10dp")
    fresh = _abi.Context(0)
    try:
        resp = get_response(inp.config)
        thr = float(inp.config.elec_params.adc_threshold)
        plain = _engine(inp, fresh)
        plain.configure_traces(inp.config, resp, thr, 0)
        want = plain.run_traces(32, seed=SEED_HI, first_event=(1 << 32) - 5)
        offsets, points, labels = _csr(_hand_made_events(resp))
        configure_traces(inp.config, fresh, resp, 40.0, 0)
        want_host = clouds_to_traces(offsets, points, labels, fresh)

        eng = _engine(inp, ctx)
        eng.configure_traces(inp.config, resp, thr, 0, noise_sigma=4.0, pedestals=_pedestals(2))
        noisy = eng.run_traces(32, seed=SEED_HI, first_event=(1 << 32) - 5)
        assert not np.array_equal(noisy["samples"][:5], want["samples"][:5])
        _configure_noise_off_in_c(ctx)
        got = eng.run_traces(32, seed=SEED_HI, first_event=(1 << 32) - 5)
        for key in ("offsets", "pads", "samples", "labels", "event_points"):
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert got["trace"] == want["trace"]
        configure_traces(inp.config, ctx, resp, 40.0, 0, noise_sigma=2.0)
        _configure_noise_off_in_c(ctx)
        configure_traces(inp.config, ctx, resp, 40.0, 0)
        _assert_same(clouds_to_traces(offsets, points, labels, ctx), want_host)
        # with noise on, attpc_traces is attpc_traces_at(seed 0, first event 0)
        configure_traces(inp.config, ctx, resp, 40.0, 0, noise_sigma=6.0, pedestals=_pedestals(4))
        at = clouds_to_traces(offsets, points, labels, ctx, seed=0, first_event=0)
        from attpc_engine_amd.detector.traces import call_with_capacity
        n = len(offsets) - 1
        arrays = call_with_capacity(ctx, n, 4096, lambda out: ctx.lib.attpc_traces(
            ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(points), _abi.iptr(labels, _abi.C.c_int64),
            out), "attpc_traces")
        _assert_same((*arrays.result(), arrays.sums()), at)
    finally:
        configure_traces(inp.config, ctx, None, None, 0)
        fresh.close()


def test_split_chunk_and_capacity_invariance(ctx):
    inp = Inputs("be10dp")
    kw = {"noise_sigma": 5.0, "pedestals": _pedestals(6), "noise_stream": 2}
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    seed, first, n = SEED_HI, (1 << 33) + 10, 96

    def run(e, k, n_ev, **more):
        res = e.run_traces(n_ev, seed=seed, first_event=k, **more)
        return (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"])

    whole = run(eng, first, n)
    for cut in (1, 37):
        a, b = run(eng, first, cut), run(eng, first + cut, n - cut)
        np.testing.assert_array_equal(np.concatenate([a[0][:-1], b[0] + a[0][-1]]), whole[0])
        for i in (1, 2, 3):
            np.testing.assert_array_equal(np.concatenate([a[i], b[i]]), whole[i])
        assert (a[4]["sample_checksum"] + b[4]["sample_checksum"]) % (1 << 64) == whole[4]["sample_checksum"]
        assert (a[4]["pad_checksum"] + b[4]["pad_checksum"]) % (1 << 64) == whole[4]["pad_checksum"]
    assert eng.run_traces(n, seed=seed, first_event=first, fetch=False)["trace"] == whole[4]
    small = _engine(inp, ctx, chunk_events=16)
    small.configure_traces(inp.config, **kw)
    _assert_same(run(small, first, n), whole)
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    from attpc_engine_amd.detector.traces import TraceArrays
    need = whole[4]["n_rows"]
    arrays = TraceArrays(n, need - 1)
    stats = _abi.RunStats()
    rc = ctx.lib.attpc_sim_run_traces(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats)
    assert rc == _abi.E_CAPACITY and arrays.out.n_rows == need
    arrays = TraceArrays(n, need)
    assert ctx.lib.attpc_sim_run_traces(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats) == 0
    _assert_same((*arrays.result(), arrays.sums()), whole)
    configure_traces(inp.config, ctx, None, None, 0)


def test_seed_and_stream(ctx):
    inp = Inputs("o16aa")
    base = _check_fused(inp, ctx, 8, seed=5, first=40, sigma=2.0, stream=0)[2]
    other_stream = _check_fused(inp, ctx, 8, seed=5, first=40, sigma=2.0, stream=1)[2]
    other_seed = _check_fused(inp, ctx, 8, seed=6, first=40, sigma=2.0, stream=0)[2]
    assert base[4]["n_rows"] > 0
    assert base[4]["sample_checksum"] != other_stream[4]["sample_checksum"]
    assert base[4]["sample_checksum"] != other_seed[4]["sample_checksum"]
    configure_traces(inp.config, ctx, None, None, 0)


def test_noise_histogram_matches_the_table(ctx):
    inp = Inputs("o16aa")
    sigma, ped0 = 6.0, 1000
    cdf, lo = gaussian_noise_table(sigma)
    configure_traces(inp.config, ctx, None, -1.0, 0, noise_sigma=sigma, pedestals=ped0)
    pads = np.arange(0, 2000 * 5, 5, dtype=np.float64)
    points = np.column_stack([pads, np.full(len(pads), 100.5), np.zeros(len(pads))])
    got = clouds_to_traces(np.array([0, len(pads)]), points, np.arange(len(pads)), ctx, seed=SEED_HI, first_event=77)
    assert got[4]["n_rows"] == len(pads)
    values = got[2].astype(np.int64).ravel() - ped0 - lo
    assert values.min() >= 0 and values.max() <= cdf.size
    counts = np.bincount(values, minlength=cdf.size + 1)
    expect = level_masses(cdf, cdf.size + 1) * values.size
    keep = expect >= 5  # the far tails pooled into one cell
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(expect[keep], expect[~keep].sum())
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    dof = len(obs) - 1
    # Wilson-Hilferty: (chi2 / dof)^(1/3) is close to normal with mean 1 - 2 / (9 dof), variance 2 / (9 dof)
    z = ((chi2 / dof) ** (1 / 3) - (1 - 2 / (9 * dof))) / math.sqrt(2 / (9 * dof))
    p = 0.5 * math.erfc(z / math.sqrt(2))
    assert p > 1e-6, (chi2, dof, p)
    assert abs(values.mean() + lo) < 0.02 and abs(values.std() - math.sqrt(sigma ** 2 + 1 / 12)) < 0.05
    configure_traces(inp.config, ctx, None, None, 0)


def test_cloud_and_spyral_unchanged_beside_noisy_trace_runs(ctx):
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_spyral(inp.config)
    before = (eng.run(40, seed=2, first_event=3, fetch=True), eng.run_spyral(40, seed=2, first_event=3),
              eng.run(40, seed=2, first_event=3)["stats"])
    eng.configure_traces(inp.config, noise_sigma=7.0, pedestals=_pedestals(9), noise_stream=5)
    eng.run_traces(40, seed=2, first_event=3)
    eng.run_traces(40, seed=2, first_event=3, fetch=False)
    after = (eng.run(40, seed=2, first_event=3, fetch=True), eng.run_spyral(40, seed=2, first_event=3),
             eng.run(40, seed=2, first_event=3)["stats"])
    np.testing.assert_array_equal(before[0]["offsets"], after[0]["offsets"])
    np.testing.assert_array_equal(before[1]["offsets"], after[1]["offsets"])
    for e in range(40):
        lo, hi = before[0]["offsets"][e], before[0]["offsets"][e + 1]
        for x, y in zip(sort_cloud(before[0]["points"][lo:hi], before[0]["labels"][lo:hi]),
                        sort_cloud(after[0]["points"][lo:hi], after[0]["labels"][lo:hi])):
            np.testing.assert_array_equal(x, y)
        lo, hi = before[1]["offsets"][e], before[1]["offsets"][e + 1]
        rows = [np.column_stack([r["rows"][lo:hi], r["labels"][lo:hi]]) for r in (before[1], after[1])]
        rows = [r[np.lexsort(r.T[::-1])] for r in rows]
        np.testing.assert_array_equal(rows[0], rows[1])
    for key in ("n_points", "charge_checksum", "key_checksum"):
        assert before[2][key] == after[2][key]
    configure_traces(inp.config, ctx, None, None, 0)


def test_writers_forward_the_noise(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd.detector import TraceWriter, run_simulation, simulate_batch
    from attpc_engine_amd.engine import run_fused
    from attpc_engine_amd.io import KinematicsFileWriter
    from tests.test_gpu_traces import _read_trace_files

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n, seed = 24, 17
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    ped = _pedestals(12)
    kw = {"noise_sigma": 4.0, "pedestals": ped, "noise_stream": 9}
    noise = _noise(4.0, ped, 9)
    eng = _engine(inp, ctx)
    cloud = eng.run(n, seed=seed, first_event=0, fetch=True)

    def check(directory, offsets, points, labels, run_seed):
        ref = noisy_traces(offsets, points, labels, resp, thr, 0, noise, run_seed, 0)
        raw = np.diff(offsets)
        want = {e: tuple(a[ref[0][e]:ref[0][e + 1]] for a in ref[1:4]) for e in range(n) if raw[e] > 0}
        got = _read_trace_files(directory)
        assert sorted(got) == sorted(want)
        for e in want:
            for a, b in zip(got[e], want[e]):
                np.testing.assert_array_equal(a, b)

    fused_dir = tmp_path / "fused"
    fused_dir.mkdir()
    run_fused(inp.pipeline, inp.config, TraceWriter(fused_dir, inp.config, max_events_per_file=16, **kw), n,
              inp.indices, seed=seed, batch_size=10, context=ctx)
    check(fused_dir, cloud["offsets"], cloud["points"], cloud["labels"], seed)

    kin_path = tmp_path / "kine.npz"
    w = KinematicsFileWriter(kin_path, n, inp.z, inp.a, 16)
    w.write_batch(0, cloud["vertex"], cloud["p4"])
    w.close()
    sim_dir = tmp_path / "sim"
    sim_dir.mkdir()
    run_simulation(inp.config, kin_path, TraceWriter(sim_dir, inp.config, max_events_per_file=16, **kw), inp.indices,
                   batch_size=10, seed=99)
    from numpy.random import default_rng
    run_seed = int(default_rng(99).integers(0, 1 << 63))
    off, pts, labs, _ = simulate_batch(cloud["p4"], cloud["vertex"], inp.z, inp.a, inp.config, run_seed, inp.indices,
                                       ctx=ctx)
    check(sim_dir, off, pts, labs, run_seed)

    # the per-event write() path: noise keyed on (noise_seed, event_number)
    one_dir = tmp_path / "one"
    one_dir.mkdir()
    w = TraceWriter(one_dir, inp.config, noise_seed=SEED_HI, **kw)
    lo, hi = cloud["offsets"][3], cloud["offsets"][4]
    w.write(cloud["points"][lo:hi], cloud["labels"][lo:hi], inp.config, 1 << 40)
    w.close()
    ref = noisy_traces([0, hi - lo], cloud["points"][lo:hi], cloud["labels"][lo:hi], resp, thr, 0, noise, SEED_HI,
                       1 << 40)
    got = _read_trace_files(one_dir)[1 << 40]
    for a, b in zip(got, ref[1:4]):
        np.testing.assert_array_equal(a, b)
    configure_traces(inp.config, ctx, None, None, 0)
