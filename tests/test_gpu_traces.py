"""Digitised pad traces on the device, bit for bit against the numpy restatement of the contract
(tests/trace_reference.py): hand-made clouds through ``attpc_traces``, the fused and file-driven runs against the
restatement applied to the device's own clouds, the CPU oracle's clouds within 1 ADC count, split / chunk / capacity
invariance, and the cloud and Spyral outputs unchanged beside trace runs.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import clouds_to_traces, configure_traces
from tests.helpers import ID_CASE_IDS, ID_CASES, Inputs, sort_cloud
from tests.trace_reference import traces as reference_traces

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine
    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _assert_same(got, ref):
    """(offsets, pads, samples, labels, sums) of the device and of the restatement: identical."""
    for a, b, what in zip(got[:4], ref[:4], ("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)
    assert got[4] == ref[4], (got[4], ref[4])


def _hand_made_events(resp):
    """A list of (points [P,3], labels [P]) that reach every corner of the contract at threshold 40 (charges in units
    of u electrons, 1 ADC count at the response's peak)."""
    u = 1.0 / float(resp.max())
    sat = 4095.0 * u
    ev = []
    ev.append((np.array([[10.0, 0.3, 50 * u], [11.0, 511.9, 80 * u]]), np.array([1, 2])))  # t = 0, t = 511 (tail cut)
    ev.append((np.array([[5.0, 100.2, 30 * u], [5.0, 103.7, 25 * u], [5.0, 98.1, 40 * u], [5.0, 140.0, 9 * u]]),
               np.array([3, 4, 5, 6])))  # overlapping rows on one pad
    ev.append((np.array([[7.0, 200.5, 0.6 * sat], [7.0, 201.5, 0.6 * sat], [8.0, 200.5, 0.9 * sat]]),
               np.array([1, 2, 3])))  # the sum saturates, no single row does
    ev.append((np.array([[0.0, 50.0, 60 * u], [10239.0, 60.0, 70 * u]]), np.array([7, 8])))  # pads 0 and 10239
    ev.append((np.zeros((0, 3)), np.zeros(0, dtype=np.int64)))  # empty event
    ev.append((np.array([[20.0, 30.0, 1 * u], [21.0, 31.0, 0.0]]), np.array([1, 2])))  # no pad kept
    ev.append((np.array([[30.0, 12.0, 70 * u], [30.0, 9.0, 70 * u], [30.0, 15.0, 70 * u]]), np.array([4, 5, 6])))  # tie
    rng = np.random.default_rng(8)
    pads = rng.choice(10240, 300, replace=False)
    rows = []
    for p in pads:
        for t in rng.choice(512, int(rng.integers(1, 9)), replace=False):
            rows.append([float(p), t + rng.random() * 0.999, float(rng.integers(0, 4000)) * u])
    rows = np.array(rows)
    order = rng.permutation(len(rows))  # rows in shuffled order
    ev.append((rows[order], rng.integers(0, 7, size=len(rows))[order]))
    return ev


def _csr(events):
    offsets = np.zeros(len(events) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(p) for p, _ in events])
    points = np.concatenate([p for p, _ in events]).reshape(-1, 3)
    labels = np.concatenate([lab for _, lab in events]).astype(np.int64)
    return offsets, points, labels


@pytest.mark.parametrize("peak", [False, True], ids=["causal", "peak_on_arrival"])
@pytest.mark.parametrize("threshold", [40.0, -1.0], ids=["thr40", "keep_all"])
def test_hand_made_clouds(ctx, peak, threshold):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    offset = int(np.argmax(resp)) if peak else 0
    configure_traces(inp.config, ctx, resp, threshold, offset)
    offsets, points, labels = _csr(_hand_made_events(resp))
    got = clouds_to_traces(offsets, points, labels, ctx)
    ref = reference_traces(offsets, points, labels, resp, threshold, offset)
    _assert_same(got, ref)
    if threshold < 0:
        assert 21 in got[1]  # the all-zero trace of the pad with 0 electrons is kept
    assert got[0][5] == got[0][6] or threshold < 0  # nothing kept in the event below threshold
    assert got[3][got[0][6]: got[0][7]].tolist() == [5]  # tie on q: smallest t


def test_threshold_is_strict(ctx):
    inp = Inputs("o16aa")
    resp = np.zeros(512)
    resp[3] = 1.0
    points = np.array([[1.0, 10.0, 40.0], [2.0, 10.0, 41.0]])
    configure_traces(inp.config, ctx, resp, 40.0, 0)
    got = clouds_to_traces(np.array([0, 2]), points, np.array([1, 2]), ctx)
    assert got[1].tolist() == [2]  # max == thr dropped, thr + 1 kept
    _assert_same(got, reference_traces([0, 2], points, np.array([1, 2]), resp, 40.0, 0))


def test_bad_host_clouds_are_refused(ctx):
    inp = Inputs("o16aa")
    configure_traces(inp.config, ctx, None, None, 0)
    for pts in ([[1.0, 3.2, 5.0], [1.0, 3.7, 6.0]], [[10240.0, 3.0, 5.0]], [[1.5, 3.0, 5.0]], [[1.0, 512.0, 5.0]],
                [[1.0, 3.0, -1.0]]):
        with pytest.raises(ValueError):
            clouds_to_traces(np.array([0, len(pts)]), np.array(pts), np.zeros(len(pts), dtype=np.int64), ctx)


def _sim_traces(eng, n, seed, first, **kw):
    res = eng.run_traces(n, seed=seed, first_event=first, **kw)
    return (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"]), res


def _check_fused_against_own_cloud(inp, ctx, n, seed, first, offset=0):
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    eng.configure_traces(inp.config, resp, thr, offset)
    cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
    got, res = _sim_traces(eng, n, seed, first)
    ref = reference_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, offset, first_event=first)
    _assert_same(got, ref)
    np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
    for key in ("n_points", "charge_checksum", "key_checksum", "n_track_samples"):
        assert res["stats"][key] == cloud["stats"][key], key
    np.testing.assert_array_equal(res["p4"], cloud["p4"])
    return eng, cloud, got


@pytest.mark.parametrize("name,kw,n", [("o16aa", {}, 48), ("be10dp", {}, 64), ("b10chain", {}, 6),
                                       ("o16aa", {"path_step": 1.0e-4}, 8)],
                         ids=["o16aa", "be10dp", "b10chain", "o16aa_path_step"])
def test_sim_run_traces_vs_restatement_of_own_cloud(ctx, name, kw, n):
    _, _, got = _check_fused_against_own_cloud(Inputs(name, **kw), ctx, n, seed=21, first=7)
    assert got[4]["n_rows"] > 0


def test_peak_on_arrival_offset_fused(ctx):
    inp = Inputs("be10dp")
    _check_fused_against_own_cloud(inp, ctx, 24, seed=5, first=100, offset=int(np.argmax(get_response(inp.config))))


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_id_cases(ctx, case):
    _check_fused_against_own_cloud(Inputs("be10dp"), ctx, 8, seed=case.seed, first=case.first_event)


def test_oracle_cloud_within_one_adc_count(ctx):
    from oracle import pyoracle as orc

    inp = Inputs("o16aa")
    n, seed, first = 8, 3, 0
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    eng.configure_traces(inp.config, resp, -1.0, 0)
    got, _ = _sim_traces(eng, n, seed, first)
    ref_cloud = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=n, capacity=1 << 20, threads=8)
    ref = reference_traces(ref_cloud["offsets"], ref_cloud["points"], ref_cloud["labels"], resp, -1.0, 0)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    diff = np.abs(got[2].astype(np.int32) - ref[2].astype(np.int32))
    assert diff.max(initial=0) <= 1, diff.max()


def test_det_run_traces_equals_fused(ctx):
    from attpc_engine_amd.detector.traces import simulate_batch_traces

    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    eng.configure_traces(inp.config, resp, thr, 0)
    got, res = _sim_traces(eng, 32, 9, 64)
    off, pads, samples, labels, raw, stats = simulate_batch_traces(
        res["p4"], res["vertex"], inp.z, inp.a, inp.config, 9, inp.indices, first_event=64, ctx=ctx, response=resp,
        threshold=thr, offset=0)
    _assert_same((off, pads, samples, labels, {k: stats[k] for k in ("n_rows", "sample_checksum", "pad_checksum")}), got)
    np.testing.assert_array_equal(raw, res["event_points"])


def test_split_chunk_and_capacity_invariance(ctx):
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config)
    whole, _ = _sim_traces(eng, 96, 4, 10)
    for cut in (1, 37):
        a, _ = _sim_traces(eng, cut, 4, 10)
        b, _ = _sim_traces(eng, 96 - cut, 4, 10 + cut)
        np.testing.assert_array_equal(np.concatenate([a[0][:-1], b[0] + a[0][-1]]), whole[0])
        for i in (1, 2, 3):
            np.testing.assert_array_equal(np.concatenate([a[i], b[i]]), whole[i])
        assert (a[4]["sample_checksum"] + b[4]["sample_checksum"]) % (1 << 64) == whole[4]["sample_checksum"]
        assert (a[4]["pad_checksum"] + b[4]["pad_checksum"]) % (1 << 64) == whole[4]["pad_checksum"]
    resident = eng.run_traces(96, seed=4, first_event=10, fetch=False)
    assert resident["trace"] == whole[4]
    small = _engine(inp, ctx, chunk_events=16)
    small.configure_traces(inp.config)
    got, _ = _sim_traces(small, 96, 4, 10)
    _assert_same(got, whole)
    # undersized buffers on a fresh context: the chunk's assembly is queued again behind its re-scatter
    tiny_ctx = _abi.Context(0)
    tiny_ctx.set_option("tiny_buffers", 1)
    tiny = _engine(inp, tiny_ctx)
    tiny.configure_traces(inp.config)
    got, _ = _sim_traces(tiny, 96, 4, 10)
    _assert_same(got, whole)
    tiny_ctx.close()
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    # too small a capacity: E_CAPACITY with the exact row count, then success
    from attpc_engine_amd.detector.traces import TraceArrays
    need = whole[4]["n_rows"]
    arrays = TraceArrays(96, need - 1)
    stats = _abi.RunStats()
    rc = ctx.lib.attpc_sim_run_traces(ctx.handle, 4, 10, 96, eng.layout, None, None, None, arrays.out, stats)
    assert rc == _abi.E_CAPACITY and arrays.out.n_rows == need
    arrays = TraceArrays(96, need)
    assert ctx.lib.attpc_sim_run_traces(ctx.handle, 4, 10, 96, eng.layout, None, None, None, arrays.out, stats) == 0
    _assert_same((*arrays.result(), arrays.sums()), whole)


def test_not_configured_is_reported():
    c = _abi.Context(0)
    inp = Inputs("be10dp")
    from attpc_engine_amd.engine import Engine
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=c)
    out = _abi.TraceOut()
    assert c.lib.attpc_sim_run_traces(c.handle, 1, 0, 4, eng.layout, None, None, None, out, None) == _abi.E_NOTCONFIGURED
    assert c.lib.attpc_traces(c.handle, 0, None, None, None, out) == _abi.E_NOTCONFIGURED
    c.close()


def test_cloud_and_spyral_unchanged_beside_trace_runs(ctx):
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_spyral(inp.config)
    before = (eng.run(40, seed=2, first_event=3, fetch=True), eng.run_spyral(40, seed=2, first_event=3),
              eng.run(40, seed=2, first_event=3)["stats"])
    eng.configure_traces(inp.config)
    eng.run_traces(40, seed=2, first_event=3)
    eng.run_traces(40, seed=2, first_event=3, fetch=False)
    after = (eng.run(40, seed=2, first_event=3, fetch=True), eng.run_spyral(40, seed=2, first_event=3),
             eng.run(40, seed=2, first_event=3)["stats"])
    # (row order inside an event is not specified: the clouds are compared in canonical order, the Spyral rows -- in
    #  ascending z, ties in cloud order -- sorted on all their columns)
    np.testing.assert_array_equal(before[0]["offsets"], after[0]["offsets"])
    np.testing.assert_array_equal(before[1]["offsets"], after[1]["offsets"])
    np.testing.assert_array_equal(before[1]["event_points"], after[1]["event_points"])
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


def _read_trace_files(directory):
    out = {}
    for path in sorted(directory.glob("run_*.npz")):
        f = np.load(path)
        for key in f.files:
            if key.startswith("trace/trace_") and "@" not in key:
                ev = int(key.split("_")[-1])
                out[ev] = (f[f"trace/pads_{ev}"], f[key], f[f"trace/labels_{ev}"])
    return out


def test_run_simulation_and_run_fused_write_the_restatement(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd.detector import TraceWriter, run_simulation
    from attpc_engine_amd.engine import run_fused
    from attpc_engine_amd.io import KinematicsFileWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n = 40
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    eng = _engine(inp, ctx)
    seed = 17
    cloud = eng.run(n, seed=seed, first_event=0, fetch=True)
    ref = reference_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, 0)

    def expect(offsets, pads, samples, labels, raw):
        return {e: (pads[offsets[e]:offsets[e + 1]], samples[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]])
                for e in range(n) if raw[e] > 0}

    fused_dir = tmp_path / "fused"
    fused_dir.mkdir()
    run_fused(inp.pipeline, inp.config, TraceWriter(fused_dir, inp.config, max_events_per_file=16), n, inp.indices,
              seed=seed, batch_size=24, context=ctx)
    want = expect(*ref[:4], np.diff(cloud["offsets"]))
    got = _read_trace_files(fused_dir)
    assert sorted(got) == sorted(want)
    for e in want:
        for a, b in zip(got[e], want[e]):
            np.testing.assert_array_equal(a, b)

    kin_path = tmp_path / "kine.npz"
    w = KinematicsFileWriter(kin_path, n, inp.z, inp.a, 16)
    w.write_batch(0, cloud["vertex"], cloud["p4"])
    w.close()
    sim_dir = tmp_path / "sim"
    sim_dir.mkdir()
    run_simulation(inp.config, kin_path, TraceWriter(sim_dir, inp.config, max_events_per_file=16), inp.indices,
                   batch_size=24, seed=99)
    from numpy.random import default_rng
    run_seed = int(default_rng(99).integers(0, 1 << 63))
    from attpc_engine_amd.detector import simulate_batch
    off, pts, labs, _ = simulate_batch(cloud["p4"], cloud["vertex"], inp.z, inp.a, inp.config, run_seed, inp.indices, ctx=ctx)
    ref2 = reference_traces(off, pts, labs, resp, thr, 0)
    want = expect(*ref2[:4], np.diff(off))
    got = _read_trace_files(sim_dir)
    assert sorted(got) == sorted(want)
    for e in want:
        for a, b in zip(got[e], want[e]):
            np.testing.assert_array_equal(a, b)


def test_every_stage_at_once_three_routes_agree(ctx):
    """Noise and pedestals, partial readout, gain fluctuations with a pad map, the Fourier baseline and a gated trigger,
    all on: the trace rows and trigger records of ``Engine.run_trace_rows`` (configured through the engine's methods),
    of ``simulate_batch_trace_rows`` on the same kinematics and of ``clouds_to_trace_rows`` on the same cloud (its
    context configured by one ``TraceChain.configure``, every slot forgotten first) are bit for bit the same.  The
    trigger is the one of tests/test_gpu_trigger.py's gated case: the multiplicity about half of the events reach."""
    from attpc_engine_amd.detector.traces import (BaselineSettings, GainSettings, PeakSettings, TraceChain, TriggerSettings,
                                                  clouds_to_trace_rows, simulate_batch_trace_rows)
    from tests.test_gpu_trigger import _assert_records, _half_multiplicity, _pedestals

    inp = Inputs("be10dp")
    n, seed = 6, 17
    trace_kw = {"noise_sigma": 5.0, "threshold": 20.0, "readout": "partial", "pedestals": _pedestals(),
                "offset": int(np.argmax(get_response(inp.config)))}
    gain = GainSettings(theta=1.0, pad_gain=0.8 + 0.4 * np.random.default_rng(4).random(_abi.NUM_PADS), stream=2)
    peaks, baseline = PeakSettings(), BaselineSettings(20.0)
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **trace_kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(peaks)
    eng.configure_baseline(baseline)
    eng.configure_gain(gain)
    try:
        eng.configure_trigger(threshold=25, window=50, group_multiplicity=1)
        reach = eng.run_trigger(n, seed=seed)["trigger"]
        trigger = TriggerSettings(25, window=50, group_multiplicity=_half_multiplicity(reach), gate=True)
        eng.configure_trigger(trigger)
        one = eng.run_trace_rows(n, seed=seed)
        fired = one["trigger"]["fired"] != 0
        seen = f"peak_group_sum {reach['peak_group_sum'].tolist()}, fired {fired.tolist()}, rows {np.diff(one['offsets']).tolist()}"
        assert 0 < fired.sum() < n, seen  # the gate is exercised: events of both kinds
        assert (np.diff(one["offsets"])[~fired] == 0).all() and (np.diff(one["offsets"])[fired] > 0).any(), seen
        off, rows, labels, raw, stats = simulate_batch_trace_rows(
            one["p4"], one["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, ctx=ctx, peaks=peaks, baseline=baseline,
            trigger=trigger, gain=gain, **trace_kw)
        cloud = eng.run(n, seed=seed, fetch=True)
        for slot in ("trace", "trace_noise", "trace_readout", "spyral", "peaks", "baseline", "trigger", "trace_gain"):
            ctx.forget(slot)
        chain = TraceChain.from_kwargs(inp.config, **trace_kw).replace(peaks=peaks, baseline=baseline, trigger=trigger, gain=gain)
        chain.configure(ctx, rows=True)
        host = clouds_to_trace_rows(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed)
        routes = {"simulate_batch_trace_rows": (off, rows, labels, stats),
                  "clouds_to_trace_rows": host}
        for name, (o, r, lab, sums) in routes.items():
            np.testing.assert_array_equal(o, one["offsets"], err_msg=name)
            assert r.tobytes() == one["rows"].tobytes() and r.shape == one["rows"].shape, name
            np.testing.assert_array_equal(lab, one["labels"], err_msg=name)
            assert {k: sums[k] for k in ("n_rows", "row_checksum")} == one["trace_rows"], name
            _assert_records(sums["trigger"], one["trigger"], name)
        np.testing.assert_array_equal(raw, one["event_points"])
    finally:
        eng.configure_trigger()
        eng.configure_gain()
        eng.configure_baseline()
