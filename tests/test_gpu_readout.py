"""Readout of noise-only pads on the device (partial and full readout), bit for bit against the numpy restatement
(tests/readout_reference.py): hand-made clouds through ``attpc_traces_at`` with a readout set that has holes and drops a
hit pad, empty events between full ones and event ids across 2^32; the fused and file-driven runs at the full pad plane
against the restatement applied to the device's own clouds over the id cases; partial readout without noise = hit mode;
hit mode after a readout run = a fresh context; full readout's offsets; chunk, buffer and fetch invariance; the device
memory of a fresh full-readout run; the number of noise-only pads against ``expected_noise_pads``; and the cloud and
Spyral outputs unchanged beside readout runs.  Needs a real MI355X: ``-m gpu``."""
import math

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (clouds_to_traces, configure_traces, expected_noise_pads,
                                              gaussian_noise_table, readout_mask, simulate_batch_traces)
from tests.helpers import ID_CASE_IDS, ID_CASES, Inputs, sort_cloud
from tests.readout_reference import FULL, PARTIAL
from tests.readout_reference import traces as readout_traces
from tests.test_gpu_traces import _assert_same, _csr, _engine, _hand_made_events
from tests.trace_noise_reference import Noise

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15
MODES = {"partial": PARTIAL, "full": FULL}


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _pedestals(seed):
    return np.random.default_rng(seed).integers(0, 4096, size=_abi.NUM_PADS).astype(np.int16)


def _noise(sigma, ped, stream=0):
    cdf, lo = gaussian_noise_table(sigma)
    return Noise(cdf, lo, pedestals=ped, stream=stream)


def _reset(ctx, config):
    configure_traces(config, ctx, None, None, 0)


def _holey_set(events):
    """A reduced readout set: every hit pad of the hand-made events but 11 and 8 (their rows are dropped), pads 0 and
    10239, and 400 more pads with holes between them."""
    hit = np.unique(np.concatenate([p[:, 0] for p, _ in events if len(p)])).astype(np.int64)
    rng = np.random.default_rng(21)
    extra = rng.choice(_abi.NUM_PADS, 400, replace=False)
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[hit] = True
    mask[extra] = True
    mask[[0, 10239]] = True
    mask[[11, 8, 12, 13, 14]] = False
    return mask


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("sigma", [1.0, 6.0])
@pytest.mark.parametrize("threshold", [-1.0, 0.0, 40.0], ids=["keep_all", "thr0", "thr40"])
def test_hand_made_clouds(ctx, mode, sigma, threshold):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    ped = _pedestals(int(sigma) + 7)
    ped[[0, 5, 20, 21]] = 0
    ped[[7, 10, 10239, 30]] = 4095
    events = _hand_made_events(resp)
    empty = (np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    events = [empty] + events[:3] + [empty, empty] + events[3:] + [empty]
    mask = _holey_set(events)
    assert mask[ped == 0].any() and mask[ped == 4095].any()
    configure_traces(inp.config, ctx, resp, threshold, 0, noise_sigma=sigma, pedestals=ped, noise_stream=3,
                     readout=mode, readout_pads=mask)
    offsets, points, labels = _csr(events)
    first = (1 << 32) - 5  # the events cross the low word
    got = clouds_to_traces(offsets, points, labels, ctx, seed=SEED_HI, first_event=first)
    ref = readout_traces(offsets, points, labels, resp, threshold, 0, _noise(sigma, ped, 3), SEED_HI, first,
                         MODES[mode], mask)
    _assert_same(got, ref)
    assert not np.isin(got[1], [8, 11]).any() and (got[3][~np.isin(got[1], points[:, 0])] == -1).all()
    if mode == "full":
        np.testing.assert_array_equal(got[0], np.arange(len(events) + 1) * int(mask.sum()))
    _reset(ctx, inp.config)


def _check_fused(inp, ctx, n, seed, first, mode, sigma=5.0, threshold=20.0, stream=0, ped_seed=1, file_driven=True):
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    ped = _pedestals(ped_seed)
    kw = {"noise_sigma": sigma, "pedestals": ped, "noise_stream": stream, "readout": mode}
    eng.configure_traces(inp.config, resp, threshold, 0, **kw)
    cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
    res = eng.run_traces(n, seed=seed, first_event=first)
    got = (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"])
    ref = readout_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, threshold, 0,
                         _noise(sigma, ped, stream), seed, first, MODES[mode], readout_mask(None).astype(bool))
    _assert_same(got, ref)
    np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
    if file_driven:
        off, pads, samples, labels, raw, stats = simulate_batch_traces(
            res["p4"], res["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, first_event=first, ctx=ctx,
            response=resp, threshold=threshold, offset=0, **kw)
        _assert_same((off, pads, samples, labels, {k: stats[k] for k in ("n_rows", "sample_checksum",
                                                                          "pad_checksum")}), got)
        np.testing.assert_array_equal(raw, res["event_points"])
    return eng, res, got


@pytest.mark.parametrize("name", ["o16aa", "be10dp"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fused_and_file_driven_full_plane(ctx, name, mode):
    inp = Inputs(name)
    _, _, got = _check_fused(inp, ctx, 3, seed=21, first=7, mode=mode)
    hit_labels = got[3] != -1
    assert hit_labels.any() and (~hit_labels).any()
    _reset(ctx, inp.config)


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_id_cases(ctx, case):
    inp = Inputs("be10dp" if case.first_event % 2 else "o16aa")
    _check_fused(inp, ctx, 2, seed=case.seed, first=case.first_event, mode="partial", sigma=3.0, threshold=11.0,
                 stream=11, file_driven=False)
    _check_fused(inp, ctx, 2, seed=case.seed, first=case.first_event, mode="full", sigma=3.0, threshold=11.0,
                 stream=11)
    _reset(ctx, inp.config)


def test_partial_without_noise_is_hit_mode_and_hit_mode_returns(ctx):
    inp = Inputs("be10dp")
    resp = get_response(inp.config)
    n, seed, first = 48, SEED_HI, (1 << 32) - 9
    fresh = _abi.Context(0)
    try:
        plain = _engine(inp, fresh)
        want = {}
        for thr in (0.0, 40.0):
            plain.configure_traces(inp.config, resp, thr, 0)
            want[thr] = plain.run_traces(n, seed=seed, first_event=first)
        plain.configure_traces(inp.config, resp, 40.0, 0, noise_sigma=5.0, pedestals=_pedestals(3))
        noisy_want = plain.run_traces(n, seed=seed, first_event=first)

        eng = _engine(inp, ctx)
        all_pads = np.ones(_abi.NUM_PADS, dtype=bool)
        for thr in (0.0, 40.0):
            eng.configure_traces(inp.config, resp, thr, 0, readout="partial", readout_pads=all_pads)
            got = eng.run_traces(n, seed=seed, first_event=first)
            for key in ("offsets", "pads", "samples", "labels", "event_points"):
                np.testing.assert_array_equal(got[key], want[thr][key], err_msg=key)
            assert got["trace"] == want[thr]["trace"]
        # hit mode after a full and a partial run is a fresh context's hit mode
        for mode in ("full", "partial"):
            eng.configure_traces(inp.config, resp, 20.0, 0, noise_sigma=5.0, pedestals=_pedestals(3), readout=mode)
            eng.run_traces(4, seed=seed, first_event=first)
            eng.configure_traces(inp.config, resp, 40.0, 0, noise_sigma=5.0, pedestals=_pedestals(3))
            got = eng.run_traces(n, seed=seed, first_event=first)
            for key in ("offsets", "pads", "samples", "labels", "event_points"):
                np.testing.assert_array_equal(got[key], noisy_want[key], err_msg=key)
            assert got["trace"] == noisy_want["trace"]
    finally:
        _reset(ctx, inp.config)
        fresh.close()


def test_full_readout_offsets_and_pads(ctx):
    inp = Inputs("o16aa")
    mask = readout_mask(None).astype(bool)
    mask[::3] = False
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, noise_sigma=2.0, readout="full", readout_pads=np.flatnonzero(mask))
    n = 6
    res = eng.run_traces(n, seed=3, first_event=(1 << 40) - 2)
    s = int(mask.sum())
    np.testing.assert_array_equal(res["offsets"], np.arange(n + 1) * s)
    np.testing.assert_array_equal(res["pads"], np.tile(np.flatnonzero(mask), n))
    assert res["trace"]["n_rows"] == n * s and (res["labels"] != -1).any()
    _reset(ctx, inp.config)


def test_chunk_buffer_and_fetch_invariance(ctx):
    inp = Inputs("be10dp")
    kw = {"noise_sigma": 5.0, "pedestals": 100, "noise_stream": 2, "threshold": 20.0, "readout": "partial"}
    seed, first, n = SEED_HI, (1 << 33) + 10, 40

    def run(e, **more):
        res = e.run_traces(n, seed=seed, first_event=first, **more)
        return (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"])

    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    whole = run(eng)
    assert (whole[3] == -1).sum() > 50 * n  # noise-only rows in every event
    assert eng.run_traces(n, seed=seed, first_event=first, fetch=False)["trace"] == whole[4]
    small = _engine(inp, ctx, chunk_events=16)
    small.configure_traces(inp.config, **kw)
    _assert_same(run(small), whole)
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    tiny_ctx = _abi.Context(0)
    try:
        tiny_ctx.set_option("tiny_buffers", 1)
        tiny = _engine(inp, tiny_ctx)
        tiny.configure_traces(inp.config, **kw)
        _assert_same(run(tiny), whole)
        full_kw = dict(kw, readout="full")
        tiny.configure_traces(inp.config, **full_kw)
        eng.configure_traces(inp.config, **full_kw)
        _assert_same(run(tiny), run(eng))
        assert tiny.run_traces(n, seed=seed, first_event=first, fetch=False)["trace"] == run(eng)[4]
    finally:
        tiny_ctx.close()
        _reset(ctx, inp.config)


# The chunk planner's bound on a readout run's device memory: two assembly sets of trace outputs, each of at most
# TRACE_CHUNK_ROWS (abi.hip) kept rows with 1/8 headroom, at 1 036 B a row (samples, pad, label), plus a stated margin
# for the cloud side of the chunks (scatter arena, event-ordered clouds, per-event scratch): about 13 GB.  A chunk sized
# without the planner -- 2 048 events of 10 118 rows -- needs 24 GB of trace outputs alone.
TRACE_CHUNK_ROWS = 4 << 20
ROW_BYTES = 512 * 2 + 4 + 8
READOUT_DEVICE_BOUND = 2 * TRACE_CHUNK_ROWS * 9 // 8 * ROW_BYTES + (3 << 30)


def _rows_without_samples(ctx, layout, n, seed, first, capacity):
    """attpc_sim_run_traces into offsets, pads, labels and event points only (the samples stay on the device) ->
    (offsets, pads, labels, event_points, out, stats)."""
    offsets = np.zeros(n + 1, dtype=np.int64)
    pads = np.empty(capacity, dtype=np.int32)
    labels = np.empty(capacity, dtype=np.int64)
    event_points = np.zeros(n, dtype=np.int64)
    out = _abi.TraceOut(capacity, _abi.iptr(offsets, _abi.C.c_int64), _abi.iptr(pads, _abi.C.c_int32), None,
                        _abi.iptr(labels, _abi.C.c_int64), _abi.iptr(event_points, _abi.C.c_int64))
    stats = _abi.RunStats()
    ctx.check(ctx.lib.attpc_sim_run_traces(ctx.handle, seed, first, n, layout, None, None, None, out, stats),
              "attpc_sim_run_traces")
    return offsets, pads[:out.n_rows], labels[:out.n_rows], event_points, out, stats


def test_fresh_context_full_readout_device_memory():
    """2 048 delivered full-readout events (pads, labels and offsets to the host; the 21 GB of samples stay on the
    device) on a fresh context: the chunks are sized by |S| from the first one, so the device holds at most
    READOUT_DEVICE_BOUND, where one unplanned chunk of all 2 048 events would need 24 GB of trace outputs."""
    inp = Inputs("o16aa")
    fresh = _abi.Context(0)
    try:
        eng = _engine(inp, fresh)
        eng.configure_traces(inp.config, readout="full")
        s = int(readout_mask(None).sum())
        n = 2048
        assert n * s * 9 // 8 * ROW_BYTES > READOUT_DEVICE_BOUND + (8 << 30)
        offsets, pads, labels, event_points, out, stats = _rows_without_samples(fresh, eng.layout, n, 5, 0, n * s)
        assert out.n_rows == n * s
        np.testing.assert_array_equal(offsets, np.arange(n + 1) * s)
        np.testing.assert_array_equal(pads, np.tile(np.flatnonzero(readout_mask(None)), n))
        assert (labels != -1).any() and event_points.sum() == stats.n_points
        assert 0 < stats.device_bytes < READOUT_DEVICE_BOUND, (stats.device_bytes, READOUT_DEVICE_BOUND)
    finally:
        fresh.close()


def test_threshold_change_keeps_readout_chunks_bounded():
    """A threshold sweep in partial readout: thr 20 keeps about 540 rows per event, thr 10 nearly every pad of S.  The
    run at thr 10 must not size its chunks from the rate the run at thr 20 saw (7 767 events a chunk: 2 048 events of
    10 000 rows, 24 GB of trace outputs, in one chunk)."""
    inp = Inputs("o16aa")
    fresh = _abi.Context(0)
    try:
        eng = _engine(inp, fresh)
        s = int(readout_mask(None).sum())
        kw = {"noise_sigma": 5.0, "pedestals": 100, "readout": "partial"}
        eng.configure_traces(inp.config, threshold=20.0, **kw)
        first = _rows_without_samples(fresh, eng.layout, 1024, 5, 0, 1024 * s)
        assert 300 * 1024 < first[4].n_rows < 1000 * 1024
        eng.configure_traces(inp.config, threshold=10.0, **kw)
        n = 2048
        offsets, pads, labels, event_points, out, stats = _rows_without_samples(fresh, eng.layout, n, 5, 1024, n * s)
        assert out.n_rows > 0.99 * n * s and (np.diff(offsets) <= s).all()
        assert 0 < stats.device_bytes < READOUT_DEVICE_BOUND, (stats.device_bytes, READOUT_DEVICE_BOUND)
    finally:
        fresh.close()


def _traces_at_rows(ctx, n, seed, first, capacity):
    """attpc_traces_at on n events without rows into offsets, pads and labels only -> (offsets, pads, labels, out)."""
    ev = np.zeros(n + 1, dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    pads = np.empty(capacity, dtype=np.int32)
    labels = np.empty(capacity, dtype=np.int64)
    out = _abi.TraceOut(capacity, _abi.iptr(offsets, _abi.C.c_int64), _abi.iptr(pads, _abi.C.c_int32), None,
                        _abi.iptr(labels, _abi.C.c_int64), None)
    ctx.check(ctx.lib.attpc_traces_at(ctx.handle, seed, first, n, _abi.iptr(ev, _abi.C.c_int64), None, None, out),
              "attpc_traces_at")
    return offsets, pads[:out.n_rows], labels[:out.n_rows], out


def test_pedestal_run_through_traces_at_in_chunks(ctx):
    """900 empty events in full readout of every pad: attpc_traces_at takes them in chunks of TRACE_CHUNK_ROWS / 10 240
    = 409 events.  The rows and both checksums equal those of three calls split elsewhere (200, 500 and 200 events)."""
    inp = Inputs("o16aa")
    configure_traces(inp.config, ctx, None, 20.0, 0, noise_sigma=5.0, pedestals=100, readout="full",
                     readout_pads=np.ones(_abi.NUM_PADS, dtype=bool))
    seed, first, n, s = SEED_HI, (1 << 32) - 450, 900, _abi.NUM_PADS
    offsets, pads, labels, out = _traces_at_rows(ctx, n, seed, first, n * s)
    np.testing.assert_array_equal(offsets, np.arange(n + 1) * s)
    np.testing.assert_array_equal(pads, np.tile(np.arange(s), n))
    assert (labels == -1).all()
    ids = np.arange(n, dtype=np.uint64) + np.uint64(first)
    pad_sum = (int(((ids << np.uint64(14)) * np.uint64(s)).sum(dtype=np.uint64)) + n * (s * (s - 1) // 2)) % (1 << 64)
    assert out.pad_checksum == pad_sum
    sample_sum, rows = 0, 0
    for a, b in ((0, 200), (200, 700), (700, 900)):
        part = _traces_at_rows(ctx, b - a, seed, first + a, (b - a) * s)[3]
        sample_sum += part.sample_checksum
        rows += part.n_rows
    assert rows == out.n_rows and sample_sum % (1 << 64) == out.sample_checksum
    _reset(ctx, inp.config)


def test_layout_without_simulated_nuclei_gets_noise_only_rows(ctx):
    """A layout with n_sim = 0 scatters nothing; in a readout mode every event still gets its noise-only rows, those
    of the restatement for events without rows."""
    import ctypes

    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    layout = _abi.EventLayout()
    ctypes.pointer(layout)[0] = eng.layout
    layout.n_sim = 0
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[::9] = True
    ped = _pedestals(5)
    resp = get_response(inp.config)
    n, seed, first = 5, 77, (1 << 32) - 2
    empty = (np.zeros(n + 1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    for mode, thr in (("full", 20.0), ("partial", 6.0)):
        eng.configure_traces(inp.config, resp, thr, 0, noise_sigma=2.0, pedestals=ped, readout=mode,
                             readout_pads=mask)
        from attpc_engine_amd.detector.traces import TraceArrays

        arrays = TraceArrays(n, n * int(mask.sum()))
        stats = _abi.RunStats()
        ctx.check(ctx.lib.attpc_sim_run_traces(ctx.handle, seed, first, n, layout, None, None, None, arrays.out,
                                               stats), "attpc_sim_run_traces")
        got = (*arrays.result(), arrays.sums())
        ref = readout_traces(*empty, resp, thr, 0, _noise(2.0, ped), seed, first, MODES[mode], mask)
        _assert_same(got, ref)
        assert got[4]["n_rows"] > 0 and (arrays.event_points == 0).all()
    _reset(ctx, inp.config)


def test_empty_events_noise_pads_match_expectation(ctx):
    inp = Inputs("o16aa")
    sigma, thr, ped = 5.0, 20.0, 100
    cdf, lo = gaussian_noise_table(sigma)
    configure_traces(inp.config, ctx, None, thr, 0, noise_sigma=sigma, pedestals=ped, readout="partial")
    n = 64
    offsets = np.zeros(n + 1, dtype=np.int64)
    got = clouds_to_traces(offsets, np.zeros((0, 3)), np.zeros(0, dtype=np.int64), ctx, seed=SEED_HI, first_event=9)
    per_pad = expected_noise_pads((cdf, lo), thr, None, ped) / readout_mask(None).sum()
    want = n * expected_noise_pads((cdf, lo), thr, None, ped)
    sd = math.sqrt(want * (1 - per_pad))
    assert abs(got[4]["n_rows"] - want) < 5 * sd, (got[4]["n_rows"], want, sd)
    assert (got[3] == -1).all() and not np.isin(got[1], np.flatnonzero(readout_mask(None) == 0)).any()
    ref = readout_traces(offsets[:3], np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros(512), thr, 0,
                         _noise(sigma, np.full(_abi.NUM_PADS, ped, dtype=np.int16)), SEED_HI, 9, PARTIAL,
                         readout_mask(None).astype(bool))
    k = int(got[0][2])
    _assert_same((got[0][:3], got[1][:k], got[2][:k], got[3][:k], ref[4]), ref)
    # a pedestal run: full readout of empty events
    configure_traces(inp.config, ctx, None, thr, 0, noise_sigma=sigma, pedestals=ped, readout="full",
                     readout_pads=np.arange(0, _abi.NUM_PADS, 7))
    got = clouds_to_traces(offsets[:5], np.zeros((0, 3)), np.zeros(0, dtype=np.int64), ctx, seed=SEED_HI, first_event=9)
    ref = readout_traces(offsets[:5], np.zeros((0, 3)), np.zeros(0, dtype=np.int64), np.zeros(512), thr, 0,
                         _noise(sigma, np.full(_abi.NUM_PADS, ped, dtype=np.int16)), SEED_HI, 9, FULL,
                         readout_mask(np.arange(0, _abi.NUM_PADS, 7)).astype(bool))
    _assert_same(got, ref)
    _reset(ctx, inp.config)


def test_cloud_and_spyral_unchanged_beside_readout_runs(ctx):
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_spyral(inp.config)
    before = (eng.run(40, seed=2, first_event=3, fetch=True), eng.run_spyral(40, seed=2, first_event=3),
              eng.run(40, seed=2, first_event=3)["stats"])
    for mode in ("partial", "full"):
        eng.configure_traces(inp.config, threshold=20.0, noise_sigma=5.0, pedestals=_pedestals(9), readout=mode)
        eng.run_traces(8, seed=2, first_event=3)
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
    _reset(ctx, inp.config)


def test_writers_forward_the_readout(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd.detector import TraceWriter
    from attpc_engine_amd.engine import run_fused
    from tests.test_gpu_traces import _read_trace_files

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n, seed, thr = 6, 17, 11.0
    resp = get_response(inp.config)
    ped = _pedestals(12)
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[::2] = True
    kw = {"noise_sigma": 3.0, "pedestals": ped, "noise_stream": 9, "readout": "partial", "readout_pads": mask,
          "threshold": thr}
    noise = _noise(3.0, ped, 9)
    cloud = _engine(inp, ctx).run(n, seed=seed, first_event=0, fetch=True)
    fused_dir = tmp_path / "fused"
    fused_dir.mkdir()
    run_fused(inp.pipeline, inp.config, TraceWriter(fused_dir, inp.config, max_events_per_file=4, **kw), n,
              inp.indices, seed=seed, batch_size=4, context=ctx)
    ref = readout_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, 0, noise, seed, 0, PARTIAL,
                         mask)
    raw = np.diff(cloud["offsets"])
    want = {e: tuple(a[ref[0][e]:ref[0][e + 1]] for a in ref[1:4]) for e in range(n) if raw[e] > 0}
    got = _read_trace_files(fused_dir)
    assert sorted(got) == sorted(want)
    for e in want:
        for a, b in zip(got[e], want[e]):
            np.testing.assert_array_equal(a, b)
    # the per-event write() path: noise keyed on (noise_seed, event_number)
    one_dir = tmp_path / "one"
    one_dir.mkdir()
    w = TraceWriter(one_dir, inp.config, noise_seed=SEED_HI, **kw)
    lo, hi = cloud["offsets"][3], cloud["offsets"][4]
    w.write(cloud["points"][lo:hi], cloud["labels"][lo:hi], inp.config, 1 << 40)
    w.close()
    ref = readout_traces([0, hi - lo], cloud["points"][lo:hi], cloud["labels"][lo:hi], resp, thr, 0, noise, SEED_HI,
                         1 << 40, PARTIAL, mask)
    got = _read_trace_files(one_dir)[1 << 40]
    for a, b in zip(got, ref[1:4]):
        np.testing.assert_array_equal(a, b)
    assert (ref[3] == -1).any()
    _reset(ctx, inp.config)
