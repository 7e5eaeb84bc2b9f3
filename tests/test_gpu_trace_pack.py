"""Packed pad traces on the device (include/attpc_engine.h, "packed pad traces"): the pack stage alone against the
numpy encoder byte for byte, and every packed entry point against its plain counterpart of the same seed -- the decoded
samples bit for bit, every other output equal, n_bytes equal to the reference encoder's size of the plain samples.
Needs a real MI355X: ``-m gpu``."""
import ctypes

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (CommonModeSettings, TriggerSettings, clouds_to_traces, configure_common_mode,
                                              configure_traces, configure_trigger, pack_traces, simulate_batch_traces,
                                              unpack_traces)
from tests import trace_pack_reference as ref
from tests.helpers import Inputs
from tests.test_gpu_traces import _csr, _hand_made_events

pytestmark = pytest.mark.gpu

N, SEED, FIRST, CHUNK = 48, 21, 7, 16  # three chunks: row_start is rebased twice


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _pedestals(seed):
    return np.random.default_rng(seed).integers(250, 350, _abi.NUM_PADS).astype(np.int16)


@pytest.fixture(scope="module")
def inp():
    return Inputs("o16aa")


NOISY = dict(threshold=20.0, noise_sigma=5.0, pedestals=_pedestals(3), readout="partial")  # 4 sigma: noise-only pads stay
COMMON = CommonModeSettings(sigma=3.0, groups=(np.arange(_abi.NUM_PADS) // 256).astype(np.uint8), stream=2)


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine

    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _reset(ctx, config):
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    ctx.set_option("trace_pack_workgroups", 0)
    configure_common_mode(ctx, None)
    configure_trigger(ctx, None)
    configure_traces(config, ctx, None, None, 0)


# ---------------------------------------------------------------- the stage alone ----
@pytest.mark.parametrize("workgroups", [0, 2], ids=["full_grid", "two_workgroups"])
def test_stage_alone_equals_the_reference_encoder(ctx, workgroups):
    """Edge rows one kind at a time, then R = 1, 65 and 1 000 mixed rows: more rows than a workgroup has waves, and with
    two workgroups (8 waves) 125 grid strides."""
    noisy, clean = ref.random_rows(680, seed=5), ref.random_rows(300, seed=6, pedestal=0, sigma=0.0)
    mixed = np.concatenate([ref.all_edge_rows(), noisy, clean])  # 20 + 680 + 300
    assert len(mixed) == 1000
    cases = {**ref.edge_rows(), "one": mixed[17:18], "r65": mixed[:65], "r1000": mixed}
    ctx.set_option("trace_pack_workgroups", workgroups)
    try:
        for name, rows in cases.items():
            row_start, packed = pack_traces(rows, ctx)
            want_start, want = ref.encode(rows)
            np.testing.assert_array_equal(row_start, want_start, err_msg=name)
            np.testing.assert_array_equal(packed, want, err_msg=name)
        np.testing.assert_array_equal(unpack_traces(*pack_traces(mixed, ctx)), mixed)
        row_start, packed = pack_traces(np.zeros((0, 512), dtype=np.int16), ctx)
        assert row_start.tolist() == [0] and len(packed) == 0
    finally:
        ctx.set_option("trace_pack_workgroups", 0)


def test_stage_alone_refuses_bad_samples_and_reports_the_bytes_it_needs(ctx):
    rows = ref.random_rows(20, seed=7)
    want_start, want = ref.encode(rows)
    row_start, n_bytes = np.zeros(21, dtype=np.int64), ctypes.c_int64()
    args = (ctx.handle, 20, _abi.iptr(rows, ctypes.c_int16), _abi.iptr(row_start, ctypes.c_int64))
    small = np.zeros(len(want) - 8, dtype=np.uint8)
    status = ctx.lib.attpc_trace_pack(*args, _abi.iptr(small, ctypes.c_uint8), len(small), ctypes.byref(n_bytes))
    assert status == _abi.E_CAPACITY and n_bytes.value == len(want)
    np.testing.assert_array_equal(row_start, want_start)
    assert ctx.lib.attpc_trace_pack(*args, None, 0, ctypes.byref(n_bytes)) == _abi.OK and n_bytes.value == len(want)  # sizes only
    for bad in (-1, 4096):
        spoiled = rows.copy()
        spoiled[11, 500] = bad
        with pytest.raises(ValueError):
            pack_traces(spoiled, ctx)
        status = ctx.lib.attpc_trace_pack(ctx.handle, 20, _abi.iptr(spoiled, ctypes.c_int16), None, None, 0, None)
        assert status == _abi.E_INVALID


# ---------------------------------------------------------------- fused ----
def _configure(eng, inp, noisy):
    if noisy:
        eng.configure_traces(inp.config, **NOISY)
        eng.configure_common_mode(COMMON)
    else:
        eng.configure_traces(inp.config)
        eng.configure_common_mode()


@pytest.fixture(scope="module", params=[False, True], ids=["noiseless_hit", "noisy_partial_common"])
def fused(ctx, inp, request):
    """The plain and the packed run of the same 48 events in three chunks, computed once and read-only."""
    eng = _engine(inp, ctx, chunk_events=CHUNK)
    _configure(eng, inp, request.param)
    try:
        plain = eng.run_traces(N, seed=SEED, first_event=FIRST)
        packed = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True)
        resident = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True, fetch=False)
    finally:
        _reset(ctx, inp.config)
    for res in (plain, packed):
        for value in res.values():
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
    return inp, request.param, plain, packed, resident


def _assert_packed_equals_plain(packed, plain, what=""):
    assert "samples" not in packed and packed["packed"].dtype == np.uint8 and packed["row_start"].dtype == np.int64
    np.testing.assert_array_equal(unpack_traces(packed["row_start"], packed["packed"]), plain["samples"], err_msg=what)
    for key in ("offsets", "pads", "labels", "event_points"):
        np.testing.assert_array_equal(packed[key], plain[key], err_msg=f"{what} {key}")
    want_start, want = ref.encode(plain["samples"])
    np.testing.assert_array_equal(packed["row_start"], want_start, err_msg=what)
    np.testing.assert_array_equal(packed["packed"], want, err_msg=what)
    trace = dict(packed["trace"])
    assert trace.pop("n_bytes") == len(want) and trace == plain["trace"], (what, packed["trace"], plain["trace"])


def test_fused_packed_run_equals_the_plain_run(fused):
    inp, noisy, plain, packed, _ = fused
    assert plain["trace"]["n_rows"] > 10 * N and plain["offsets"][CHUNK] < plain["offsets"][2 * CHUNK] < plain["offsets"][N]
    _assert_packed_equals_plain(packed, plain)
    for key in ("p4", "vertex", "status"):
        np.testing.assert_array_equal(packed[key], plain[key], err_msg=key)
    for key in ("n_events", "n_points", "n_track_samples", "n_sample_limit", "n_failed", "charge_checksum", "key_checksum",
                "n_inconsistent", "n_tracks_capped"):  # (not the timings, launch counts and buffer sizes)
        assert packed["stats"][key] == plain["stats"][key], key
    if noisy:
        assert (plain["labels"] == -1).any()  # noise-only pads were kept
    # one event decodes alone
    e = N - 5
    lo, hi = plain["offsets"][e], plain["offsets"][e + 1]
    np.testing.assert_array_equal(unpack_traces(packed["row_start"], packed["packed"], rows=slice(lo, hi)), plain["samples"][lo:hi])


def test_resident_packed_run_reports_the_delivered_sums(fused):
    _, _, _, packed, resident = fused
    assert resident["trace"] == packed["trace"] and resident["trace"]["n_bytes"] > 0
    assert set(resident) <= {"stats", "trace", "trigger"}


def test_capacity_retry_returns_the_same_bytes(ctx, fused):
    inp, noisy, _, packed, _ = fused
    eng = _engine(inp, ctx, chunk_events=CHUNK)
    _configure(eng, inp, noisy)
    try:
        # the C ABI first: too few bytes, then too few rows -- both needs are reported either way
        from attpc_engine_amd.outputs import PackedTraceArrays

        n_rows, n_bytes = packed["trace"]["n_rows"], packed["trace"]["n_bytes"]
        for capacity, byte_capacity in ((n_rows, n_bytes - 8), (n_rows - 1, n_bytes)):
            arrays, stats = PackedTraceArrays(N, capacity, byte_capacity=byte_capacity), _abi.RunStats()
            status = ctx.lib.attpc_sim_run_traces_packed(ctx.handle, SEED, FIRST, N, eng.layout, None, None, None, arrays.out, stats)
            assert status == _abi.E_CAPACITY
            assert (arrays.out.n_rows, arrays.out.n_bytes) == (n_rows, n_bytes)
        arrays = PackedTraceArrays(N, n_rows, byte_capacity=n_bytes)  # exactly enough of both
        ctx.check(ctx.lib.attpc_sim_run_traces_packed(ctx.handle, SEED, FIRST, N, eng.layout, None, None, None, arrays.out, stats),
                  "attpc_sim_run_traces_packed")
        np.testing.assert_array_equal(arrays.result()[3], packed["packed"])
        # through the retry of the run layer: 16 bytes per row never fit these rows; one row per event neither
        for kw in ({"packed_bytes_per_row": 16}, {"capacity_per_event": 1}):
            again = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True, **kw)
            np.testing.assert_array_equal(again["packed"], packed["packed"], err_msg=str(kw))
            np.testing.assert_array_equal(again["row_start"], packed["row_start"], err_msg=str(kw))
            assert again["trace"] == packed["trace"]
    finally:
        _reset(ctx, inp.config)


def test_pinned_packed_run(ctx, fused):
    inp, noisy, _, packed, _ = fused
    eng = _engine(inp, ctx, chunk_events=CHUNK)
    _configure(eng, inp, noisy)
    try:
        pinned = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True, pinned=True)
        np.testing.assert_array_equal(pinned["packed"], packed["packed"])
        np.testing.assert_array_equal(pinned["row_start"], packed["row_start"])
    finally:
        _reset(ctx, inp.config)


def test_events_without_rows(ctx, inp):
    """A layout with no simulated nucleus scatters nothing: in hit mode every event of the run has no rows, the packed
    run delivers offsets of zeros, row_start = [0] and no bytes -- as the plain run delivers no samples."""
    eng = _engine(inp, ctx, chunk_events=CHUNK)
    eng.configure_traces(inp.config)
    layout = _abi.EventLayout()
    ctypes.pointer(layout)[0] = eng.layout
    layout.n_sim = 0
    eng.layout = layout
    try:
        plain = eng.run_traces(N, seed=SEED, first_event=FIRST)
        packed = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True)
        assert plain["trace"]["n_rows"] == 0 and packed["row_start"].tolist() == [0] and len(packed["packed"]) == 0
        _assert_packed_equals_plain(packed, plain)
        assert eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True, fetch=False)["trace"] == packed["trace"]
    finally:
        _reset(ctx, inp.config)


# ---------------------------------------------------------------- host cloud and batch paths ----
def test_host_cloud_path(ctx, inp):
    """The hand-made clouds of tests/test_gpu_traces.py: an empty event, an event that keeps no pad, 300 pads."""
    resp = get_response(inp.config)
    offsets, points, labels = _csr(_hand_made_events(resp))
    try:
        for kw in ({"threshold": 40.0}, {"threshold": 20.0, "noise_sigma": 4.0, "pedestals": _pedestals(4)}):
            configure_traces(inp.config, ctx, resp, offset=0, **kw)
            plain = clouds_to_traces(offsets, points, labels, ctx, seed=3, first_event=11)
            packed = clouds_to_traces(offsets, points, labels, ctx, seed=3, first_event=11, packed=True)
            keys = ("offsets", "pads", "samples", "labels", "trace")
            got = dict(zip(("offsets", "pads", "row_start", "packed", "labels", "trace"), packed), event_points=None)
            want = dict(zip(keys, plain), event_points=None)
            assert want["offsets"][4] == want["offsets"][5]  # the empty event
            _assert_packed_equals_plain(got, want, str(kw))
    finally:
        _reset(ctx, inp.config)


def test_batch_path(ctx, fused):
    inp, noisy, plain, _, _ = fused
    kw = {**NOISY, "common_mode": COMMON} if noisy else {}
    n = 20
    args = (plain["p4"][:n], plain["vertex"][:n], inp.z, inp.a, inp.config, SEED, inp.indices)
    try:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 8), "attpc_set_chunk_events")
        off, pads, samples, labels, raw, stats = simulate_batch_traces(*args, first_event=FIRST, ctx=ctx, **kw)
        p_off, p_pads, row_start, packed, p_labels, p_raw, p_stats = simulate_batch_traces(*args, first_event=FIRST, ctx=ctx,
                                                                                          packed=True, **kw)
        sums = ("n_rows", "sample_checksum", "pad_checksum")
        _assert_packed_equals_plain(
            dict(offsets=p_off, pads=p_pads, row_start=row_start, packed=packed, labels=p_labels, event_points=p_raw,
                 trace={k: p_stats[k] for k in (*sums, "n_bytes")}),
            dict(offsets=off, pads=pads, samples=samples, labels=labels, event_points=raw, trace={k: stats[k] for k in sums}))
        # the file-driven run of the fused run's own kinematics gives the fused run's rows
        np.testing.assert_array_equal(samples, plain["samples"][:plain["offsets"][n]])
    finally:
        _reset(ctx, inp.config)


# ---------------------------------------------------------------- trigger ----
def test_trigger_records_are_those_of_the_plain_call(ctx, inp):
    eng = _engine(inp, ctx, chunk_events=CHUNK)
    eng.configure_traces(inp.config, **NOISY)
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=5, min_groups=1))  # one group, 5 pads in 50 samples
    try:
        plain = eng.run_traces(N, seed=SEED, first_event=FIRST)
        packed = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True)
        resident = eng.run_traces(N, seed=SEED, first_event=FIRST, packed=True, fetch=False)
        assert plain["trigger"]["fired"].any() and len(plain["trigger"]) == N
        assert packed["trigger"].tobytes() == plain["trigger"].tobytes() == resident["trigger"].tobytes()
        _assert_packed_equals_plain(packed, plain)
    finally:
        _reset(ctx, inp.config)
