"""Packed pad traces on the host (include/attpc_engine.h, "packed pad traces"): the host encoder against the numpy
restatement byte for byte, the decoder's round trip and its refusals, and the Python layer around them (unpack_traces,
the packed TraceWriter, read_traces, the flag's validation).  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.traces import PackedRows, pack_traces_host, unpack_traces
from tests import trace_pack_reference as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


@pytest.fixture(scope="module")
def config():
    from attpc_engine_amd import workloads

    return workloads.be10dp()[1]


@pytest.fixture(scope="module")
def noisy():
    return ref.random_rows(300, seed=1)


def _unpack(lib, row_start, packed, n_threads=0, n_bytes=None):
    row_start = np.ascontiguousarray(row_start, dtype=np.int64)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    out = np.full((len(row_start) - 1, 512), -1, dtype=np.int16)
    status = lib.attpc_trace_unpack(_abi.iptr(packed, C.c_uint8), len(packed) if n_bytes is None else n_bytes,
                                    _abi.iptr(row_start, C.c_int64), len(out), _abi.iptr(out, C.c_int16), n_threads)
    return status, out


# ---------------------------------------------------------------- the format's sizes, from the reference itself
def test_reference_sizes_and_round_trip():
    rows = ref.edge_rows()
    size = lambda r: np.diff(ref.encode(r)[0])  # noqa: E731
    assert size(rows["zeros"]).tolist() == [16] and size(rows["full"]).tolist() == [16]
    assert size(rows["alternating"]).tolist() == [784] and size(rows["constant7"]).tolist() == [16]
    assert ref.encode(rows["constant7"])[1][:2].view("<u2")[0] == 7  # base 7, width 0
    # range 2^k - 1 takes k planes, range 2^k takes k + 1 (at 100 and against 4095)
    assert size(rows["width_steps"]).tolist() == [16 + 8 * (k + (k + 1) + (k + 1)) for k in range(12)]
    every = ref.all_edge_rows()
    assert np.array_equal(ref.decode(*ref.encode(every)), every)


# ---------------------------------------------------------------- host encoder and decoder
@pytest.mark.parametrize("name", ["zeros", "full", "alternating", "constant7", "width_steps", "single", "noisy", "noiseless",
                                  "empty"])
def test_host_encoder_equals_reference_and_decodes(lib, noisy, name):
    rows = {"noisy": noisy, "noiseless": ref.random_rows(100, seed=2, pedestal=0, sigma=0.0),
            "empty": np.zeros((0, 512), dtype=np.int16), **ref.edge_rows()}[name]
    row_start, packed = pack_traces_host(rows)
    want_start, want = ref.encode(rows)
    assert row_start.dtype == np.int64 and packed.dtype == np.uint8
    assert np.array_equal(row_start, want_start) and np.array_equal(packed, want)
    status, back = _unpack(lib, row_start, packed)
    assert status == _abi.OK and np.array_equal(back, rows)
    assert np.array_equal(unpack_traces(row_start, packed), rows)


def test_base_is_lowered_where_minimum_plus_width_would_pass_4095(lib):
    """Minimum 290, maximum 4095: w = 12, and the base is 4096 - 2^12 = 0 -- the header alone keeps every decodable
    sample inside 0 .. 4095, and the row still comes back."""
    row = np.full((1, 512), 290, dtype=np.int16)
    row[0, 70] = 4095
    row_start, packed = pack_traces_host(row)
    headers = packed[:16].view("<u2")
    assert headers[0] == 290 and headers[1] == (12 << 12 | 0)
    assert np.array_equal(packed, ref.encode(row)[1]) and np.array_equal(unpack_traces(row_start, packed), row)


def test_host_encoder_capacity_and_invalid_samples(lib, noisy):
    rows = noisy[:10]
    want_start, want = ref.encode(rows)
    row_start, n_bytes = np.zeros(11, dtype=np.int64), C.c_int64()
    args = (10, _abi.iptr(rows, C.c_int16), _abi.iptr(row_start, C.c_int64))
    assert lib.attpc_trace_pack_host(*args, None, 0, C.byref(n_bytes)) == _abi.OK  # sizes only
    assert n_bytes.value == len(want) and np.array_equal(row_start, want_start)
    small = np.full(len(want) - 8, 0xAA, dtype=np.uint8)
    guard = small.copy()
    assert lib.attpc_trace_pack_host(*args, _abi.iptr(small, C.c_uint8), len(small), C.byref(n_bytes)) == _abi.E_CAPACITY
    assert n_bytes.value == len(want)
    fit = int(want_start[9])  # the rows that fit in front are written, nothing behind them
    assert np.array_equal(small[:fit], want[:fit]) and np.array_equal(small[fit:], guard[fit:])
    for bad in (-1, 4096):
        rows_bad = rows.copy()
        rows_bad[3, 17] = bad
        assert lib.attpc_trace_pack_host(10, _abi.iptr(rows_bad, C.c_int16), None, None, 0, C.byref(n_bytes)) == _abi.E_INVALID
        with pytest.raises(ValueError):
            pack_traces_host(rows_bad)


@pytest.mark.parametrize("n_threads", [1, 3, 0])
def test_decoder_thread_counts(lib, n_threads):
    rows = np.concatenate([ref.random_rows(400, seed=3)] * 32)  # 12 800 rows: more than one thread's share
    row_start, packed = pack_traces_host(rows)
    status, back = _unpack(lib, row_start, packed, n_threads)
    assert status == _abi.OK and np.array_equal(back, rows)


def test_decoder_refuses_malformed_records(lib, noisy):
    rows = noisy[:6]
    row_start, packed = pack_traces_host(rows)
    ok, _ = _unpack(lib, row_start, packed)
    assert ok == _abi.OK

    def refused(start=row_start, data=packed, n_bytes=None):
        status, _ = _unpack(lib, start, data, 1, n_bytes)
        with pytest.raises(ValueError):
            ref.decode(start, data[:len(data) if n_bytes is None else n_bytes])
        return status == _abi.E_INVALID

    # a record whose header-implied size differs from its span (one plane word more / less in the middle row)
    for delta in (8, -8):
        start = row_start.copy()
        start[3] += delta
        assert refused(start)
    # w > 12
    data = packed.copy()
    data[int(row_start[2]) + 1] = (13 << 4) | (data[int(row_start[2]) + 1] & 0x0f)
    assert refused(data=data)
    # base + 2^w - 1 > 4095: width 3 on a base of 4090, with the span grown to match so that only this rule refuses it
    one = np.full((1, 512), 4090, dtype=np.int16)
    one[0, :8] = np.arange(4088, 4096) - 2
    start1, data1 = pack_traces_host(one)
    header = data1[:2].view("<u2")
    assert header[0] >> 12 == 3 and (header[0] & 0xfff) + 7 <= 4095
    data1 = data1.copy()
    data1[:2].view("<u2")[0] = (3 << 12) | 4090
    assert refused(start1, data1)
    # offsets that decrease, and offsets that are no multiples of 8
    start = row_start.copy()
    start[2], start[3] = row_start[3], row_start[2]
    assert refused(start)
    assert refused(row_start + 4, np.concatenate([np.zeros(4, np.uint8), packed]))
    start = row_start.copy()
    start[0] = -8
    assert refused(start)
    # a span past n_bytes
    assert refused(n_bytes=len(packed) - 8)
    start = row_start.copy()
    start[-1] += 8
    assert refused(start)


def test_decoder_reads_nothing_past_a_short_record(lib):
    """A span shorter than the 16 header bytes is refused before the header is read."""
    status, _ = _unpack(lib, np.array([0, 8]), np.zeros(8, dtype=np.uint8))
    assert status == _abi.E_INVALID


# ---------------------------------------------------------------- the Python layer
def test_unpack_traces_subsets(noisy):
    row_start, packed = pack_traces_host(noisy)
    assert np.array_equal(unpack_traces(row_start, packed, rows=slice(40, 75)), noisy[40:75])
    assert unpack_traces(row_start, packed, rows=slice(5, 5)).shape == (0, 512)
    index = np.array([7, 0, 299, 7, -2])
    assert np.array_equal(unpack_traces(row_start, packed, rows=index), noisy[index])
    assert np.array_equal(unpack_traces(row_start, packed, rows=slice(0, 300, 7), n_threads=2), noisy[::7])
    mask = np.zeros(300, dtype=bool)
    mask[[3, 150]] = True
    assert np.array_equal(unpack_traces(row_start, packed, rows=mask), noisy[mask])
    with pytest.raises(IndexError):
        unpack_traces(row_start, packed, rows=[300])
    with pytest.raises(ValueError):
        unpack_traces(row_start, packed[:-8])
    event = PackedRows(row_start, packed)[10:20]  # one event of a run, as the event loops slice it
    assert len(event) == 10 and np.array_equal(event.samples(), noisy[10:20])


def test_pack_traces_host_validates_its_input():
    with pytest.raises(ValueError):
        pack_traces_host(np.zeros((2, 511), dtype=np.int16))
    with pytest.raises(TypeError):
        pack_traces_host(np.zeros((2, 512), dtype=np.float64))
    row_start, packed = pack_traces_host(np.zeros((2, 512), dtype=np.int64))  # any integer dtype
    assert row_start.tolist() == [0, 16, 32] and len(packed) == 32


def _write(tmp_path, config, name, rows, **kwargs):
    from attpc_engine_amd.detector.writer import TraceWriter

    writer = TraceWriter(tmp_path / name, config, max_events_per_file=2, npz_fallback=True, **kwargs)
    pads = np.arange(len(rows), dtype=np.int32)
    for event, (lo, hi) in {3: (0, 100), 4: (100, 100), 9: (100, 300)}.items():
        writer.write_traces(pads[lo:hi], rows[lo:hi], pads[lo:hi].astype(np.int64) % 3, event)
    writer.close()
    return sorted((tmp_path / name).glob("run_*"))


def test_packed_writer_round_trip_and_plain_files_unchanged(tmp_path, config, noisy, monkeypatch):
    from attpc_engine_amd import io
    from attpc_engine_amd.detector.writer import TraceWriter, read_traces

    monkeypatch.setattr(io, "hdf5_or_fallback", lambda path, fallback: None)  # the .npz path, h5py or not
    for name in ("packed", "plain", "default"):
        (tmp_path / name).mkdir()
    packed_files = _write(tmp_path, config, "packed", noisy, packed=True)
    plain_files = _write(tmp_path, config, "plain", noisy, packed=False)
    default_files = _write(tmp_path, config, "default", noisy)
    assert [f.name for f in packed_files] == [f.name for f in plain_files] == ["run_0000.npz", "run_0001.npz"]
    pads = np.arange(300, dtype=np.int32)
    for files in (packed_files, plain_files):
        for path, event, (lo, hi) in ((files[0], 3, (0, 100)), (files[0], 4, (100, 100)), (files[1], 9, (100, 300))):
            got_pads, samples, labels = read_traces(path, event)
            assert samples.dtype == np.int16 and samples.shape == (hi - lo, 512)
            assert np.array_equal(samples, noisy[lo:hi]) and np.array_equal(got_pads, pads[lo:hi])
            assert np.array_equal(labels, pads[lo:hi] % 3) and labels.dtype == np.int64
    with np.load(packed_files[1]) as f:
        assert str(f["trace@trace_format"]) == ref.FORMAT == _abi.TRACE_PACK_FORMAT
        assert "trace/trace_9" not in f.files and f["trace/trace_9_packed"].dtype == np.uint8
        start = f["trace/trace_9_row_start"]
        assert start.dtype == np.int64 and start[0] == 0 and start[-1] == len(f["trace/trace_9_packed"])
        assert np.array_equal(f["trace/trace_9_packed"], ref.encode(noisy[100:300])[1])
        assert int(f["trace/trace_9_packed@orig_event"]) == 9 and int(f["trace@max_event"]) == 9
    # a writer without the flag, or with it off, writes the datasets it always wrote and nothing else
    for a, b in zip(plain_files, default_files):
        with np.load(a) as fa, np.load(b) as fb:
            assert sorted(fa.files) == sorted(fb.files)
            assert all(np.array_equal(fa[k], fb[k]) for k in fa.files)
            assert not any("packed" in k or "row_start" in k or "trace_format" in k for k in fa.files)
            assert {"trace/trace_3", "trace/pads_3", "trace/labels_3"} <= set(fa.files) or "trace/trace_9" in fa.files
    plain = TraceWriter(tmp_path / "plain", config)
    with pytest.raises(TypeError):
        plain.write_packed_traces(pads[:1], np.array([0, 16]), np.zeros(16, np.uint8), pads[:1], 0)


def test_read_traces_refuses_an_unknown_format(tmp_path, noisy):
    from attpc_engine_amd.detector.writer import read_traces

    row_start, packed = pack_traces_host(noisy[:2])
    np.savez(tmp_path / "run_0000.npz", **{"trace@trace_format": np.asarray("for64-bitplane-v9"), "trace/pads_0": np.arange(2),
                                           "trace/labels_0": np.arange(2), "trace/trace_0_packed": packed,
                                           "trace/trace_0_row_start": row_start})
    with pytest.raises(ValueError, match="trace_format"):
        read_traces(tmp_path / "run_0000.npz", 0)


def test_packed_flag_is_validated(config):
    from attpc_engine_amd.detector.traces import TraceChain, clouds_to_traces
    from attpc_engine_amd.detector.writer import TraceWriter

    with pytest.raises(TypeError, match="packed"):
        TraceWriter(Path("/nonexistent"), config, packed="yes")
    with pytest.raises(TypeError, match="packed"):
        clouds_to_traces(np.zeros(1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64), None, packed=1)
    with pytest.raises(TypeError, match="packed"):
        TraceChain(config).run_batch(False, None, None, None, None, 0, None, packed=1, ctx=object())
    with pytest.raises(ValueError, match="trace rows"):
        TraceChain(config).run_batch(True, None, None, None, None, 0, None, packed=True, ctx=object())


def test_two_capacity_retry_lives_in_call_with_capacity():
    """A packed call that reports more bytes than its byte_capacity is run again with what it reported -- rows and
    bytes each grow only when they were too small."""
    from attpc_engine_amd.outputs import PackedTraceArrays, call_with_capacity

    class Ctx:
        pinned_empty = None

        def check(self, status, what):
            assert status == _abi.OK, what

    seen = []

    def call(out):
        seen.append((int(out.capacity), int(out.byte_capacity)))
        out.n_rows, out.n_bytes = 50, 5000
        return _abi.E_CAPACITY if out.capacity < 50 or out.byte_capacity < 5000 else _abi.OK

    arrays = call_with_capacity(Ctx(), 2, 100, call, "fake", holder=PackedTraceArrays, byte_capacity=1024)
    assert seen == [(100, 1024), (100, 5000)] and len(arrays.packed) == 5000 and len(arrays.row_start) == 101
    seen.clear()
    call_with_capacity(Ctx(), 2, 10, call, "fake", holder=PackedTraceArrays, byte_capacity=1 << 20)
    assert seen == [(10, 1 << 20), (50, 1 << 20)]
    seen.clear()
    call_with_capacity(Ctx(), 2, 10, call, "fake", holder=PackedTraceArrays, byte_capacity=64)
    assert seen == [(10, 64), (50, 5000)]
    offsets, pads, row_start, packed, labels = arrays.result()
    assert len(pads) == len(labels) == 50 and len(row_start) == 51 and len(packed) == 5000
    assert arrays.sums()["n_bytes"] == 5000


# ---------------------------------------------------------------- the ABI lists
def test_entry_points_are_declared_bound_and_exported(lib):
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    names = ("attpc_sim_run_traces_packed", "attpc_det_run_traces_packed", "attpc_traces_packed_at", "attpc_trace_pack",
             "attpc_trace_pack_host", "attpc_trace_unpack")
    assert set(_abi.TRACE_PACK_SYMBOLS) == set(names)
    for name in names:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert f'#define ATTPC_TRACE_PACK_FORMAT "{_abi.TRACE_PACK_FORMAT}"' in header
    assert f"#define ATTPC_TRACE_PACK_MAX_ROW_BYTES {_abi.TRACE_PACK_MAX_ROW_BYTES}" in header
    # the struct of the binding has the header's fields in the header's order
    body = re.search(r"typedef struct attpc_trace_packed_out \{(.*?)\} attpc_trace_packed_out;", header, re.S).group(1)
    declared = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert declared == [name for name, _ in _abi.TracePackedOut._fields_]
    import __graft_entry__ as entry

    assert "trace_pack.hip" in entry.HIP_SOURCES and "trace_pack_host.cpp" in entry.HOST_SOURCES
    assert "trace_pack" not in (ROOT / "attpc_engine_amd" / "csrc" / "traces.hip").read_text()
