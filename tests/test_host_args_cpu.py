"""csrc/host_args.hpp compiled alone (tests/native/host_args_check.cpp; no GPU): the walk over chunks of whole events
against a restatement of its rule, the first failure the CSR offsets check reports, the 12-bit sample check at the
corners of a row range, and the noise table against numpy.  Every test runs on a plain build and on one under
AddressSanitizer + UBSan (a stand-alone program: nothing is preloaded)."""
import itertools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as entry
from attpc_engine_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
BUILDS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                                           "-fno-sanitize-recover=undefined"]}
MAX_LEVELS = 512  # ATTPC_MAX_NOISE_LEVELS


@pytest.fixture(scope="module", params=list(BUILDS))
def native(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp(f"host_args_{request.param}")
    exe = tmp / "host_args_check"
    built = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[request.param], f"-I{ROOT / 'attpc_engine_amd' / 'csrc'}",
                            f"-I{ROOT / 'include'}", "-o", str(exe), str(ROOT / "tests" / "native" / "host_args_check.cpp")],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(mode, cases, *limits):
        """``cases``: a list of lists of arrays, one list per case -> the bytes the program wrote."""
        (tmp / "in.bin").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for case in cases for a in case))
        done = subprocess.run([str(exe), mode, *map(str, limits), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True,
                              text=True, env=env)
        assert done.returncode == 0 and "ERROR" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-3000:]
        return (tmp / "out.bin").read_bytes()

    return run


def i64(*values):
    return np.array(values, dtype=np.int64)


def test_the_header_is_a_dependency_of_the_library():
    assert "host_args.hpp" in Path(entry.__file__).read_text().split("deps = ")[1].split("\n")[0]
    assert '#include "host_args.hpp"' in (ROOT / "attpc_engine_amd" / "csrc" / "abi.hip").read_text()
    assert _abi.MAX_NOISE_LEVELS == MAX_LEVELS


# ---------------------------------------------------------------- the chunk walk ----
def greedy_chunks(offsets, max_rows, max_events):
    """The rule as the operators state it: a chunk starts with one event, whatever its size, and takes the next event
    while it has fewer than max_events events and its rows with that event are at most max_rows."""
    n, chunks, e0 = len(offsets) - 1, [], 0
    while e0 < n:
        e1 = e0 + 1
        while e1 < n and e1 - e0 < max_events and offsets[e1 + 1] - offsets[e0] <= max_rows:
            e1 += 1
        chunks.append((e0, e1))
        e0 = e1
    return chunks


def test_chunk_walk(native):
    max_rows, max_events = 8, 3
    sizes = [0, 1, 3, 4, 5, 8, 9, 20]
    rng = np.random.default_rng(5)
    cases = [(0, list(s)) for length in range(6) for s in itertools.product(sizes, repeat=length)]
    cases += [(int(rng.integers(0, 50)), rng.choice(sizes, 40).tolist()) for _ in range(300)]
    cases += [(7, list(s)) for s in itertools.product(sizes, repeat=3)]  # offsets[0] != 0
    all_offsets = [np.concatenate([[first], first + np.cumsum(s, dtype=np.int64)]).astype(np.int64) for first, s in cases]
    out = np.frombuffer(native("walk", [[i64(len(o) - 1), o] for o in all_offsets], max_rows, max_events), dtype=np.int64)
    at = 0
    for offsets in all_offsets:
        n, count = len(offsets) - 1, int(out[at])
        at += 1
        chunks, next_event = [], 0
        for _ in range(count):
            e0, e1 = int(out[at]), int(out[at + 1])
            start = out[at + 2:at + 2 + e1 - e0 + 1]
            at += 2 + e1 - e0 + 1
            rows = int(offsets[e1] - offsets[e0])
            assert e0 == next_event and 1 <= e1 - e0 <= max_events, (offsets, e0, e1)  # a partition, in order
            assert rows <= max_rows or e1 - e0 == 1, (offsets, e0, e1)
            assert start[0] == 0 and start[-1] == rows and start.tolist() == (offsets[e0:e1 + 1] - offsets[e0]).tolist()
            chunks.append((e0, e1))
            next_event = e1
        assert next_event == n and chunks == greedy_chunks(offsets, max_rows, max_events), offsets
    assert at == len(out)


# ---------------------------------------------------------------- the CSR offsets check ----
OPERATOR, CLOUD = 0, 1
BIG = 1 << 31
OFFSETS_CASES = [  # (order, n_events, offsets or None) -> the line
    ((OPERATOR, 0, None), "ok"),                      # n_events = 0 with a null pointer
    ((OPERATOR, 0, [0]), "ok"),                       # empty input
    ((OPERATOR, 0, [-1]), "ok"),                      # (offsets of no event are not read)
    ((OPERATOR, 2, None), "bare"),
    ((OPERATOR, -1, [0]), "bare"),
    ((OPERATOR, 1 << 31, None), "bare"),
    ((OPERATOR, 3, [0, 1, 1, 5]), "ok"),
    ((OPERATOR, 3, [-1, 1, 1, 5]), "offsets[0] < 0"),
    ((OPERATOR, 3, [3, 2, 4, 5]), "offsets decrease at event 0"),
    ((OPERATOR, 3, [0, 4, 3, 5]), "offsets decrease at event 1"),
    ((OPERATOR, 3, [0, 1, 5, 4]), "offsets decrease at event 2"),
    ((OPERATOR, 3, [7, 7 + BIG - 1, 7 + BIG - 1, 7 + 2 * BIG - 2]), "ok"),              # events of exactly 2^31 - 1 rows
    ((OPERATOR, 3, [7, 8, 8 + BIG, 8 + BIG]), "event 1 has 2^31 rows or more"),         # of 2^31 rows
    # two faults in one array: the first event's comes first, and within an event the decrease before the limit
    ((OPERATOR, 3, [-1, -2, 4, 3]), "offsets[0] < 0"),
    ((OPERATOR, 3, [0, BIG, BIG - 1, 0]), "event 0 has 2^31 rows or more"),
    ((OPERATOR, 3, [0, 3, 2, 2 + BIG]), "offsets decrease at event 1"),
    # the host clouds: the decrease first, and no limit per event
    ((CLOUD, 3, [-1, -2, 4, 3]), "offsets decrease at event 0"),
    ((CLOUD, 3, [-1, 1, 1, 5]), "offsets[0] < 0"),
    ((CLOUD, 3, [-5, -4, -3, -4]), "offsets decrease at event 2"),
    ((CLOUD, 3, [7, 8, 8 + BIG, 8 + BIG]), "ok"),
    ((CLOUD, 2, None), "bare"),
    ((CLOUD, 0, None), "ok"),
]


def test_offsets_check_reports_the_first_failure(native):
    cases = [[i64(order, n, offsets is not None)] + ([i64(*offsets)] if offsets is not None else []) for (order, n, offsets), _ in OFFSETS_CASES]
    for (_, n, offsets), _ in OFFSETS_CASES:
        assert offsets is None or n <= 0 or len(offsets) == n + 1
    lines = native("offsets", cases).decode().splitlines()
    assert lines == [want for _, want in OFFSETS_CASES]


# ---------------------------------------------------------------- the sample check ----
def test_sample_check_at_the_corners_of_a_row_range(native):
    first, last, rows = 2, 5, 7  # the range is rows 2 .. 4 of 7
    cases, want = [], []
    for row, sample in itertools.product((first, last - 1), (0, _abi.NUM_TB - 1)):
        for value in (-1, 0, 4095, 4096):
            samples = np.full((rows, _abi.NUM_TB), 100, dtype=np.int16)
            samples[:first], samples[last:] = -7, 5000  # (outside the range: not looked at)
            samples[row, sample] = value
            cases.append([i64(first, last, rows), samples])
            want.append("ok" if 0 <= value <= 4095 else f"sample {sample} of row {row} is {value}: 0 .. 4095")
    samples = np.full((rows, _abi.NUM_TB), 100, dtype=np.int16)
    samples[3, 9], samples[3, 10], samples[4, 0] = 4096, -1, -1  # the first of several
    cases.append([i64(first, last, rows), samples])
    want.append("sample 9 of row 3 is 4096: 0 .. 4095")
    cases.append([i64(3, 3, rows), np.full((rows, _abi.NUM_TB), -1, dtype=np.int16)])  # an empty range
    want.append("ok")
    assert native("samples", cases).decode().splitlines() == want


# ---------------------------------------------------------------- the noise table ----
def test_noise_table_against_numpy(native):
    rng = np.random.default_rng(9)
    step = 1 << 24
    tables = [np.zeros(0, dtype=np.uint32) for _ in (0, 1)]  # n_levels 0 and 1: no cdf
    tables.append(np.array([5 * step], dtype=np.uint32))  # n_levels 2
    tables.append(np.sort(rng.integers(0, 1 << 32, MAX_LEVELS - 1, dtype=np.uint64)).astype(np.uint32))  # the full table
    tables.append(np.array([0, 0, 7, 7, 7, 3 * step, 3 * step, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32))  # repeated entries
    tables.append(np.array([0, 1, step - 1, step, step + 1, 200 * step - 1, 200 * step, 200 * step + 1, 255 * step - 1, 255 * step,
                            255 * step + 1, 0xFFFFFFFE], dtype=np.uint32))  # both sides of multiples of 2^24
    levels = [0, 1] + [len(t) + 1 for t in tables[2:]]
    assert levels[3] == MAX_LEVELS
    out = native("noise", [[i64(n), t] for n, t in zip(levels, tables)])
    record = np.dtype([("cdf", "<u4", MAX_LEVELS), ("guide", "<u2", 256)])
    got = np.frombuffer(out, dtype=record)
    assert len(got) == len(tables)
    for n_levels, cdf, table in zip(levels, tables, got):
        padded = np.full(MAX_LEVELS, 0xFFFFFFFF, dtype=np.uint32)
        padded[:len(cdf)] = cdf
        assert table["cdf"].tolist() == padded.tolist(), n_levels
        edges = np.arange(256, dtype=np.uint64) << 24
        guide = [int(np.count_nonzero(cdf[:max(n_levels - 1, 0)].astype(np.uint64) <= edge)) for edge in edges]
        assert table["guide"].tolist() == guide, n_levels
