"""The flush of the scatter kernel (the row loop behind a window's last barrier) and what it shares with the insert
loop, in the five builds of tests/test_gpu_rows_step.py:

* the row loop at the edges of a wave (64 rows), of the small workgroup (512) and of the big one (1 024): hand-made
  events of ONE time bucket, so that the event is one window and its key count is the loop's row count;
* the two checksums, which the loop forms from pieces (the 24-bit keys row by row, the event's share once per window;
  u64 charge sums): against sums formed in Python integers mod 2^64 from the oracle's clouds, at event ids around 2^32
  and 2^40 and a seed with the high word set, and with flushed sums beyond 2^32 in the u64 build;
* a launch that runs out of row capacity: its windows only reset the table, the host repeats the launch, and arrays and
  checksums equal those of a run with ample buffers.

Needs a real MI355X: ``-m gpu``.

Tolerances (as in tests/test_gpu_rows_step.py): keys, labels, zero-charge inserts and the f64
time column (time bucket + jitter) exact, charges within 2 electrons where a pixel weight enters (numpy's exp in the
oracle's pdf against the kernel's constant weight table).  The key checksum is exact everywhere.  The charge checksum
equals the oracle's sum exactly where no weight enters a charge (zero transverse diffusion: every electron of a sample
lands on the pad below it); with diffusion it equals the Python-integer sum of the device's own rows exactly, and each
of those rows is within 2 electrons of the oracle's."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests.helpers import SEED_ALL_ONES, U64, Inputs
from tests.test_gpu_parity import _engine
from tests.test_gpu_rows_step import (BUILD_IDS, BUILDS, LABEL, _assert_clouds_equal_oracle, _configure_cpu, _edge_events,
                                      _oracle_dict, _run)
from tests.test_gpu_scatter_fixtures import _compare_with_dict, _configure, device_scatter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _kept(tbpad):
    """The rows of a cloud among the oracle's dictionary keys (simulator.py:111-113)."""
    return (tbpad[:, 0] >= 0) & (tbpad[:, 0] < 512) & (tbpad[:, 1] >= 0)


# ---- the row loop at the edges of a wave and of a workgroup ----
# rows of the window: either side of one wave's 64, of the small workgroup's 512 and of the big workgroup's 1 024
ROW_RANGES = [(1, 64), (65, 128), (449, 512), (513, 576), (961, 1024), (1025, 1088)]


def _one_bucket_event(n):
    """n samples on a 4 mm grid over the small pads beside the beam region, all in time bucket 300."""
    k = np.arange(n, dtype=np.float64)
    x, y = 0.0213 + 4.0e-3 * (k % 24), -0.0487 + 4.0e-3 * (k // 24)
    t = 300.25 + 1.0e-4 * k
    return [(np.column_stack([x, y, t]), (200_001 + 1_013 * np.arange(n)).astype(np.int64), LABEL)]


@pytest.fixture(scope="module")
def edge_events(orc):
    """One event per range of ROW_RANGES, found by sweeping the number of samples with the oracle on the CPU: the key
    count grows with the samples, by a few pads per sample."""
    cfg, raw, keep = _configure_cpu()
    counts = {}

    def rows(n):
        if n not in counts:
            tbpad, _, _ = _oracle_dict(orc, raw, _one_bucket_event(n))
            counts[n] = int(_kept(tbpad).sum())
        return counts[n]

    events, found = [], []
    for lo, hi in ROW_RANGES:
        a, b = 1, 600  # the smallest n with rows(n) >= lo
        assert rows(b) >= lo, (b, rows(b), lo)
        while a < b:
            mid = (a + b) // 2
            a, b = (a, mid) if rows(mid) >= lo else (mid + 1, b)
        events.append(_one_bucket_event(a))
        found.append(rows(a))
    return events, found


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_row_loop_at_wave_and_workgroup_edges_vs_oracle(orc, edge_events, variant, merge):
    events, found = edge_events
    # the premise, from the oracle alone: one time bucket per event, a key count in every range
    cfg, raw_cpu, keep_cpu = _configure_cpu()
    for ev, n_keys, (lo, hi) in zip(events, found, ROW_RANGES):
        tbpad, _, _ = _oracle_dict(orc, raw_cpu, ev)
        kept = tbpad[_kept(tbpad)]
        assert len(kept) == n_keys and lo <= n_keys <= hi, (n_keys, lo, hi)
        assert (kept[:, 0] == 300).all()
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events)
    print("row-loop edges", variant, merge, "rows per event", [len(pts) for pts, _ in clouds], "oracle", found, "lone buckets",
          stats["n_lone_buckets"], "retried windows", stats["n_lds_overflow"])
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0 and stats["n_lone_buckets"] == 0, stats
    assert [len(pts) for pts, _ in clouds] == found
    assert _assert_clouds_equal_oracle(orc, raw, events, clouds) == sum(found)


# ---- the checksums ----
def _run_at(variant, merge, diffusion, events, seed, first):
    ctx = _abi.Context(0)
    try:
        ctx.set_option("scatter_variant", variant)
        ctx.set_option("scatter_merge", merge)
        cfg, raw, keep = _configure(ctx, diffusion)
        clouds, stats = device_scatter(ctx, events, seed=seed, first_event=first)
    finally:
        ctx.close()
    return clouds, stats, (raw, keep)


_ORACLE = {}


def _oracle_sums(orc, raw, events, first, tag):
    """Per event the oracle's dictionary, and the two checksums of its clouds in Python integers mod 2^64; computed once
    per (events, first event) and shared by the builds."""
    if tag not in _ORACLE:
        dicts, key_sum, charge_sum = [], 0, 0
        for e, ev in enumerate(events):
            tbpad, charge, labels = _oracle_dict(orc, raw, ev)
            ok = _kept(tbpad)
            key_sum += sum(((first + e) << 24) + ((int(t) << 14) | int(p)) for t, p in tbpad[ok])
            charge_sum += sum(int(q) for q in charge[ok])
            dicts.append((tbpad, charge, labels))
        _ORACLE[tag] = (dicts, key_sum % U64, charge_sum % U64)
    return _ORACLE[tag]


def _check_sums(orc, variant, merge, diffusion, events, first, tag):
    seed = SEED_ALL_ONES
    clouds, stats, (raw, keep) = _run_at(variant, merge, diffusion, events, seed, first)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    dicts, key_sum, charge_sum = _oracle_sums(orc, raw, events, first, (tag, diffusion, first))
    device_charge, rows = 0, 0
    for e, ((pts, lab), (tbpad, charge, labels)) in enumerate(zip(clouds, dicts)):
        _compare_with_dict(pts, lab, tbpad[:, 0], tbpad[:, 1], charge, labels, seed, first + e)
        device_charge += sum(int(q) for q in pts[:, 2])
        rows += len(pts)
    print("checksums", tag, variant, merge, "diffusion", diffusion, "first", first, "rows", rows, "key", stats["key_checksum"],
          key_sum, "charge", stats["charge_checksum"], "oracle", charge_sum, "device rows", device_charge % U64)
    assert stats["key_checksum"] == key_sum
    assert stats["charge_checksum"] == device_charge % U64
    if diffusion == 0.0:
        assert stats["charge_checksum"] == charge_sum
    else:
        assert abs(int(stats["charge_checksum"]) - charge_sum) <= 2 * rows
    return rows, device_charge


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("first", [2 ** 32 - 4, 2 ** 40 - 4], ids=["across-2^32", "across-2^40"])
@pytest.mark.parametrize("diffusion", [0.0, 0.277], ids=["no-diffusion", "diffusion"])
def test_checksums_equal_python_integer_sums_of_the_oracle(orc, diffusion, first, variant, merge):
    """8 events (1 to 205 samples, spread over many time buckets: several windows per event) whose ids cross 2^32 /
    2^40, where event << 24 leaves the low / all 64 bits of the key checksum."""
    events = _edge_events(True)
    rows, _ = _check_sums(orc, variant, merge, diffusion, events, first, "edges")
    # the premise, from the oracle alone: more rows than one wave writes in one turn of the loop, in several time buckets
    dicts, _, _ = _ORACLE[("edges", diffusion, first)]
    kept = [tbpad[_kept(tbpad)] for tbpad, _, _ in dicts]
    assert sum(len(k) for k in kept) > 64 and max(len(np.unique(k[:, 0])) for k in kept) > 8
    assert rows == sum(len(k) for k in kept)


def test_flushed_sums_beyond_2_pow_32_in_the_u64_build(orc):
    """The same events with the electrons of a gain of 2e6 (3 000 and more primary electrons per sample), no diffusion:
    every sample's charge lands on one pad, and a flushed sum is above 2^32."""
    events = [[(xyt, (3_000 + 17 * np.arange(len(el), dtype=np.int64)) * 2_000_000, lab) for xyt, el, lab in ev]
              for ev in _edge_events(True)]
    rows, device_charge = _check_sums(orc, 3, 0, 0.0, events, 2 ** 32 - 4, "gain-2e6")
    dicts, _, charge_sum = _ORACLE[("gain-2e6", 0.0, 2 ** 32 - 4)]
    assert max(int(charge.max()) for _, charge, _ in dicts) > 2 ** 32  # the premise, from the oracle alone
    assert device_charge > 2 ** 40 and rows == sum(int(_kept(tbpad).sum()) for tbpad, _, _ in dicts) > 64


# ---- a launch that runs out of row capacity ----
def _sorted_run(res):
    """Rows in a canonical order (event, pad, time bucket): inside a window they come in the order of the table's slots,
    which depends on which wave claimed a slot first."""
    off = res["offsets"]
    event = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort((np.floor(res["points"][:, 1]), res["points"][:, 0], event))
    return res["points"][order], res["labels"][order]


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_launch_out_of_row_capacity_is_repeated_with_equal_results(variant, merge):
    inp = Inputs("o16aa")
    n, seed, first = 64, SEED_ALL_ONES, 2 ** 32 - 32
    runs = []
    # (the caller's arrays are ample both times: a call that fails on THEIR size is simply made again, and the second
    #  call's statistics show no growth.  What is too small for the first attempt is the device's row buffer)
    for tiny, capacity_per_event in ((1, 16384), (0, 16384)):
        ctx = _abi.Context(0)
        try:
            ctx.set_option("scatter_variant", variant)
            ctx.set_option("scatter_merge", merge)
            ctx.set_option("tiny_buffers", tiny)  # the first launch gets 64 rows of device buffer
            runs.append(_engine(inp, ctx).run(n, seed=seed, first_event=first, fetch=True, capacity_per_event=capacity_per_event))
        finally:
            ctx.close()
    small, ample = runs
    print("capacity", variant, merge, "growths", small["stats"]["n_buffer_growths"], ample["stats"]["n_buffer_growths"],
          "points", small["stats"]["n_points"], "key", small["stats"]["key_checksum"], "charge", small["stats"]["charge_checksum"])
    # every buffer is allocated once in either run (counted as growths), the row buffers once more after the overflow
    assert small["stats"]["n_buffer_growths"] >= 1 and small["stats"]["n_buffer_growths"] > ample["stats"]["n_buffer_growths"]
    assert small["stats"]["n_failed"] == 0 and small["stats"]["n_inconsistent"] == 0
    np.testing.assert_array_equal(small["offsets"], ample["offsets"])
    for mine, ref in zip(_sorted_run(small), _sorted_run(ample)):
        np.testing.assert_array_equal(mine, ref)
    for key in ("n_points", "key_checksum", "charge_checksum"):
        assert small["stats"][key] == ample["stats"][key], key
    assert small["stats"]["n_points"] > 64 * 64
