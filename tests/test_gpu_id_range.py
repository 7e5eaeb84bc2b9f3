"""The device at the event ids and seeds the engine really runs at: ids past 2^24 / 2^31 / 2^32 / 2^40 / 2^53 up to the
top of the u64 range, 63- and 64-bit seeds with the high word set (tests/helpers.py ID_CASES).  Every draw is a function
of (seed, global event id, ...); a device that dropped a high word, or carried an id through int / float, passes every
test at small ids and seeds, and fails these (tests/test_id_range_cpu.py shows that the oracle discriminates at every
case).  Everything is compared with the CPU oracle, at the tolerances of tests/test_gpu_parity.py: status, attempts,
keys, labels, jittered time buckets, electron counts, point and sample counts, key checksums exact; p4 1e-9 MeV,
vertices 1e-12 m, charges within 2 electrons.  Needs a real MI355X: ``-m gpu``."""
import copy
import os
import time

import numpy as np
import pytest

from attpc_engine_amd import _abi, nuclear_map
from tests.helpers import (ID_CASE_IDS, ID_CASES, SEED_ALL_ONES, SEED_LO_ZERO, SEED_TYPICAL, U64, IdCase, Inputs,
                           compare_clouds, id_case, sort_cloud)
from tests.test_gpu_parity import _device_tracks, _engine
from tests.test_gpu_scatter_fixtures import _compare_with_dict, _configure, _plane_filling_event, device_scatter

pytestmark = pytest.mark.gpu

THREADS = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 8)
_T0 = time.monotonic()


@pytest.fixture(scope="module", autouse=True)
def _report_runtime():
    yield
    print(f"\ntests/test_gpu_id_range.py: {time.monotonic() - _T0:.1f} s")


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _key_checksum(first_event, offsets, points):
    """sum over rows of (event << 24) + (tb << 14 | pad), mod 2^64 (RunStats.key_checksum)."""
    event = np.repeat(np.arange(len(offsets) - 1, dtype=np.uint64), np.diff(offsets)) + np.uint64(first_event)
    key = (np.floor(points[:, 1]).astype(np.uint64) << np.uint64(14)) | points[:, 0].astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(((event << np.uint64(24)) + key).sum(dtype=np.uint64))


def _compare_run_with_oracle(res, ref, n):
    np.testing.assert_array_equal(res["status"], ref["status"])
    np.testing.assert_allclose(res["p4"], ref["p4"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res["vertex"], ref["vertex"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(res["offsets"], ref["offsets"])
    for e in range(n):
        lo, hi = ref["offsets"][e], ref["offsets"][e + 1]
        compare_clouds(*sort_cloud(res["points"][lo:hi], res["labels"][lo:hi]),
                       *sort_cloud(ref["points"][lo:hi], ref["labels"][lo:hi]))
    st = res["stats"]
    assert st["n_points"] == ref["stats"][0] and st["n_track_samples"] == ref["stats"][1]
    assert st["key_checksum"] == ref["stats"][3] % U64
    assert abs(int(st["charge_checksum"]) - int(ref["stats"][2] % U64)) <= 2 * max(8, st["n_points"] // 10_000)
    assert st["n_failed"] == 0 and st["n_inconsistent"] == 0


# ---------------------------------------------------------------- a. kinematics ----------------------------------------
@pytest.mark.parametrize("name", ["o16aa", "b10chain"])
@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_kinematics_at_wide_ids(ctx, orc, name, case):
    inp = Inputs(name)
    inp.pipeline._ctx = ctx
    vertex, p4, status, attempts = inp.pipeline.run_many(case.n, first_event=case.first_event, seed=case.seed,
                                                         return_status=True)
    ov, op4, ostatus, oatt = orc.kin_batch(inp.kin, case.seed, case.first_event, case.n, threads=THREADS)
    np.testing.assert_array_equal(status, ostatus)
    np.testing.assert_array_equal(attempts, oatt)
    np.testing.assert_allclose(p4, op4, rtol=0, atol=1e-9)
    np.testing.assert_allclose(vertex, ov, rtol=0, atol=1e-12)


# ---------------------------------------------------------------- b. tracks and Fano draws -----------------------------
def _tracks_vs_oracle(ctx, orc, inp, seed, first, n):
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=THREADS)
    samples, counts, steps = _device_tracks(ctx, inp, p4, vertex, seed, first)
    total = 0
    for e in range(n):
        for i, row in enumerate(inp.indices):
            sp = inp.layout.species_of_row[row]
            ref, ref_rows = orc.point_cloud_samples(inp.det_raw, sp, p4[e, row], vertex[e], seed, first + e, row)
            t = e * inp.layout.n_sim + i
            assert steps[t] == ref_rows and counts[t] == len(ref), (e, row, steps[t], ref_rows, counts[t], len(ref))
            mine = samples[t, : counts[t]]
            np.testing.assert_allclose(mine[:, :2], ref[:, :2], rtol=0, atol=1e-9)
            np.testing.assert_allclose(mine[:, 2], ref[:, 2], rtol=0, atol=1e-7)
            np.testing.assert_array_equal(mine[:, 3], ref[:, 3])  # electron counts x gain: the Fano draws
            total += len(ref)
    return total


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_tracks_at_wide_ids(ctx, orc, case):
    assert _tracks_vs_oracle(ctx, orc, Inputs("o16aa"), case.seed, case.first_event, case.n) > 1000


def test_tracks_with_a_path_step_at_a_wide_id(ctx, orc):
    """The path-length sampling extension (b10chain, 0.1 mm step: a decay chain, more draw indices per event)."""
    inp = Inputs("b10chain", path_step=1.0e-4)
    case = id_case("u32_wrap")
    assert _tracks_vs_oracle(ctx, orc, inp, case.seed, (1 << 32) - 2, 4) > 1000


# ---------------------------------------------------------------- c. detector: the scatter flush ------------------------
def _det_vs_oracle(ctx, orc, inp, case, det_raw=None, charge_tol=2.0):
    from attpc_engine_amd.detector.simulator import simulate_batch
    seed, first, n = case.seed, case.first_event, case.n
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=THREADS)
    offsets, points, labels, stats = simulate_batch(p4, vertex, inp.z, inp.a, inp.config, seed, inp.indices,
                                                    first_event=first, ctx=ctx)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0
    for e in range(n):
        det = inp.det_raw if det_raw is None else det_raw
        ref_pts, ref_lab, _ = orc.simulate(det, inp.layout, seed, first + e, p4[e], vertex[e], capacity=1 << 20)
        compare_clouds(*sort_cloud(points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]),
                       *sort_cloud(ref_pts, ref_lab), charge_tol=charge_tol)
    assert stats["key_checksum"] == _key_checksum(first, offsets, points)
    assert offsets[-1] > 1000
    return stats


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_detector_at_wide_ids(ctx, orc, case):
    _det_vs_oracle(ctx, orc, Inputs("o16aa"), case)


@pytest.mark.parametrize("variant,merge", [(1, -1), (2, -1), (3, -1), (2, 1)])
def test_scatter_builds_at_a_wide_id(orc, variant, merge):
    """The three scatter builds and the merge variant are separately compiled code objects, each with its own
    register placement of ev_lo / ev_hi in the flush loop."""
    fresh = _abi.Context(0)
    try:
        fresh.set_option("scatter_variant", variant)
        fresh.set_option("scatter_merge", merge)
        _det_vs_oracle(fresh, orc, Inputs("o16aa"), id_case("u32_wrap"))
    finally:
        fresh.close()


# ---------------------------------------------------------------- d. fused runs, chunk boundaries on 2^32 ---------------
@pytest.mark.parametrize("compact", [2, 0])
@pytest.mark.parametrize("offset", [16, 13], ids=["chunk_starts_on_2^32", "chunk_straddles_2^32"])
def test_fused_run_across_2_pow_32(ctx, orc, compact, offset):
    """Engine.run(fetch=True) in chunks of 8 events from 2^32 - offset: with 16 a chunk begins exactly on 2^32, with 13
    one straddles it.  compact_transfer 2: 8-byte records, the host regenerates the jitter from the chunk's first
    global id (unpack_host.cpp); 0: plain rows."""
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx, chunk_events=8)
    n, first, seed = 32, (1 << 32) - offset, SEED_ALL_ONES
    ctx.set_option("compact_transfer", compact)
    try:
        res = eng.run(n, seed=seed, first_event=first, fetch=True)
    finally:
        ctx.set_option("compact_transfer", 2)
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "chunk")
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=n, capacity=1 << 21,
                        threads=THREADS)
    _compare_run_with_oracle(res, ref, n)
    assert res["stats"]["launches_scatter"] >= 4


# ---------------------------------------------------------------- e. extensions ----------------------------------------
@pytest.mark.parametrize("case", [IdCase("u32_wrap", (1 << 32) - 4, SEED_ALL_ONES, 8), IdCase("top", U64 - 8, SEED_LO_ZERO, 8)],
                         ids=["u32_wrap", "top"])
@pytest.mark.parametrize("mc,d_l", [(True, 0.0), (True, 0.1), (False, 0.3)])
def test_diffusion_extensions_at_wide_ids(ctx, orc, case, mc, d_l):
    """Per-electron Monte-Carlo diffusion (Philox domain 0x200 + entry) and the longitudinal slices."""
    from attpc_engine_amd.detector.luts import build_det_desc
    inp = Inputs("o16aa")
    inp.config = copy.copy(inp.config)
    inp.config.det_params = copy.copy(inp.config.det_params)
    inp.config.det_params.mc_diffusion = mc
    inp.config.det_params.longitudinal_diffusion = d_l
    nuclei = [nuclear_map.get_data(z, a) for z, a in inp.species]
    det_raw, keep = build_det_desc(inp.config, nuclei, fold_beam=False)
    _det_vs_oracle(ctx, orc, inp, case, det_raw=det_raw, charge_tol=0.0 if mc else 2.0)


# ---------------------------------------------------------------- f. lone-bucket kernel ---------------------------------
@pytest.mark.parametrize("mc", [False, True])
def test_lone_bucket_kernel_at_a_wide_id_and_seed(ctx, orc, mc):
    """The plane-filling time bucket (more lit pads than the 6144-slot table holds) through lone_bucket_kernel, with
    events at 2^40 - 2 .. 2^40 (the jitter counter wraps between the last two) and a seed with every bit set: jitter,
    keys, charges, labels and the key checksum of lone_bucket_kernel's own flush."""
    seed, first = SEED_ALL_ONES, (1 << 40) - 2
    cfg, raw, keep = _configure(ctx, 0.277, mc_diffusion=mc)
    if mc:
        big = _plane_filling_event(cfg, n_tracks=2, pitch_mm=4.8, electrons=20 * 175000)
    else:
        big = _plane_filling_event(cfg)
    small = [(xyt[:40] * np.array([1.0, 1.0, 0.5]), el[:40], lab) for xyt, el, lab in big]
    events = [small, big, small]
    ctx.set_option("scatter_variant", 1)
    try:
        clouds, stats = device_scatter(ctx, events, seed=seed, first_event=first)
    finally:
        ctx.set_option("scatter_variant", 0)
        if mc:
            _configure(ctx, 0.277)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0
    assert stats["n_lone_buckets"] >= 1 or len(clouds[1][0]) <= 6144
    key_sum = 0
    for e, (ev, (pts, lab)) in enumerate(zip(events, clouds)):
        keys, charge, labels = orc.transport(raw, ev, seed=seed, event=first + e)
        tb, pad = np.array([orc.unpair(int(k)) for k in keys], dtype=np.int64).T
        worst, _ = _compare_with_dict(pts, lab, tb, pad, charge, labels, seed, first + e)
        if mc:
            assert worst == 0  # whole electrons
        ok = (tb >= 0) & (tb < 512) & (pad >= 0)
        key_sum += sum((((first + e) << 24) + ((int(t) << 14) | int(p))) for t, p in zip(tb[ok], pad[ok]))
    assert stats["key_checksum"] == key_sum % U64
    assert len(clouds[1][0]) > 4096
    print("mc", mc, "pads lit:", len(clouds[1][0]), "lone buckets:", stats["n_lone_buckets"])


# ---------------------------------------------------------------- g. Spyral rows ---------------------------------------
def test_spyral_rows_at_a_wide_id_and_seed(ctx, orc):
    """Engine.run_spyral (attpc_sim_run_spyral) and simulate_batch_spyral (attpc_det_run_spyral) against the cloud path
    + convert_to_spyral + threshold + z-sort, where the cloud path equals the oracle's."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.detector.simulator import simulate_batch_spyral
    from attpc_engine_amd.detector.writer import convert_to_spyral
    case = id_case("jitter40")
    seed, first, n = case.seed, case.first_event + 14, 10
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx, chunk_events=4)
    try:
        fused = eng.run_spyral(n, seed=seed, first_event=first)
        cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "chunk")
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=n, capacity=1 << 21, threads=THREADS)
    _compare_run_with_oracle(cloud, ref, n)
    det = simulate_batch_spyral(cloud["p4"], cloud["vertex"], inp.z, inp.a, inp.config, seed, inp.indices,
                                first_event=first, ctx=ctx)
    cfg = inp.config
    resp = get_response(cfg)
    thr = cfg.elec_params.adc_threshold
    for off, rows, labels, event_points in ((fused["offsets"], fused["rows"], fused["labels"], fused["event_points"]),
                                            det[:4]):
        for e in range(n):
            lo, hi = cloud["offsets"][e], cloud["offsets"][e + 1]
            pts, lab = np.ascontiguousarray(cloud["points"][lo:hi]), cloud["labels"][lo:hi]
            want = convert_to_spyral(pts, 560, 10, 1.0, resp, cfg.pad_centers, cfg.pad_sizes, ctx=ctx)
            keep = want[:, 3] > thr
            want, want_lab = want[keep], lab[keep]
            got, got_lab = rows[off[e]:off[e + 1]], labels[off[e]:off[e + 1]]
            assert event_points[e] == hi - lo and len(got) == len(want)
            o1, o2 = np.lexsort((got[:, 6], got[:, 5])), np.lexsort((want[:, 6], want[:, 5]))
            np.testing.assert_array_equal(got[o1][:, [0, 1, 2, 3, 5, 6, 7]], want[o2][:, [0, 1, 2, 3, 5, 6, 7]])
            np.testing.assert_allclose(got[o1][:, 4], want[o2][:, 4], rtol=1e-12, atol=0)
            np.testing.assert_array_equal(got_lab[o1], want_lab[o2])
            assert (np.diff(got[:, 2]) >= 0).all()
    assert fused["offsets"][-1] > 1000


# ---------------------------------------------------------------- h. invariance across 2^32 ----------------------------
def test_invariance_across_2_pow_32(ctx, orc):
    """[2^32 - m, 2^32 + m) in one call == the two calls split at 2^32 (checksums add mod 2^64), at the default chunk
    size, at 1024 events per chunk and with the second half announced by hint_next; and == the oracle."""
    inp = Inputs("o16aa")
    m, seed = 1500, SEED_TYPICAL
    first = (1 << 32) - m
    eng = _engine(inp, ctx)
    whole = eng.run(2 * m, seed=seed, first_event=first)["stats"]
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=2 * m, threads=THREADS)["stats"]
    assert whole["n_points"] == ref[0] and whole["n_track_samples"] == ref[1] and whole["key_checksum"] == ref[3] % U64
    assert abs(int(whole["charge_checksum"]) - int(ref[2] % U64)) <= 2 * max(8, whole["n_points"] // 10_000)
    assert whole["n_failed"] == 0 and whole["n_inconsistent"] == 0
    for chunk, hint in ((0, False), (1024, False), (1024, True)):
        eng = _engine(inp, ctx, chunk_events=chunk or None)
        try:
            if hint:
                eng.hint_next(m, seed=seed, first_event=1 << 32)
            a = eng.run(m, seed=seed, first_event=first)["stats"]
            b = eng.run(m, seed=seed, first_event=1 << 32)["stats"]
            one = eng.run(2 * m, seed=seed, first_event=first)["stats"]
        finally:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "chunk")
        for k in ("n_points", "n_track_samples", "n_failed", "n_inconsistent"):
            assert a[k] + b[k] == whole[k] == one[k], (chunk, hint, k)
        for k in ("charge_checksum", "key_checksum"):
            assert (a[k] + b[k]) % U64 == whole[k] == one[k], (chunk, hint, k)


# ---------------------------------------------------------------- i. bulk checksums at 2^40 -----------------------------
def test_bulk_checksums_at_2_pow_40(ctx, orc):
    """About 20 000 o16aa events from 2^40 - 10 000 (the jitter counter and (event << 24) of the checksum both wrap in
    the range) at seed 2^64 - 1: point and sample counts and the key checksum equal the oracle's exactly."""
    inp = Inputs("o16aa")
    n, first, seed = 20_000, (1 << 40) - 10_000, SEED_ALL_ONES
    st = _engine(inp, ctx).run(n, seed=seed, first_event=first)["stats"]
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=n, threads=THREADS)["stats"]
    assert st["n_points"] == ref[0] and st["n_track_samples"] == ref[1]
    assert st["key_checksum"] == ref[3] % U64
    assert st["n_failed"] == 0 and st["n_inconsistent"] == 0
    diff = (int(st["charge_checksum"]) - int(ref[2] % U64) + (1 << 63)) % U64 - (1 << 63)
    gain = int(inp.config.det_params.mpgd_gain)
    flips = round(diff / gain)  # Fano draws off by one primary electron (test_gpu_parity.py::test_bulk_checksums_vs_oracle)
    assert abs(diff - flips * gain) <= 2 * max(8, st["n_points"] // 10_000), diff
    assert abs(flips) <= 1 + st["n_track_samples"] // 10_000_000, (flips, diff)
    print("events", n, "points", st["n_points"], "charge checksum difference", diff, "Fano flips", flips)


# ---------------------------------------------------------------- j. simulate() with its own 63-bit seed -----------------
def test_simulate_draws_a_63_bit_seed_and_the_device_uses_all_of_it(ctx, orc):
    import attpc_engine_amd._abi as abi_mod
    from attpc_engine_amd.detector import simulate
    inp = Inputs("o16aa")
    vertex, p4, _, _ = orc.kin_batch(inp.kin, 7, 0, 3, threads=4)
    old = abi_mod._default_ctx
    abi_mod._default_ctx = ctx
    wide = 0
    try:
        for e, entropy in enumerate((1234, 99, 2024)):
            rng, twin = np.random.default_rng(entropy), np.random.default_rng(entropy)
            seed = int(twin.integers(0, 1 << 63))
            wide += seed >= 1 << 32
            points, labels = simulate(p4[e], vertex[e], inp.z, inp.a, inp.config, rng, inp.indices)
            ref_pts, ref_lab, _ = orc.simulate(inp.det_raw, inp.layout, seed, 0, p4[e], vertex[e], capacity=1 << 19)
            compare_clouds(*sort_cloud(points, labels), *sort_cloud(ref_pts, ref_lab))
            assert len(points) > 0
    finally:
        abi_mod._default_ctx = old
    assert wide == 3


# ---------------------------------------------------------------- ranges that wrap are refused --------------------------
def test_ranges_past_2_pow_64_and_bad_seeds_are_refused(ctx):
    inp = Inputs("o16aa")
    inp.pipeline._ctx = ctx
    eng = _engine(inp, ctx)
    for kw in ({"seed": -1}, {"seed": U64}, {"first_event": -3}, {"first_event": U64 - 5}):
        with pytest.raises(ValueError):
            eng.run(10, **kw)
        with pytest.raises(ValueError):
            eng.run_spyral(10, **kw)
        with pytest.raises(ValueError):
            eng.hint_next(10, **kw)
        with pytest.raises(ValueError):
            inp.pipeline.run_many(10, **kw)
    st = _abi.RunStats()
    lay = inp.layout
    p4, vertex = np.zeros((16, 8, 4)), np.zeros((16, 3))
    counts, steps = np.zeros(64, np.int32), np.zeros(64, np.int32)
    wraps = [
        ("attpc_sim_run", lambda f, n: ctx.lib.attpc_sim_run(ctx.handle, 1, f, n, lay, None, None, None, None, st)),
        ("attpc_kin_run", lambda f, n: ctx.lib.attpc_kin_run(ctx.handle, 1, f, n, None, None, None, None)),
        ("attpc_sim_hint_next", lambda f, n: ctx.lib.attpc_sim_hint_next(ctx.handle, 1, f, n, lay)),
        ("attpc_det_tracks", lambda f, n: ctx.lib.attpc_det_tracks(ctx.handle, 1, f, n, lay, _abi.dptr(p4), _abi.dptr(vertex),
                                                                  0, None, _abi.iptr(counts, _abi.C.c_int32),
                                                                  _abi.iptr(steps, _abi.C.c_int32))),
        ("attpc_det_scatter", lambda f, n: ctx.lib.attpc_det_scatter(ctx.handle, 1, f, n, lay, None,
                                                                    _abi.iptr(counts, _abi.C.c_int32), None, st)),
    ]
    for name, call in wraps:
        for f, n in ((U64 - 5, 10), (U64 - 1, 2), (2, U64 - 1)):
            with pytest.raises(ValueError):  # (a range that does not wrap would start a real run here)
                _abi.check_id_range(1, f, n)
            assert call(f, n) == _abi.E_INVALID, (name, f, n)
            assert b"2^64" in ctx.lib.attpc_last_error(ctx.handle), name
    ctx.check(ctx.lib.attpc_sim_hint_next(ctx.handle, 1, 0, 0, lay), "withdraw")
    # the last ids of the range are fine
    inp.pipeline.run_many(4, first_event=U64 - 4, seed=SEED_LO_ZERO, return_status=True)
    st_top = eng.run(4, seed=SEED_LO_ZERO, first_event=U64 - 4)["stats"]
    assert st_top["n_events"] == 4 and st_top["n_failed"] == 0
