"""The drift distortion on the device (``distort_kernel``, csrc/distort.hip) against its restatement
(tests/distortion_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The kernel reads the records the track kernel left and the arithmetic of one record is written down operation by
operation (include/attpc_engine.h, "drift distortion"), so every comparison of records here is bit for bit: the
tolerance is zero by construction, not by measurement.  M is the named map of tests/distortion_cases.py."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.distortion import DistortionMap, samples_to_distortion
from tests import distortion_cases as dc
from tests import distortion_reference as dref
from tests.helpers import Inputs, sort_cloud

pytestmark = pytest.mark.gpu

C = _abi.C
CALL = "attpc_det_configure_distortion"


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.check(context.lib.attpc_det_configure_distortion(context.handle, None), CALL)
    context.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _desc(m: dref.Map, **changes):
    """(attpc_distort_desc of ``m``, the arrays it refers to); ``changes`` overwrite scalar fields."""
    keep = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in (m.radial, m.azimuthal, m.time)]
    n_rho, n_tau = m.shape if any(t is not None for t in keep) else (2, 2)
    fields = {"rho_step": m.rho_step, "tau_step": m.tau_step, "tb_origin": m.tb_origin, "n_rho": n_rho, "n_tau": n_tau, **changes}
    return _abi.DistortDesc(fields["rho_step"], fields["tau_step"], fields["tb_origin"], fields["n_rho"], fields["n_tau"],
                            *(_abi.dptr(t) for t in keep)), keep


def _distortion(ctx, m):
    """``attpc_det_configure_distortion`` through the C ABI directly (None: NULL, the stage off)."""
    ctx.forget("distortion")
    desc, keep = (None, None) if m is None else _desc(m)
    ctx.check(ctx.lib.attpc_det_configure_distortion(ctx.handle, desc), CALL)
    del keep


def _tracks(ctx, layout, p4, vertex, seed, first, max_samples=_abi.TIME_SAMPLES):
    """(samples [tracks, max_samples, 4], counts, n_steps) of ``attpc_det_tracks`` on the configured detector."""
    n = len(p4)
    nt = n * layout.n_sim
    samples = np.zeros((nt, max_samples, 4))
    counts = np.empty(nt, dtype=np.int32)
    steps = np.empty(nt, dtype=np.int32)
    ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, seed, first, n, layout, _abi.dptr(np.ascontiguousarray(p4)),
                                       _abi.dptr(np.ascontiguousarray(vertex)), max_samples, _abi.dptr(samples),
                                       _abi.iptr(counts, C.c_int32), _abi.iptr(steps, C.c_int32)), "attpc_det_tracks")
    return samples, counts, steps


def _device_tracks(ctx, inp, p4, vertex, seed, first):
    ctx.forget("det")
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, inp.det), "attpc_det_configure")
    return _tracks(ctx, inp.layout, p4, vertex, seed, first)


def _kept(samples, counts):
    """The kept records of every track, one behind the other [sum(counts), 4]."""
    return np.concatenate([samples[t, :c] for t, c in enumerate(counts)]) if len(counts) else np.zeros((0, 4))


def _same(a, b):
    for x, y in zip(a, b):
        assert dref.same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)


# 1 ------------------------------------------------------------------------------------------ off is off ----
def test_null_and_zero_maps_equal_unconfigured(ctx, orc):
    inp = Inputs("be10dp")
    seed, first, n = 13, 5, 8
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    m = dc.reference_map()
    plain = _device_tracks(ctx, inp, p4, vertex, seed, first)  # a context that was never configured
    assert plain[1].sum() > 100
    zero = np.zeros(m.shape)
    for off in (None, dref.Map(m.rho_step, m.tau_step, m.tb_origin, None, None, None),
                dref.Map(m.rho_step, m.tau_step, m.tb_origin, zero, zero, zero),
                dref.Map(m.rho_step, m.tau_step, m.tb_origin, None, -zero, None)):
        _distortion(ctx, m)
        _distortion(ctx, off)
        _same(plain, _device_tracks(ctx, inp, p4, vertex, seed, first))
    _distortion(ctx, m)
    on = _device_tracks(ctx, inp, p4, vertex, seed, first)
    assert np.array_equal(on[1], plain[1]) and np.array_equal(on[2], plain[2])
    assert not np.array_equal(_kept(on[0], on[1])[:, :3], _kept(plain[0], plain[1])[:, :3])
    # reconfiguring the detector keeps the stage (_device_tracks does), NULL drops it
    _same(on, _device_tracks(ctx, inp, p4, vertex, seed, first))
    _distortion(ctx, None)
    _same(plain, _device_tracks(ctx, inp, p4, vertex, seed, first))
    # every invalid desc is refused, by the configure call and by the stage alone, and leaves the stage as it was
    _distortion(ctx, m)
    records = dc.random_records(16)
    out = np.empty_like(records)
    for what, value in dc.bad_descs():
        bad = dref.Map(m.rho_step, m.tau_step, m.tb_origin, m.radial.copy(), m.azimuthal.copy(), m.time.copy())
        changes = {}
        if what in ("radial", "azimuthal", "time"):
            getattr(bad, what)[5, 7] = value
        else:
            changes[what] = value
            if what in ("n_rho", "n_tau"):
                bad.radial = bad.azimuthal = bad.time = None
        desc, keep = _desc(bad, **changes)
        assert ctx.lib.attpc_det_configure_distortion(ctx.handle, desc) == _abi.E_INVALID, (what, value)
        assert ctx.lib.attpc_samples_distort(ctx.handle, len(records), _abi.dptr(records), desc, _abi.dptr(out)) == _abi.E_INVALID
    assert ctx.lib.attpc_samples_distort(ctx.handle, len(records), _abi.dptr(records), None, _abi.dptr(out)) == _abi.E_INVALID
    assert ctx.lib.attpc_samples_distort(ctx.handle, -1, _abi.dptr(records), _desc(m)[0], _abi.dptr(out)) == _abi.E_INVALID
    _same(on, _device_tracks(ctx, inp, p4, vertex, seed, first))
    _distortion(ctx, None)


# 2 ------------------------------------------------------------------------------------------ records, exactly ----
@pytest.mark.parametrize("name,n,options", [("be10dp", 8, {}), ("o16aa", 24, {}), ("be10dp", 8, {"track_workgroups": 1}),
                                            ("o16aa", 24, {"track_workgroups": 1}), ("b10chain", 2, {})])
def test_records_equal_the_restatement(ctx, orc, name, n, options):
    inp = Inputs(name)
    seed, first = 13, 5
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    m = dc.reference_map()
    for key, value in options.items():
        ctx.set_option(key, value)
    try:
        _distortion(ctx, None)
        plain = _device_tracks(ctx, inp, p4, vertex, seed, first)
        _distortion(ctx, m)
        on = _device_tracks(ctx, inp, p4, vertex, seed, first)
    finally:
        for key in options:
            ctx.set_option(key, 0)
        _distortion(ctx, None)
    counts = plain[1]
    blocks = (counts + 127) // 128
    print(name, options, "tracks", len(counts), "records", int(counts.sum()), "blocks per track", blocks.tolist())
    assert np.array_equal(on[1], counts) and np.array_equal(on[2], plain[2])
    # (chains of one block and of several; the path-length step fills whole chains of 79)
    assert counts.sum() > 1000 and (counts % 128 != 0).any()
    assert blocks.max() == 79 if name == "b10chain" else (blocks.min() <= 1 and blocks.max() >= 8)
    want = dref.shift_records(m, _kept(plain[0], counts))
    got = _kept(on[0], counts)
    differ = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert differ.size == 0, (name, differ[:10], got[differ[:3]], want[differ[:3]])
    assert (got[:, :3] != _kept(plain[0], counts)[:, :3]).any(axis=1).mean() > 0.5
    # nothing past a track's count was written to the caller's array
    for t, c in enumerate(counts):
        assert not on[0][t, c:].any()


def test_records_equal_the_restatement_behind_the_straggling(ctx, orc):
    """Straggling and the distortion both act on the track samples in front of the scatter, the distortion last: with
    both on, the records are the restatement's shift of the device's own straggled records, bit for bit."""
    from attpc_engine_amd.detector.straggling import StragglingSettings, configure_straggling
    inp = Inputs("be10dp")
    seed, first, n = 13, 5, 8
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    m = dc.reference_map()
    try:
        _distortion(ctx, None)
        plain = _device_tracks(ctx, inp, p4, vertex, seed, first)
        configure_straggling(ctx, StragglingSettings(stream=3), inp.config)
        straggled = _device_tracks(ctx, inp, p4, vertex, seed, first)
        _distortion(ctx, m)
        both = _device_tracks(ctx, inp, p4, vertex, seed, first)
    finally:
        configure_straggling(ctx, None)
        _distortion(ctx, None)
    counts = straggled[1]
    print("tracks", len(counts), "records", int(counts.sum()), "unstraggled", int(plain[1].sum()))
    assert np.array_equal(both[1], counts) and np.array_equal(both[2], straggled[2]) and counts.sum() > 1000
    # the straggling is there: other records than without it
    assert not np.array_equal(counts, plain[1]) or not dref.same_bits(_kept(straggled[0], counts), _kept(plain[0], plain[1]))
    want = dref.shift_records(m, _kept(straggled[0], counts))
    got = _kept(both[0], counts)
    differ = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert differ.size == 0, (differ[:10], got[differ[:3]], want[differ[:3]])
    assert (got[:, :3] != _kept(straggled[0], counts)[:, :3]).any(axis=1).mean() > 0.5
    for t, c in enumerate(counts):
        assert not both[0][t, c:].any()
    # ... and with the stages off again the records are the first ones
    _same(plain, _device_tracks(ctx, inp, p4, vertex, seed, first))


# 3 ------------------------------------------------------------------------------------------ the stage alone ----
def test_stage_alone(ctx):
    named, m, config = dc.named_map(), dc.reference_map(), dc.drift()
    _distortion(ctx, None)
    edge = dc.edge_records()
    got = samples_to_distortion(edge, named, config, ctx)
    assert dref.same_bits(got, dref.shift_records(m, edge))
    pool = np.concatenate([edge, dc.random_records(30000 - len(edge), seed=3, rho_limit=0.35)])
    for n in (0, 1, 127, 128, 129, 10112, 10113, 30000):
        records = np.ascontiguousarray(pool[:n])
        got = samples_to_distortion(records, named, config, ctx)
        assert got.shape == (n, 4) and dref.same_bits(got, dref.shift_records(m, records)), n
    ctx.set_option("track_workgroups", 1)  # one workgroup: its waves loop over the chains
    try:
        assert dref.same_bits(samples_to_distortion(pool, named, config, ctx), dref.shift_records(m, pool))
    finally:
        ctx.set_option("track_workgroups", 0)
    # a map that shifts nothing copies the records; in place is allowed
    assert dref.same_bits(samples_to_distortion(edge, DistortionMap(np.zeros((2, 2))), config, ctx), edge)
    records = pool[:1000].copy()
    desc, keep = _desc(m)
    ctx.check(ctx.lib.attpc_samples_distort(ctx.handle, len(records), _abi.dptr(records), desc, _abi.dptr(records)), "in place")
    assert dref.same_bits(records, dref.shift_records(m, pool[:1000]))
    # single tables, and a map of the smallest and of the largest size
    rng = np.random.default_rng(5)
    for shape in ((2, 2), (256, 256), (2, 256)):
        tables = [rng.uniform(-0.02, 0.02, size=shape), rng.uniform(-0.02, 0.02, size=shape), rng.uniform(-5.0, 5.0, size=shape)]
        for keep_only in (None, 0, 1, 2):
            part = dref.Map(0.3 / (shape[0] - 1), 550.0 / (shape[1] - 1), 10.0,
                            *(t if keep_only in (None, k) else None for k, t in enumerate(tables)))
            desc, keep = _desc(part)
            out = np.empty_like(edge)
            ctx.check(ctx.lib.attpc_samples_distort(ctx.handle, len(edge), _abi.dptr(edge), desc, _abi.dptr(out)), "stage alone")
            assert dref.same_bits(out, dref.shift_records(part, edge)), (shape, keep_only)


# 4 ------------------------------------------------------------------------------------------ consumed once, by everything ----
def _sorted_events(res):
    return [sort_cloud(res["points"][lo:hi], res["labels"][lo:hi]) for lo, hi in zip(res["offsets"][:-1], res["offsets"][1:])]


def _same_events(a, b):
    assert len(a) == len(b)
    for (pa, la), (pb, lb) in zip(a, b):
        np.testing.assert_array_equal(pa, pb)
        np.testing.assert_array_equal(la, lb)


def _scatter(ctx, layout, samples, counts, seed, first, n, capacity):
    offsets = np.zeros(n + 1, dtype=np.int64)
    points = np.empty((capacity, 3))
    labels = np.empty(capacity, dtype=np.int64)
    out = _abi.CloudOut(capacity, _abi.iptr(offsets, C.c_int64), _abi.dptr(points), _abi.iptr(labels, C.c_int64), None)
    stats = _abi.RunStats()
    packed = np.ascontiguousarray(_kept(samples, counts))
    ctx.check(ctx.lib.attpc_det_scatter(ctx.handle, seed, first, n, layout, _abi.dptr(packed),
                                        _abi.iptr(np.ascontiguousarray(counts), C.c_int32), out, stats), "attpc_det_scatter")
    return {"offsets": offsets, "points": points[:offsets[-1]], "labels": labels[:offsets[-1]], "stats": stats.as_dict()}


SEED, FIRST, N = 17, (1 << 32) - 10, 24
MASK = (1 << 64) - 1


def test_the_shift_is_consumed_once_by_everything():
    from attpc_engine_amd.detector.simulator import simulate_batch
    from attpc_engine_amd.engine import Engine
    inp = Inputs("o16aa")
    named, m = dc.named_map(), dc.reference_map()
    fresh = _abi.Context(0)
    try:
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=fresh)
        off = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
        eng.configure_distortion(named)
        whole = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
        for key in ("charge_checksum", "key_checksum"):
            assert whole["stats"][key] != off["stats"][key], key
        assert whole["stats"]["n_track_samples"] == off["stats"]["n_track_samples"]
        events = _sorted_events(whole)
        assert sum(len(p) for p, _ in events) > 1000
        # the records of test 2, and the scatter fed with them: the same clouds
        on = _tracks(fresh, eng.layout, whole["p4"], whole["vertex"], SEED, FIRST)
        eng.configure_distortion()
        plain = _tracks(fresh, eng.layout, whole["p4"], whole["vertex"], SEED, FIRST)
        assert np.array_equal(on[1], plain[1]) and np.array_equal(on[2], plain[2])
        assert dref.same_bits(_kept(on[0], on[1]), dref.shift_records(m, _kept(plain[0], plain[1])))
        fed = _scatter(fresh, eng.layout, on[0], on[1], SEED, FIRST, N, len(whole["points"]) + 64)
        _same_events(events, _sorted_events(fed))
        for key in ("charge_checksum", "key_checksum", "n_points"):
            assert fed["stats"][key] == whole["stats"][key], key
        _same_events(_sorted_events(off), _sorted_events(_scatter(fresh, eng.layout, plain[0], plain[1], SEED, FIRST, N,
                                                                  len(off["points"]) + 64)))
        # one call, two calls, chunks of 5, resident
        eng.configure_distortion(named)
        resident = eng.run(N, seed=SEED, first_event=FIRST)["stats"]
        halves = [eng.run(12, seed=SEED, first_event=FIRST + lo, fetch=True) for lo in (0, 12)]
        fresh.check(fresh.lib.attpc_set_chunk_events(fresh.handle, 5), "attpc_set_chunk_events")
        chunked = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
        chunked_resident = eng.run(N, seed=SEED, first_event=FIRST)["stats"]
        fresh.check(fresh.lib.attpc_set_chunk_events(fresh.handle, 0), "attpc_set_chunk_events")
        _same_events(events, _sorted_events(chunked))
        _same_events(events, _sorted_events(halves[0]) + _sorted_events(halves[1]))
        for key in ("charge_checksum", "key_checksum"):
            assert whole["stats"][key] == resident[key] == chunked["stats"][key] == chunked_resident[key], key
            assert whole["stats"][key] == (halves[0]["stats"][key] + halves[1]["stats"][key]) & MASK, key
        for key in ("n_points", "n_track_samples"):
            assert whole["stats"][key] == resident[key] == chunked["stats"][key] == halves[0]["stats"][key] + halves[1]["stats"][key]
        # the summaries' end points are those of the shifted, apparent record
        summary = eng.run_summary(N, seed=SEED, first_event=FIRST)
        tracks = summary["tracks"].reshape(-1)
        has = on[1] > 0
        assert has.sum() > 10
        last = np.stack([on[0][t, on[1][t] - 1, :3] for t in np.flatnonzero(has)])
        for k, field in enumerate(("end_x", "end_y", "end_tb")):
            assert dref.same_bits(np.ascontiguousarray(tracks[field][has]), np.ascontiguousarray(last[:, k])), field
        assert np.array_equal(tracks["n_samples"], on[1])
        # the file-driven form, and a call without the keyword
        args = (whole["p4"], whole["vertex"], inp.z, inp.a, inp.config, SEED, inp.indices)
        for want, distortion in ((whole, named), (off, None), (off, DistortionMap(np.zeros((3, 3))))):
            offsets, points, labels, stats = simulate_batch(*args, first_event=FIRST, ctx=fresh, distortion=distortion)
            np.testing.assert_array_equal(offsets, want["offsets"])
            _same_events(_sorted_events(want), _sorted_events({"offsets": offsets, "points": points, "labels": labels}))
            assert stats["key_checksum"] == want["stats"]["key_checksum"]
    finally:
        fresh.close()
    # a fresh context with undersized buffers: the arena and the cloud buffers grow and the launches run again
    tiny = _abi.Context(0)
    try:
        tiny.set_option("tiny_buffers", 1)
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=tiny, chunk_events=7)
        eng.configure_distortion(named)
        res = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
        assert res["stats"]["n_buffer_growths"] > 0
        _same_events(events, _sorted_events(res))
        # a call whose output capacity was too small (4096 rows) is repeated
        assert len(whole["points"]) > 4096
        small = eng.run(N, seed=SEED, first_event=FIRST, fetch=True, capacity_per_event=64)
        _same_events(events, _sorted_events(small))
        again = eng.run(N, seed=SEED, first_event=FIRST)["stats"]
        for key in ("charge_checksum", "key_checksum", "n_points"):
            assert res["stats"][key] == small["stats"][key] == whole["stats"][key] == again[key], key
    finally:
        tiny.close()
    resident_ctx = _abi.Context(0)
    try:
        resident_ctx.set_option("tiny_buffers", 1)
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=resident_ctx, chunk_events=7)
        eng.configure_distortion(named)
        stats = eng.run(N, seed=SEED, first_event=FIRST)["stats"]
        assert stats["n_buffer_growths"] > 0
        for key in ("charge_checksum", "key_checksum", "n_points"):
            assert stats[key] == whole["stats"][key], key
    finally:
        resident_ctx.close()


# 5 ------------------------------------------------------------------------------------------ downstream ----
def test_trace_rows_and_estimates_across_a_split():
    from attpc_engine_amd.engine import Engine
    inp = Inputs("o16aa")
    fresh = _abi.Context(0)
    try:
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=fresh)
        eng.configure_estimates(min_points=10)
        eng.configure_thinning(z_step=10)
        off = eng.run_trace_rows(N, seed=SEED, first_event=FIRST)
        eng.configure_distortion(dc.named_map())
        rows = eng.run_trace_rows(N, seed=SEED, first_event=FIRST)
        parts = [eng.run_trace_rows(12, seed=SEED, first_event=FIRST + lo) for lo in (0, 12)]
        assert rows["estimates"].shape == (N, len(inp.indices)) and rows["trace_rows"]["n_rows"] > 100
        assert rows["estimates"].tobytes() == np.concatenate([p["estimates"] for p in parts]).tobytes()
        assert rows["rows"].tobytes() == np.concatenate([p["rows"] for p in parts]).tobytes()
        assert rows["labels"].tobytes() == np.concatenate([p["labels"] for p in parts]).tobytes()
        assert rows["estimates"].tobytes() != off["estimates"].tobytes() and rows["rows"].tobytes() != off["rows"].tobytes()
        eng.configure_distortion()
        assert eng.run_trace_rows(N, seed=SEED, first_event=FIRST)["estimates"].tobytes() == off["estimates"].tobytes()
    finally:
        fresh.close()
