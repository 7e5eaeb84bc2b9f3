"""Event and track summaries on the device, exactly (integers equal, doubles bit-equal, NaN where NaN) against the numpy
restatement of the contract (tests/summary_reference.py) applied to the device's own delivered clouds and track
samples; cross-checks against the paths that exist (event_points, the charge checksum, the Spyral rows, the resident
run's statistics); invariance under splits, chunk sizes, scatter builds and undersized buffers; hand-made clouds through
``attpc_cloud_summary``; and the other outputs unchanged beside summary runs.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.summary import (NEVER_KEPT, clouds_to_summary, configure_summary,
                                               electrons_above_threshold, simulate_batch_summary)
from tests.helpers import Inputs, id_case
from tests.summary_reference import (assert_same_records, check_expected, csr, hand_made_centers, hand_made_events,
                                     summary)

pytestmark = pytest.mark.gpu

WORKLOADS = {"be10dp": 300, "o16aa": 300, "b10chain": 40}  # events per workload
SEED, FIRST = 5, 1000
CLOUD_FIELDS = ["n_points", "n_kept", "n_pads", "tb_min", "tb_max", "reserved", "charge", "rho2_max"]
TRACK_FIELDS = ["n_steps", "n_samples", "electrons", "end_x", "end_y", "end_tb"]
# the counts and checksums of attpc_run_stats (not its times, launches, growths or bytes; not n_lds_overflow, which
# counts windows redone by the scatter build a context happens to use)
STAT_KEYS = ["n_events", "n_points", "n_track_samples", "n_sample_limit", "n_failed", "charge_checksum", "key_checksum",
             "n_inconsistent", "n_lone_buckets", "n_tracks_capped"]


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine
    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _fresh(**options):
    ctx = _abi.Context(0)
    for key, value in options.items():
        ctx.set_option(key, value)
    return ctx


_cache = {}


def _workload(name, ctx):
    """(inputs, engine on the shared context, its delivered clouds of the workload's events)."""
    if name not in _cache:
        inp = Inputs(name)
        eng = _engine(inp, ctx)
        _cache[name] = (inp, eng.run(WORKLOADS[name], seed=SEED, first_event=FIRST, fetch=True))
    inp, fetched = _cache[name]
    return inp, _engine(inp, ctx), fetched


def _same(got, ref, what):
    assert_same_records(got["events"] if isinstance(got, dict) else got[0], ref["events"] if isinstance(ref, dict) else ref[0],
                        what + " events")
    assert_same_records(got["tracks"] if isinstance(got, dict) else got[1], ref["tracks"] if isinstance(ref, dict) else ref[1],
                        what + " tracks")


@pytest.mark.parametrize("min_electrons", [0, None, NEVER_KEPT], ids=["keep_all", "default", "none_kept"])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_run_summary_vs_restatement_of_own_cloud(ctx, name, min_electrons):
    inp, eng, fetched = _workload(name, ctx)
    n = WORKLOADS[name]
    eng.configure_summary(min_electrons=min_electrons)
    res = eng.run_summary(n, seed=SEED, first_event=FIRST)
    threshold = electrons_above_threshold(inp.config) if min_electrons is None else min_electrons
    ref_events, ref_tracks = summary(fetched["offsets"], fetched["points"], fetched["labels"], inp.indices, threshold,
                                     inp.config.pad_centers)
    assert_same_records(res["events"], ref_events, f"{name} events")
    assert_same_records(res["tracks"][CLOUD_FIELDS], ref_tracks[CLOUD_FIELDS], f"{name} tracks (cloud part)")
    events, tracks = res["events"], res["tracks"]
    print(name, "min_electrons", threshold, "rows", int(events["n_points"].sum()), "kept", int(events["n_kept"].sum()),
          "pads per event", float(events["n_pads"].mean()), "events without a kept row", int((events["n_kept"] == 0).sum()))
    # ---- the paths that exist ----
    np.testing.assert_array_equal(events["n_points"], fetched["event_points"])
    assert int(events["charge"].astype(object).sum()) % (1 << 64) == res["stats"]["charge_checksum"]
    for key in ("vertex", "p4", "status"):
        np.testing.assert_array_equal(res[key], fetched[key], err_msg=key)
    assert res["indices"] == list(inp.indices)
    resident = eng.run(n, seed=SEED, first_event=FIRST)["stats"]
    assert {k: res["stats"][k] for k in STAT_KEYS} == {k: resident[k] for k in STAT_KEYS}
    assert {k: fetched["stats"][k] for k in STAT_KEYS} == {k: resident[k] for k in STAT_KEYS}
    if min_electrons is None:  # kept = survives the ADC threshold as a Spyral row
        rows = eng.run_spyral(n, seed=SEED, first_event=FIRST)
        np.testing.assert_array_equal(tracks["n_kept"].sum(axis=1), np.diff(rows["offsets"]))
        np.testing.assert_array_equal(events["n_kept"], np.diff(rows["offsets"]))
        assert events["n_kept"].sum() > 0
    if min_electrons == NEVER_KEPT:
        assert (events["n_kept"] == 0).all() and (tracks["rho2_max"] == -1.0).all() and (events["tb_max"] == -1).all()
    if min_electrons == 0:
        assert (events["n_kept"] == events["n_points"]).all()
        # every row carries the label of a simulated nucleus: the tracks partition the event
        np.testing.assert_array_equal(tracks["n_points"].sum(axis=1), events["n_points"])
        np.testing.assert_array_equal(tracks["charge"].sum(axis=1), events["charge"])


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_track_part_vs_det_tracks(ctx, name):
    """The whole track record through the file-driven entry point, on the kinematics of the fused run: the cloud part
    against the clouds of attpc_det_run, the track part against attpc_det_tracks; and the fused run's records equal."""
    from attpc_engine_amd.detector.simulator import simulate_batch

    inp, eng, fetched = _workload(name, ctx)
    n = min(WORKLOADS[name], 48)
    p4, vertex = np.ascontiguousarray(fetched["p4"][:n]), np.ascontiguousarray(fetched["vertex"][:n])
    min_electrons = electrons_above_threshold(inp.config)
    got = simulate_batch_summary(p4, vertex, inp.z, inp.a, inp.config, SEED, inp.indices, first_event=FIRST, ctx=ctx)
    offsets, points, labels, _ = simulate_batch(p4, vertex, inp.z, inp.a, inp.config, SEED, inp.indices, first_event=FIRST,
                                                ctx=ctx)
    nt = n * len(inp.indices)
    samples = np.zeros((nt, _abi.TIME_SAMPLES, 4))
    counts, steps = np.empty(nt, dtype=np.int32), np.empty(nt, dtype=np.int32)
    ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, SEED, FIRST, n, inp.layout, _abi.dptr(p4), _abi.dptr(vertex),
                                       _abi.TIME_SAMPLES, _abi.dptr(samples), _abi.iptr(counts, _abi.C.c_int32),
                                       _abi.iptr(steps, _abi.C.c_int32)), "attpc_det_tracks")
    ref = summary(offsets, points, labels, inp.indices, min_electrons, inp.config.pad_centers, samples, counts, steps)
    _same(got, ref, name)
    tracks = got[1]
    assert (tracks["n_samples"] > 0).any() and (tracks["electrons"] > 0).any() and np.isfinite(tracks["end_tb"]).any()
    skipped = [s for s, row in enumerate(inp.indices) if inp.layout.species_of_row[row] < 0]
    for s in skipped:  # an all-empty record
        assert (tracks[:, s]["n_steps"] == 0).all() and np.isnan(tracks[:, s]["end_x"]).all() and (tracks[:, s]["n_points"] == 0).all()
    print(name, "tracks", nt, "samples per track", float(tracks["n_samples"].mean()), "skipped positions", skipped)
    assert (fetched["status"][:n] == 0).all()  # (an event at the sample limit has no tracks in the fused run)
    eng.configure_summary()
    fused = eng.run_summary(n, seed=SEED, first_event=FIRST)
    _same(fused, got, name + " fused against file-driven")


def test_invariance_under_splits_chunks_builds_and_small_buffers(ctx):
    case = id_case("u32_wrap")  # the ids cross 2^32 inside the range
    first, seed, n = case.first_event - 150, case.seed, 200
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_summary()
    whole = eng.run_summary(n, seed=seed, first_event=first)
    assert (whole["events"]["n_points"] > 0).any()
    # the same ids in three calls with uneven first_event
    parts = [eng.run_summary(m, seed=seed, first_event=first + at) for at, m in ((0, 37), (37, 101), (138, 62))]
    assert_same_records(np.concatenate([p["events"] for p in parts]), whole["events"], "split events")
    assert_same_records(np.concatenate([p["tracks"] for p in parts]), whole["tracks"], "split tracks")
    for options, kw in (({}, {"chunk_events": 7}), ({}, {"chunk_events": 1000}), ({"scatter_variant": 1}, {}),
                        ({"scatter_variant": 2}, {}), ({"scatter_variant": 3}, {}), ({"scatter_merge": 1}, {}),
                        ({"tiny_buffers": 1}, {})):
        other_ctx = _fresh(**options)
        other = _engine(inp, other_ctx, **kw)
        other.configure_summary()
        res = other.run_summary(n, seed=seed, first_event=first)
        _same(res, whole, f"{options} {kw}")
        assert {k: res["stats"][k] for k in STAT_KEYS} == {k: whole["stats"][k] for k in STAT_KEYS}, (options, kw)
        if options.get("tiny_buffers"):  # the chunks were scattered again, and their records written again
            assert res["stats"]["n_buffer_growths"] > 0
            again = other.run_summary(n, seed=seed, first_event=first)
            _same(again, whole, "tiny buffers, second call")
        other_ctx.close()


def test_cloud_with_a_lone_bucket(ctx):
    """A time bucket that went through lone_bucket_kernel (the fixture and forced build of
    tests/test_gpu_scatter_fixtures.py): its cloud through attpc_cloud_summary."""
    from tests.test_gpu_scatter_fixtures import _configure, _plane_filling_event, device_scatter

    cfg, _, keep = _configure(ctx, 0.277)
    big = _plane_filling_event(cfg)
    small = [(xyt[:40] * np.array([1.0, 1.0, 0.5]), el[:40], lab) for xyt, el, lab in big]
    ctx.set_option("scatter_variant", 1)
    try:
        clouds, stats = device_scatter(ctx, [small, big, small])
    finally:
        ctx.set_option("scatter_variant", 0)
    assert stats["n_lone_buckets"] >= 1 and stats["n_failed"] == 0
    indices = [lab for _, _, lab in big]
    offsets, points, labels = csr(clouds)
    for min_electrons in (0, int(np.median(points[:, 2]))):
        configure_summary(cfg, ctx, min_electrons)
        got = clouds_to_summary(offsets, points, labels, indices, ctx, n_rows=18)
        _same(got, summary(offsets, points, labels, indices, min_electrons, cfg.pad_centers), f"lone bucket, {min_electrons}")
    assert got[0]["n_points"][1] > 8192 and 0 < got[0]["n_kept"][1] < got[0]["n_points"][1]


def test_host_clouds(ctx):
    inp = Inputs("o16aa")
    centers = hand_made_centers()
    config = type("Geometry", (), {"pad_centers": centers, "elec_params": inp.config.elec_params})()
    ev, indices, min_electrons, expected = hand_made_events()
    offsets, points, labels = csr(ev)
    configure_summary(config, ctx, min_electrons)
    got = clouds_to_summary(offsets, points, labels, indices, ctx)
    check_expected(got[0], got[1], expected)
    _same(got, summary(offsets, points, labels, indices, min_electrons, centers), "hand-made")
    assert (got[1]["n_steps"] == 0).all() and (got[1]["electrons"] == 0).all() and np.isnan(got[1]["end_tb"]).all()
    # 1 000 empty events
    events, tracks = clouds_to_summary(np.zeros(1001, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64), [2, 5], ctx)
    assert events.shape == (1000,) and (events["n_points"] == 0).all() and (events["tb_min"] == -1).all()
    assert (events["charge"] == 0).all() and (tracks["rho2_max"] == -1.0).all() and (tracks["n_pads"] == 0).all()
    # one event of 100 000 rows: many segments' worth in one segment, (pad, t) cells repeated
    rng = np.random.default_rng(3)
    rows = 100_000
    points = np.column_stack([rng.integers(0, _abi.NUM_PADS, rows).astype(np.float64), rng.random(rows) * 511.999,
                              rng.integers(0, 1 << 40, rows).astype(np.float64)])
    labels = rng.choice([2, 5, 9, 17, 33, -1], rows)
    offsets = np.array([0, 0, rows, rows])
    for threshold in (0, 1 << 39):
        configure_summary(config, ctx, threshold)
        got = clouds_to_summary(offsets, points, labels, [5, 2, 17, 0], ctx, n_rows=18)
        _same(got, summary(offsets, points, labels, [5, 2, 17, 0], threshold, centers), f"100 000 rows, {threshold}")
    assert got[0]["n_points"].tolist() == [0, rows, 0] and 0 < got[0]["n_kept"][1] < rows
    # rows the contract refuses
    for bad in ([10240.0, 3.0, 5.0], [-1.0, 3.0, 5.0], [1.5, 3.0, 5.0], [1.0, 512.0, 5.0], [1.0, -0.5, 5.0], [1.0, 3.0, -1.0],
                [1.0, 3.0, np.nan], [1.0, 3.0, np.inf]):
        with pytest.raises(ValueError):
            clouds_to_summary(np.array([0, 2]), np.array([[4.0, 4.0, 4.0], bad]), np.zeros(2, dtype=np.int64), [0], ctx)
    clouds_to_summary(np.array([0, 2]), np.array([[4.0, 4.5, 4.0], [4.0, 4.2, 6.0]]), np.zeros(2, dtype=np.int64), [0], ctx)


def test_not_configured():
    ctx = _fresh()
    lib, layout, out = ctx.lib, Inputs("o16aa").layout, _abi.SummaryOut()
    offsets = np.zeros(2, dtype=np.int64)
    call = lambda: lib.attpc_cloud_summary(ctx.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, layout, out)  # noqa: E731
    assert call() == _abi.E_NOTCONFIGURED
    centers = hand_made_centers()
    for desc in (_abi.SummaryDesc(-1, _abi.dptr(centers), len(centers), 0), _abi.SummaryDesc(0, None, len(centers), 0),
                 _abi.SummaryDesc(0, _abi.dptr(centers), _abi.NUM_PADS - 1, 0)):
        assert lib.attpc_summary_configure(ctx.handle, desc) == _abi.E_INVALID
    assert call() == _abi.E_NOTCONFIGURED
    assert lib.attpc_summary_configure(ctx.handle, _abi.SummaryDesc(0, _abi.dptr(centers), len(centers), 0)) == _abi.OK
    assert call() == _abi.OK
    assert lib.attpc_summary_configure(ctx.handle, None) == _abi.OK
    assert call() == _abi.E_NOTCONFIGURED
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    stats = _abi.RunStats()
    assert lib.attpc_sim_run_summary(ctx.handle, 1, 0, 4, eng.layout, None, None, None, out, stats) == _abi.E_NOTCONFIGURED
    ctx.close()


def _canonical(offsets, rows, labels):
    """Rows in a canonical order per event (the order of a delivered cloud's rows within an event is unspecified)."""
    event = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort(tuple(rows[:, c] for c in range(rows.shape[1] - 1, -1, -1)) + (event,))
    return rows[order], labels[order]


def test_summary_runs_leave_nothing_behind():
    inp = Inputs("be10dp")
    n, seed, first = 96, 4, 10

    def outputs(summaries_first):
        ctx = _fresh()
        eng = _engine(inp, ctx)
        if summaries_first:
            eng.run_summary(n, seed=seed, first_event=first)
            eng.configure_summary(min_electrons=0)
            eng.run_summary(n // 2, seed=seed + 1, first_event=first + 7)
        cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
        if summaries_first:
            eng.run_summary(n, seed=seed, first_event=first)
        rows = eng.run_spyral(n, seed=seed, first_event=first)
        traces = eng.run_traces(n, seed=seed, first_event=first)
        ctx.close()
        return cloud, rows, traces

    (cloud_a, rows_a, traces_a), (cloud_b, rows_b, traces_b) = outputs(True), outputs(False)
    for a, b, key in ((cloud_a, cloud_b, "points"), (rows_a, rows_b, "rows")):
        np.testing.assert_array_equal(a["offsets"], b["offsets"])
        np.testing.assert_array_equal(a["event_points"], b["event_points"])
        for x, y in zip(_canonical(a["offsets"], a[key], a["labels"]), _canonical(b["offsets"], b[key], b["labels"])):
            np.testing.assert_array_equal(x, y, err_msg=key)
    for key in ("offsets", "pads", "samples", "labels", "event_points"):
        np.testing.assert_array_equal(traces_a[key], traces_b[key], err_msg=key)
    assert traces_a["trace"] == traces_b["trace"]
