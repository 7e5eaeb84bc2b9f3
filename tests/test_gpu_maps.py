"""Run maps on the device, exactly, against the numpy restatement of the contract (tests/maps_reference.py): hand-made
host clouds through ``attpc_cloud_maps`` with literal answers; ``run_maps`` against the restatement applied to the
device's own delivered clouds, with and without a selection; the contract's invariants against the returned records;
invariance under splits, chunk sizes, scatter builds and undersized buffers (a chunk that is scattered again counts
once); mode handling; the file-driven entry point.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.maps import FULL_MASK, MapsSettings, RunMaps, clouds_to_maps, configure_maps, simulate_batch_maps
from attpc_engine_amd.detector.selection import Selection, configure_selection
from attpc_engine_amd.detector.summary import NEVER_KEPT, configure_summary, electrons_above_threshold
from tests import maps_reference as ref
from tests.helpers import Inputs, id_case
from tests.summary_reference import assert_same_records, csr, hand_made_centers, hand_made_events

pytestmark = pytest.mark.gpu

WORKLOADS = {"be10dp": 300, "o16aa": 300, "b10chain": 40}  # events per workload (those of tests/test_gpu_summary.py)
SEED, FIRST = 5, 1000
STAT_KEYS = ["n_events", "n_points", "n_track_samples", "n_sample_limit", "n_failed", "charge_checksum", "key_checksum",
             "n_inconsistent", "n_lone_buckets", "n_tracks_capped"]
FIELDS = ("pad_events", "pad_charge", "tb_events", "tb_rows", "tb_charge")


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
        _cache[name] = (inp, _engine(inp, ctx).run(WORKLOADS[name], seed=SEED, first_event=FIRST, fetch=True))
    inp, fetched = _cache[name]
    return inp, _engine(inp, ctx), fetched


def _geometry():
    return type("Geometry", (), {"pad_centers": hand_made_centers()})()


def _cells(maps: RunMaps) -> dict:
    """The non-zero cells of every field, for literal comparisons."""
    return {name: {int(i): int(getattr(maps, name)[i]) for i in np.flatnonzero(getattr(maps, name))} for name in FIELDS}


def _host(ctx, events, indices, min_electrons, what, selection=None, fast=False, **settings):
    """The cloud ``events`` ([(points, labels)]) through attpc_cloud_maps, compared with the restatement -> the maps."""
    offsets, points, labels = csr(events)
    configure_summary(_geometry(), ctx, min_electrons)
    if selection is not None:
        configure_selection(ctx, selection)
    maps_settings = configure_maps(ctx, **settings) if settings else configure_maps(ctx, MapsSettings(other_labels=True))
    got, passed, records, tracks = clouds_to_maps(offsets, points, labels, indices, ctx, n_rows=18)
    want_passed = selection.passes(records, tracks) if maps_settings.selected else np.ones(len(events), dtype=bool)
    np.testing.assert_array_equal(passed, want_passed, err_msg=what + " passed")
    restate = ref.maps_fast if fast else ref.maps
    ref.assert_same_maps(got, restate(offsets, points, labels, indices, min_electrons, maps_settings.track_mask,
                                      want_passed if maps_settings.selected else None), what)
    return got


def _rows(*rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _labels(*labels):
    return np.array(labels, dtype=np.int64)


# ---------------------------------------------------------------- 1. host clouds ----
def test_host_clouds_one_pad_edges_and_threshold(ctx):
    # one pad in 40 time buckets of one event
    ev = [(_rows(*[[77.0, t + 0.5, 200.0] for t in range(100, 140)]), np.full(40, 2))]
    got = _host(ctx, ev, [2, 5], 100, "one pad, 40 buckets")
    assert _cells(got) == {"pad_events": {77: 1}, "pad_charge": {77: 8000}, "tb_events": {t: 1 for t in range(100, 140)},
                           "tb_rows": {t: 1 for t in range(100, 140)}, "tb_charge": {t: 200 for t in range(100, 140)}}
    assert (got.n_events, got.n_hit) == (1, 1)
    # pads 0 and 10239; tau = 0.0 and 511.99
    ev = [(_rows([0.0, 0.0, 300.0], [10239.0, 511.99, 400.0]), _labels(2, 5))]
    got = _host(ctx, ev, [2, 5], 100, "the edges of the pad and bucket ranges")
    assert _cells(got) == {"pad_events": {0: 1, 10239: 1}, "pad_charge": {0: 300, 10239: 400}, "tb_events": {0: 1, 511: 1},
                           "tb_rows": {0: 1, 511: 1}, "tb_charge": {0: 300, 511: 400}}
    # a row at exactly min_electrons and one a single electron below it
    ev = [(_rows([5.0, 7.2, 1000.0], [6.0, 8.2, 999.0]), _labels(2, 2))]
    got = _host(ctx, ev, [2, 5], 1000, "at and below min_electrons")
    assert _cells(got) == {"pad_events": {5: 1}, "pad_charge": {5: 1000}, "tb_events": {7: 1}, "tb_rows": {7: 1},
                           "tb_charge": {7: 1000}}
    # an empty event between two full ones (both on the same pad and bucket: the bitmaps of the first are gone)
    full = (_rows([9.0, 3.5, 150.0], [9.0, 4.5, 150.0]), _labels(2, 5))
    got = _host(ctx, [full, (np.zeros((0, 3)), np.zeros(0, dtype=np.int64)), full], [2, 5], 100, "an empty event between")
    assert _cells(got) == {"pad_events": {9: 2}, "pad_charge": {9: 600}, "tb_events": {3: 2, 4: 2}, "tb_rows": {3: 2, 4: 2},
                           "tb_charge": {3: 300, 4: 300}}
    assert (got.n_events, got.n_hit) == (3, 2)
    # three rows of 2e9 electrons on one pad in three buckets: the pad's charge passes 2^32
    ev = [(_rows([4000.0, 10.0, 2e9], [4000.0, 11.0, 2e9], [4000.0, 12.0, 2e9]), _labels(2, 2, 2))]
    got = _host(ctx, ev, [2, 5], 100, "charge beyond 2^32")
    assert got.pad_charge[4000] == 6_000_000_000 > 1 << 32 and got.pad_events[4000] == 1 and got.tb_charge[11] == 2_000_000_000
    # nothing kept: every map zero, the events still count
    got = _host(ctx, ev, [2, 5], NEVER_KEPT, "nothing kept")
    assert got == RunMaps(n_events=1)


def test_host_clouds_masks_and_a_label_twice(ctx):
    # labels in a masked position (2), in an unmasked position (5) and in no position (9, 40)
    ev = [(_rows([1.0, 1.5, 100.0], [2.0, 2.5, 200.0], [3.0, 3.5, 300.0], [1.0, 4.5, 400.0]), _labels(2, 5, 9, 40))]
    got = _host(ctx, ev, [2, 5], 50, "position 0", tracks=[0])
    assert _cells(got)["pad_charge"] == {1: 100} and got.n_hit == 1
    got = _host(ctx, ev, [2, 5], 50, "position 0 and the other labels", tracks=[0], other_labels=True)
    assert _cells(got)["pad_charge"] == {1: 500, 3: 300} and _cells(got)["pad_events"] == {1: 1, 3: 1}
    got = _host(ctx, ev, [2, 5], 50, "the other labels alone", tracks=[], other_labels=True)
    assert _cells(got)["pad_charge"] == {1: 400, 3: 300} and _cells(got)["tb_rows"] == {3: 1, 4: 1}
    got = _host(ctx, ev, [2, 5], 50, "every position", tracks=range(8))
    assert _cells(got)["pad_charge"] == {1: 100, 2: 200}
    got = _host(ctx, ev, [2, 5], 50, "a position above n_sim names no row", tracks=[5])
    assert got == RunMaps(n_events=1)
    # a label that occurs twice in indices belongs to its first position; the hand-made clouds of the CPU tests
    events, indices, min_electrons, _ = hand_made_events()
    for mask, cells in ref.hand_made_maps().items():
        tracks = [s for s in range(8) if mask >> s & 1]
        got = _host(ctx, events, indices, min_electrons, f"hand-made, mask {mask:#x}", tracks=tracks,
                    other_labels=bool(mask & ref.OTHER))
        ref.assert_same_maps(got, ref.from_cells(cells), f"hand-made literal, mask {mask:#x}")


def test_host_clouds_many_events_one_long_event_and_a_selection(ctx):
    # 2 000 one-row events on the same pad and bucket: more events than workgroups
    one = (_rows([1234.0, 56.7, 500.0]), _labels(2))
    got = _host(ctx, [one] * 2000, [2, 5], 100, "2 000 one-row events", fast=True)
    assert _cells(got) == {"pad_events": {1234: 2000}, "pad_charge": {1234: 1_000_000}, "tb_events": {56: 2000},
                           "tb_rows": {56: 2000}, "tb_charge": {56: 1_000_000}}
    assert (got.n_events, got.n_hit) == (2000, 2000)
    # one event of 100 000 rows in one segment, (pad, t) cells repeated, between two empty events
    rng = np.random.default_rng(3)
    rows = 100_000
    points = np.column_stack([rng.integers(0, _abi.NUM_PADS, rows).astype(np.float64), rng.random(rows) * 511.999,
                              rng.integers(0, 1 << 40, rows).astype(np.float64)])
    labels = rng.choice([2, 5, 9, 17, 33, -1], rows)
    empty = (np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    for threshold in (0, 1 << 39):
        got = _host(ctx, [empty, (points, labels), empty], [5, 2, 17, 0], threshold, f"100 000 rows, {threshold}", fast=True,
                    tracks=[0, 2], other_labels=True)
        assert (got.n_events, got.n_hit) == (3, 1) and 0 < got.tb_rows.sum() < rows and got.pad_events.max() == 1
    # a cut on n_pads that rejects some events: only the passed ones contribute
    events = [(_rows(*[[100.0 * e + p, 20.0 + e, 300.0] for p in range(e % 5 + 1)]), np.full(e % 5 + 1, 2)) for e in range(40)]
    got = _host(ctx, events, [2, 5], 100, "selected", selection=Selection(n_pads=(3, None)), other_labels=True, selected=True)
    assert got.n_events == sum(1 for e in range(40) if e % 5 + 1 >= 3) == 24 and got.n_hit == 24
    assert got.pad_events[0] == 0 and got.pad_events[200] == 1 and got.tb_events[21] == 0 and got.tb_rows[22] == 3
    both = _host(ctx, events, [2, 5], 100, "the same events, not selected", other_labels=True)
    assert both.n_events == 40 and both.pad_events[0] == 1
    configure_selection(ctx, Selection(n_pads=(_abi.NUM_PADS + 1, None)))  # nothing passes
    configure_maps(ctx, other_labels=True, selected=True)
    none, passed, _, _ = clouds_to_maps(*csr(events), [2, 5], ctx)
    assert none == RunMaps() and not passed.any()
    # no event at all
    got, passed, records, _ = clouds_to_maps(np.zeros(1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64), [2, 5], ctx)
    assert got == RunMaps() and passed.shape == (0,) and records.shape == (0,)


# ---------------------------------------------------------------- 2. run_maps against delivered clouds ----
@pytest.mark.parametrize("min_electrons", [0, None, NEVER_KEPT], ids=["keep_all", "default", "none_kept"])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_run_maps_vs_restatement_of_own_cloud(ctx, name, min_electrons):
    inp, eng, fetched = _workload(name, ctx)
    n = WORKLOADS[name]
    eng.configure_summary(min_electrons=min_electrons)
    eng.configure_maps(other_labels=True)
    res = eng.run_maps(n, seed=SEED, first_event=FIRST)
    threshold = electrons_above_threshold(inp.config) if min_electrons is None else min_electrons
    maps, events = res["maps"], res["events"]
    cloud = (fetched["offsets"], fetched["points"], fetched["labels"], inp.indices, threshold)
    ref.assert_same_maps(maps, ref.maps_fast(*cloud), name)
    print(name, "min_electrons", threshold, "n_hit", maps.n_hit, "pads hit", int((maps.pad_events > 0).sum()),
          "largest pad_events", int(maps.pad_events.max()), "rows", int(maps.tb_rows.sum()))
    # ---- the invariants of the contract, against the returned records ----
    assert maps.n_events == n and res["passed"].all() and res["passed"].shape == (n,)
    assert int(maps.pad_events.sum()) == int(events["n_pads"].sum()) and int(maps.tb_rows.sum()) == int(events["n_kept"].sum())
    assert maps.n_hit == int((events["n_kept"] > 0).sum())
    assert (maps.tb_events <= maps.tb_rows).all() and (maps.pad_events <= n).all() and (maps.tb_events <= n).all()
    if min_electrons == 0:
        assert int(maps.pad_charge.sum()) == int(maps.tb_charge.sum()) == int(events["charge"].sum()) > 0
    if min_electrons == NEVER_KEPT:
        assert maps == RunMaps(n_events=n)
    else:
        assert maps.n_hit > 0
    # ---- the records, kinematics and statistics are those of run_summary ----
    summary = eng.run_summary(n, seed=SEED, first_event=FIRST)
    assert_same_records(events, summary["events"], f"{name} events")
    assert_same_records(res["tracks"], summary["tracks"], f"{name} tracks")
    for key in ("vertex", "p4", "status"):
        np.testing.assert_array_equal(res[key], fetched[key], err_msg=key)
    assert res["indices"] == list(inp.indices)
    assert {k: res["stats"][k] for k in STAT_KEYS} == {k: summary["stats"][k] for k in STAT_KEYS}
    if min_electrons is None:  # one plane per mask: the positions' planes add up to the plane of all of them in rows and charge
        planes = []
        for s in range(len(inp.indices)):
            eng.configure_maps(tracks=[s])
            planes.append(eng.run_maps(n, seed=SEED, first_event=FIRST)["maps"])
            ref.assert_same_maps(planes[-1], ref.maps_fast(*cloud, track_mask=1 << s), f"{name} position {s}")
        total = sum(planes)
        for field in ("pad_charge", "tb_rows", "tb_charge"):  # (every row carries the label of a simulated nucleus)
            np.testing.assert_array_equal(getattr(total, field), getattr(maps, field), err_msg=field)


# ---------------------------------------------------------------- 3. run_maps with a selection ----
def _two_class_range(values):
    values = np.sort(np.asarray(values))
    med = values[len(values) // 2].item()
    return (med, None) if values[0] < med else (None, med)


@pytest.mark.parametrize("cut", ["readme", "median_pads"])
def test_run_maps_of_the_selected_events(ctx, cut):
    inp, eng, fetched = _workload("o16aa", ctx)
    n = WORKLOADS["o16aa"]
    eng.configure_summary()
    if cut == "readme":
        cuts = dict(n_pads=(30, None), tracks=[0], track_end_rho2=(None, 0.0729))
    else:
        cuts = dict(n_pads=_two_class_range(eng.run_summary(n, seed=SEED, first_event=FIRST)["events"]["n_pads"]))
    eng.configure_selection(**cuts)
    eng.configure_maps(other_labels=True, selected=True)
    res = eng.run_maps(n, seed=SEED, first_event=FIRST)
    dry = eng.run_selected(n, seed=SEED, first_event=FIRST, fetch=False)
    passed = res["passed"]
    print(cut, cuts, "passed", int(passed.sum()), "of", n)
    np.testing.assert_array_equal(passed, dry["passed"])
    np.testing.assert_array_equal(passed, Selection(**cuts).passes(res["events"], res["tracks"]))
    if cut == "median_pads":
        assert 0 < passed.sum() < n  # both classes
    threshold = electrons_above_threshold(inp.config)
    ref.assert_same_maps(res["maps"], ref.maps_fast(fetched["offsets"], fetched["points"], fetched["labels"], inp.indices,
                                                    threshold, passed=passed), cut)
    assert res["maps"].n_events == int(passed.sum())
    assert_same_records(res["events"], dry["events"], "the records are of all events")
    assert {k: res["stats"][k] for k in STAT_KEYS} == {k: dry["stats"][k] for k in STAT_KEYS}


# ---------------------------------------------------------------- 4. invariance ----
def test_invariance_under_splits_chunks_builds_and_small_buffers(ctx):
    case = id_case("u32_wrap")  # the ids cross 2^32 inside the range
    first, seed, n = case.first_event - 150, case.seed, 200
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_summary()
    eng.configure_maps(other_labels=True)
    whole = eng.run_maps(n, seed=seed, first_event=first)
    assert whole["maps"].n_hit > 0 and whole["maps"].n_events == n
    # the same ids in three calls with uneven first_event: the maps add
    parts = [eng.run_maps(m, seed=seed, first_event=first + at)["maps"] for at, m in ((0, 37), (37, 101), (138, 62))]
    ref.assert_same_maps(sum(parts), whole["maps"], "three splits")
    ref.assert_same_maps(eng.run_maps(n, seed=seed, first_event=first)["maps"], whole["maps"], "the same call again")
    for options, kw in (({}, {"chunk_events": 7}), ({}, {"chunk_events": 1000}), ({"scatter_variant": 1}, {}),
                        ({"scatter_variant": 2}, {}), ({"scatter_variant": 3}, {}), ({"scatter_merge": 1}, {}),
                        ({"tiny_buffers": 1}, {})):
        other_ctx = _fresh(**options)
        other = _engine(inp, other_ctx, **kw)
        other.configure_summary()
        other.configure_maps(other_labels=True)
        res = other.run_maps(n, seed=seed, first_event=first)
        ref.assert_same_maps(res["maps"], whole["maps"], f"{options} {kw}")
        assert_same_records(res["events"], whole["events"], f"{options} {kw}")
        if options.get("tiny_buffers"):  # the chunks were scattered again: their maps count once
            assert res["stats"]["n_buffer_growths"] > 0
            again = other.run_maps(n, seed=seed, first_event=first)
            ref.assert_same_maps(again["maps"], whole["maps"], "tiny buffers, second call")
        other_ctx.close()


# ---------------------------------------------------------------- 5. mode handling ----
def test_not_configured_and_invalid():
    ctx = _fresh()
    lib = ctx.lib
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    maps, stats, records = RunMaps(), _abi.RunStats(), _abi.SummaryOut()
    out = maps.out()
    run = lambda: lib.attpc_sim_run_maps(ctx.handle, 1, 0, 4, eng.layout, None, None, None, records, None, out, stats)  # noqa: E731
    offsets = np.zeros(2, dtype=np.int64)
    cloud = lambda: lib.attpc_cloud_maps(ctx.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, eng.layout, None, None, out)  # noqa: E731
    assert run() == _abi.E_NOTCONFIGURED and cloud() == _abi.E_NOTCONFIGURED  # neither summary nor maps
    eng.configure_summary()
    assert run() == _abi.E_NOTCONFIGURED and cloud() == _abi.E_NOTCONFIGURED  # no maps
    for desc in (_abi.MapsDesc(0, 0), _abi.MapsDesc(1 << 9, 0), _abi.MapsDesc(0x3ff, 0), _abi.MapsDesc(1, 2)):
        assert lib.attpc_maps_configure(ctx.handle, desc) == _abi.E_INVALID
    assert run() == _abi.E_NOTCONFIGURED
    assert lib.attpc_maps_configure(ctx.handle, _abi.MapsDesc(FULL_MASK, 1)) == _abi.OK
    assert run() == _abi.E_NOTCONFIGURED and cloud() == _abi.E_NOTCONFIGURED  # selected, without a selection
    assert lib.attpc_maps_configure(ctx.handle, _abi.MapsDesc(FULL_MASK, 0)) == _abi.OK
    assert run() == _abi.OK and out.n_events == 4 and cloud() == _abi.OK and out.n_events == 1 and out.n_hit == 0
    assert lib.attpc_sim_run_maps(ctx.handle, 1, 0, 4, eng.layout, None, None, None, None, None, None, stats) == _abi.E_INVALID
    assert lib.attpc_maps_configure(ctx.handle, None) == _abi.OK
    assert run() == _abi.E_NOTCONFIGURED and cloud() == _abi.E_NOTCONFIGURED
    ctx.close()


def _canonical(offsets, rows, labels):
    """Rows in a canonical order per event (the order of a delivered cloud's rows within an event is unspecified)."""
    event = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort(tuple(rows[:, c] for c in range(rows.shape[1] - 1, -1, -1)) + (event,))
    return rows[order], labels[order]


def test_maps_runs_leave_nothing_behind():
    inp = Inputs("be10dp")
    n, seed, first = 96, 4, 10

    def outputs(maps_first):
        ctx = _fresh()
        eng = _engine(inp, ctx)
        eng.configure_summary()
        if maps_first:
            eng.run_maps(n, seed=seed, first_event=first)
            eng.configure_selection(n_pads=(10, None))
            eng.configure_maps(tracks=[0], selected=True)
            eng.run_maps(n // 2, seed=seed + 1, first_event=first + 7)
            configure_maps(ctx)  # attpc_maps_configure(NULL)
            configure_selection(ctx, Selection())
        summary = eng.run_summary(n, seed=seed, first_event=first)
        cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
        ctx.close()
        return summary, cloud

    (summary_a, cloud_a), (summary_b, cloud_b) = outputs(True), outputs(False)
    assert_same_records(summary_a["events"], summary_b["events"], "events")
    assert_same_records(summary_a["tracks"], summary_b["tracks"], "tracks")
    assert {k: summary_a["stats"][k] for k in STAT_KEYS} == {k: summary_b["stats"][k] for k in STAT_KEYS}
    np.testing.assert_array_equal(cloud_a["offsets"], cloud_b["offsets"])
    np.testing.assert_array_equal(cloud_a["event_points"], cloud_b["event_points"])
    for x, y in zip(_canonical(cloud_a["offsets"], cloud_a["points"], cloud_a["labels"]),
                    _canonical(cloud_b["offsets"], cloud_b["points"], cloud_b["labels"])):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------- 6. the file-driven path ----
@pytest.mark.parametrize("selected", [False, True], ids=["all", "selected"])
def test_file_driven_entry_point_equals_the_fused_run(ctx, selected):
    inp, eng, fetched = _workload("o16aa", ctx)
    n = 48
    p4, vertex = np.ascontiguousarray(fetched["p4"][:n]), np.ascontiguousarray(fetched["vertex"][:n])
    assert (fetched["status"][:n] == 0).all()  # (an event at the sample limit has no tracks in the fused run)
    settings = MapsSettings(other_labels=True, selected=selected)
    eng.configure_summary()
    n_pads = eng.run_summary(n, seed=SEED, first_event=FIRST)["events"]["n_pads"]
    selection = Selection(n_pads=_two_class_range(n_pads)) if selected else None
    got = simulate_batch_maps(p4, vertex, inp.z, inp.a, inp.config, SEED, inp.indices, maps=settings, selection=selection,
                              first_event=FIRST, ctx=ctx)
    if selected:
        eng.configure_selection(selection)
    eng.configure_maps(settings)
    fused = eng.run_maps(n, seed=SEED, first_event=FIRST)
    ref.assert_same_maps(got["maps"], fused["maps"], "file-driven against fused")
    np.testing.assert_array_equal(got["passed"], fused["passed"])
    assert_same_records(got["events"], fused["events"], "events")
    assert_same_records(got["tracks"], fused["tracks"], "tracks")
    assert got["maps"].n_hit > 0 and got["maps"].n_events == int(got["passed"].sum())
    assert got["passed"].all() if not selected else 0 < got["passed"].sum() < n
