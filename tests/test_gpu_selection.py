"""Selected delivery on the device, exactly (no tolerance anywhere): ``passed`` against the independent restatement of
the predicate (tests/selection_reference.py) on ``run_summary``'s records, the returned records against ``run_summary``'s
bit for bit, every passed event's rows against the same event's slice of the unselected delivered run, every rejected
event an empty range; invariance under splits, chunk sizes, scatter builds, transfer records and undersized buffers;
the capacity contract; the file-driven entry point; hand-made clouds through ``attpc_cloud_select``; the 8-nuclei
layout with a full mask; and the other outputs unchanged beside selected runs.  Needs a real MI355X: ``-m gpu``.

The cuts are taken from the run's own ``run_summary`` records (a median of ``n_pads`` for the event cut, a median of
``rho2_max`` on one masked position for the track cut), so that both classes are non-empty whenever the field takes
two values over the events; that is asserted, not assumed."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.selection import (Selection, clouds_to_selection, configure_selection,
                                                 simulate_batch_selected)
from attpc_engine_amd.detector.summary import configure_summary
from attpc_engine_amd.outputs import SelectedArrays
from tests.helpers import Inputs, chain8, id_case
from tests.selection_reference import passes, selection_of
from tests.summary_reference import assert_same_records, csr, hand_made_centers, hand_made_events

pytestmark = pytest.mark.gpu

WORKLOADS = {"be10dp": 300, "o16aa": 300, "b10chain": 40}  # events per workload (those of tests/test_gpu_summary.py)
SEED, FIRST = 5, 1000
KINDS = {"cloud": "points", "spyral": "rows"}
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
    """(inputs, an engine on the shared context, the unselected runs of the workload's events: cloud, spyral, summary)."""
    if name not in _cache:
        inp = Inputs(name)
        eng = _engine(inp, ctx)
        n = WORKLOADS[name]
        eng.configure_summary()
        _cache[name] = (inp, {"cloud": eng.run(n, seed=SEED, first_event=FIRST, fetch=True),
                              "spyral": eng.run_spyral(n, seed=SEED, first_event=FIRST),
                              "summary": eng.run_summary(n, seed=SEED, first_event=FIRST)})
    inp, base = _cache[name]
    eng = _engine(inp, ctx)
    eng.configure_summary()
    return inp, eng, base


def _two_class_range(values):
    """An inclusive range at a median of ``values`` that some events meet and some miss (asserted by the caller's
    check of both classes; possible whenever the field takes two values)."""
    values = np.sort(np.asarray(values))
    med = values[len(values) // 2].item()
    return (med, None) if values[0] < med else (None, med)


def _cuts(kind, summary):
    """The event cut or the track cut of the module's docstring, from a run's own records."""
    events, tracks = summary["events"], summary["tracks"]
    if kind == "event":
        return dict(n_pads=_two_class_range(events["n_pads"]))
    spread = [len(np.unique(tracks["rho2_max"][:, s])) for s in range(tracks.shape[1])]
    s = int(np.argmax(spread))  # the position whose rho2_max varies most
    return dict(track_mask=1 << s, min_tracks=1, track_rho2_max=_two_class_range(tracks["rho2_max"][:, s]))


def _canonical(offsets, rows, labels):
    """Rows in a canonical order per event (the order of a delivered cloud's rows within an event is unspecified)."""
    event = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    order = np.lexsort(tuple(rows[:, c] for c in range(rows.shape[1] - 1, -1, -1)) + (event,))
    return rows[order], labels[order]


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                  b.view(np.uint64) if b.dtype == np.float64 else b, err_msg=what)


def _check_against_unselected(res, base, key, want_passed, what):
    """``res`` (a selected run) against ``base`` (the unselected delivered run of the same events) and the mask."""
    passed = res["passed"]
    np.testing.assert_array_equal(passed, want_passed, err_msg=what + " passed")
    assert res["n_passed"] == int(passed.sum()) and res["n_rows"] == int(res["offsets"][-1]) == len(res[key]) == len(res["labels"])
    base_rows = np.diff(base["offsets"])
    np.testing.assert_array_equal(np.diff(res["offsets"]), np.where(passed, base_rows, 0), err_msg=what + " offsets")
    assert res["offsets"][0] == 0
    # the rows of the passed events, event by event, are the same event's slice of the unselected run
    keep = np.repeat(passed, base_rows)
    for got, ref in zip(_canonical(res["offsets"], res[key], res["labels"]),
                        _canonical(res["offsets"], base[key][keep], base["labels"][keep])):
        _same_bits(got, ref, what + " rows")
    np.testing.assert_array_equal(res["event_points"], base["event_points"], err_msg=what + " event_points")
    for name in ("vertex", "p4", "status"):
        if name in res:
            _same_bits(res[name], base[name], f"{what} {name}")


@pytest.mark.parametrize("cut", ["event", "track"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_run_selected_vs_restatement_and_unselected_run(ctx, name, kind, cut):
    inp, eng, base = _workload(name, ctx)
    n = WORKLOADS[name]
    summary = base["summary"]
    cuts = _cuts(cut, summary)
    want = passes(summary["events"], summary["tracks"], cuts)
    print(name, kind, cuts, "passed", int(want.sum()), "of", n)
    assert 0 < want.sum() < n, cuts  # both classes
    eng.configure_selection(selection_of(cuts))
    res = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind)
    _check_against_unselected(res, base[kind], KINDS[kind], want, f"{name} {kind} {cut}")
    np.testing.assert_array_equal(selection_of(cuts).passes(res["events"], res["tracks"]), want)
    assert_same_records(res["events"], summary["events"], f"{name} events")
    assert_same_records(res["tracks"], summary["tracks"], f"{name} tracks")
    assert res["indices"] == list(inp.indices)
    # the run statistics keep their cloud meaning over all events, in either kind
    assert {k: res["stats"][k] for k in STAT_KEYS} == {k: base["cloud"]["stats"][k] for k in STAT_KEYS}
    # what the selection would deliver, without delivering it
    dry = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind, fetch=False)
    assert dry[KINDS[kind]] is None and dry["labels"] is None and dry["n_rows"] == res["n_rows"]
    np.testing.assert_array_equal(dry["offsets"], res["offsets"])
    np.testing.assert_array_equal(dry["passed"], res["passed"])
    assert_same_records(dry["tracks"], summary["tracks"], f"{name} tracks, fetch=False")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_pass_all_and_pass_none(ctx, name, kind):
    inp, eng, base = _workload(name, ctx)
    n = WORKLOADS[name]
    key = KINDS[kind]
    eng.configure_selection(Selection())
    res = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind)
    assert res["passed"].all() and res["n_passed"] == n
    _check_against_unselected(res, base[kind], key, np.ones(n, dtype=bool), f"{name} {kind} all")
    np.testing.assert_array_equal(res["offsets"], base[kind]["offsets"])
    for got, ref in zip(_canonical(res["offsets"], res[key], res["labels"]),
                        _canonical(base[kind]["offsets"], base[kind][key], base[kind]["labels"])):
        _same_bits(got, ref, "every array of the unselected run")
    eng.configure_selection(n_pads=(_abi.NUM_PADS + 1, None))  # more pads than there are
    res = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind)
    assert not res["passed"].any() and res["n_passed"] == 0 and res["n_rows"] == 0
    assert len(res[key]) == 0 and len(res["labels"]) == 0 and (res["offsets"] == 0).all()
    np.testing.assert_array_equal(res["event_points"], base[kind]["event_points"])
    assert_same_records(res["events"], base["summary"]["events"], "pass none: events")


def _selected_both(eng, n, seed, first):
    return {kind: eng.run_selected(n, seed=seed, first_event=first, rows=kind) for kind in KINDS}


def _same_selected(got, ref, what):
    for kind, key in KINDS.items():
        a, b = got[kind], ref[kind]
        np.testing.assert_array_equal(a["passed"], b["passed"], err_msg=f"{what} {kind} passed")
        np.testing.assert_array_equal(a["offsets"], b["offsets"], err_msg=f"{what} {kind} offsets")
        np.testing.assert_array_equal(a["event_points"], b["event_points"], err_msg=f"{what} {kind} event_points")
        assert (a["n_passed"], a["n_rows"]) == (b["n_passed"], b["n_rows"]), (what, kind)
        assert_same_records(a["events"], b["events"], f"{what} {kind} events")
        assert_same_records(a["tracks"], b["tracks"], f"{what} {kind} tracks")
        for x, y in zip(_canonical(a["offsets"], a[key], a["labels"]), _canonical(b["offsets"], b[key], b["labels"])):
            _same_bits(x, y, f"{what} {kind} rows")
        assert {k: a["stats"][k] for k in STAT_KEYS} == {k: b["stats"][k] for k in STAT_KEYS}, (what, kind)


def test_invariance_under_splits_chunks_builds_records_and_small_buffers(ctx):
    case = id_case("u32_wrap")  # the ids cross 2^32 inside the range
    first, seed, n = case.first_event - 150, case.seed, 200
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    eng.configure_summary()
    summary = eng.run_summary(n, seed=seed, first_event=first)
    cuts = {**_cuts("event", summary), **_cuts("track", summary)}
    want = passes(summary["events"], summary["tracks"], cuts)
    assert 0 < want.sum() < n, cuts
    sel = selection_of(cuts)
    eng.configure_selection(sel)
    whole = _selected_both(eng, n, seed, first)
    np.testing.assert_array_equal(whole["cloud"]["passed"], want)
    # the same ids in three calls with uneven first_event
    parts = [_selected_both(eng, m, seed, first + at) for at, m in ((0, 37), (37, 101), (138, 62))]
    for kind, key in KINDS.items():
        np.testing.assert_array_equal(np.concatenate([p[kind]["passed"] for p in parts]), whole[kind]["passed"])
        assert_same_records(np.concatenate([p[kind]["tracks"] for p in parts]), whole[kind]["tracks"], "split tracks")
        assert sum(p[kind]["n_rows"] for p in parts) == whole[kind]["n_rows"]
        np.testing.assert_array_equal(np.concatenate([np.diff(p[kind]["offsets"]) for p in parts]), np.diff(whole[kind]["offsets"]))
        rows = np.concatenate([p[kind][key] for p in parts])
        labels = np.concatenate([p[kind]["labels"] for p in parts])
        for x, y in zip(_canonical(whole[kind]["offsets"], rows, labels),
                        _canonical(whole[kind]["offsets"], whole[kind][key], whole[kind]["labels"])):
            _same_bits(x, y, f"split {kind} rows")
    for options, kw in (({}, {"chunk_events": 7}), ({"deliver_chunk_events": 64}, {"chunk_events": 1000}),
                        ({"scatter_variant": 1}, {}), ({"scatter_variant": 2}, {}), ({"scatter_variant": 3}, {}),
                        ({"compact_transfer": 0}, {}), ({"compact_transfer": 1}, {}), ({"compact_transfer": 2, "deliver_chunk_events": 64}, {}),
                        ({"tiny_buffers": 1}, {}), ({"tiny_buffers": 1, "deliver_chunk_events": 64}, {})):
        other_ctx = _fresh(**options)
        other = _engine(inp, other_ctx, **kw)
        other.configure_summary()
        other.configure_selection(sel)
        res = _selected_both(other, n, seed, first)
        _same_selected(res, whole, f"{options} {kw}")
        if options.get("tiny_buffers"):  # the chunks were scattered, summarised and selected again
            assert res["cloud"]["stats"]["n_buffer_growths"] > 0
            _same_selected(_selected_both(other, n, seed, first), whole, "tiny buffers, second call")
        other_ctx.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_capacity_binds_the_selected_rows(ctx, kind):
    inp, eng, base = _workload("o16aa", ctx)
    n = WORKLOADS["o16aa"]
    cuts = _cuts("event", base["summary"])
    eng.configure_selection(selection_of(cuts))
    if kind == "spyral":
        eng.configure_spyral()
    full = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind)
    n_rows = full["n_rows"]
    unselected = int(base[kind]["offsets"][-1])
    assert 0 < n_rows < unselected  # a capacity of n_rows is below what the unselected run needs
    lib, width = ctx.lib, 3 if kind == "cloud" else 8

    def call(capacity):
        arrays, stats = SelectedArrays(n, capacity, width=width, n_sim=len(inp.indices)), _abi.RunStats()
        status = lib.attpc_sim_run_selected(ctx.handle, SEED, FIRST, n, eng.layout, None, None, None, arrays.out, stats)
        return status, arrays, stats

    status, arrays, stats = call(n_rows)
    assert status == _abi.OK and arrays.out.n_rows == n_rows and arrays.out.n_passed == full["n_passed"]
    for got, ref in zip(_canonical(arrays.offsets, *arrays.result()[1:]), _canonical(full["offsets"], full[KINDS[kind]], full["labels"])):
        _same_bits(got, ref, "capacity = n_rows")
    status, arrays, stats = call(n_rows - 1)
    assert status == _abi.E_CAPACITY and arrays.out.n_rows == n_rows
    assert stats.n_points == base["cloud"]["stats"]["n_points"] != n_rows  # (the cloud's rows of all events)
    np.testing.assert_array_equal(arrays.passed.astype(bool), full["passed"])
    with pytest.raises(BufferError):
        ctx.check(status, "attpc_sim_run_selected")
    # the run layer's one retry gets there from a capacity that is too small
    again = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind, capacity_per_event=1)
    assert again["n_rows"] == n_rows and len(again[KINDS[kind]]) == n_rows


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_file_driven_entry_point_equals_the_fused_run(ctx, name, kind):
    inp, eng, base = _workload(name, ctx)
    n = min(WORKLOADS[name], 48)
    fetched = base["cloud"]
    assert (fetched["status"][:n] == 0).all()  # (an event at the sample limit has no tracks in the fused run)
    p4, vertex = np.ascontiguousarray(fetched["p4"][:n]), np.ascontiguousarray(fetched["vertex"][:n])
    summary = {k: base["summary"][k][:n] for k in ("events", "tracks")}
    cuts = {**_cuts("event", summary), **_cuts("track", summary)}
    sel = selection_of(cuts)
    got = simulate_batch_selected(p4, vertex, inp.z, inp.a, inp.config, SEED, inp.indices, sel, kind=kind, first_event=FIRST, ctx=ctx)
    eng.configure_summary()
    eng.configure_selection(sel)
    fused = eng.run_selected(n, seed=SEED, first_event=FIRST, rows=kind)
    key = KINDS[kind]
    np.testing.assert_array_equal(got["passed"], passes(summary["events"], summary["tracks"], cuts))
    np.testing.assert_array_equal(got["passed"], fused["passed"])
    np.testing.assert_array_equal(got["offsets"], fused["offsets"])
    np.testing.assert_array_equal(got["event_points"], fused["event_points"])
    assert (got["n_passed"], got["n_rows"]) == (fused["n_passed"], fused["n_rows"])
    assert_same_records(got["events"], fused["events"], f"{name} events")
    assert_same_records(got["tracks"], fused["tracks"], f"{name} tracks")
    for x, y in zip(_canonical(got["offsets"], got[key], got["labels"]), _canonical(fused["offsets"], fused[key], fused["labels"])):
        _same_bits(x, y, f"{name} {kind} rows")


def test_cloud_select_on_hand_made_clouds(ctx):
    """The clouds of tests/summary_reference.py (pad centres (pad, 2 pad) mm, min_electrons 100, indices [2, 5, 2]):
    n_pads 2, 0, 2, 0, 3; spans 10, 0, 512, 0, 3; charges 1949, 99, 850, 0, 7000000201; rho2_max of position 0 (label 2)
    245, -1, 80, -1, 0; kept rows of position 0 / 1: 1 / 3, 0 / 0, 1 / 0, 0 / 0, 1 / 1.  The track part of the records is
    empty: n_samples 0, the end point NaN."""
    inp = Inputs("o16aa")
    centers = hand_made_centers()
    config = type("Geometry", (), {"pad_centers": centers, "elec_params": inp.config.elec_params})()
    ev, indices, min_electrons, _ = hand_made_events()
    offsets, points, labels = csr(ev)
    configure_summary(config, ctx, min_electrons)
    T, F = True, False
    for cuts, expected in ((dict(n_pads=(2, 2)), [T, F, T, F, F]), (dict(tb_span=(0, 0)), [F, T, F, T, F]),
                           (dict(tb_span=(10, 512)), [T, F, T, F, F]), (dict(charge=(99, 850)), [F, T, T, F, F]),
                           (dict(n_kept=(3, 3), charge=(None, 850)), [F, F, T, F, F]),
                           (dict(track_mask=1, min_tracks=1, track_rho2_max=(-1.0, 0.0)), [F, T, F, T, T]),  # -1.0 compares as -1.0
                           (dict(track_mask=1, min_tracks=1, track_rho2_max=(80.0, 245.0)), [T, F, T, F, F]),
                           (dict(track_mask=0b011, min_tracks=1, track_n_kept=(3, None)), [T, F, F, F, F]),
                           (dict(track_mask=0b011, min_tracks=2, track_n_kept=(1, None)), [T, F, F, F, T]),
                           (dict(track_mask=0b011, min_tracks=0, track_n_kept=(1000, None)), [T, T, T, T, T]),
                           (dict(track_mask=1, min_tracks=1), [T, T, T, T, T]),  # NaN end, no cut on it
                           (dict(track_mask=1, min_tracks=1, track_end_tb=(0.0, 512.0)), [F, F, F, F, F]),  # NaN end under a cut
                           (dict(track_mask=1, min_tracks=1, track_end_rho2=(0.0, None)), [F, F, F, F, F]),
                           (dict(track_mask=0b100, min_tracks=1, track_n_samples=(0, 0)), [T, T, T, T, T]),
                           (dict(), [T, T, T, T, T])):
        configure_selection(ctx, selection_of(cuts))
        passed, events, tracks = clouds_to_selection(offsets, points, labels, indices, ctx)
        assert passed.tolist() == expected, cuts
        assert passes(events, tracks, cuts).tolist() == expected, cuts
        assert np.isnan(tracks["end_x"]).all() and (tracks["n_samples"] == 0).all()
    # a mask bit at or above the call's n_sim
    configure_selection(ctx, Selection(tracks=[3], min_tracks=0))
    with pytest.raises(ValueError):
        clouds_to_selection(offsets, points, labels, indices, ctx)
    configure_selection(ctx, Selection())
    passed, _, _ = clouds_to_selection(np.zeros(1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64), indices, ctx)
    assert passed.shape == (0,)


def test_eight_nuclei_with_a_full_mask(ctx):
    """The n_sim = 8 layout of tests/test_gpu_layout_limits.py, every position masked."""
    inp = Inputs(chain8)
    eng = _engine(inp, ctx)
    n, seed, first = 48, 3, 77
    assert len(inp.indices) == _abi.MAX_SIM
    eng.configure_summary(min_electrons=0)
    summary = eng.run_summary(n, seed=seed, first_event=first)
    n_pads = summary["tracks"]["n_pads"]
    lo = int(np.sort(n_pads[n_pads > 0])[(n_pads > 0).sum() // 2])  # a median over the tracks that lit a pad
    counts = (n_pads >= lo).sum(axis=1)
    assert counts.min() < counts.max(), counts  # positions that meet the cut: not the same number in every event
    med = int(np.sort(counts)[n // 2])
    cuts = dict(track_mask=0xff, min_tracks=med if counts.min() < med else int(counts.max()), track_n_pads=(lo, None))
    want = passes(summary["events"], summary["tracks"], cuts)
    assert 0 < want.sum() < n, cuts
    eng.configure_selection(selection_of(cuts))
    for kind, key in KINDS.items():
        base = eng.run(n, seed=seed, first_event=first, fetch=True) if kind == "cloud" else eng.run_spyral(n, seed=seed, first_event=first)
        res = eng.run_selected(n, seed=seed, first_event=first, rows=kind)
        _check_against_unselected(res, base, key, want, f"chain8 {kind}")
        assert_same_records(res["tracks"], summary["tracks"], "chain8 tracks")
    # "all of them": 8 of 8
    eng.configure_selection(track_mask=0xff, track_n_samples=(1, None))
    res = eng.run_selected(n, seed=seed, first_event=first, fetch=False)
    np.testing.assert_array_equal(res["passed"], (summary["tracks"]["n_samples"] >= 1).all(axis=1))


def test_not_configured_and_invalid():
    import math

    ctx = _fresh()
    lib = ctx.lib
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    n_sim = len(inp.indices)
    centers = np.ascontiguousarray(inp.config.pad_centers, dtype=np.float64)
    summary_desc = _abi.SummaryDesc(0, _abi.dptr(centers), len(centers), 0)

    def call(kind="cloud"):
        arrays, stats = SelectedArrays(4, 1 << 16, width=3 if kind == "cloud" else 8, n_sim=n_sim), _abi.RunStats()
        return lib.attpc_sim_run_selected(ctx.handle, 1, 0, 4, eng.layout, None, None, None, arrays.out, stats)

    assert call() == _abi.E_NOTCONFIGURED  # neither
    assert lib.attpc_select_configure(ctx.handle, Selection().desc()) == _abi.OK
    assert call() == _abi.E_NOTCONFIGURED  # no summary configuration
    assert lib.attpc_summary_configure(ctx.handle, summary_desc) == _abi.OK
    assert call() == _abi.OK
    assert call("spyral") == _abi.E_NOTCONFIGURED  # the Spyral kind needs attpc_spyral_configure
    eng.configure_spyral()
    assert call("spyral") == _abi.OK
    assert lib.attpc_select_configure(ctx.handle, None) == _abi.OK  # off again; no other configuration was reset
    assert call() == _abi.E_NOTCONFIGURED
    offsets, passed = np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.uint8)
    cloud = lambda: lib.attpc_cloud_select(ctx.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, eng.layout,  # noqa: E731
                                           None, _abi.iptr(passed, _abi.C.c_uint8))
    assert cloud() == _abi.E_NOTCONFIGURED
    assert eng.run_summary(4, seed=1)["events"].shape == (4,) and eng.run_spyral(4, seed=1)["offsets"].shape == (5,)
    # descriptors the library refuses
    good = Selection(tracks=[0]).desc()
    for field, value in (("n_pads_lo", 5), ("charge_lo", 1 << 62), ("track_rho2_max_lo", math.nan), ("track_end_tb_hi", math.nan),
                         ("track_end_rho2_lo", math.inf), ("min_tracks", 2), ("track_mask", 1 << _abi.MAX_SIM),
                         ("track_n_samples_lo", 7)):
        bad = _abi.SelectDesc.from_buffer_copy(bytes(good))
        setattr(bad, field, value)
        if field in ("n_pads_lo", "track_n_samples_lo"):
            setattr(bad, field[:-2] + "hi", 4)
        if field == "charge_lo":
            bad.charge_hi = 0
        if field == "track_end_rho2_lo":
            bad.track_end_rho2_hi = 0.0
        assert lib.attpc_select_configure(ctx.handle, bad) == _abi.E_INVALID, field
    assert call() == _abi.E_NOTCONFIGURED  # a refused descriptor configures nothing
    # a mask bit at or above the call's n_sim comes from the run entry point
    assert lib.attpc_select_configure(ctx.handle, Selection(tracks=[n_sim], min_tracks=0).desc()) == _abi.OK
    assert call() == _abi.E_INVALID
    assert lib.attpc_select_configure(ctx.handle, good) == _abi.OK
    assert call() == _abi.OK and cloud() == _abi.OK
    ctx.close()


def test_selected_runs_leave_nothing_behind():
    """run, run_spyral, run_summary and run_traces on one context, before and after selected runs."""
    inp = Inputs("be10dp")
    n, seed, first = 96, 4, 10
    ctx = _fresh()
    eng = _engine(inp, ctx)

    def outputs():
        return (eng.run(n, seed=seed, first_event=first, fetch=True), eng.run_spyral(n, seed=seed, first_event=first),
                eng.run_summary(n, seed=seed, first_event=first), eng.run_traces(n, seed=seed, first_event=first),
                eng.run(n, seed=seed, first_event=first)["stats"])

    cloud_a, rows_a, summary_a, traces_a, resident_a = outputs()
    cuts = _cuts("event", summary_a)
    eng.configure_selection(selection_of(cuts))
    for kind in KINDS:
        res = eng.run_selected(n, seed=seed, first_event=first, rows=kind)
        assert 0 < res["n_passed"] < n
        eng.run_selected(n // 2, seed=seed + 1, first_event=first + 7, rows=kind, fetch=False)
    eng.configure_selection(n_pads=(_abi.NUM_PADS + 1, None))
    eng.run_selected(n, seed=seed, first_event=first)
    cloud_b, rows_b, summary_b, traces_b, resident_b = outputs()
    for a, b, key in ((cloud_a, cloud_b, "points"), (rows_a, rows_b, "rows")):
        np.testing.assert_array_equal(a["offsets"], b["offsets"])
        np.testing.assert_array_equal(a["event_points"], b["event_points"])
        for x, y in zip(_canonical(a["offsets"], a[key], a["labels"]), _canonical(b["offsets"], b[key], b["labels"])):
            _same_bits(x, y, key)
        assert {k: a["stats"][k] for k in STAT_KEYS} == {k: b["stats"][k] for k in STAT_KEYS}
    assert_same_records(summary_a["events"], summary_b["events"], "events")
    assert_same_records(summary_a["tracks"], summary_b["tracks"], "tracks")
    for key in ("offsets", "pads", "samples", "labels", "event_points"):
        np.testing.assert_array_equal(traces_a[key], traces_b[key], err_msg=key)
    assert traces_a["trace"] == traces_b["trace"]
    assert {k: resident_a[k] for k in STAT_KEYS} == {k: resident_b[k] for k in STAT_KEYS}
    ctx.close()
