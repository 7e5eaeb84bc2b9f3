"""The clustering on the device (``cluster_kernel``, csrc/cluster.hip) against its restatement
(tests/cluster_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The contract is integer arithmetic with every tie made definite (include/attpc_engine.h, "clustering"), so every
comparison here is exact: labels, event records and cluster records equal or not; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.clustering import CLUSTER_DTYPE, CLUSTER_EVENT_DTYPE, ClusterSettings, rows_to_clusters
from attpc_engine_amd.detector.correction import CorrectionSettings, rows_to_correction
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from attpc_engine_amd.detector.traces import PeakSettings, TriggerSettings
from tests import cluster_cases as cc
from tests import cluster_reference as cref
from tests import distortion_cases as dc
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu

C = _abi.C
ESTIMATES, THINNING, CIRCLE, HELIX = EstimateSettings(min_points=10), ThinSettings(5.0), CircleFitSettings(), HelixSlopeSettings()
PARTIAL = {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"}
SEED, FIRST, EVENTS = 23, (1 << 32) - 100, 256
CLUSTERING = ClusterSettings()  # the defaults: 20 mm, 20 mm, 5, 10, truth
GATE_MULTIPLICITY = 60
# (at the default peak threshold of 40 counts a noise of 5 makes no row: 20 counts with a prominence of 15 lets some 30 noise
#  rows into every event, with the truth label -1)
PEAKS = PeakSettings(prominence=15.0, threshold=20.0)


def _device(s: cref.Settings) -> ClusterSettings:
    return ClusterSettings(s.eps_xy, s.eps_z, s.min_samples, s.min_cluster_size, s.max_rows, s.match)


def _reference(s: ClusterSettings) -> cref.Settings:
    return cref.Settings(s.eps_xy, s.eps_z, s.min_samples, s.min_cluster_size, s.max_rows, s.match)


def _assert_same(got, want, what=""):
    labels, events, records = got
    assert labels.dtype == np.int64 and events.dtype == CLUSTER_EVENT_DTYPE and records.dtype == CLUSTER_DTYPE
    for name in cref.EVENT_DTYPE.names:
        differ = np.flatnonzero(np.asarray(events[name] != want[1][name]).reshape(len(events), -1).any(axis=1))
        assert differ.size == 0, (what, name, differ[:10], events[name][differ[:3]], want[1][name][differ[:3]])
    for name in cref.RECORD_DTYPE.names:
        differ = np.flatnonzero((records[name] != want[2][name]).any(axis=1))
        assert differ.size == 0, (what, name, differ[:10], records[name][differ[:3]], want[2][name][differ[:3]])
    differ = np.flatnonzero(labels != want[0])
    assert differ.size == 0, (what, differ[:10], labels[differ[:10]], want[0][differ[:10]])


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.close()


# 1 ------------------------------------------------------------------------------------------ the stage alone ----
def test_case_set_is_not_empty():
    cc.check_cases()


@pytest.mark.parametrize("group", list(cc.GROUPS))
def test_stage_alone_equals_the_restatement(ctx, group):
    offsets, rows, labels, names = cc.csr()
    got = rows_to_clusters(offsets, rows, labels, cc.INDICES, _device(cc.GROUPS[group]), ctx)
    _assert_same(got, cc.reference()[group], group)
    assert not (got[1]["status"] & cref.INTERNAL).any()


def test_order_and_chunking_do_not_matter(ctx):
    """The same events concatenated in another order, and each as a call of its own, give the same per-event results."""
    offsets, rows, labels, names = cc.csr()
    for group in ("base", "four"):
        s, want = _device(cc.GROUPS[group]), cc.reference()[group]
        order = np.random.default_rng(3).permutation(len(names))
        new_rows = np.concatenate([rows[offsets[e]:offsets[e + 1]] for e in order])
        new_labels = np.concatenate([labels[offsets[e]:offsets[e + 1]] for e in order])
        new_offsets = np.concatenate([[0], np.cumsum(np.diff(offsets)[order])]).astype(np.int64)
        got = rows_to_clusters(new_offsets, new_rows, new_labels, cc.INDICES, s, ctx)
        expect = (np.concatenate([want[0][offsets[e]:offsets[e + 1]] for e in order]), want[1][order], want[2][order])
        _assert_same(got, expect, (group, "shuffled"))
        for e, name in enumerate(names):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            one = np.array([0, hi - lo], dtype=np.int64)
            got = rows_to_clusters(one, rows[lo:hi], labels[lo:hi], cc.INDICES, s, ctx)
            _assert_same(got, (want[0][lo:hi], want[1][e:e + 1], want[2][e:e + 1]), (group, name))
    # a window of the array (offsets[0] > 0: the rows in front belong to no event and get -1)
    window = offsets[9:]
    got = rows_to_clusters(window, rows, labels, cc.INDICES, _device(cc.GROUPS["base"]), ctx)
    want = cc.reference()["base"]
    expect = want[0].copy()
    expect[:window[0]] = -1
    _assert_same(got, (expect, want[1][9:], want[2][9:]), "window")


def test_stage_alone_arguments(ctx):
    offsets, rows, labels, names = cc.csr()
    base = cc.GROUPS["base"]
    # without truth labels nobody votes; other layouts: a label given twice, a negative index, eight positions, none
    for s in (cc.GROUPS["rank"], base):
        _assert_same(rows_to_clusters(offsets, rows, None, cc.INDICES, _device(s), ctx), cref.cluster(s, offsets, rows, None, cc.INDICES), "no labels")
    for indices in ((2, 2, 0), (0, 1, 2, 3, 4, 5, 6, 7), ()):
        for s in (base, cc.GROUPS["rank"]):
            _assert_same(rows_to_clusters(offsets, rows, labels, indices, _device(s), ctx), cref.cluster(s, offsets, rows, labels, indices), indices)
    layout = _abi.EventLayout()
    layout.n_rows, layout.n_sim = 4, 3
    layout.indices[0], layout.indices[1], layout.indices[2] = -1, 2, 0
    _assert_same(rows_to_clusters(offsets, rows, labels, layout, _device(base), ctx), cref.cluster(base, offsets, rows, labels, (-1, 2, 0)), "negative index")
    empty = rows_to_clusters([0], np.zeros((0, 8)), [], cc.INDICES, _device(base), ctx)
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and empty[2].shape == (0, 8)
    # rows out of z order are refused, by the host
    swapped = rows.copy()
    lo = offsets[names.index("line of 255")]
    swapped[[lo + 3, lo + 4]] = swapped[[lo + 4, lo + 3]]
    with pytest.raises(ValueError, match="nondecreasing z"):
        rows_to_clusters(offsets, swapped, labels, cc.INDICES, _device(base), ctx)
    # what the library refuses
    i64 = C.c_int64
    out = np.empty(len(rows), dtype=np.int64)
    from attpc_engine_amd.detector.estimate import _layout
    good = _device(base)
    for field, value in (("eps_xy", 0.0), ("eps_xy", 65.0), ("eps_xy", float("nan")), ("eps_z", 0.01), ("eps_z", float("inf")),
                         ("min_samples", 0), ("min_cluster_size", 0), ("max_rows", 0), ("max_rows", 65536), ("match", 2)):
        desc = good.desc()
        setattr(desc, field, value)
        args = (ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64), _layout(cc.INDICES), desc,
                _abi.iptr(out, i64), None, None)
        assert ctx.lib.attpc_rows_cluster(*args) == _abi.E_INVALID, (field, value)
        assert ctx.lib.attpc_trace_configure_clustering(ctx.handle, desc) == _abi.E_INVALID, (field, value)
    desc = good.desc()
    desc.reserved[1] = 1
    assert ctx.lib.attpc_trace_configure_clustering(ctx.handle, desc) == _abi.E_INVALID
    bad_layout = _layout(cc.INDICES)
    bad_layout.n_sim = 9
    assert ctx.lib.attpc_rows_cluster(ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64), bad_layout,
                                      good.desc(), _abi.iptr(out, i64), None, None) == _abi.E_INVALID
    # labels alone: events and records may be NULL
    ctx.check(ctx.lib.attpc_rows_cluster(ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64),
                                         _layout(cc.INDICES), good.desc(), _abi.iptr(out, i64), None, None), "attpc_rows_cluster")
    assert np.array_equal(out, cc.reference()["base"][0])


# 2 ------------------------------------------------------------------------------------------ in the run ----
def _stages(eng, on: bool):
    eng.configure_thinning(THINNING if on else None)
    eng.configure_circle_fit(CIRCLE if on else None)
    eng.configure_helix_slope(HELIX if on else None)


@pytest.fixture(scope="module")
def run(ctx):
    """A few hundred events of o16aa in partial readout with noise: the run with the stage off, with it on, and the
    restatement on the delivered rows and truth labels.  Read-only."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    inp = Inputs("o16aa")
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), **PARTIAL)
    eng.configure_peaks(PEAKS)
    eng.configure_estimates(ESTIMATES)
    _stages(eng, False)
    eng.configure_clustering()
    off = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    eng.configure_clustering(CLUSTERING)
    on = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    eng.configure_clustering()
    want = cref.cluster(_reference(CLUSTERING), off["offsets"], off["rows"], off["labels"], [int(i) for i in inp.indices])
    return inp, eng, off, on, want


def test_run_delivers_what_the_stage_off_run_delivers(run, ctx):
    inp, eng, off, on, want = run
    per_event = np.diff(off["offsets"])
    print("events", EVENTS, "rows", len(off["rows"]), "largest event", int(per_event.max()), "noise rows", int((off["labels"] < 0).sum()))
    assert "clusters" not in off and "cluster_labels" not in off and len(off["rows"]) > 10000 and (off["labels"] < 0).sum() > 1000
    for key in ("offsets", "rows", "labels", "event_points", "p4", "vertex", "status"):
        assert on[key].tobytes() == off[key].tobytes(), key
    assert on["trace_rows"] == off["trace_rows"] and on["stats"]["key_checksum"] == off["stats"]["key_checksum"]
    events = np.zeros(1, dtype=CLUSTER_EVENT_DTYPE)
    labels = np.zeros(1, dtype=np.int64)
    eng.run_trace_rows(2, seed=SEED, first_event=FIRST)  # a stage-off call
    assert ctx.lib.attpc_clusters_last(ctx.handle, 0, 1, _abi.iptr(events, _abi.ClusterEvent), None) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_cluster_labels_last(ctx.handle, 0, 1, _abi.iptr(labels, C.c_int64)) == _abi.E_NOTCONFIGURED


def test_run_equals_the_restatement(run):
    inp, eng, off, on, want = run
    _assert_same((on["cluster_labels"], *on["clusters"]), want, "run")
    events, records = on["clusters"]
    # the comparison is not empty: noise rows are rejected, and events have two surviving clusters and more
    noise = off["labels"] < 0
    print("noise rows", int(noise.sum()), "rejected", int((on["cluster_labels"][noise] == -1).sum()))
    assert (on["cluster_labels"][noise] == -1).sum() > 0.9 * noise.sum() and (events["n_noise"] > 0).sum() > EVENTS // 2
    assert (events["n_clusters"] >= 2).sum() > EVENTS // 4 and (records["label"][:, 1] >= 0).sum() > EVENTS // 8
    assert not events["status"].any() and events["n_rows"].sum() == len(off["rows"])
    print("clusters per event", np.bincount(events["n_clusters"]), "split", int((events["n_split"] > 0).sum()),
          "fake", int((events["n_fake"] > 0).sum()), "small", int((events["n_small"] > 0).sum()))


def test_run_estimates_are_those_of_the_cluster_labels(run, ctx):
    inp, eng, off, on, want = run
    got = rows_to_estimates(on["offsets"], on["rows"], on["cluster_labels"], inp.indices, ESTIMATES, ctx, config=inp.config)
    assert on["estimates"].tobytes() == got.tobytes()
    assert on["estimates"].tobytes() != off["estimates"].tobytes() and (on["estimates"]["n_fit"] > 0).sum() > EVENTS // 2


def test_run_composes_with_correction_and_thinning(run, ctx):
    """With the drift correction and the thinning (circle fit and helix slope too) on, the records equal those of the
    stage-alone calls chained: correction of the stage-off rows, clustering of those, thinning and estimates of the
    cluster labels."""
    inp, eng, off, on, want = run
    named = dc.named_map()
    correction = CorrectionSettings(named)
    eng.configure_correction(correction)
    eng.configure_clustering(CLUSTERING)
    _stages(eng, True)
    try:
        res = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    finally:
        _stages(eng, False)
        eng.configure_clustering()
        eng.configure_correction()
    rows, labels, _, counts = rows_to_correction(off["offsets"], off["rows"], off["labels"], correction, inp.config, ctx)
    assert res["rows"].tobytes() == rows.tobytes() and np.array_equal(res["labels"], labels) and res["correction"] == counts
    alone = rows_to_clusters(off["offsets"], rows, labels, inp.indices, CLUSTERING, ctx)
    _assert_same((res["cluster_labels"], *res["clusters"]), cref.cluster(_reference(CLUSTERING), off["offsets"], rows, labels,
                                                                          [int(i) for i in inp.indices]), "corrected")
    _assert_same(alone, (res["cluster_labels"], *res["clusters"]), "stage alone")
    point_offsets, points, point_labels, info = rows_to_points(off["offsets"], rows, alone[0], inp.indices, THINNING, ctx)
    records = rows_to_estimates(point_offsets, points, point_labels, inp.indices, ESTIMATES, ctx, config=inp.config, circle=CIRCLE, helix=HELIX)
    records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    assert res["estimates"].tobytes() == records.tobytes() and (records["n_fit"] > 0).sum() > EVENTS // 2


def test_resident_runs_and_chunks_give_the_same(run, ctx):
    inp, eng, off, on, want = run
    eng.configure_clustering(CLUSTERING)
    try:
        resident = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST, fetch=False)
        alone = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        for other in (resident, alone):
            assert "cluster_labels" not in other and "rows" not in other
            assert all(a.tobytes() == b.tobytes() for a, b in zip(other["clusters"], on["clusters"]))
            assert other["estimates"].tobytes() == on["estimates"].tobytes() and other["trace_rows"] == on["trace_rows"]
        labels = np.zeros(1, dtype=np.int64)  # the rows were not fetched: no labels to give
        assert ctx.lib.attpc_cluster_labels_last(ctx.handle, 0, 1, _abi.iptr(labels, C.c_int64)) == _abi.E_NOTCONFIGURED
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 1), "attpc_set_chunk_events")  # every event a chunk of its own
        try:
            n = 48
            chunked = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
            chunked_resident = eng.run_estimates(n, seed=SEED, first_event=FIRST)
        finally:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        rows = int(on["offsets"][n])
        assert np.array_equal(chunked["cluster_labels"], on["cluster_labels"][:rows]) and chunked["rows"].tobytes() == on["rows"][:rows].tobytes()
        for other in (chunked, chunked_resident):
            assert all(a.tobytes() == b[:n].tobytes() for a, b in zip(other["clusters"], on["clusters"]))
            assert other["estimates"].tobytes() == on["estimates"][:n].tobytes()
        # a call whose capacity was too small is repeated: the same records and labels
        small = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST, capacity_per_event=1)
        assert np.array_equal(small["cluster_labels"], on["cluster_labels"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(small["clusters"], on["clusters"]))
        # the ranges of the two readers
        events = np.zeros(4, dtype=CLUSTER_EVENT_DTYPE)
        ctx.check(ctx.lib.attpc_clusters_last(ctx.handle, EVENTS - 4, 4, _abi.iptr(events, _abi.ClusterEvent), None), "attpc_clusters_last")
        assert events.tobytes() == on["clusters"][0][-4:].tobytes()
        assert ctx.lib.attpc_clusters_last(ctx.handle, EVENTS - 3, 4, _abi.iptr(events, _abi.ClusterEvent), None) == _abi.E_INVALID
        total = len(on["rows"])
        ctx.check(ctx.lib.attpc_cluster_labels_last(ctx.handle, total - 1, 1, _abi.iptr(labels, C.c_int64)), "attpc_cluster_labels_last")
        assert labels[0] == on["cluster_labels"][-1]
        assert ctx.lib.attpc_cluster_labels_last(ctx.handle, total, 1, _abi.iptr(labels, C.c_int64)) == _abi.E_INVALID
    finally:
        eng.configure_clustering()


def test_rank_mode_and_track_fit_run(run, ctx):
    """The label-free mode in the run equals the restatement; with the track fit on, the fits are those of the stage
    alone on the cluster labels."""
    from attpc_engine_amd.detector.fit import TrackFitSettings, rows_to_fit

    inp, eng, off, on, want = run
    rank = ClusterSettings(match="rank")
    fit = TrackFitSettings(max_evaluations=2)
    n = 32
    eng.configure_clustering(rank)
    eng.configure_track_fit(fit)
    try:
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    finally:
        eng.configure_track_fit()
        eng.configure_clustering()
    rows = int(off["offsets"][n])
    expect = cref.cluster(_reference(rank), off["offsets"][:n + 1], off["rows"][:rows], off["labels"][:rows], [int(i) for i in inp.indices])
    _assert_same((res["cluster_labels"], *res["clusters"]), expect, "rank")
    assert not np.array_equal(res["cluster_labels"], on["cluster_labels"][:rows])
    estimates = rows_to_estimates(res["offsets"], res["rows"], res["cluster_labels"], inp.indices, ESTIMATES, ctx, config=inp.config)
    assert res["estimates"].tobytes() == estimates.tobytes()
    fits = rows_to_fit(res["offsets"], res["rows"], res["cluster_labels"], eng.layout, estimates, ctx, fit, estimate_settings=ESTIMATES.for_field(
        float(inp.config.det_params.bfield)))
    assert res["fits"].tobytes() == fits.tobytes() and (fits["evaluations"] > 0).sum() > n // 2


def test_behind_a_trigger_gate(run, ctx):
    """An event that did not fire has no rows and a record of zeros."""
    inp, eng, off, on, want = run
    n = 64
    eng.configure_clustering(CLUSTERING)
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=GATE_MULTIPLICITY, gate=True))
    try:
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    finally:
        eng.configure_trigger()
        eng.configure_clustering()
    fired = res["trigger"]["fired"] != 0
    events, records = res["clusters"]
    print("fired", int(fired.sum()), "of", n)
    assert 0 < fired.sum() < n and np.all(np.diff(res["offsets"])[~fired] == 0)
    zero = np.zeros(1, dtype=CLUSTER_EVENT_DTYPE)[0]
    assert all(events[e] == zero for e in np.flatnonzero(~fired))
    assert np.all(records["first_row"][~fired] == -1) and not any(records[name][~fired].any() for name in CLUSTER_DTYPE.names if name != "first_row")
    expect = cref.cluster(_reference(CLUSTERING), res["offsets"], res["rows"], res["labels"], [int(i) for i in inp.indices])
    _assert_same((res["cluster_labels"], events, records), expect, "gated")
    assert (events["n_clusters"][fired] > 0).any()
