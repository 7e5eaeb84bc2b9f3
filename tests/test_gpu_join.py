"""The cluster joining on the device (``cluster_join_kernel``, csrc/cluster_join.hip) against its restatement
(tests/join_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The contract has every tie made definite and every f64 operation written down (include/attpc_engine.h, "cluster
joining"), so every comparison here is exact: labels, cluster events and records, join events and records equal or
not -- the f64 fields byte for byte, NaN slots included; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.circle import CircleFitSettings
from attpc_engine_amd.detector.clustering import CLUSTER_DTYPE, CLUSTER_EVENT_DTYPE, ClusterSettings, cluster_scores, rows_to_clusters
from attpc_engine_amd.detector.correction import CorrectionSettings, rows_to_correction
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.helix import HelixSlopeSettings
from attpc_engine_amd.detector.joining import JOIN_DTYPE, JOIN_EVENT_DTYPE, JoinSettings, rows_to_joined_clusters
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from attpc_engine_amd.detector.traces import PeakSettings, TriggerSettings
from tests import cluster_reference as cref
from tests import distortion_cases as dc
from tests import join_cases as jc
from tests import join_reference as jref
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu

C = _abi.C
ESTIMATES, THINNING, CIRCLE, HELIX = EstimateSettings(min_points=10), ThinSettings(5.0), CircleFitSettings(), HelixSlopeSettings()
PARTIAL = {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"}  # as tests/test_gpu_cluster.py
SEED, FIRST, EVENTS = 23, (1 << 32) - 100, 128
CLUSTERING = ClusterSettings()
JOIN = JoinSettings()
GATE_MULTIPLICITY = 60
PEAKS = PeakSettings(prominence=15.0, threshold=20.0)


def _device(s: cref.Settings) -> ClusterSettings:
    return ClusterSettings(s.eps_xy, s.eps_z, s.min_samples, s.min_cluster_size, s.max_rows, s.match)


def _device_join(j: jref.JoinSettings) -> JoinSettings:
    return JoinSettings(j.overlap_ratio, j.min_radius, j.radius_ratio or None, j.max_clusters)


def _reference(s: ClusterSettings) -> cref.Settings:
    return cref.Settings(s.eps_xy, s.eps_z, s.min_samples, s.min_cluster_size, s.max_rows, s.match)


def _reference_join(j: JoinSettings) -> jref.JoinSettings:
    return jref.JoinSettings(j.overlap_ratio, j.min_radius, j.radius_ratio or 0.0, j.max_clusters)


def _assert_same(got, want, what=""):
    labels, events, records, jevents, jrecords = got
    assert labels.dtype == np.int64 and events.dtype == CLUSTER_EVENT_DTYPE and records.dtype == CLUSTER_DTYPE
    assert jevents.dtype == JOIN_EVENT_DTYPE and jrecords.dtype == JOIN_DTYPE
    for mine, theirs in ((events, want[1]), (records, want[2]), (jevents, want[3]), (jrecords, want[4])):
        for name in theirs.dtype.names:
            a = np.ascontiguousarray(mine[name]).reshape(len(mine), -1)
            b = np.ascontiguousarray(theirs[name]).astype(a.dtype).reshape(len(mine), -1)
            differ = np.flatnonzero((a.view(np.uint8).reshape(len(mine), -1) != b.view(np.uint8).reshape(len(mine), -1)).any(axis=1))
            assert differ.size == 0, (what, name, differ[:10], a[differ[:3]], b[differ[:3]])
            assert a.tobytes() == b.tobytes(), (what, name)
    differ = np.flatnonzero(labels != want[0])
    assert differ.size == 0, (what, differ[:10], labels[differ[:10]], want[0][differ[:10]])


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.close()


# 1 ------------------------------------------------------------------------------------------ the stages alone ----
def test_case_set_is_not_empty():
    jc.check_cases()


@pytest.mark.parametrize("run_name", list(jc.RUNS))
def test_stages_alone_equal_the_restatement(ctx, run_name):
    offsets, rows, labels, names = jc.csr()
    s, j = jc.RUNS[run_name]
    got = rows_to_joined_clusters(offsets, rows, labels, jc.INDICES, _device(s), _device_join(j), ctx)
    _assert_same(got, jc.reference()[run_name], run_name)
    assert not (got[1]["status"] & cref.INTERNAL).any()
    # the clustering alone is what it was
    alone = rows_to_clusters(offsets, rows, labels, jc.INDICES, _device(s), ctx)
    want = jc.clustering_alone()[s.match]
    assert np.array_equal(alone[0], want[0]) and all(np.array_equal(alone[1][f], want[1][f]) for f in cref.EVENT_DTYPE.names)


def test_order_and_chunking_do_not_matter(ctx):
    """The same events in another order, and each as a call of its own, give the same per-event results."""
    offsets, rows, labels, names = jc.csr()
    for run_name in ("defaults", "quarter"):
        s, j = jc.RUNS[run_name]
        want = jc.reference()[run_name]
        order = np.random.default_rng(3).permutation(len(names))
        new_rows = np.concatenate([rows[offsets[e]:offsets[e + 1]] for e in order])
        new_labels = np.concatenate([labels[offsets[e]:offsets[e + 1]] for e in order])
        new_offsets = np.concatenate([[0], np.cumsum(np.diff(offsets)[order])]).astype(np.int64)
        got = rows_to_joined_clusters(new_offsets, new_rows, new_labels, jc.INDICES, _device(s), _device_join(j), ctx)
        expect = (np.concatenate([want[0][offsets[e]:offsets[e + 1]] for e in order]), *(w[order] for w in want[1:]))
        _assert_same(got, expect, (run_name, "shuffled"))
        for e, name in enumerate(names):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            one = np.array([0, hi - lo], dtype=np.int64)
            got = rows_to_joined_clusters(one, rows[lo:hi], labels[lo:hi], jc.INDICES, _device(s), _device_join(j), ctx)
            _assert_same(got, (want[0][lo:hi], *(w[e:e + 1] for w in want[1:])), (run_name, name))


def test_library_refusals(ctx):
    from attpc_engine_amd.detector.estimate import _layout

    offsets, rows, labels, names = jc.csr()
    i64 = C.c_int64
    out = np.empty(len(rows), dtype=np.int64)
    cluster_desc = _device(jc.CLUSTERING).desc()
    nan, inf = float("nan"), float("inf")
    for field, value in (("overlap_ratio", 0.0), ("overlap_ratio", 1.5), ("overlap_ratio", -1.0), ("overlap_ratio", nan),
                         ("min_radius", 0.0), ("min_radius", 0.06), ("min_radius", 5001.0), ("min_radius", nan),
                         ("radius_ratio", 0.5), ("radius_ratio", -2.0), ("radius_ratio", nan), ("radius_ratio", inf),
                         ("max_clusters", 1), ("max_clusters", 65), ("max_clusters", -1)):
        desc = JOIN.desc()
        setattr(desc, field, value)
        args = (ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64), _layout(jc.INDICES), cluster_desc,
                desc, _abi.iptr(out, i64), None, None, None, None)
        assert ctx.lib.attpc_rows_cluster_join(*args) == _abi.E_INVALID, (field, value)
        assert ctx.lib.attpc_trace_configure_cluster_join(ctx.handle, desc) == _abi.E_INVALID, (field, value)
    desc = JOIN.desc()
    desc.reserved[2] = 1
    assert ctx.lib.attpc_trace_configure_cluster_join(ctx.handle, desc) == _abi.E_INVALID
    assert ctx.lib.attpc_rows_cluster_join(ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64),
                                           _layout(jc.INDICES), cluster_desc, None, _abi.iptr(out, i64), None, None, None, None) == _abi.E_INVALID
    # labels alone: the four kinds of records may be NULL
    ctx.check(ctx.lib.attpc_rows_cluster_join(ctx.handle, len(names), _abi.iptr(offsets, i64), _abi.dptr(rows), _abi.iptr(labels, i64),
                                              _layout(jc.INDICES), cluster_desc, JOIN.desc(), _abi.iptr(out, i64), None, None, None, None),
              "attpc_rows_cluster_join")
    assert np.array_equal(out, jc.reference()["defaults"][0])


# 2 ------------------------------------------------------------------------------------------ in the run ----
def _stages(eng, on: bool):
    eng.configure_thinning(THINNING if on else None)
    eng.configure_circle_fit(CIRCLE if on else None)
    eng.configure_helix_slope(HELIX if on else None)


def _joined_reference(clustering, join, offsets, rows, labels, indices):
    return jref.join(_reference(clustering), _reference_join(join), offsets, rows, labels, [int(i) for i in indices])


@pytest.fixture(scope="module")
def run(ctx):
    """128 events of o16aa in partial readout with noise: the run with the clustering alone, with the joining on, and
    the restatements on the delivered rows and truth labels.  If the restatement joins nothing at the default
    overlap_ratio, the joining runs at 0.1 (see profiles/r32_cluster_join.md).  Read-only."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    inp = Inputs("o16aa")
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), **PARTIAL)
    eng.configure_peaks(PEAKS)
    eng.configure_estimates(ESTIMATES)
    _stages(eng, False)
    eng.configure_clustering(CLUSTERING)
    eng.configure_cluster_join()
    off = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    join = JOIN
    want = _joined_reference(CLUSTERING, join, off["offsets"], off["rows"], off["labels"], inp.indices)
    if want[3]["n_joined"].sum() == 0:
        join = JoinSettings(overlap_ratio=0.1)
        want = _joined_reference(CLUSTERING, join, off["offsets"], off["rows"], off["labels"], inp.indices)
    eng.configure_cluster_join(join)
    on = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    eng.configure_cluster_join()
    eng.configure_clustering()
    alone = cref.cluster(_reference(CLUSTERING), off["offsets"], off["rows"], off["labels"], [int(i) for i in inp.indices])
    return inp, eng, off, on, want, alone, join


def test_joining_off_is_the_clustering_alone(run, ctx):
    inp, eng, off, on, want, alone, join = run
    assert "joins" not in off and "clusters" in off and len(off["rows"]) > 5000
    assert np.array_equal(off["cluster_labels"], alone[0])
    for got, expect in zip(off["clusters"], alone[1:]):
        assert all(np.array_equal(got[name], expect[name]) for name in expect.dtype.names)
    for key in ("offsets", "rows", "labels", "event_points", "p4", "vertex", "status"):
        assert on[key].tobytes() == off[key].tobytes(), key
    assert on["trace_rows"] == off["trace_rows"] and on["stats"]["key_checksum"] == off["stats"]["key_checksum"]
    # attpc_joins_last after a stage-off call, and with the joining configured without the clustering
    jevents = np.zeros(1, dtype=JOIN_EVENT_DTYPE)
    eng.configure_clustering(CLUSTERING)
    try:
        eng.run_trace_rows(2, seed=SEED, first_event=FIRST)  # the joining is off
        assert ctx.lib.attpc_joins_last(ctx.handle, 0, 1, _abi.iptr(jevents, _abi.JoinEvent), None) == _abi.E_NOTCONFIGURED
        eng.configure_clustering()
        eng.configure_cluster_join(join)
        res = eng.run_trace_rows(2, seed=SEED, first_event=FIRST)  # the joining is on, the clustering is not
        assert "joins" not in res and "clusters" not in res
        assert ctx.lib.attpc_joins_last(ctx.handle, 0, 1, _abi.iptr(jevents, _abi.JoinEvent), None) == _abi.E_NOTCONFIGURED
    finally:
        eng.configure_cluster_join()
        eng.configure_clustering()


def test_run_equals_the_restatement(run):
    inp, eng, off, on, want, alone, join = run
    _assert_same((on["cluster_labels"], *on["clusters"], *on["joins"]), want, "run")
    # the comparison is not empty, by the restatement's own counts
    fewer_split = int((want[1]["n_split"] < alone[1]["n_split"]).sum())
    print("overlap_ratio", join.overlap_ratio, "n_joined", int(want[3]["n_joined"].sum()), "events joined", int((want[3]["n_joined"] > 0).sum()),
          "n_split", int(alone[1]["n_split"].sum()), "->", int(want[1]["n_split"].sum()), "events whose n_split falls", fewer_split,
          "capped", int((want[3]["status"] == jref.JOIN_CAPPED).sum()))
    assert want[3]["n_joined"].sum() > 0 and fewer_split >= 1
    assert not on["clusters"][0]["status"].any() and not (on["joins"][0]["status"] & jref.JOIN_NOT_CLUSTERED).any()
    completeness, purity = cluster_scores(*on["clusters"])  # works unchanged on joined records
    assert np.isfinite(completeness).any() and np.nanmax(purity) <= 1.0


def test_run_estimates_are_those_of_the_joined_labels(run, ctx):
    inp, eng, off, on, want, alone, join = run
    got = rows_to_estimates(on["offsets"], on["rows"], on["cluster_labels"], inp.indices, ESTIMATES, ctx, config=inp.config)
    assert on["estimates"].tobytes() == got.tobytes()
    assert on["estimates"].tobytes() != off["estimates"].tobytes() and (on["estimates"]["n_fit"] > 0).sum() > EVENTS // 2


def test_resident_runs_and_chunks_give_the_same(run, ctx):
    inp, eng, off, on, want, alone, join = run
    eng.configure_clustering(CLUSTERING)
    eng.configure_cluster_join(join)
    try:
        resident = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST, fetch=False)
        estimated = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        for other in (resident, estimated):
            assert "cluster_labels" not in other and "rows" not in other
            assert all(a.tobytes() == b.tobytes() for a, b in zip(other["clusters"] + other["joins"], on["clusters"] + on["joins"]))
            assert other["estimates"].tobytes() == on["estimates"].tobytes() and other["trace_rows"] == on["trace_rows"]
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 1), "attpc_set_chunk_events")  # every event a chunk of its own
        try:
            n = 48
            chunked = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
            chunked_resident = eng.run_estimates(n, seed=SEED, first_event=FIRST)
        finally:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
        rows = int(on["offsets"][n])
        assert np.array_equal(chunked["cluster_labels"], on["cluster_labels"][:rows])
        for other in (chunked, chunked_resident):
            assert all(a.tobytes() == b[:n].tobytes() for a, b in zip(other["clusters"] + other["joins"], on["clusters"] + on["joins"]))
            assert other["estimates"].tobytes() == on["estimates"][:n].tobytes()
        # a call whose capacity was too small is repeated: the same records and labels
        small = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST, capacity_per_event=1)
        assert np.array_equal(small["cluster_labels"], on["cluster_labels"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(small["clusters"] + small["joins"], on["clusters"] + on["joins"]))
        # the range of the reader
        jevents = np.zeros(4, dtype=JOIN_EVENT_DTYPE)
        jrecords = np.zeros((4, 8), dtype=JOIN_DTYPE)
        ctx.check(ctx.lib.attpc_joins_last(ctx.handle, EVENTS - 4, 4, _abi.iptr(jevents, _abi.JoinEvent), _abi.iptr(jrecords, _abi.JoinRecord)),
                  "attpc_joins_last")
        assert jevents.tobytes() == on["joins"][0][-4:].tobytes() and jrecords.tobytes() == on["joins"][1][-4:].tobytes()
        assert ctx.lib.attpc_joins_last(ctx.handle, EVENTS - 3, 4, _abi.iptr(jevents, _abi.JoinEvent), None) == _abi.E_INVALID
        assert ctx.lib.attpc_joins_last(ctx.handle, -1, 1, _abi.iptr(jevents, _abi.JoinEvent), None) == _abi.E_INVALID
        assert ctx.lib.attpc_joins_last(ctx.handle, EVENTS, 0, None, None) == _abi.OK
    finally:
        eng.configure_cluster_join()
        eng.configure_clustering()


def test_run_composes_with_every_stage(run, ctx):
    """Correction, thinning, circle fit, helix slope and a track fit on, 32 events: the records equal those of the
    stage-alone calls chained."""
    from attpc_engine_amd.detector.fit import TrackFitSettings, rows_to_fit

    inp, eng, off, on, want, alone, join = run
    n = 32
    correction = CorrectionSettings(dc.named_map())
    fit = TrackFitSettings(max_evaluations=2)
    eng.configure_correction(correction)
    eng.configure_clustering(CLUSTERING)
    eng.configure_cluster_join(join)
    eng.configure_track_fit(fit)
    _stages(eng, True)
    try:
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    finally:
        _stages(eng, False)
        eng.configure_track_fit()
        eng.configure_cluster_join()
        eng.configure_clustering()
        eng.configure_correction()
    offsets = off["offsets"][:n + 1]
    total = int(offsets[-1])
    rows, labels, _, counts = rows_to_correction(offsets, off["rows"][:total], off["labels"][:total], correction, inp.config, ctx)
    assert res["rows"].tobytes() == rows.tobytes() and np.array_equal(res["labels"], labels) and res["correction"] == counts
    stage_alone = rows_to_joined_clusters(offsets, rows, labels, inp.indices, CLUSTERING, join, ctx)
    got = (res["cluster_labels"], *res["clusters"], *res["joins"])
    _assert_same(got, _joined_reference(CLUSTERING, join, offsets, rows, labels, inp.indices), "corrected")
    _assert_same(stage_alone, got, "stage alone")
    point_offsets, points, point_labels, info = rows_to_points(offsets, rows, stage_alone[0], inp.indices, THINNING, ctx)
    records = rows_to_estimates(point_offsets, points, point_labels, inp.indices, ESTIMATES, ctx, config=inp.config, circle=CIRCLE, helix=HELIX)
    records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
    assert res["estimates"].tobytes() == records.tobytes() and (records["n_fit"] > 0).sum() > n // 2
    fits = rows_to_fit(point_offsets, points, point_labels, eng.layout, records, ctx, fit,
                       estimate_settings=ESTIMATES.for_field(float(inp.config.det_params.bfield)))
    assert res["fits"].tobytes() == fits.tobytes() and (fits["evaluations"] > 0).sum() > n // 4


def test_behind_a_trigger_gate(run, ctx):
    """An event that did not fire has no rows: a join event of zeros plus NOT_CLUSTERED, unused join records."""
    inp, eng, off, on, want, alone, join = run
    n = 64
    eng.configure_clustering(CLUSTERING)
    eng.configure_cluster_join(join)
    eng.configure_trigger(TriggerSettings(25, window=50, group_multiplicity=GATE_MULTIPLICITY, gate=True))
    try:
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
    finally:
        eng.configure_trigger()
        eng.configure_cluster_join()
        eng.configure_clustering()
    fired = res["trigger"]["fired"] != 0
    jevents, jrecords = res["joins"]
    print("fired", int(fired.sum()), "of", n)
    assert 0 < fired.sum() < n and np.all(np.diff(res["offsets"])[~fired] == 0)
    for name in JOIN_EVENT_DTYPE.names:
        expect = jref.JOIN_NOT_CLUSTERED if name == "status" else 0
        assert np.all(jevents[name][~fired] == expect), name
    assert np.all(jrecords["first_row"][~fired] == -1) and not any(jrecords[name][~fired].any() for name in JOIN_DTYPE.names if name != "first_row")
    expect = _joined_reference(CLUSTERING, join, res["offsets"], res["rows"], res["labels"], inp.indices)
    _assert_same((res["cluster_labels"], *res["clusters"], jevents, jrecords), expect, "gated")
    assert (jevents["n_candidates"][fired] > 0).any()
