"""The particle identification on the device (``pid_kernel``, csrc/pid.hip, and ``fit_kernel<true>``, csrc/fit.hip)
against its restatement (tests/pid_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The edge rule is written operation by operation and the assignment is integer work (include/attpc_engine.h, "particle
identification"), so every comparison here is exact: records equal or not, the fits' f64 fields bit for bit, NaN in
the same places; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.clustering import ClusterSettings
from attpc_engine_amd.detector.fit import TrackFitSettings, rows_to_fit
from attpc_engine_amd.detector.pid import PID_DTYPE, Gate, PidSettings, by_position, estimates_to_pid
from attpc_engine_amd.detector.thinning import rows_to_points
from tests import fit_reference as fref
from tests import pid_cases as pc
from tests import pid_reference as pref
from tests import thin_reference as thin
from tests.helpers import Inputs
from tests.test_gpu_join import CIRCLE, ESTIMATES, EVENTS, FIRST, HELIX, JOIN, PARTIAL, PEAKS, SEED, THINNING, _stages

pytestmark = pytest.mark.gpu

RANK = ClusterSettings(match="rank")
FIT = dict(time_step=2e-9, max_steps=600, max_evaluations=3, tolerance_momentum=1e-3, tolerance_position=1e-3)  # (cheap in numpy)
EVERYTHING = Gate.rectangle((1e-30, 1e30), (1e-30, 1e30))  # every positive point the estimates can give


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.close()


def _settings(case: pc.Case) -> PidSettings:
    return PidSettings(list(case.gates), "own" if case.mode == pref.OWN else "any")


def _same(got, want, what=""):
    assert got.dtype == PID_DTYPE and got.shape == want.shape, what
    for name in PID_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())
    assert got.tobytes() == np.ascontiguousarray(want.astype(PID_DTYPE)).tobytes(), what


# 1 ------------------------------------------------------------------------------------------ the stage alone ----
@pytest.mark.parametrize("name", list(pc.cases()))
def test_stage_alone_equals_the_restatement(ctx, name):
    case = pc.cases()[name]
    _same(estimates_to_pid(case.estimates, _settings(case), ctx), pc.reference()[name], name)


def test_the_library_checks_its_arguments(ctx):
    case = pc.cases()["alphas"]
    good = _settings(case).desc()
    estimates = np.ascontiguousarray(case.estimates)
    out = np.zeros(estimates.shape, dtype=PID_DTYPE)
    args = (ctx.handle, len(estimates), case.n_sim, _abi.iptr(estimates, _abi.TrackEstimate))
    for field, value in (("mode", 2), ("mode", -1), ("reserved", 1)):
        desc = _settings(case).desc()
        setattr(desc, field, value)
        assert ctx.lib.attpc_estimates_pid(*args, desc, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID, (field, value)
        assert ctx.lib.attpc_trace_configure_pid(ctx.handle, desc) == _abi.E_INVALID, (field, value)
    for position, count in ((0, 2), (1, 33), (2, -1), (7, 1)):
        desc = _settings(case).desc()
        desc.n_vertices[position] = count
        assert ctx.lib.attpc_estimates_pid(*args, desc, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID, (position, count)
        assert ctx.lib.attpc_trace_configure_pid(ctx.handle, desc) == _abi.E_INVALID, (position, count)
    for value in (float("nan"), float("inf")):
        desc = _settings(case).desc()
        desc.vertices[1][2][1] = value
        assert ctx.lib.attpc_estimates_pid(*args, desc, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID, value
        assert ctx.lib.attpc_trace_configure_pid(ctx.handle, desc) == _abi.E_INVALID, value
    assert ctx.lib.attpc_estimates_pid(*args, None, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID
    assert ctx.lib.attpc_estimates_pid(ctx.handle, 1, 9, _abi.iptr(estimates, _abi.TrackEstimate), good, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID
    assert ctx.lib.attpc_estimates_pid(ctx.handle, -1, 4, _abi.iptr(estimates, _abi.TrackEstimate), good, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID
    assert ctx.lib.attpc_estimates_pid(ctx.handle, 1, 4, None, good, _abi.iptr(out, _abi.PidRecord)) == _abi.E_INVALID
    assert ctx.lib.attpc_estimates_pid(ctx.handle, 0, 4, None, good, None) == _abi.OK
    assert ctx.lib.attpc_estimates_pid(ctx.handle, 5, 0, None, good, None) == _abi.OK
    # a NaN behind n_vertices is not read
    desc = _settings(case).desc()
    desc.vertices[0][4][0] = float("nan")
    ctx.check(ctx.lib.attpc_estimates_pid(*args, desc, _abi.iptr(out, _abi.PidRecord)), "attpc_estimates_pid")
    _same(out, pc.reference()["alphas"], "a NaN behind n_vertices")
    assert ctx.lib.attpc_pid_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED  # no trace-row call has made records


# 2 ------------------------------------------------------------------------------------------ in the run ----
def _species(inp):
    lay = inp.layout
    return [int(lay.species_of_row[lay.indices[p]]) for p in range(lay.n_sim)]


def _last_gate(inp):
    return {len(inp.indices) - 1: EVERYTHING}


@pytest.fixture(scope="module")
def run(ctx):
    """The 128 events of o16aa of tests/test_gpu_join.py's run (partial readout with noise), label-free: clustering in
    match="rank" with the joining, thinning, estimates with circle fit and helix slope, and the track fit.  One gate,
    on the LAST position, holds every positive point.  (inp, eng, the run with the identification off, the run with it
    on), read-only."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    inp = Inputs("o16aa")
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), **PARTIAL)
    eng.configure_peaks(PEAKS)
    eng.configure_estimates(ESTIMATES)
    _stages(eng, True)
    eng.configure_clustering(RANK)
    eng.configure_cluster_join(JOIN)
    eng.configure_track_fit(TrackFitSettings(**FIT))
    off = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)  # (this context has never configured the stage)
    eng.configure_pid(_last_gate(inp))
    on = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    eng.configure_pid()
    return inp, eng, off, on


def test_fused_label_free_chain(run, ctx):
    inp, eng, off, on = run
    n_sim = len(inp.indices)
    last = n_sim - 1
    assert n_sim >= 2 and "pid" not in off and on["pid"].shape == (EVENTS, n_sim)
    for key in ("offsets", "rows", "labels", "cluster_labels", "estimates"):
        assert on[key].tobytes() == off[key].tobytes(), key
    pid, estimates = on["pid"], on["estimates"]
    gates = [None] * 8
    gates[last] = EVERYTHING.vertices
    _same(pid, pref.records(estimates, gates, pref.ANY, species=_species(inp)), "run")
    # by construction: the first slot with a point gets the last position, every later one finds it taken
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(estimates["brho"]) & np.isfinite(estimates["dedx"]) & (estimates["brho"] > 0) & (estimates["dedx"] > 0)
    first = finite & (np.cumsum(finite, axis=1) == 1)
    assert first.sum() > EVENTS // 2 and (finite & ~first).sum() > EVENTS // 4 and (~finite).sum() > 0
    assert np.all(pid["position"][first] == last) and np.all(pid["status"][first] == 0) and np.all(pid["held"][finite] == 1 << last)
    assert np.all(pid["species"][first] == _species(inp)[last]) and _species(inp)[last] >= 0
    assert np.all(pid["status"][finite & ~first] == pref.TAKEN) and np.all(pid["position"][~first] == -1)
    assert np.all(pid["status"][~finite] == pref.NO_ESTIMATE) and np.all(pid["species"][~first] == -1)
    # the fits: the stage alone behind the records, and the restatement, on the delivered rows and cluster labels
    point_offsets, points, point_labels, _ = rows_to_points(on["offsets"], on["rows"], on["cluster_labels"], inp.indices, THINNING, ctx)
    field = ESTIMATES.for_field(float(inp.config.det_params.bfield))
    alone = rows_to_fit(point_offsets, points, point_labels, eng.layout, estimates, ctx, TrackFitSettings(**FIT), estimate_settings=field, pid=pid)
    assert on["fits"].tobytes() == alone.tobytes()
    t_offsets, t_points, t_labels, _ = thin.thin(on["offsets"], on["rows"], on["cluster_labels"], inp.indices, THINNING.z_step)
    want = pref.fit_with_pid(t_offsets, t_points, t_labels, inp.indices, fref.Model(inp.det, inp.layout), estimates, pid,
                             fref.Settings(**FIT), ESTIMATES.beam_region_radius)
    fref.assert_same_records(on["fits"], want)
    fits = on["fits"]
    assert np.all(fits["status"][pid["position"] < 0] == pref.FIT_NO_PID) and not (fits["status"][first] & pref.FIT_NO_PID).any()
    assert np.all(fits["evaluations"][pid["position"] < 0] == 0) and np.all(np.isnan(fits["brho"][pid["position"] < 0]))
    # an assigned slot that is not the last was fitted with another species' table: its fit is another one
    other_species = np.array(_species(inp)) != _species(inp)[last]
    moved = first & other_species[None, :] & (fits["evaluations"] >= 2) & (off["fits"]["evaluations"] >= 2)
    different = moved & (fits["brho"] != off["fits"]["brho"])
    print("assigned", int(first.sum()), "taken", int((finite & ~first).sum()), "fitted as another species", int(moved.sum()), "different", int(different.sum()))
    assert first.sum() >= 1 and moved.sum() >= 1 and different.sum() == moved.sum()
    same_slot = first[:, last] & (fits["evaluations"][:, last] >= 1)
    assert fits[:, last][same_slot].tobytes() == off["fits"][:, last][same_slot].tobytes()  # its own species: the same fit
    # by_position: the record of position `last` is the one of the slot that got it
    moved_fits, slot_of = by_position(fits, pid)
    events, slots = np.nonzero(first)
    assert np.array_equal(slot_of[events, last], slots) and moved_fits[events, last].tobytes() == fits[events, slots].tobytes()


# 3 ------------------------------------------------------------------------------------------ mode OWN ----
def test_own_mode_on_a_truth_labelled_run(run, ctx):
    """Truth labels (no clustering), the fit off; the gates are the bands of this run's own estimates."""
    inp, eng, off, on = run
    n_sim = len(inp.indices)
    eng.configure_clustering()
    eng.configure_cluster_join()
    eng.configure_track_fit()
    try:
        plain = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
        gates = []
        for p in range(n_sim):
            try:
                gates.append(Gate.from_band(plain["estimates"]["brho"][:, p], plain["estimates"]["dedx"][:, p], bins=4, coverage=(0.05, 0.95)))
            except ValueError:  # (too few estimated tracks at this position)
                gates.append(None)
        assert sum(g is not None for g in gates) >= 2
        eng.configure_pid(gates, mode="own")
        res = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)
    finally:
        eng.configure_pid()
        eng.configure_track_fit(TrackFitSettings(**FIT))
        eng.configure_clustering(RANK)
        eng.configure_cluster_join(JOIN)
    assert "fits" not in res and res["estimates"].tobytes() == plain["estimates"].tobytes()
    reference = [None if g is None else g.vertices for g in gates] + [None] * (8 - n_sim)
    _same(res["pid"], pref.records(res["estimates"], reference, pref.OWN, species=_species(inp)), "own")
    assigned = res["pid"]["position"] >= 0
    share = [float(assigned[:, p].mean()) for p in range(n_sim)]
    print("assigned share per position", share)
    assert np.all(res["pid"]["position"][assigned] == np.nonzero(assigned)[1]) and not (res["pid"]["status"] & (pref.TAKEN | pref.AMBIGUOUS)).any()
    assert assigned.sum() > EVENTS // 2 and (res["pid"]["status"] & pref.NONE).any()


# 4 ------------------------------------------------------------------------------------------ purity ----
def test_resident_runs_and_chunks_give_the_same(run, ctx):
    inp, eng, off, on = run
    eng.configure_pid(_last_gate(inp))
    try:
        resident = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST, fetch=False)
        estimated = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        for other in (resident, estimated):
            assert "rows" not in other
            assert other["pid"].tobytes() == on["pid"].tobytes() and other["fits"].tobytes() == on["fits"].tobytes()
            assert other["estimates"].tobytes() == on["estimates"].tobytes()
        n = 48
        for chunk in (1, 7):
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, chunk), "attpc_set_chunk_events")
            try:
                chunked = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
                chunked_resident = eng.run_estimates(n, seed=SEED, first_event=FIRST)
            finally:
                ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
            for other in (chunked, chunked_resident):
                assert other["pid"].tobytes() == on["pid"][:n].tobytes() and other["fits"].tobytes() == on["fits"][:n].tobytes(), chunk
        # the range of the reader
        records = np.zeros((4, len(inp.indices)), dtype=PID_DTYPE)
        eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        ctx.check(ctx.lib.attpc_pid_last(ctx.handle, EVENTS - 4, 4, _abi.iptr(records, _abi.PidRecord)), "attpc_pid_last")
        assert records.tobytes() == on["pid"][-4:].tobytes()
        assert ctx.lib.attpc_pid_last(ctx.handle, EVENTS - 3, 4, _abi.iptr(records, _abi.PidRecord)) == _abi.E_INVALID
        assert ctx.lib.attpc_pid_last(ctx.handle, -1, 1, _abi.iptr(records, _abi.PidRecord)) == _abi.E_INVALID
        assert ctx.lib.attpc_pid_last(ctx.handle, EVENTS, 0, None) == _abi.OK
    finally:
        eng.configure_pid()


# 5, 6 ------------------------------------------------------------------------------------------ off, and half on ----
def test_stage_off_nothing_moves(run, ctx):
    inp, eng, off, on = run
    again = eng.run_trace_rows(EVENTS, seed=SEED, first_event=FIRST)  # configured and turned off again
    assert "pid" not in again and "pid" not in off
    records = np.zeros((1, len(inp.indices)), dtype=PID_DTYPE)
    assert ctx.lib.attpc_pid_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.PidRecord)) == _abi.E_NOTCONFIGURED
    for key in ("offsets", "rows", "labels", "cluster_labels", "estimates", "fits", "event_points", "p4", "vertex", "status"):
        assert again[key].tobytes() == off[key].tobytes(), key
    assert again["trace_rows"] == off["trace_rows"] and again["stats"]["key_checksum"] == off["stats"]["key_checksum"]
    assert not (off["fits"]["status"] & pref.FIT_NO_PID).any()
    # the stage-alone fit without pid= is the fit of the stage off
    point_offsets, points, point_labels, _ = rows_to_points(off["offsets"], off["rows"], off["cluster_labels"], inp.indices, THINNING, ctx)
    field = ESTIMATES.for_field(float(inp.config.det_params.bfield))
    alone = rows_to_fit(point_offsets, points, point_labels, eng.layout, off["estimates"], ctx, TrackFitSettings(**FIT), estimate_settings=field)
    assert alone.tobytes() == off["fits"].tobytes()
    bad = on["pid"].copy()
    bad["position"][3, 0] = len(inp.indices)
    with pytest.raises(ValueError, match="position"):
        rows_to_fit(point_offsets, points, point_labels, eng.layout, off["estimates"], ctx, TrackFitSettings(**FIT), estimate_settings=field, pid=bad)


def test_on_without_the_fit_and_without_the_estimates(run, ctx):
    inp, eng, off, on = run
    n = 32
    eng.configure_pid(_last_gate(inp))
    eng.configure_track_fit()
    try:
        res = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
        assert "fits" not in res and res["pid"].tobytes() == on["pid"][:n].tobytes()
        assert res["estimates"].tobytes() == on["estimates"][:n].tobytes()
        rows = int(on["offsets"][n])
        assert res["rows"].tobytes() == on["rows"][:rows].tobytes() and np.array_equal(res["cluster_labels"], on["cluster_labels"][:rows])
        eng.configure_estimates()
        _stages(eng, False)
        bare = eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
        assert "pid" not in bare and "estimates" not in bare and "fits" not in bare
        records = np.zeros((1, len(inp.indices)), dtype=PID_DTYPE)
        assert ctx.lib.attpc_pid_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.PidRecord)) == _abi.E_NOTCONFIGURED
        assert bare["rows"].tobytes() == res["rows"].tobytes() and np.array_equal(bare["cluster_labels"], res["cluster_labels"])
    finally:
        eng.configure_pid()
        eng.configure_estimates(ESTIMATES)
        _stages(eng, True)
        eng.configure_track_fit(TrackFitSettings(**FIT))
