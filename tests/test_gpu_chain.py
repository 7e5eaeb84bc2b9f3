"""Every pair of opt-in stages together on the device -- the trace stages, and straggling, drift distortion, drift
correction, helix slope and track fit around them: one test per row of the table of tests/chain_cases.py (16 factors),
the device against the composition of the stages' numpy restatements (tests/chain_reference.py) on the device's own
cloud -- traces, trigger records, trace rows (the corrected ones with the drift correction on, and its counts), thinned
points, estimates and track fits equal, every comparison an equality (integer fields equal, f64 fields bit for bit);
the one exception is the Fourier baseline's operator, held to its restatement under the rule and the constants of
tests/test_gpu_baseline.py, the rows then exact given its y.  Each row states on the restatement's own figures that it
is not vacuous.  Then every run kind in turn on one context against fresh contexts, with every stage of the all-on row
configured, and the file-driven forms against the ``Engine``.  Needs a real MI355X: ``-m gpu``.

The cloud behind every later call is held to the first one's by the run statistics: both checksums and the number of
track samples everywhere, ``n_points`` for the trace calls -- a trace-row call reports its rows there (the contract of
``run_trace_rows``), which are held to the restatement's count instead.  Straggling and the drift distortion shape
that cloud and nothing behind it: with either on, every run kind still reports the first call's sums.

Measured on an MI355X, wall time per row with its restatement: 5.5 s for the all-on row (36 735 traces, 4 track fits;
1.0 s at the other chunking and 1.5 s with every event a chunk of its own, the restatement made once), 0.3 .. 2.9 s
for the others (the rows with the track fit: 1.2 .. 2.9 s); the same file with the table of 12 factors, on the same
machine: 4.4 s, 1.0 s and 0.3 .. 2.2 s.  No row found a difference.  The figures of the non-vacuity conditions of every
row are in DESIGN.md §6; each test prints its own."""
import sys
import time
import warnings

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.thinning import rows_to_points
from attpc_engine_amd.detector.traces import remove_baseline, simulate_batch_trace_rows, unpack_traces
from tests import chain_cases as cc
from tests import chain_reference as cr
from tests import estimate_reference as est
from tests import fit_reference, thin_reference, trace_pack_reference, trigger_reference
from tests.helpers import Inputs
from tests.maps_reference import assert_same_maps
from tests.test_gpu_baseline import _assert_operator_equals_restatement, _read_spyral_files

pytestmark = pytest.mark.gpu

CLOUD_SUMS = ("charge_checksum", "key_checksum")
RUN_COUNTS = ("n_events", "n_points", "n_track_samples", "n_failed", "n_inconsistent") + CLOUD_SUMS


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def inp():
    return Inputs(cc.WORKLOAD)


def _configure(eng, s) -> None:
    """Every stage of the chain as the settings have it, on or off."""
    eng.configure_straggling(s["straggling"])
    eng.configure_distortion(s["distortion"])
    eng.configure_traces(eng.config, **s["traces"])
    eng.configure_spyral(eng.config)
    eng.configure_gain(s["gain"])
    eng.configure_common_mode(s["common_mode"])
    eng.configure_peaks(s["peaks"])
    eng.configure_baseline(s["baseline"])
    eng.configure_trigger(s["trigger"])
    eng.configure_estimates(s["estimates"])
    eng.configure_thinning(s["thinning"])
    eng.configure_circle_fit(s["circle"])
    eng.configure_helix_slope(s["helix"])
    eng.configure_track_fit(s["fit"])
    eng.configure_correction(s["correction"])


def _engine(inp, ctx, s, chunks: int = 1):
    from attpc_engine_amd.engine import Engine

    chunk_events = {1: None, 3: cc.CHUNK_EVENTS, "one event each": 1}[chunks]
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx, chunk_events=chunk_events)
    _configure(eng, s)
    return eng


def _reset(inp, ctx) -> None:
    from attpc_engine_amd.detector.traces import configure_traces
    from attpc_engine_amd.engine import Engine

    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    _configure(Engine(inp.pipeline, inp.config, inp.indices, context=ctx), cc.settings(cc.case("all_off"), inp.config))
    configure_traces(inp.config, ctx, None, None, 0)


def _canonical(offsets, rows, labels):
    """Rows whose order inside an event is not specified (clouds; Spyral rows of equal z): every event sorted on all
    columns."""
    table = np.column_stack([np.asarray(rows, dtype=np.float64).reshape(len(labels), -1), np.asarray(labels, dtype=np.float64)])
    event = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return table[np.lexsort(tuple(table.T[::-1]) + (event,))]


def _same_cloud(got, want, what):
    np.testing.assert_array_equal(got["offsets"], want["offsets"], err_msg=what)
    np.testing.assert_array_equal(_canonical(got["offsets"], got["points"], got["labels"]),
                                  _canonical(want["offsets"], want["points"], want["labels"]), err_msg=what)


def _device_baseline(ctx, what):
    """Step 5 of the chain as the device does it: the operator held to its restatement, then its own y."""
    def operator(samples, scale):
        _assert_operator_equals_restatement(samples, scale, ctx, what)
        return remove_baseline(samples, scale, ctx)
    return operator


_REFERENCE = {}  # case name -> (the device's cloud, the chain of it, the ungated chain or None): made once, read-only


def _reference(inp, ctx, c, s, cloud):
    if c.name in _REFERENCE:
        _same_cloud(cloud, _REFERENCE[c.name][0], f"{c.name}: the cloud does not depend on the chunks")
        return _REFERENCE[c.name][1:]
    first = cc.first_event(c)
    csr = (cloud["offsets"], cloud["points"], cloud["labels"])
    operator = _device_baseline(ctx, c.name)
    want = cr.chain(s, inp.config, inp.indices, csr, cc.SEED, first, baseline=operator, inp=inp)
    ungated = None
    if c.trigger == "gate":
        ungated = cr.chain({**s, "trigger": s["trigger"].gated(False)}, inp.config, inp.indices, csr, cc.SEED, first,
                           baseline=operator, traces=want.traces, inp=inp)
    figures = cr.counts(s, inp.config, inp.indices, csr, cc.SEED, first, want)
    print(f"{c.name}: {figures}")
    cr.assert_not_vacuous(figures, c.n_events)
    _REFERENCE[c.name] = (cloud, want, ungated)
    return want, ungated


def _assert_run(res, cloud, what, n_points=None):
    """The cloud behind a later call is the chain's input: its sums, and its size (a trace-row call counts its rows)."""
    for key in CLOUD_SUMS:
        assert res["stats"][key] == cloud["stats"][key], (what, key)
    assert res["stats"]["n_points"] == (cloud["stats"]["n_points"] if n_points is None else n_points), what
    assert res["stats"]["n_track_samples"] == cloud["stats"]["n_track_samples"], what


def _assert_trigger(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, trigger_reference.differing(got, want))


def _check_case(inp, ctx, c, chunks):
    s = cc.settings(c, inp.config)
    n, seed, first = c.n_events, cc.SEED, cc.first_event(c)
    run = dict(seed=seed, first_event=first)
    started = time.perf_counter()
    try:
        eng = _engine(inp, ctx, s, chunks)
        cloud = eng.run(n, fetch=True, **run)
        want, ungated = _reference(inp, ctx, c, s, cloud)
        fetch = c.delivery == "fetch"
        # ---- traces
        resident = eng.run_traces(n, fetch=False, **run)
        assert resident["trace"] == want.traces[4], (resident["trace"], want.traces[4])
        _assert_run(resident, cloud, "run_traces, resident")
        triggers = [resident.get("trigger")]
        if fetch:
            tr = eng.run_traces(n, **run)
            for k, key in enumerate(("offsets", "pads", "samples", "labels")):
                np.testing.assert_array_equal(tr[key], want.traces[k], err_msg=f"traces {key}")
            assert tr["trace"] == want.traces[4]
            np.testing.assert_array_equal(tr["event_points"], np.diff(cloud["offsets"]))
            np.testing.assert_array_equal(tr["p4"], cloud["p4"])
            _assert_run(tr, cloud, "run_traces")
            triggers.append(tr.get("trigger"))
        if c.packed:
            row_start, packed = trace_pack_reference.encode(want.traces[2])
            small = eng.run_traces(n, fetch=False, packed=True, **run)
            assert small["trace"] == {**want.traces[4], "n_bytes": len(packed)}
            if fetch:
                pk = eng.run_traces(n, packed=True, **run)
                np.testing.assert_array_equal(pk["row_start"], row_start)
                np.testing.assert_array_equal(pk["packed"], packed)
                np.testing.assert_array_equal(pk["pads"], want.traces[1])
                np.testing.assert_array_equal(unpack_traces(pk["row_start"], pk["packed"]), want.traces[2])
                few = slice(0, 64)
                np.testing.assert_array_equal(trace_pack_reference.decode(pk["row_start"][:65], pk["packed"]), want.traces[2][few])
                triggers.append(pk.get("trigger"))
        # ---- rows
        kept = eng.run_trace_rows(n, fetch=False, **run)
        assert kept["trace_rows"] == want.rows[3], (kept["trace_rows"], want.rows[3])
        _assert_run(kept, cloud, "run_trace_rows, resident", n_points=want.rows[3]["n_rows"])
        triggers.append(kept.get("trigger"))
        records, fits, corrections = [kept.get("estimates")], [kept.get("fits")], [kept.get("correction")]
        rows = want.rows  # (with the drift correction on: the corrected rows and the labels that moved with them)
        if fetch:
            res = eng.run_trace_rows(n, **run)
            for k, key in enumerate(("offsets", "rows", "labels")):
                np.testing.assert_array_equal(res[key], want.rows[k], err_msg=f"trace rows {key}")
            assert res["trace_rows"] == want.rows[3]
            _assert_run(res, cloud, "run_trace_rows", n_points=want.rows[3]["n_rows"])
            np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
            triggers.append(res.get("trigger"))
            records.append(res.get("estimates"))
            fits.append(res.get("fits"))
            corrections.append(res.get("correction"))
            rows = (res["offsets"], res["rows"], res["labels"])
        # ---- trigger: one set of records, whichever call made them
        if s["trigger"] is None:
            assert triggers == [None] * len(triggers)
        else:
            triggers.append(eng.run_trigger(n, **run)["trigger"])
            for k, got in enumerate(triggers):
                _assert_trigger(got, want.trigger, f"trigger records {k}")
        # ---- points and estimates
        if s["thinning"] is not None:
            thin_reference.assert_same_points(rows_to_points(*rows[:3], inp.indices, s["thinning"], ctx), want.points)
        if s["estimates"] is None:
            assert records == [None] * len(records) and "slope" not in kept
        else:
            only = eng.run_estimates(n, **run)
            assert only["trace_rows"] == want.rows[3]
            records.append(only["estimates"])
            fits.append(only.get("fits"))
            corrections.append(only.get("correction"))
            for got in records:
                est.assert_same_records(got, want.records)
            assert kept.get("thinning") == (cc.THIN_STEP if c.estimates == "thinned" else None)
            assert kept.get("circle") == ("geometric" if c.circle else None)
            assert kept.get("slope") == only.get("slope") == ("helix" if c.helix else None)
        # ---- the drift correction's counts and the track fits: one set, whichever call made them; absent when off
        if s["correction"] is None:
            assert corrections == [None] * len(corrections) and want.correction is None
        else:
            assert corrections == [want.correction] * len(corrections), (corrections, want.correction)
        if s["fit"] is None:
            assert fits == [None] * len(fits) and want.fits is None
        else:
            assert len(fits) >= 2
            for got in fits:
                fit_reference.assert_same_records(got, want.fits)
        # ---- gate
        if c.trigger == "gate":
            fired = want.fired
            assert 0 < fired.sum() < n
            for e in range(n):
                lo, hi = rows[0][e], rows[0][e + 1]
                if not fired[e]:
                    assert lo == hi
                    continue
                ulo, uhi = ungated.rows[0][e], ungated.rows[0][e + 1]
                np.testing.assert_array_equal(rows[1][lo:hi], ungated.rows[1][ulo:uhi], err_msg=f"event {e}")
                np.testing.assert_array_equal(rows[2][lo:hi], ungated.rows[2][ulo:uhi], err_msg=f"event {e}")
            if s["estimates"] is not None:
                empty = records[0][~fired]
                assert (empty["status"] == _abi.EST_EMPTY).all() and (empty["n_rows"] == 0).all() and (empty["reserved"] == 0).all()
                est.assert_same_records(records[0][fired], ungated.records[fired])
            if s["fit"] is not None:
                empty = fits[0][~fired]
                assert (empty["status"] == _abi.FIT_EMPTY).all() and not empty["reserved"].any()
                for field in ("evaluations", "n_points", "n_inside", "steps", "end"):
                    assert not empty[field].any(), field
                for field in ("f", "lambda", "g", "vertex", "ke", "brho", "path"):  # (every f64 field but the reserved ones)
                    assert np.isnan(empty[field]).all(), field
                fit_reference.assert_same_records(fits[0][fired], ungated.fits[fired])
    finally:
        _reset(inp, ctx)
    print(f"{c.name}, {chunks} chunk(s): {time.perf_counter() - started:.1f} s")


@pytest.mark.parametrize("name", cc.CASE_IDS)
def test_row_equals_the_composed_restatement(ctx, inp, name):
    c = cc.case(name)
    _check_case(inp, ctx, c, c.chunks)


def test_all_on_does_not_depend_on_the_chunks(ctx, inp):
    """The all-on row at the other chunking: the same cloud, and every output the same restatement's."""
    c = cc.case("all_on")
    _check_case(inp, ctx, c, 1 if c.chunks == 3 else 3)


def test_all_on_in_chunks_of_one_event(ctx, inp):
    """The all-on row once more, every event a chunk of its own: the chunk of an event that did not fire holds no row,
    so the drift correction is not run on it while the thinning, the estimates and the track fit behind it still are;
    and the chunk of one that fired uses the sort keys and the fit's scratch its neighbours left."""
    _check_case(inp, ctx, cc.case("all_on"), "one event each")


# ---------------------------------------------------------------- one context, every run kind ----
def _same_result(got, want, what, unordered=None):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if key == "stats":
            assert {k: g[k] for k in RUN_COUNTS} == {k: w[k] for k in RUN_COUNTS}, what
        elif key == "maps":
            assert_same_maps(g, w, what)
        elif key == "estimates":
            est.assert_same_records(g, w)
        elif key == "fits":
            fit_reference.assert_same_records(g, w)
        elif key == "correction":
            assert g == w and set(w) == {"n_rows", "n_skipped", "n_unconverged", "n_moved"}, (what, g, w)
        elif key in (unordered, "labels") and unordered:
            pass  # (below, in canonical order)
        elif isinstance(w, np.ndarray) and w.dtype.names:
            assert g.tobytes() == w.tobytes(), (what, key)
        elif isinstance(w, np.ndarray):
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {key}")
        else:
            assert g == w, (what, key, g, w)
    if unordered:
        np.testing.assert_array_equal(_canonical(got["offsets"], got[unordered], got["labels"]),
                                      _canonical(want["offsets"], want[unordered], want["labels"]), err_msg=what)


RUN_KINDS = (  # (name, the call, the rows whose order inside an event is free)
    ("run", lambda e, n, kw: e.run(n, fetch=True, **kw), "points"),
    ("run_spyral", lambda e, n, kw: e.run_spyral(n, **kw), "rows"),
    ("run_summary", lambda e, n, kw: e.run_summary(n, **kw), None),
    ("run_selected cloud", lambda e, n, kw: e.run_selected(n, rows="cloud", **kw), "points"),
    ("run_selected spyral", lambda e, n, kw: e.run_selected(n, rows="spyral", **kw), "rows"),
    ("run_maps", lambda e, n, kw: e.run_maps(n, **kw), None),
    ("run_traces", lambda e, n, kw: e.run_traces(n, **kw), None),
    ("run_traces packed", lambda e, n, kw: e.run_traces(n, packed=True, **kw), None),
    ("run_trigger", lambda e, n, kw: e.run_trigger(n, **kw), None),
    ("run_trace_rows", lambda e, n, kw: e.run_trace_rows(n, **kw), None),
    ("run_estimates", lambda e, n, kw: e.run_estimates(n, **kw), None),
)
SEQUENCE = RUN_KINDS + RUN_KINDS[:3]


def test_every_run_kind_in_turn_on_one_context(inp):
    """The kinds share device buffers (the sort keys, which the drift correction borrows, the assembly sets, the
    uncorrected rows, the track fit's scratch, the per-chunk buffers that only grow): each call on the one context, with
    every stage of the all-on row configured, gives what the same call gives on a context that never ran anything else
    -- at two event counts, the smaller one second, so that the buffers both grow and are used again at a smaller size."""
    c = cc.case("all_on")
    s = cc.settings(c, inp.config)
    kw = dict(seed=cc.SEED, first_event=cc.first_event(c))
    shared = _abi.Context(0)

    def engine(context):
        eng = _engine(inp, context, s, c.chunks)
        eng.configure_selection(n_pads=(100, None))
        eng.configure_maps()
        return eng

    try:
        eng = engine(shared)
        for n in (c.n_events, 7):
            passed = None
            for name, call, unordered in SEQUENCE:
                got = call(eng, n, kw)
                fresh = _abi.Context(0)
                try:
                    want = call(engine(fresh), n, kw)
                finally:
                    fresh.close()
                _same_result(got, want, f"{name}, {n} events", unordered)
                if n == c.n_events and name in ("run_trace_rows", "run_estimates"):  # (the sort and the fit had work to do)
                    assert want["correction"]["n_moved"] > 0 and (want["fits"]["evaluations"] >= 2).any(), name
                if name.startswith("run_selected"):
                    passed = want["passed"]
            assert 0 < passed.sum() < n  # (the selection takes some of the events and leaves some)
    finally:
        shared.close()


# ---------------------------------------------------------------- the file-driven forms ----
def test_file_driven_forms_give_the_rows_and_records_of_the_engine(ctx, inp, tmp_path, monkeypatch):
    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.engine import run_fused

    c = cc.case("all_on")
    s = cc.settings(c, inp.config)
    n, seed = c.n_events, cc.SEED
    stages = dict(peaks=s["peaks"], baseline=s["baseline"], gain=s["gain"], common_mode=s["common_mode"])
    try:
        for first in (cc.first_event(c), 0):
            res = _engine(inp, ctx, s).run_trace_rows(n, seed=seed, first_event=first)
            assert res["trace_rows"]["n_rows"] > 0 and 0 < (res["trigger"]["fired"] != 0).sum() < n
            if first:  # simulate_batch_trace_rows, from the kinematics of the engine's events
                off, rows, labels, event_points, stats = simulate_batch_trace_rows(
                    res["p4"], res["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, first_event=first, ctx=ctx,
                    trigger=s["trigger"], estimates=s["estimates"], thinning=s["thinning"], circle=s["circle"],
                    straggling=s["straggling"], distortion=s["distortion"], correction=s["correction"], helix=s["helix"],
                    fit=s["fit"], **stages, **s["traces"])
                np.testing.assert_array_equal(off, res["offsets"])
                np.testing.assert_array_equal(rows, res["rows"])
                np.testing.assert_array_equal(labels, res["labels"])
                np.testing.assert_array_equal(event_points, res["event_points"])
                assert {k: stats[k] for k in ("n_rows", "row_checksum")} == res["trace_rows"]
                est.assert_same_records(stats["estimates"], res["estimates"])
                _assert_trigger(stats["trigger"], res["trigger"], "simulate_batch_trace_rows")
                assert stats["thinning"] == cc.THIN_STEP and stats["circle"] == "geometric" and stats["slope"] == "helix"
                fit_reference.assert_same_records(stats["fits"], res["fits"])
                assert stats["correction"] == res["correction"] and res["correction"]["n_moved"] > 0
                assert (res["fits"]["evaluations"] >= 2).any()
                continue
            # SpyralWriter(peaks=...) through run_fused: events 0 .. n - 1, those that fired and are not empty
            monkeypatch.setitem(sys.modules, "h5py", None)
            warnings.simplefilter("ignore", RuntimeWarning)
            writer = SpyralWriter(tmp_path, inp.config, max_events_per_file=5, correction=s["correction"], **stages, **s["traces"])
            run_fused(inp.pipeline, inp.config, writer, n, inp.indices, seed=seed, batch_size=cc.CHUNK_EVENTS, context=ctx,
                      trigger=s["trigger"], straggling=s["straggling"], distortion=s["distortion"], correction=s["correction"])
            got = _read_spyral_files(tmp_path)
            written = [e for e in range(n) if res["event_points"][e] > 0 and res["trigger"]["fired"][e]]
            assert sorted(got) == written and written
            for e in written:
                lo, hi = res["offsets"][e], res["offsets"][e + 1]
                np.testing.assert_array_equal(got[e][0], res["rows"][lo:hi], err_msg=f"event {e}")
                np.testing.assert_array_equal(got[e][1], res["labels"][lo:hi], err_msg=f"event {e}")
    finally:
        _reset(inp, ctx)
