"""Trace rows on the device -- kept pad traces -> peaks -> Spyral rows -- against the numpy restatement of the contract
(tests/peaks_reference.py) applied to the device's own traces of the same ids: offsets, all eight columns and labels
EXACTLY equal (integers, table look-ups and single-rounded f64 operations only: there is nothing to tolerate).  The
hand-made clouds of tests/peaks_cases.py through ``clouds_to_trace_rows``; fused and file-driven runs in hit mode with
and without noise, partial and full readout; the id cases; chunk, fetch and shard invariance; empty events and a layout
without simulated nuclei; every other output unchanged beside trace-row runs; the writers.  Two checks need no
restatement: a lone arrival gives one point on its pad and bucket, and every point sits on a kept trace pad with z
non-decreasing per event.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (PeakSettings, clouds_to_trace_rows, clouds_to_traces, configure_trace_rows,
                                              configure_traces, simulate_batch_trace_rows)
from tests import peaks_cases
from tests.helpers import ID_CASE_IDS, ID_CASES, Inputs
from tests.peaks_reference import Geometry, Peaks, trace_rows

pytestmark = pytest.mark.gpu

SEED_HI = 0x9E3779B97F4A7C15
LOOSE = Peaks(separation=12.0, prominence=6.0, min_width=1.0, max_width=60.0, rel_height=0.9, threshold=9.0)


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine
    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _pedestals(seed):
    return np.random.default_rng(seed).integers(0, 1500, size=_abi.NUM_PADS).astype(np.int16)


def _reset(ctx, config):
    configure_traces(config, ctx, None, None, 0)


def _assert_same(got, ref, what=""):
    """(offsets, rows, labels, sums) of the device and of the restatement: identical."""
    np.testing.assert_array_equal(np.asarray(got[0]), np.asarray(ref[0]), err_msg=f"{what} offsets")
    assert np.asarray(got[1]).shape == np.asarray(ref[1]).shape, what
    for col, name in enumerate(("x", "y", "z", "amplitude", "integral", "pad", "centroid", "pad scale")):
        np.testing.assert_array_equal(np.asarray(got[1])[:, col], np.asarray(ref[1])[:, col], err_msg=f"{what} {name}")
    np.testing.assert_array_equal(np.asarray(got[2]), np.asarray(ref[2]), err_msg=f"{what} labels")
    assert got[3] == ref[3], (what, got[3], ref[3])


def _points_sit_on_kept_pads_in_ascending_z(offsets, rows, trace_offsets, trace_pads):
    for e in range(len(offsets) - 1):
        ev = rows[offsets[e]:offsets[e + 1]]
        assert (np.diff(ev[:, 2]) >= 0).all(), e
        assert np.isin(ev[:, 5], trace_pads[trace_offsets[e]:trace_offsets[e + 1]]).all(), e


def test_hand_made_clouds(ctx):
    inp = Inputs("o16aa")
    ped, resp = peaks_cases.pedestals(), peaks_cases.box_response()
    configure_trace_rows(inp.config, ctx, PeakSettings(), response=resp, threshold=peaks_cases.TRACE_THRESHOLD,
                         offset=peaks_cases.TRACE_OFFSET, pedestals=ped)
    offsets, points, labels = peaks_cases.hand_cloud()
    seed, first = SEED_HI, (1 << 32) - 5  # the events cross the low word
    got = clouds_to_trace_rows(offsets, points, labels, ctx, seed=seed, first_event=first)
    tr = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
    ref = trace_rows(tr[0], tr[1], tr[2], tr[3], Peaks(), Geometry.of(inp.config), seed, first, ped)
    _assert_same(got, ref)
    for i, (name, _, _, expected) in enumerate(peaks_cases.hand_cases()):
        ev = got[1][got[0][i]:got[0][i + 1]]
        assert sorted((int(r[5]), int(r[6]), int(r[3])) for r in ev) == sorted(expected), name
    _reset(ctx, inp.config)


MODES = {
    "hit": ({}, Peaks(), 12),
    "hit_noise": ({"noise_sigma": 5.0, "pedestals": "random"}, Peaks(), 8),
    "hit_noise_loose": ({"noise_sigma": 5.0, "pedestals": "random", "noise_stream": 4}, LOOSE, 4),
    "partial": ({"noise_sigma": 5.0, "pedestals": "random", "threshold": 20.0, "readout": "partial"}, LOOSE, 4),
    "full": ({"noise_sigma": 5.0, "pedestals": "random", "threshold": 20.0, "readout": "full"}, Peaks(), 2),
}


def _check_fused(inp, ctx, n, seed, first, kw, pk, file_driven=True, offset=None):
    kw = dict(kw)
    ped = _pedestals(3) if kw.get("pedestals") == "random" else None
    if ped is not None:
        kw["pedestals"] = ped
    resp = get_response(inp.config)
    kw.setdefault("offset", int(np.argmax(resp)) if offset is None else offset)
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings(*pk))
    tr = eng.run_traces(n, seed=seed, first_event=first)
    res = eng.run_trace_rows(n, seed=seed, first_event=first)
    got = (res["offsets"], res["rows"], res["labels"], res["trace_rows"])
    ref = trace_rows(tr["offsets"], tr["pads"], tr["samples"], tr["labels"], pk, Geometry.of(inp.config), seed, first, ped)
    _assert_same(got, ref)
    np.testing.assert_array_equal(res["event_points"], tr["event_points"])
    np.testing.assert_array_equal(res["p4"], tr["p4"])
    assert res["stats"]["n_points"] == got[3]["n_rows"] == len(got[1])
    for key in ("charge_checksum", "key_checksum", "n_track_samples"):
        assert res["stats"][key] == tr["stats"][key], key
    _points_sit_on_kept_pads_in_ascending_z(got[0], got[1], tr["offsets"], tr["pads"])
    if file_driven:
        off, rows, labels, raw, stats = simulate_batch_trace_rows(
            res["p4"], res["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, first_event=first, ctx=ctx,
            peaks=PeakSettings(*pk), **kw)
        _assert_same((off, rows, labels, {k: stats[k] for k in ("n_rows", "row_checksum")}), got, "file-driven")
        np.testing.assert_array_equal(raw, res["event_points"])
    return eng, tr, got


@pytest.mark.parametrize("name", ["o16aa", "be10dp"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fused_and_file_driven(ctx, name, mode):
    inp = Inputs(name)
    kw, pk, n = MODES[mode]
    _, tr, got = _check_fused(inp, ctx, n, seed=21, first=7, kw=kw, pk=pk)
    assert got[3]["n_rows"] > 0
    if mode in ("partial", "full"):
        assert (tr["labels"] == -1).any()  # noise-only pads went through the stage
    if mode == "partial":
        assert (got[2] == -1).any()  # ... and, with the loose parameters, gave points
    _reset(ctx, inp.config)


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_id_cases(ctx, case):
    inp = Inputs("be10dp" if case.first_event % 2 else "o16aa")
    kw = {"noise_sigma": 3.0, "pedestals": "random", "noise_stream": 11}
    _check_fused(inp, ctx, 2, seed=case.seed, first=case.first_event, kw=kw, pk=LOOSE)
    _reset(ctx, inp.config)


def test_chunk_fetch_and_shard_invariance(ctx):
    inp = Inputs("be10dp")
    kw = {"noise_sigma": 5.0, "pedestals": 100, "noise_stream": 2, "threshold": 20.0, "readout": "partial", "offset": 7}
    seed, first, n = SEED_HI, (1 << 33) + 10, 40

    def run(e, lo=0, hi=n, **more):
        res = e.run_trace_rows(hi - lo, seed=seed, first_event=first + lo, **more)
        return res["offsets"], res["rows"], res["labels"], res["trace_rows"]

    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_peaks(PeakSettings(*LOOSE))
    whole = run(eng)
    assert whole[3]["n_rows"] > 20 * n and (whole[2] == -1).any()
    resident = eng.run_trace_rows(n, seed=seed, first_event=first, fetch=False)
    assert resident["trace_rows"] == whole[3] and resident["stats"]["n_points"] == whole[3]["n_rows"]
    small = _engine(inp, ctx, chunk_events=16)
    small.configure_traces(inp.config, **kw)
    small.configure_peaks(PeakSettings(*LOOSE))
    _assert_same(run(small), whole, "chunk_events 16")
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    a, b = run(eng, 0, 17), run(eng, 17, n)
    np.testing.assert_array_equal(np.concatenate([a[0], a[0][-1] + b[0][1:]]), whole[0])
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), whole[1])
    np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), whole[2])
    assert a[3]["n_rows"] + b[3]["n_rows"] == whole[3]["n_rows"]
    assert (a[3]["row_checksum"] + b[3]["row_checksum"]) % (1 << 64) == whole[3]["row_checksum"]
    # a capacity that is too small is reported with the rows needed, and the retry delivers the same rows
    from attpc_engine_amd.outputs import RowArrays

    arrays, stats = RowArrays(n, 8, width=8), _abi.RunStats()
    status = ctx.lib.attpc_sim_run_trace_rows(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats)
    assert status == _abi.E_CAPACITY and stats.n_points == whole[3]["n_rows"] == ctx.trace_rows_last()["n_rows"]
    assert whole[3]["n_rows"] > 1024  # (run_trace_rows below starts at 1024 rows and has to ask again)
    tight = eng.run_trace_rows(n, seed=seed, first_event=first, capacity_per_event=1)
    _assert_same((tight["offsets"], tight["rows"], tight["labels"], tight["trace_rows"]), whole, "capacity retry")
    _reset(ctx, inp.config)


def test_empty_events_and_a_layout_without_simulated_nuclei(ctx):
    import ctypes

    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    mask = np.zeros(_abi.NUM_PADS, dtype=bool)
    mask[::9] = True
    ped = _pedestals(5)
    kw = {"threshold": 6.0, "offset": 0, "noise_sigma": 2.0, "pedestals": ped, "readout": "partial", "readout_pads": mask}
    pk = Peaks(separation=10.0, prominence=3.0, min_width=0.5, max_width=50.0, rel_height=0.8, threshold=5.0)
    eng.configure_traces(inp.config, **kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings(*pk))
    geo = Geometry.of(inp.config)
    # a host cloud with empty events between full ones
    rows = np.array([[18.0, 100.5, 3.0e6], [27.0, 300.2, 5.0e6]])
    offsets = np.array([0, 0, 1, 1, 2, 2])
    labels = np.array([3, 4])
    seed, first = 77, (1 << 32) - 2
    got = clouds_to_trace_rows(offsets, rows, labels, ctx, seed=seed, first_event=first)
    tr = clouds_to_traces(offsets, rows, labels, ctx, seed=seed, first_event=first)
    _assert_same(got, trace_rows(tr[0], tr[1], tr[2], tr[3], pk, geo, seed, first, ped), "host cloud")
    assert (np.diff(got[0]) > 0).all() and (got[2] == -1).any() and {3, 4} <= set(got[2].tolist())
    # a layout with n_sim = 0 scatters nothing: every event still gets the points of its noise-only rows
    layout = _abi.EventLayout()
    ctypes.pointer(layout)[0] = eng.layout
    layout.n_sim = 0
    n = 5
    from attpc_engine_amd.outputs import RowArrays

    arrays, stats = RowArrays(n, 1 << 16, width=8), _abi.RunStats()
    ctx.check(ctx.lib.attpc_sim_run_trace_rows(ctx.handle, seed, first, n, layout, None, None, None, arrays.out, stats),
              "attpc_sim_run_trace_rows")
    empty = (np.zeros(n + 1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    tr = clouds_to_traces(*empty, ctx, seed=seed, first_event=first)
    ref = trace_rows(tr[0], tr[1], tr[2], tr[3], pk, geo, seed, first, ped)
    _assert_same((*arrays.result(), ctx.trace_rows_last()), ref, "no simulated nuclei")
    assert ref[3]["n_rows"] > 0 and (arrays.result()[2] == -1).all() and (arrays.event_points == 0).all()
    assert stats.n_points == ref[3]["n_rows"]
    _reset(ctx, inp.config)


def test_every_other_output_is_unchanged_beside_trace_row_runs():
    inp = Inputs("o16aa")
    kw = {"threshold": 20.0, "noise_sigma": 5.0, "pedestals": _pedestals(9), "readout": "partial"}

    def outputs(eng):
        cloud = eng.run(40, seed=2, first_event=3)["stats"]
        spyral = eng.run_spyral(40, seed=2, first_event=3)
        traces = eng.run_traces(40, seed=2, first_event=3, fetch=False)["trace"]
        fetched = eng.run_traces(6, seed=2, first_event=3)
        return ({k: cloud[k] for k in ("n_points", "charge_checksum", "key_checksum")}, spyral["offsets"].tolist(),
                float(spyral["rows"].sum()), spyral["stats"]["n_points"], traces, fetched["samples"].tobytes(),
                fetched["pads"].tolist(), fetched["labels"].tolist())

    fresh = _abi.Context(0)
    try:
        eng = _engine(inp, fresh)
        eng.configure_traces(inp.config, **kw)
        eng.configure_spyral(inp.config)
        before = outputs(eng)
        eng.configure_peaks(PeakSettings(*LOOSE))
        assert outputs(eng) == before  # peaks configured but not asked for
        assert eng.run_trace_rows(8, seed=2, first_event=3)["trace_rows"]["n_rows"] > 0
        eng.run_trace_rows(40, seed=2, first_event=3, fetch=False)
        assert outputs(eng) == before
    finally:
        fresh.close()


def test_entry_points_refuse_what_is_not_configured():
    inp = Inputs("be10dp")
    fresh = _abi.Context(0)
    try:
        eng = _engine(inp, fresh)
        out, stats = _abi.CloudOut(), _abi.RunStats()

        def call():
            return fresh.lib.attpc_sim_run_trace_rows(fresh.handle, 1, 0, 2, eng.layout, None, None, None, out, stats)

        assert call() == _abi.E_INVALID  # no trace settings
        eng.configure_traces(inp.config)
        assert call() == _abi.E_INVALID  # no Spyral geometry
        eng.configure_spyral(inp.config)
        assert call() == _abi.E_NOTCONFIGURED  # no peak parameters
        for bad in ((0.5, 20, 1, 50, 0.95, 40), (50, -1, 1, 50, 0.95, 40), (50, 20, 5, 4, 0.95, 40), (50, 20, 1, 50, 0.0, 40),
                    (50, 20, 1, 50, 1.5, 40), (50, 20, 1, 50, 0.95, float("nan"))):
            assert fresh.lib.attpc_trace_configure_peaks(fresh.handle, _abi.PeakDesc(*bad)) == _abi.E_INVALID
        eng.configure_peaks()
        assert call() == _abi.OK and stats.n_points == fresh.trace_rows_last()["n_rows"]
        # a geometry with fewer pads than the traces can name is refused, not looked up out of range
        from attpc_engine_amd.detector.simulator import configure_spyral

        resp = np.ascontiguousarray(get_response(inp.config))
        centers = np.ascontiguousarray(inp.config.pad_centers[:5000], dtype=np.float64)
        sizes = np.ascontiguousarray(inp.config.pad_sizes[:5000], dtype=np.float64)
        small = _abi.SpyralDesc(_abi.dptr(resp), _abi.dptr(centers), _abi.dptr(sizes), 5000,
                                int(inp.config.elec_params.windows_edge), int(inp.config.elec_params.micromegas_edge), 0,
                                float(inp.config.det_params.length), 40.0)
        assert fresh.lib.attpc_spyral_configure(fresh.handle, small) == _abi.OK
        assert call() == _abi.E_INVALID
        fresh.forget("spyral")
        configure_spyral(inp.config, fresh)
        assert call() == _abi.OK
        assert fresh.lib.attpc_trace_configure_peaks(fresh.handle, None) == _abi.OK  # off again
        assert call() == _abi.E_NOTCONFIGURED
    finally:
        fresh.close()


def test_a_lone_arrival_is_one_point_on_its_pad_and_bucket(ctx):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    r_max, at = float(resp.max()), int(np.argmax(resp))
    configure_trace_rows(inp.config, ctx, PeakSettings(), response=resp, threshold=40.0, offset=at)
    cases = [(5, 100, 50.0 / r_max), (77, 3, 4000.0 / r_max), (10239, 480, 333.3 / r_max), (4000, 250, 2.0e6),
             (1234, 17, 1.0e8), (9, 300, 41.0 / r_max)]
    for i, (pad, t, q) in enumerate(cases):
        assert 40.0 < q * r_max <= 4094.0
        got = clouds_to_trace_rows(np.array([0, 1]), np.array([[float(pad), t + 0.37, q]]), np.array([6]), ctx, seed=5,
                                   first_event=i)
        assert got[0].tolist() == [0, 1] and got[2].tolist() == [6], (pad, t, q)
        row = got[1][0]
        assert row[5] == pad and t <= row[6] < t + 1 and row[3] == np.rint(q * r_max), (pad, t, q, row)
    _reset(ctx, inp.config)


def _read_spyral_files(directory):
    """{event: (rows, labels)} and {file name: (min_event, max_event)} of a SpyralWriter's .npz files."""
    events, files = {}, {}
    for path in sorted(directory.iterdir()):
        f = np.load(path)
        files[path.name] = (int(f["cloud@min_event"]), int(f["cloud@max_event"]))
        for key in f.files:
            if key.startswith("cloud/cloud_") and "@" not in key:
                e = int(key.rsplit("_", 1)[1])
                events[e] = (f[key], f[f"cloud/labels_{e}"])
    return events, files


def test_writers_write_the_rows_of_run_trace_rows(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from numpy.random import default_rng

    from attpc_engine_amd.detector import SpyralWriter, run_simulation
    from attpc_engine_amd.engine import run_fused
    from attpc_engine_amd.io import KinematicsFileWriter

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n, seed = 24, 17
    kw = {"noise_sigma": 4.0, "pedestals": _pedestals(12), "noise_stream": 9, "offset": 7}
    peaks = PeakSettings(*LOOSE)
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_peaks(peaks)

    def check(directory, plain_directory, res):
        got, files = _read_spyral_files(directory)
        want = [e for e in range(n) if res["event_points"][e] > 0]
        assert sorted(got) == want
        for e in want:
            lo, hi = res["offsets"][e], res["offsets"][e + 1]
            np.testing.assert_array_equal(got[e][0], res["rows"][lo:hi])
            np.testing.assert_array_equal(got[e][1], res["labels"][lo:hi])
        plain, plain_files = _read_spyral_files(plain_directory)
        assert files == plain_files and sorted(plain) == want and len(files) > 1  # rolled over at the same events

    res = eng.run_trace_rows(n, seed=seed, first_event=0)
    dirs = {name: tmp_path / name for name in ("fused", "fused_plain", "sim", "sim_plain", "one")}
    for d in dirs.values():
        d.mkdir()
    run_fused(inp.pipeline, inp.config, SpyralWriter(dirs["fused"], inp.config, max_events_per_file=10, peaks=peaks, **kw),
              n, inp.indices, seed=seed, batch_size=7, context=ctx)
    run_fused(inp.pipeline, inp.config, SpyralWriter(dirs["fused_plain"], inp.config, max_events_per_file=10), n,
              inp.indices, seed=seed, batch_size=7, context=ctx)
    check(dirs["fused"], dirs["fused_plain"], res)

    kin_path = tmp_path / "kine.npz"
    w = KinematicsFileWriter(kin_path, n, inp.z, inp.a, 16)
    w.write_batch(0, res["vertex"], res["p4"])
    w.close()
    run_simulation(inp.config, kin_path, SpyralWriter(dirs["sim"], inp.config, max_events_per_file=10, peaks=peaks, **kw),
                   inp.indices, batch_size=7, seed=99)
    run_simulation(inp.config, kin_path, SpyralWriter(dirs["sim_plain"], inp.config, max_events_per_file=10),
                   inp.indices, batch_size=7, seed=99)
    run_seed = int(default_rng(99).integers(0, 1 << 63))
    off, rows, labels, raw, _ = simulate_batch_trace_rows(res["p4"], res["vertex"], inp.z, inp.a, inp.config, run_seed,
                                                          inp.indices, ctx=ctx, peaks=peaks, **kw)
    check(dirs["sim"], dirs["sim_plain"], {"offsets": off, "rows": rows, "labels": labels, "event_points": raw})

    # the per-event write() path: draws keyed on (noise_seed, event_number)
    cloud = eng.run(n, seed=seed, first_event=0, fetch=True)
    lo, hi = cloud["offsets"][3], cloud["offsets"][4]
    w = SpyralWriter(dirs["one"], inp.config, peaks=peaks, noise_seed=SEED_HI, **kw)
    w.write(cloud["points"][lo:hi], cloud["labels"][lo:hi], inp.config, 1 << 40)
    w.close()
    configure_trace_rows(inp.config, ctx, peaks, **kw)
    want = clouds_to_trace_rows(np.array([0, hi - lo]), cloud["points"][lo:hi], cloud["labels"][lo:hi], ctx, seed=SEED_HI,
                                first_event=1 << 40)
    got = _read_spyral_files(dirs["one"])[0][1 << 40]
    np.testing.assert_array_equal(got[0], want[1])
    np.testing.assert_array_equal(got[1], want[2])
    assert len(want[1]) > 0
    _reset(ctx, inp.config)
