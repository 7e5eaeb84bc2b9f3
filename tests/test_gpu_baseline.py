"""The Fourier baseline of the trace rows on the device (include/attpc_engine.h, "Fourier baseline") against its numpy
restatement (tests/baseline_reference.py).  The stage alone (``remove_baseline``): generated rows at three window
scales, y equal except where the baseline lies within 1e-6 of a half-integer (there |dy| <= 1, and such samples are
capped at 1e-4 of all), the f64 baseline within 1e-8; edge rows; a row's result bit for bit whatever shares its call.
The fused path: exactly the peak restatement (tests/peaks_reference.py) applied to the device's own y; chunk invariance;
nothing else moves; a wide pulse loses amplitude and a lone arrival does not; the writers.  Needs a real MI355X:
``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (BaselineSettings, PeakSettings, clouds_to_trace_rows, clouds_to_traces,
                                              configure_baseline, configure_trace_rows, configure_traces,
                                              remove_baseline, simulate_batch_trace_rows)
from tests import baseline_reference as ref
from tests.helpers import Inputs
from tests.peaks_reference import Geometry, Peaks, trace_points, trace_rows

pytestmark = pytest.mark.gpu

SCALES = (5.0, 20.0, 100.0)
AMBIGUOUS_CAP = 1.0e-4   # of all samples (the contract's rule must stay an exception)
BASELINE_TOL = 1.0e-8    # 10x the forward-error bound of two 512-point f64 transforms of data below 4095
NOISY = {"noise_sigma": 5.0, "pedestals": "random", "threshold": 20.0, "readout": "partial"}


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def generated():
    x = ref.mixed_rows(2000, seed=101)
    x.setflags(write=False)
    return x


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine
    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _pedestals(seed):
    return np.random.default_rng(seed).integers(0, 1500, size=_abi.NUM_PADS).astype(np.int16)


def _trace_kwargs(inp, kw):
    kw = dict(kw)
    if kw.get("pedestals") == "random":
        kw["pedestals"] = _pedestals(3)
    kw.setdefault("offset", int(np.argmax(get_response(inp.config))))
    return kw


def _reset(ctx, config):
    configure_traces(config, ctx, None, None, 0)
    configure_baseline(ctx, None)


def _assert_operator_equals_restatement(x, scale, ctx, what=""):
    """-> (ambiguous samples, max |baseline difference|) after the contract's comparison."""
    y, baseline = remove_baseline(x, scale, ctx, return_baseline=True)
    want_y, want_baseline, _ = ref.remove(x, scale)
    assert y.dtype == np.int16 and y.shape == want_y.shape and baseline.shape == want_baseline.shape
    loose = ref.ambiguous(want_baseline)
    dy = y.astype(np.int64) - want_y
    worst = float(np.abs(baseline - want_baseline).max()) if baseline.size else 0.0
    print(f"{what} scale {scale}: {int(loose.sum())} ambiguous of {loose.size} samples, "
          f"{int((dy != 0).sum())} of them differ, max |baseline - numpy| = {worst:.3e}")
    assert not dy[~loose].any(), (what, scale, np.argwhere((dy != 0) & ~loose)[:5].tolist())
    assert (np.abs(dy[loose]) <= 1).all(), (what, scale)
    assert loose.sum() <= AMBIGUOUS_CAP * loose.size, (what, scale, int(loose.sum()))
    assert worst <= BASELINE_TOL, (what, scale, worst)
    return int(loose.sum()), worst


@pytest.mark.parametrize("scale", SCALES)
def test_operator_against_restatement(ctx, generated, scale):
    """Measured on an MI355X (2 000 rows = 1 024 000 samples a scale): max |baseline - numpy| 2.3e-13 at scale 5 and
    4.5e-13 at 20 and 100; 1 ambiguous sample at every scale, y equal there too."""
    _assert_operator_equals_restatement(generated, scale, ctx, "generated rows")
    y_only = remove_baseline(generated[:7], scale, ctx)
    np.testing.assert_array_equal(y_only, remove_baseline(generated[:7], scale, ctx, return_baseline=True)[0])


def _edge_rows():
    rows, names = [], []

    def add(name, row):
        names.append(name)
        rows.append(np.asarray(row, dtype=np.int16))

    add("all zero", np.zeros(512))
    add("all 4095", np.full(512, 4095))
    add("constant 300", np.full(512, 300))
    for at in (0, 1, 255, 510, 511):
        for floor in (0, 300):
            spike = np.full(512, floor)
            spike[at] = 4095
            add(f"spike at {at} on {floor}", spike)
    for duty, width in (("10 %", 51), ("50 %", 256)):
        square = np.full(512, 300)
        square[128:128 + width] = 1300
        add(f"{duty} duty square pulse", square)
    single = 300 + (np.arange(512) % 3)  # a ripple far below 1.5 std once the spike is in
    single[77] = 2000
    add("one masked sample", single)
    return names, np.stack(rows)


def test_edge_rows(ctx):
    names, x = _edge_rows()
    _, _, mask = ref.remove(x, 20.0)
    counts = dict(zip(names, mask.sum(axis=1).tolist()))
    assert counts["10 % duty square pulse"] == 51 and counts["50 % duty square pulse"] == 0
    assert counts["one masked sample"] == 1 and counts["spike at 255 on 300"] == 1
    assert counts["spike at 0 on 0"] == 0 and counts["spike at 1 on 0"] == 2  # the edge fix: gone / doubled
    for scale in SCALES:
        loose, _ = _assert_operator_equals_restatement(x, scale, ctx, "edge rows")
        assert loose == 0  # (nothing here sits on a half-integer: the rows are equal outright)
    y = remove_baseline(x, 20.0, ctx)
    assert not y[:3].any()
    assert y[names.index("spike at 255 on 300"), 255] == 4095 - 300
    assert not y[names.index("spike at 511 on 300")].any()


def test_purity(ctx, generated):
    """A row's y and baseline are the same bits at positions 0, 1 and last of calls of 1 .. 1000 rows (and of one
    call longer than the operator's chunk), whatever the other rows are."""
    own = np.concatenate([generated[[3, 700, 1200, 1900]], _edge_rows()[1][-2:-1]])  # 5 rows: every kind + a square pulse
    assert len(own) == 5
    alone = [remove_baseline(own[i:i + 1], 20.0, ctx, return_baseline=True) for i in range(5)]
    for n in (1, 5, 63, 64, 65, 1000, 16385):
        filler = np.resize(generated[::-1], (n, 512)) if n > len(generated) else generated[::-1][:n]
        for i in range(5 if n <= 1000 else 1):
            x = filler.copy()
            places = sorted({0, min(1, n - 1), n - 1})
            x[places] = own[i]
            y, baseline = remove_baseline(x, 20.0, ctx, return_baseline=True)
            for p in places:
                assert y[p].tobytes() == alone[i][0][0].tobytes(), (n, i, p)
                assert baseline[p].tobytes() == alone[i][1][0].tobytes(), (n, i, p)
    y, baseline = remove_baseline(np.zeros((0, 512), dtype=np.int16), 20.0, ctx, return_baseline=True)
    assert y.shape == (0, 512) and baseline.shape == (0, 512)
    assert ctx.lib.attpc_trace_baseline(ctx.handle, 0, None, 20.0, None, None) == _abi.OK


def test_operator_refuses_bad_input(ctx):
    i16 = _abi.C.c_int16
    x = np.zeros((2, 512), dtype=np.int16)
    y = np.empty_like(x)
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        assert ctx.lib.attpc_trace_baseline(ctx.handle, 2, _abi.iptr(x, i16), bad, _abi.iptr(y, i16), None) == _abi.E_INVALID
        assert ctx.lib.attpc_trace_configure_baseline(ctx.handle, _abi.BaselineDesc(bad)) == _abi.E_INVALID
    for sample in (-1, 4096):
        x[1, 500] = sample
        assert ctx.lib.attpc_trace_baseline(ctx.handle, 2, _abi.iptr(x, i16), 20.0, _abi.iptr(y, i16), None) == _abi.E_INVALID
    assert ctx.lib.attpc_trace_baseline(ctx.handle, -1, _abi.iptr(x, i16), 20.0, _abi.iptr(y, i16), None) == _abi.E_INVALID


def _possible(offsets, pads, y, labels, pk):
    """The trace rows in CSR form without those that cannot hold a point: a point needs y[k] > threshold (step 6 of the
    trace-row contract), so a row whose largest sample is not above it gives none.  (The restatement walks every
    candidate of a row in Python; most noise-only rows of a partial readout end here.)"""
    keep = y.max(axis=1) > pk.threshold if len(y) else np.zeros(0, dtype=bool)
    return np.concatenate([[0], np.cumsum(keep)])[np.asarray(offsets)], pads[keep], y[keep], labels[keep]


def _assert_same(got, want, what=""):
    """(offsets, rows, labels, sums): identical in every column."""
    np.testing.assert_array_equal(np.asarray(got[0]), np.asarray(want[0]), err_msg=f"{what} offsets")
    assert np.asarray(got[1]).shape == np.asarray(want[1]).shape, what
    for col, name in enumerate(("x", "y", "z", "amplitude", "integral", "pad", "centroid", "pad scale")):
        np.testing.assert_array_equal(np.asarray(got[1])[:, col], np.asarray(want[1])[:, col], err_msg=f"{what} {name}")
    np.testing.assert_array_equal(np.asarray(got[2]), np.asarray(want[2]), err_msg=f"{what} labels")
    assert got[3] == want[3], (what, got[3], want[3])


@pytest.mark.parametrize("name,mode", [("o16aa", "noisy"), ("be10dp", "noisy"), ("o16aa", "hit")])
def test_fused_path_is_exact_given_y(ctx, name, mode):
    inp = Inputs(name)
    kw = _trace_kwargs(inp, NOISY if mode == "noisy" else {})
    n, seed, first, scale = 64, 21, 7, BaselineSettings().window_scale
    pk, geo = Peaks(), Geometry.of(inp.config)
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings(*pk))
    plain = eng.run_trace_rows(n, seed=seed, first_event=first)
    eng.configure_baseline(BaselineSettings())
    tr = eng.run_traces(n, seed=seed, first_event=first)
    y = remove_baseline(tr["samples"], scale, ctx)
    want = trace_rows(*_possible(tr["offsets"], tr["pads"], y, tr["labels"], pk), pk, geo, seed, first, None)
    res = eng.run_trace_rows(n, seed=seed, first_event=first)
    got = (res["offsets"], res["rows"], res["labels"], res["trace_rows"])
    _assert_same(got, want, "fused")
    assert got[3]["n_rows"] > 0 and res["stats"]["n_points"] == got[3]["n_rows"]
    np.testing.assert_array_equal(res["event_points"], tr["event_points"])
    # (the stage is really on: pedestal subtraction gives other rows)
    assert plain["trace_rows"] != got[3] or not np.array_equal(plain["rows"], got[1])
    resident = eng.run_trace_rows(n, seed=seed, first_event=first, fetch=False)
    assert resident["trace_rows"] == got[3]
    # the file-driven entry point, and a host cloud of the first events
    off, rows, labels, raw, stats = simulate_batch_trace_rows(
        res["p4"], res["vertex"], inp.z, inp.a, inp.config, seed, inp.indices, first_event=first, ctx=ctx,
        peaks=PeakSettings(*pk), baseline=BaselineSettings(), **kw)
    _assert_same((off, rows, labels, {k: stats[k] for k in ("n_rows", "row_checksum")}), got, "file-driven")
    few = 6
    cloud = eng.run(few, seed=seed, first_event=first, fetch=True)
    configure_trace_rows(inp.config, ctx, PeakSettings(*pk), BaselineSettings(), **kw)
    host = clouds_to_trace_rows(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed, first_event=first)
    htr = clouds_to_traces(cloud["offsets"], cloud["points"], cloud["labels"], ctx, seed=seed, first_event=first)
    hy = remove_baseline(htr[2], scale, ctx)
    want = trace_rows(htr[0], htr[1], hy, htr[3], pk, geo, seed, first, None)  # every row, nothing left out
    _assert_same(host, want, "host cloud")
    # ... which also checks the shortcut of _possible: the rows it drops give no row, offset or checksum term
    kept = _possible(htr[0], htr[1], hy, htr[3], pk)
    assert len(kept[1]) < len(htr[1]) or mode == "hit"
    _assert_same(trace_rows(*kept, pk, geo, seed, first, None), want, "rows that cannot hold a point")
    assert host[3]["n_rows"] > 0
    _reset(ctx, inp.config)


def test_chunk_invariance(ctx):
    inp = Inputs("o16aa")
    kw = _trace_kwargs(inp, NOISY)
    seed, first, n = 5, (1 << 32) - 150, 300  # the events cross the low word
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_peaks()
    eng.configure_baseline(window_scale=20.0)

    def run(e, lo, hi):
        res = e.run_trace_rows(hi - lo, seed=seed, first_event=first + lo)
        return res["offsets"], res["rows"], res["labels"], res["trace_rows"]

    whole = run(eng, 0, n)
    parts = [run(eng, lo, lo + 100) for lo in (0, 100, 200)]
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    np.testing.assert_array_equal(np.concatenate([p[2] for p in parts]), whole[2])
    np.testing.assert_array_equal(np.cumsum([0] + [c for p in parts for c in np.diff(p[0]).tolist()]), whole[0])
    assert sum(p[3]["n_rows"] for p in parts) == whole[3]["n_rows"] > 0
    assert sum(p[3]["row_checksum"] for p in parts) % (1 << 64) == whole[3]["row_checksum"]
    small = _engine(inp, ctx, chunk_events=64)
    small.configure_traces(inp.config, **kw)
    small.configure_peaks()
    _assert_same(run(small, 0, n), whole, "chunk_events 64")
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    _reset(ctx, inp.config)


def test_nothing_else_moves():
    inp = Inputs("o16aa")
    kw = _trace_kwargs(inp, NOISY)

    def outputs(eng, rows=True):
        cloud = eng.run(40, seed=2, first_event=3)["stats"]
        spyral = eng.run_spyral(40, seed=2, first_event=3)
        traces = eng.run_traces(40, seed=2, first_event=3, fetch=False)["trace"]
        fetched = eng.run_traces(6, seed=2, first_event=3)
        out = ({k: cloud[k] for k in ("n_points", "charge_checksum", "key_checksum")}, spyral["offsets"].tolist(),
               float(spyral["rows"].sum()), spyral["stats"]["n_points"], traces, fetched["samples"].tobytes(),
               fetched["pads"].tolist(), fetched["labels"].tolist())
        if rows:
            res = eng.run_trace_rows(40, seed=2, first_event=3)
            out += (res["trace_rows"], res["rows"].tobytes(), res["labels"].tolist(), res["offsets"].tolist())
        return out

    fresh = _abi.Context(0)
    try:
        eng = _engine(inp, fresh)
        eng.configure_traces(inp.config, **kw)
        eng.configure_spyral(inp.config)
        eng.configure_peaks()
        before = outputs(eng)
        eng.configure_baseline(BaselineSettings())
        assert outputs(eng, rows=False) == before[:8]  # on: the traces and the cloud outputs are what they were
        on = eng.run_trace_rows(40, seed=2, first_event=3)
        assert on["rows"].tobytes() != before[9]
        eng.run_trace_rows(40, seed=2, first_event=3, fetch=False)
        eng.configure_baseline(None)
        assert outputs(eng) == before  # off again: everything, trace rows included
        # off through the C ABI, and on again with another scale: no call resets another
        assert fresh.lib.attpc_trace_configure_baseline(fresh.handle, _abi.BaselineDesc(50.0)) == _abi.OK
        other = eng.run_trace_rows(40, seed=2, first_event=3)
        assert other["rows"].tobytes() not in (before[9], on["rows"].tobytes())
        assert fresh.lib.attpc_trace_configure_baseline(fresh.handle, None) == _abi.OK
        assert outputs(eng) == before
    finally:
        fresh.close()


WIDE = Peaks(separation=512.0, prominence=1.0, min_width=0.0, max_width=512.0, rel_height=0.5, threshold=10.0)


def test_a_wide_pulse_loses_amplitude_and_a_lone_arrival_does_not(ctx):
    inp = Inputs("o16aa")
    resp = get_response(inp.config)
    r_max, at = float(resp.max()), int(np.argmax(resp))
    wide_pad, lone_pad, ped = 1200, 4321, 300
    t = np.arange(150)
    points = np.concatenate([np.column_stack([np.full(150, float(wide_pad)), 150.0 + t + 0.5, (40.0 + 0.2 * t) / r_max]),
                             [[float(lone_pad), 250.5, 1000.0 / r_max]]])
    offsets, labels = np.array([0, len(points)]), np.zeros(len(points), dtype=np.int64)
    kw = {"response": resp, "threshold": 20.0, "offset": at, "pedestals": ped}
    seed, first = 9, 4

    def amplitudes(baseline):
        configure_trace_rows(inp.config, ctx, PeakSettings(*WIDE), baseline, **kw)
        _, rows, _, sums = clouds_to_trace_rows(offsets, points, labels, ctx, seed=seed, first_event=first)
        assert sums["n_rows"] == 2 and sorted(rows[:, 5].tolist()) == [wide_pad, lone_pad], rows
        return {int(r[5]): int(r[3]) for r in rows}

    plain, fitted = amplitudes(None), amplitudes(BaselineSettings())
    tr = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
    assert tr[1].tolist() == [wide_pad, lone_pad]
    y, _, _ = ref.remove(tr[2], 20.0)
    want = {pad: max(p[1] for p in trace_points(y[i].astype(np.int64), WIDE)) for i, pad in enumerate(tr[1].tolist())}
    print(f"wide pad: {plain[wide_pad]} above the pedestal, {fitted[wide_pad]} above the fitted baseline; "
          f"lone arrival: {plain[lone_pad]} and {fitted[lone_pad]}")
    assert fitted == want
    assert plain[lone_pad] == 1000 and plain[wide_pad] == int(tr[2][0].max()) - ped
    assert fitted[wide_pad] < 0.9 * plain[wide_pad]
    assert abs(fitted[lone_pad] - plain[lone_pad]) <= 0.05 * plain[lone_pad]
    _reset(ctx, inp.config)


def _read_spyral_files(directory):
    events = {}
    for path in sorted(directory.iterdir()):
        f = np.load(path)
        for key in f.files:
            if key.startswith("cloud/cloud_") and "@" not in key:
                e = int(key.rsplit("_", 1)[1])
                events[e] = (f[key], f[f"cloud/labels_{e}"])
    return events


def test_writers_write_the_rows_of_run_trace_rows(ctx, tmp_path, monkeypatch):
    import sys
    import warnings

    from attpc_engine_amd.detector import SpyralWriter
    from attpc_engine_amd.engine import run_fused

    monkeypatch.setitem(sys.modules, "h5py", None)
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    warnings.simplefilter("ignore", RuntimeWarning)
    inp = Inputs("be10dp")
    n, seed = 24, 17
    kw = {"noise_sigma": 4.0, "pedestals": _pedestals(12), "noise_stream": 9, "offset": 7}
    peaks, baseline = PeakSettings(), BaselineSettings()
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, **kw)
    eng.configure_peaks(peaks)
    plain = eng.run_trace_rows(n, seed=seed, first_event=0)
    eng.configure_baseline(baseline)
    res = eng.run_trace_rows(n, seed=seed, first_event=0)
    assert res["rows"].tobytes() != plain["rows"].tobytes()
    for name in ("fitted", "plain"):
        (tmp_path / name).mkdir()
    run_fused(inp.pipeline, inp.config, SpyralWriter(tmp_path / "fitted", inp.config, max_events_per_file=10, peaks=peaks,
                                                     baseline=baseline, **kw), n, inp.indices, seed=seed, batch_size=7,
              context=ctx)
    # ... and a writer without baseline= turns the stage off again on the same context
    run_fused(inp.pipeline, inp.config, SpyralWriter(tmp_path / "plain", inp.config, max_events_per_file=10, peaks=peaks,
                                                     **kw), n, inp.indices, seed=seed, batch_size=7, context=ctx)
    for name, run in (("fitted", res), ("plain", plain)):
        got = _read_spyral_files(tmp_path / name)
        want = [e for e in range(n) if run["event_points"][e] > 0]
        assert sorted(got) == want and want, name
        for e in want:
            lo, hi = run["offsets"][e], run["offsets"][e + 1]
            np.testing.assert_array_equal(got[e][0], run["rows"][lo:hi], err_msg=name)
            np.testing.assert_array_equal(got[e][1], run["labels"][lo:hi], err_msg=name)
    # the per-event write() path
    cloud = eng.run(n, seed=seed, first_event=0, fetch=True)
    lo, hi = cloud["offsets"][3], cloud["offsets"][4]
    (tmp_path / "one").mkdir()
    w = SpyralWriter(tmp_path / "one", inp.config, peaks=peaks, baseline=baseline, noise_seed=31, **kw)
    w.write(cloud["points"][lo:hi], cloud["labels"][lo:hi], inp.config, 12)
    w.close()
    configure_trace_rows(inp.config, ctx, peaks, baseline, **kw)
    want = clouds_to_trace_rows(np.array([0, hi - lo]), cloud["points"][lo:hi], cloud["labels"][lo:hi], ctx, seed=31,
                                first_event=12)
    got = _read_spyral_files(tmp_path / "one")[12]
    np.testing.assert_array_equal(got[0], want[1])
    np.testing.assert_array_equal(got[1], want[2])
    assert len(want[1]) > 0
    _reset(ctx, inp.config)
