"""The common-mode noise of the pad traces on the device (include/attpc_engine.h, "common-mode noise of the traces")
against its numpy restatement (tests/common_mode_reference.py), every comparison exact: the stage alone
(``common_mode_values``), hit mode on hand-made clouds, partial and full readout where only the common-mode term can
cross the threshold, the fused pipeline against the restatement of its own cloud, in chunks and split, off is off, and
the trigger and the trace rows on the delivered traces -- with the case the stage exists for: a multiplicity trigger
that fires on empty events through coherent noise alone.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import (CommonModeSettings, PeakSettings, TriggerSettings, clouds_to_traces,
                                              common_mode_values, configure_common_mode, configure_traces,
                                              configure_trigger, gaussian_noise_table)
from tests import common_mode_reference as cmr
from tests.helpers import ID_CASE_IDS, ID_CASES, Inputs, sort_cloud
from tests.trace_noise_reference import Noise

pytestmark = pytest.mark.gpu

NUM_TB, NUM_PADS = _abi.NUM_TB, _abi.NUM_PADS
SEED_HI = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _assert_traces(got, want, what=""):
    """(offsets, pads, samples, labels, sums) of the device and of the restatement: identical."""
    for k, name in enumerate(("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=f"{what} {name}")
    assert got[4] == want[4], (what, got[4], want[4])


def _traces_of(res):
    return res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"]


def _pedestals(seed=3):
    ped = np.random.default_rng(seed).integers(200, 401, size=NUM_PADS).astype(np.int16)
    ped[[0, 7]] = 0
    ped[[6, 10239]] = 4095
    return ped


def _groups_of(n_groups):
    """None for one group; else a map over 0 .. n_groups - 1 with every group in use and pads of group 255 among them."""
    if n_groups == 1:
        return None
    g = (np.arange(NUM_PADS) * 7 % n_groups).astype(np.uint8)
    g[5::11] = 255
    g[0], g[10239] = 0, n_groups - 1
    return g


def _reference(cm: CommonModeSettings):
    return cmr.CommonMode((cm.cdf, cm.min_level), cm.groups, cm.stream)


# ---------------------------------------------------------------- 1. the stage alone ----
@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_values_alone_equal_the_restatement(ctx, case):
    first, n = case.first_event + 18, 4  # the four events cross the case's power of two
    seen = []
    for n_groups in (1, 3, 255):
        for stream in (0, (1 << 29) - 1):
            cm = CommonModeSettings(sigma=3.0, groups=_groups_of(n_groups), stream=stream)
            assert cm.n_groups == n_groups
            got = common_mode_values(n, cm, seed=case.seed, first_event=first, ctx=ctx)
            assert got.shape == (n, n_groups, NUM_TB) and got.dtype == np.int16
            ref = _reference(cm)
            want = np.stack([ref.all_values(case.seed, first + e) for e in range(n)])
            np.testing.assert_array_equal(got, want, err_msg=f"{case} groups {n_groups} stream {stream}")
            seen.append(got[:, 0])
    assert (seen[0] != seen[1]).mean() > 0.5  # the streams differ
    np.testing.assert_array_equal(seen[0], seen[2])  # group 0 does not depend on how many groups there are
    # events asked for alone: event i of a call is the global event first_event + i
    cm = CommonModeSettings(sigma=3.0, groups=_groups_of(3))
    whole = common_mode_values(n, cm, seed=case.seed, first_event=first, ctx=ctx)
    np.testing.assert_array_equal(common_mode_values(2, cm, seed=case.seed, first_event=first + 2, ctx=ctx), whole[2:])
    configure_common_mode(ctx, None)


def test_the_library_validates_the_descriptor(ctx):
    cdf, lo = gaussian_noise_table(2.0)

    def configure(cdf=cdf, n_levels=len(cdf) + 1, min_level=lo, stream=0):
        cdf = None if cdf is None else np.ascontiguousarray(cdf, dtype=np.uint32)
        desc = _abi.TraceCommonDesc(None, _abi.iptr(cdf, _abi.C.c_uint32), n_levels, min_level, stream, 0)
        ctx.check(ctx.lib.attpc_trace_configure_common_mode(ctx.handle, desc), "attpc_trace_configure_common_mode")

    for bad in ({"cdf": cdf[::-1]}, {"n_levels": 513}, {"n_levels": -1}, {"min_level": 4096}, {"min_level": -4096},
                {"stream": 1 << 29}, {"cdf": None}):
        with pytest.raises(ValueError):
            configure(**bad)
    configure(stream=(1 << 29) - 1)
    out = np.zeros((1, 1, NUM_TB), dtype=np.int16)
    ctx.check(ctx.lib.attpc_common_mode_rows(ctx.handle, 1, 2, 1, _abi.iptr(out, _abi.C.c_int16)), "attpc_common_mode_rows")
    want = cmr.values(1, 2, [0], (cdf, lo), (1 << 29) - 1)
    np.testing.assert_array_equal(out[0], want)
    # the calls above went past the package's token: turn the stage off the same way, then the token is right again
    ctx.check(ctx.lib.attpc_trace_configure_common_mode(ctx.handle, None), "attpc_trace_configure_common_mode")
    ctx.forget("trace_common")
    with pytest.raises(RuntimeError):  # the stage alone needs the stage
        ctx.check(ctx.lib.attpc_common_mode_rows(ctx.handle, 1, 2, 1, _abi.iptr(out, _abi.C.c_int16)), "attpc_common_mode_rows")


# ---------------------------------------------------------------- 2. hit mode on hand-made clouds ----
def _box_response():
    resp = np.zeros(NUM_TB)
    resp[:24] = np.concatenate([np.linspace(0.1, 0.5, 12), np.linspace(0.5, 0.05, 12)])
    return resp


def _hand_groups():
    g = np.array([0, 254, 255], dtype=np.uint8)[np.arange(NUM_PADS) % 3]
    g[[0, 6, 300]] = 0
    g[[7, 10239]] = 254
    g[5] = 255
    return g


def _hand_cloud():
    """Three events, the middle one empty: pads 0 and 10 239, pedestals 0 and 4095 (``_pedestals``), groups 0, 254 and
    255, a pile-up, rows around the threshold 40 at R = 0.5, rows at both ends of the time axis."""
    ev0 = [[0, 0.0, 300.0], [10239, 511.99, 5000.0], [5, 40.5, 90.0], [6, 40.5, 90.0], [7, 40.5, 70.0], [8, 10.1, 1e5]]
    ev0 += [[300, 100.0 + 3 * k, 150.0 + k] for k in range(40)]
    ev2 = [[p, 20.0 + (p % 7), 60.0 + p % 40] for p in range(1000, 1060)]
    ev2 += [[2000, 200.5, 6000.0], [2000, 205.5, 6000.0], [0, 300.0, 1.0], [10239, 2.0, 81.0]]
    events = [ev0, [], ev2]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in events])])
    points = np.array([r for e in events for r in e], dtype=np.float64)
    labels = np.arange(len(points), dtype=np.int64) % 5
    return offsets, points, labels


HAND_NOISE = {
    "sigma1": lambda: (dict(noise_sigma=1.0, pedestals=_pedestals()), Noise(*gaussian_noise_table(1.0), pedestals=_pedestals())),
    "no_table": lambda: (dict(pedestals=_pedestals()), Noise(pedestals=_pedestals())),
    "never_configured": lambda: ({}, None),
}


@pytest.mark.parametrize("threshold", [-1.0, 0.0, 40.0])
@pytest.mark.parametrize("noise", list(HAND_NOISE))
def test_hit_mode_on_hand_made_clouds(ctx, noise, threshold):
    inp = Inputs("o16aa")
    kwargs, ref_noise = HAND_NOISE[noise]()
    resp, offset = _box_response(), 3
    offsets, points, labels = _hand_cloud()
    cm = CommonModeSettings(sigma=3.0, groups=_hand_groups(), stream=2)
    seed, first = SEED_HI, (1 << 32) - 2  # the events cross the low word
    configure_traces(inp.config, ctx, resp, threshold, offset, **kwargs)
    configure_common_mode(ctx, cm)
    try:
        got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
        want = cmr.traces(offsets, points, labels, resp, threshold, offset, ref_noise, _reference(cm), seed, first)
        _assert_traces(got, want, f"{noise}, threshold {threshold}")
        assert want[0][1] == want[0][2] and want[4]["n_rows"] > 20
        # the term is there: without it the restatement gives other samples
        plain = cmr.traces(offsets, points, labels, resp, threshold, offset, ref_noise, None, seed, first)
        assert plain[4]["sample_checksum"] != want[4]["sample_checksum"]
        if threshold < 0:  # every hit pad is kept either way: the pads of group 255 have the samples without the term
            none = _hand_groups()[want[1]] == 255
            assert none.any() and not none.all()
            np.testing.assert_array_equal(want[2][none], plain[2][none])
            assert (want[2][~none] != plain[2][~none]).any()
    finally:
        configure_common_mode(ctx, None)
        configure_traces(inp.config, ctx, None, None, 0)


# ---------------------------------------------------------------- 3. partial and full readout ----
def _readout_case():
    """96 pads of three groups (0, 1, 2; one pad of them in group 255), pad noise sigma 1 and thr 12 -- the pad table
    alone never crosses: its levels end at 8 --, common-mode sigma 3; three events, the middle one empty, one row on a
    pad outside the set.  The seed is searched for here, on the CPU: the restatement keeps at least one noise-only pad
    and drops at least one."""
    pads = np.concatenate([np.arange(64, 96), np.arange(4000, 4032), np.arange(10208, 10240)])
    groups = np.full(NUM_PADS, 255, dtype=np.uint8)
    groups[64:96], groups[4000:4032], groups[10208:10240] = 0, 1, 2
    groups[70] = 255
    ped = _pedestals(5)
    channels = np.zeros(NUM_PADS, dtype=bool)
    channels[pads] = True
    ev0 = [[64, 30.5, 400.0], [4001, 100.0, 30.0], [3, 50.0, 500.0], [70, 60.0, 20.0]]  # (pad 3 is outside the set)
    ev2 = [[10239, 500.0, 300.0], [10208, 2.5, 25.0]]
    events = [ev0, [], ev2]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in events])])
    points = np.array([r for e in events for r in e], dtype=np.float64)
    labels = np.arange(len(points), dtype=np.int64) + 1
    return pads, groups, ped, channels, offsets, points, labels


def test_partial_and_full_readout_where_only_the_common_mode_crosses(ctx):
    from attpc_engine_amd.detector.traces import readout_cutoff

    inp = Inputs("o16aa")
    pads, groups, ped, channels, offsets, points, labels = _readout_case()
    resp, offset, thr, first = _box_response(), 3, 12.0, (1 << 32) - 1
    cdf, lo = gaussian_noise_table(1.0)
    assert readout_cutoff(cdf, lo, thr)[0] == "never"  # the pad table alone decides "never"
    noise = Noise(cdf, lo, pedestals=ped)
    cm = CommonModeSettings(sigma=3.0, groups=groups, stream=1)
    ref = _reference(cm)
    assert len(pads) == 96 and ref.n_groups == 3
    for seed in range(SEED_HI, SEED_HI + 50):
        want = cmr.traces(offsets, points, labels, resp, thr, offset, noise, ref, seed, first, cmr.PARTIAL, channels)
        noise_only = int((want[3] == -1).sum())
        candidates = 3 * 96 - 5  # (the five pads of the set with rows)
        if 0 < noise_only < candidates and want[0][2] > want[0][1]:  # ... and the empty event keeps some as well
            break
    else:
        raise AssertionError("no seed keeps and drops a noise-only pad")
    assert (want[3] == -1).any() and noise_only < candidates
    assert 70 not in want[1][want[3] == -1]  # the pad of group 255 is never kept on noise alone
    without = cmr.traces(offsets, points, labels, resp, thr, offset, noise, None, seed, first, cmr.PARTIAL, channels)
    assert not (without[3] == -1).any()  # without the stage no noise-only pad crosses
    try:
        for mode, name in ((cmr.PARTIAL, "partial"), (cmr.FULL, "full")):
            configure_traces(inp.config, ctx, resp, thr, offset, noise_sigma=1.0, pedestals=ped, readout=name, readout_pads=pads)
            configure_common_mode(ctx, cm)
            got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
            if mode == cmr.FULL:
                want = cmr.traces(offsets, points, labels, resp, thr, offset, noise, ref, seed, first, cmr.FULL, channels)
                assert np.diff(want[0]).tolist() == [96, 96, 96]
            _assert_traces(got, want, name)
            # the same without a pad table: the common-mode table alone decides
            configure_traces(inp.config, ctx, resp, thr, offset, pedestals=ped, readout=name, readout_pads=pads)
            got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
            bare = cmr.traces(offsets, points, labels, resp, thr, offset, Noise(pedestals=ped), ref, seed, first, mode, channels)
            _assert_traces(got, bare, name + ", no pad table")
        # a threshold no sum of two levels reaches (8 + 24): the scan is skipped, the hit pads alone remain
        configure_traces(inp.config, ctx, resp, 32.0, offset, noise_sigma=1.0, pedestals=ped, readout="partial", readout_pads=pads)
        got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
        high = cmr.traces(offsets, points, labels, resp, 32.0, offset, noise, ref, seed, first, cmr.PARTIAL, channels)
        _assert_traces(got, high, "thr 32")
        assert not (high[3] == -1).any() and high[4]["n_rows"] > 0
    finally:
        configure_common_mode(ctx, None)
        configure_traces(inp.config, ctx, None, None, 0)


# ---------------------------------------------------------------- 4. the pipeline ----
N, SEED, FIRST = 8, 29, (1 << 32) - 3
COMMON = CommonModeSettings(sigma=3.0, groups=_groups_of(40), stream=3)
PEDESTALS = _pedestals(9)


def _engine(inp, ctx, common=COMMON, **kw):
    from attpc_engine_amd.engine import Engine

    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), noise_sigma=2.0, pedestals=PEDESTALS)
    eng.configure_common_mode(common)
    return eng


@pytest.fixture(scope="module")
def pipeline(ctx):
    """o16aa: the delivered cloud of events FIRST .. FIRST + N - 1 and the restatement of its traces with the stage on,
    computed once and read-only."""
    inp = Inputs("o16aa")
    eng = _engine(inp, ctx)
    cloud = eng.run(N, seed=SEED, first_event=FIRST, fetch=True)
    resp, thr = get_response(inp.config), float(inp.config.elec_params.adc_threshold)
    noise = Noise(*gaussian_noise_table(2.0), pedestals=PEDESTALS)
    want = cmr.traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, int(np.argmax(resp)), noise,
                      _reference(COMMON), SEED, FIRST)
    for a in want[:4]:
        a.setflags(write=False)
    eng.configure_common_mode()
    return inp, cloud, want


def test_run_traces_equals_the_restatement_of_its_own_cloud(ctx, pipeline):
    inp, cloud, want = pipeline
    eng = _engine(inp, ctx)
    try:
        res = eng.run_traces(N, seed=SEED, first_event=FIRST)
        _assert_traces(_traces_of(res), want, "run_traces")
        assert want[4]["n_rows"] > 10 * N
        # unchanged: the cloud's statistics, event_points, the kinematics
        np.testing.assert_array_equal(res["event_points"], np.diff(cloud["offsets"]))
        for key in ("n_points", "charge_checksum", "key_checksum", "n_track_samples"):
            assert res["stats"][key] == cloud["stats"][key], key
        np.testing.assert_array_equal(res["p4"], cloud["p4"])
        assert eng.run_traces(N, seed=SEED, first_event=FIRST, fetch=False)["trace"] == want[4]  # device resident
    finally:
        eng.configure_common_mode()


def test_chunks_and_split_calls_play_no_part(ctx, pipeline):
    inp, _, want = pipeline
    n, lo1, lo6 = 6, want[0][1], want[0][6]
    eng = _engine(inp, ctx)
    try:
        whole = eng.run_traces(n, seed=SEED, first_event=FIRST)
        for k, key in enumerate(("offsets", "pads", "samples", "labels")):
            np.testing.assert_array_equal(whole[key], want[k][:n + 1] if k == 0 else want[k][:lo6], err_msg=key)
        head = eng.run_traces(1, seed=SEED, first_event=FIRST)
        tail = eng.run_traces(5, seed=SEED, first_event=FIRST + 1)
        np.testing.assert_array_equal(head["offsets"], whole["offsets"][:2])
        np.testing.assert_array_equal(tail["offsets"], whole["offsets"][1:] - lo1)
        for key in ("pads", "samples", "labels"):
            np.testing.assert_array_equal(np.concatenate([head[key], tail[key]]), whole[key], err_msg=key)
        small = _engine(inp, ctx, chunk_events=2)
        try:
            _assert_traces(_traces_of(small.run_traces(n, seed=SEED, first_event=FIRST)), _traces_of(whole), "chunk_events 2")
        finally:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    finally:
        eng.configure_common_mode()


# ---------------------------------------------------------------- 5. off is off ----
TRIGGER = TriggerSettings(25, window=50, group_multiplicity=20, min_groups=2,
                          groups=(np.arange(NUM_PADS) * 7 % 10).astype(np.uint8))


def _all_outputs(eng, n, seed, first):
    traces = eng.run_traces(n, seed=seed, first_event=first)
    rows = eng.run_trace_rows(n, seed=seed, first_event=first)
    return traces, rows


def test_off_is_off(ctx, pipeline):
    inp, cloud, _ = pipeline
    n, seed, first = 6, 7, 100
    fresh = _abi.Context(0)  # never saw the stage
    eng0 = _engine(inp, fresh, common=None)
    eng0.configure_trigger(TRIGGER)
    never_traces, never_rows = _all_outputs(eng0, n, seed, first)
    never_cloud = eng0.run(n, seed=seed, first_event=first, fetch=True)
    never_spyral = eng0.run_spyral(n, seed=seed, first_event=first)
    fresh.close()
    eng = _engine(inp, ctx)
    eng.configure_trigger(TRIGGER)
    try:
        on_traces, _ = _all_outputs(eng, n, seed, first)
        assert on_traces["trace"]["sample_checksum"] != never_traces["trace"]["sample_checksum"]
        # clouds and cloud-based Spyral rows are unchanged while the stage is on
        on_cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
        on_spyral = eng.run_spyral(n, seed=seed, first_event=first)
        # (row order inside an event is not specified: the clouds are compared in canonical order, the Spyral rows -- in
        #  ascending z, ties in cloud order -- sorted on all their columns)
        np.testing.assert_array_equal(on_cloud["offsets"], never_cloud["offsets"])
        np.testing.assert_array_equal(on_spyral["offsets"], never_spyral["offsets"])
        for e in range(n):
            lo, hi = never_cloud["offsets"][e], never_cloud["offsets"][e + 1]
            for x, y in zip(sort_cloud(on_cloud["points"][lo:hi], on_cloud["labels"][lo:hi]),
                            sort_cloud(never_cloud["points"][lo:hi], never_cloud["labels"][lo:hi])):
                np.testing.assert_array_equal(x, y, err_msg=f"cloud of event {e}")
            lo, hi = never_spyral["offsets"][e], never_spyral["offsets"][e + 1]
            rows = [np.column_stack([r["rows"][lo:hi], r["labels"][lo:hi]]) for r in (on_spyral, never_spyral)]
            rows = [r[np.lexsort(r.T[::-1])] for r in rows]
            np.testing.assert_array_equal(rows[0], rows[1], err_msg=f"Spyral rows of event {e}")
        for key in ("n_points", "charge_checksum", "key_checksum"):
            assert on_cloud["stats"][key] == never_cloud["stats"][key], key
        for what, setting in (("turned off", None), ("a table without levels", CommonModeSettings()),
                              ("a map of 255 alone", CommonModeSettings(sigma=3.0, groups=np.full(NUM_PADS, 255, dtype=np.uint8)))):
            eng.configure_common_mode(COMMON)
            eng.configure_common_mode(setting)
            off_traces, off_rows = _all_outputs(eng, n, seed, first)
            _assert_traces(_traces_of(off_traces), _traces_of(never_traces), what)
            for key in ("offsets", "rows", "labels"):
                np.testing.assert_array_equal(off_rows[key], never_rows[key], err_msg=f"{what}: trace rows {key}")
            assert off_rows["trace_rows"] == never_rows["trace_rows"]
            assert off_traces["trigger"].tobytes() == never_traces["trigger"].tobytes(), what
            assert off_rows["trigger"].tobytes() == never_rows["trigger"].tobytes(), what
    finally:
        eng.configure_common_mode()
        eng.configure_trigger()


# ---------------------------------------------------------------- 6. composition, on the delivered traces ----
def test_trigger_and_trace_rows_see_the_stage(ctx, pipeline):
    from tests import trigger_reference
    from tests.peaks_reference import Geometry, Peaks, trace_rows

    inp, _, _ = pipeline
    n, seed, first = 8, 41, 3
    eng = _engine(inp, ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), noise_sigma=2.0, threshold=20.0,
                         pedestals=PEDESTALS)
    eng.configure_spyral(inp.config)
    eng.configure_peaks(PeakSettings())
    eng.configure_trigger(TRIGGER)
    try:
        tr = eng.run_traces(n, seed=seed, first_event=first)
        rows = eng.run_trace_rows(n, seed=seed, first_event=first)
        want = trace_rows(tr["offsets"], tr["pads"], tr["samples"], tr["labels"], Peaks(), Geometry.of(inp.config), seed, first,
                          PEDESTALS)
        np.testing.assert_array_equal(rows["offsets"], want[0])
        np.testing.assert_array_equal(rows["rows"], want[1])
        np.testing.assert_array_equal(rows["labels"], want[2])
        assert rows["trace_rows"] == want[3] and want[3]["n_rows"] > 0
        records = trigger_reference.records(tr["offsets"], tr["pads"], tr["samples"], TRIGGER, PEDESTALS)
        for got in (tr["trigger"], rows["trigger"], eng.run_trigger(n, seed=seed, first_event=first)["trigger"]):
            assert got.tobytes() == records.tobytes(), trigger_reference.differing(got, records)
        eng.configure_common_mode()  # the stage reached them: without it the same ids give other traces
        assert eng.run_traces(n, seed=seed, first_event=first, fetch=False)["trace"] != tr["trace"]
    finally:
        eng.configure_common_mode()
        eng.configure_trigger()
        configure_traces(inp.config, ctx, None, None, 0)


def test_coherent_noise_fires_the_trigger_on_empty_events(ctx):
    """What the stage exists for.  96 pads in three boards of 32, pad noise sigma 1, zero suppression and discriminator
    at 6 counts above the pedestal, a board asserts at 16 pads in one sample.  Independent noise never reaches 7
    (P about 1e-11 a sample), so no pad is read out and nothing fires.  With a common-mode sigma of 3 a board's draw
    reaches 8 in some sample of nearly every event (P about 0.6 % a sample), and then all of its pads with n >= -1 --
    nine in ten -- cross together.  Chosen on the CPU, asserted on the restatement's own output."""
    from tests import trigger_reference

    inp = Inputs("o16aa")
    pads, groups, ped, channels, _, _, _ = _readout_case()
    groups = groups.copy()
    groups[70] = 0  # (every pad of the set on its board here)
    thr, n, seed, first = 6.0, 4, SEED_HI + 1, (1 << 33) + 5
    trigger = TriggerSettings(6, window=1, group_multiplicity=16, min_groups=1, groups=groups)
    cm = CommonModeSettings(sigma=3.0, groups=groups)
    noise = Noise(*gaussian_noise_table(1.0), pedestals=ped)
    offsets, points, labels = np.zeros(n + 1, dtype=np.int64), np.zeros((0, 3)), np.zeros(0, dtype=np.int64)
    resp = _box_response()
    on = cmr.traces(offsets, points, labels, resp, thr, 0, noise, _reference(cm), seed, first, cmr.PARTIAL, channels)
    off = cmr.traces(offsets, points, labels, resp, thr, 0, noise, None, seed, first, cmr.PARTIAL, channels)
    want_on = trigger_reference.records(on[0], on[1], on[2], trigger, ped)
    want_off = trigger_reference.records(off[0], off[1], off[2], trigger, ped)
    assert want_on["fired"].any() and not want_off["fired"].any() and off[4]["n_rows"] == 0
    configure_traces(inp.config, ctx, resp, thr, 0, noise_sigma=1.0, pedestals=ped, readout="partial", readout_pads=pads)
    configure_trigger(ctx, trigger)
    try:
        configure_common_mode(ctx, cm)
        got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
        _assert_traces(got[:4] + ({k: v for k, v in got[4].items() if k != "trigger"},), on, "stage on")
        assert got[4]["trigger"].tobytes() == want_on.tobytes(), trigger_reference.differing(got[4]["trigger"], want_on)
        configure_common_mode(ctx, None)
        got = clouds_to_traces(offsets, points, labels, ctx, seed=seed, first_event=first)
        assert got[4]["n_rows"] == 0 and got[4]["trigger"].tobytes() == want_off.tobytes()
    finally:
        configure_common_mode(ctx, None)
        configure_trigger(ctx, None)
        configure_traces(inp.config, ctx, None, None, 0)
