"""The table of stage combinations (tests/chain_cases.py) and the composed restatement (tests/chain_reference.py),
without a device: the committed table covers every valid pair of levels of its 16 factors in at most 14 rows, and its
first generation of 12 factors stands in it unchanged; with every stage off, and with each stage on alone, the
composition is what the stage's own restatement gives on the same oracle cloud; the settings can meet the non-vacuity
conditions of every row (on the oracle's cloud, without straggling and distortion: tests/test_gpu_chain.py asserts them
again on the device's); and a composition that is wrong in one of eight ways fails the comparison on the all-on row."""
import itertools

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import normal_quantile_table
from tests import chain_cases as cc
from tests import chain_reference as cr
from tests import (circle_reference, common_mode_reference, distortion_cases, estimate_reference, fit_reference,
                   gain_reference, helix_reference, peaks_reference, thin_reference, trace_noise_reference, trace_reference,
                   trigger_reference, undistort_reference)
from tests.helpers import Inputs


# ---------------------------------------------------------------- 1. the table ----
def test_table_covers_every_valid_pair():
    assert len(cc.NAMES) == 16 and cc.NAMES[12:] == ("distortion", "correction", "helix", "fit")
    assert 9 <= len(cc.TABLE) <= 14 and len({c.name for c in cc.TABLE}) == len(cc.TABLE)
    for c in cc.TABLE:
        assert cc.valid(c.levels()), c
        for name, level in zip(cc.NAMES, c.levels()):
            assert level in cc.FACTORS[name], (c.name, name, level)
    # coverage from the rows alone: every pair of levels of two factors, except those no valid assignment can hold
    covered = set()
    for c in cc.TABLE:
        covered |= set(itertools.combinations(zip(cc.NAMES, c.levels()), 2))
    every = {((f, a), (g, b)) for f, g in itertools.combinations(cc.NAMES, 2) for a in cc.FACTORS[f] for b in cc.FACTORS[g]}
    assert covered <= every and len(every) == 541
    assert every - covered == {(("estimates", "off"), (stage, True)) for stage in ("circle", "helix", "fit")}
    assert covered == cc.valid_pairs()
    # ... and those pairs are invalid by the stated rule, as is a partial readout without a noise source -- and nothing else
    invalid = [levels for levels in itertools.product(*cc.FACTORS.values()) if not cc.valid(levels)]
    for levels in invalid:
        a = dict(zip(cc.NAMES, levels))
        assert ((a["circle"] or a["helix"] or a["fit"]) and a["estimates"] == "off") \
            or (a["readout"] == "partial" and not a["noise"] and not a["common"])
    n_all = int(np.prod([len(v) for v in cc.FACTORS.values()]))
    # (7 of 8 circle/helix/fit cells in one of 3 estimates cells; one of 8 readout/noise/common cells)
    estimates_rule, readout_rule = 7 * n_all // 24, n_all // 8
    assert len(invalid) == estimates_rule + readout_rule - 7 * n_all // 192
    levels = [c.levels() for c in cc.TABLE]
    assert cc.ALL_ON in levels and cc.ALL_OFF in levels
    assert cc.case("all_on").levels() == cc.ALL_ON and cc.case("all_off").levels() == cc.ALL_OFF
    assert levels == cc.generate()  # (the table is what the generator in the module gives)
    # the table's first generation runs on as it was: its eleven rows and their twelve columns, by name and in order
    assert [c.levels()[:cc.N_BASE] for c in cc.TABLE[:11]] == cc.generate_base() == FIRST_GENERATION
    assert [c.name for c in cc.TABLE[:11]] == FIRST_GENERATION_NAMES


FIRST_GENERATION_NAMES = ["all_on", "all_off", "noise_partial_trigger_rows", "gain_common_gate_circle", "common_baseline_thinned_circle",
                          "gain_common_partial_baseline", "noise_hit_thinned_circle", "noise_partial_baseline_gate",
                          "gain_common_trigger", "straggle_gain_baseline_rows", "noise_trigger_thinned"]
FIRST_GENERATION = [
    (True, True, True, True, "partial", True, "gate", "thinned", True, 3, "straddle", "fetch"),
    (False, False, False, False, "hit", False, "off", "off", False, 1, "zero", "resident"),
    (True, False, True, False, "partial", False, "on", "rows", False, 1, "straddle", "fetch"),
    (False, True, False, True, "hit", False, "gate", "rows", True, 3, "zero", "resident"),
    (False, False, False, True, "hit", True, "on", "thinned", True, 1, "straddle", "resident"),
    (True, True, False, True, "partial", True, "off", "off", False, 3, "zero", "resident"),
    (True, False, True, False, "hit", False, "off", "thinned", True, 3, "zero", "fetch"),
    (False, False, True, False, "partial", True, "gate", "off", False, 1, "straddle", "resident"),
    (False, True, False, True, "hit", False, "on", "off", False, 1, "zero", "fetch"),
    (True, True, False, False, "hit", True, "off", "rows", False, 3, "straddle", "resident"),
    (True, False, True, False, "hit", False, "on", "thinned", False, 3, "zero", "resident"),
]


def test_chunks_of_the_workload():
    for c in cc.TABLE:
        sizes = [min(cc.CHUNK_EVENTS, c.n_events - lo) for lo in range(0, c.n_events, cc.CHUNK_EVENTS)]
        assert len(sizes) >= 3 and sizes[-1] < cc.CHUNK_EVENTS, c
        ids = range(cc.FIRST_STRADDLE + cc.CHUNK_EVENTS, cc.FIRST_STRADDLE + 2 * cc.CHUNK_EVENTS)  # the middle chunk
        assert ids[0] < 1 << 32 <= ids[-1]


# ---------------------------------------------------------------- the oracle's clouds ----
@pytest.fixture(scope="module")
def inp():
    return Inputs(cc.WORKLOAD)


@pytest.fixture(scope="module")
def clouds(inp):
    """{first: (offsets, points, labels)} of the workload from the CPU oracle, read-only."""
    from oracle import pyoracle as orc

    out = {}
    n = max(c.n_events for c in cc.TABLE)
    for first in (0, cc.FIRST_STRADDLE):
        ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=cc.SEED, first=first, n=n, capacity=1 << 20, threads=4)
        out[first] = (ref["offsets"], ref["points"], ref["labels"])
        for a in out[first]:
            a.setflags(write=False)
    return out


def _head(cloud, n):
    offsets, points, labels = cloud
    return offsets[:n + 1], points[:offsets[n]], labels[:offsets[n]]


def _chain(inp, c, cloud, **kw):
    s = cc.settings(c, inp.config)
    return s, cr.chain(s, inp.config, inp.indices, _head(cloud, c.n_events), cc.SEED, cc.first_event(c), inp=inp, **kw)


# ---------------------------------------------------------------- 2. off, and one stage at a time ----
FEW = 6
OFF = cc.Case("off", *cc.ALL_OFF)._replace(n_events=FEW)


def _plain(inp, cloud, first=0):
    """(traces, rows) of the restatements as they are, every stage off."""
    offsets, points, labels = cloud
    resp = get_response(inp.config)
    tr = trace_reference.traces(offsets, points, labels, resp, cc.TRACE_THRESHOLD, int(np.argmax(resp)), first_event=first)
    return tr, _rows(inp, tr, first)


def _rows(inp, tr, first=0, pedestals=None):
    return peaks_reference.trace_rows(tr[0], tr[1], tr[2], tr[3], peaks_reference.Peaks(**{**peaks_reference.Peaks()._asdict(), **cc.PEAKS}),
                                      peaks_reference.Geometry.of(inp.config), cc.SEED, first, pedestals)


def _assert_traces_and_rows(got, traces, rows):
    for k, name in enumerate(("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(got.traces[k], traces[k], err_msg=f"traces {name}")
    assert got.traces[4] == traces[4]
    for k, name in enumerate(("offsets", "rows", "labels")):
        np.testing.assert_array_equal(got.rows[k], rows[k], err_msg=f"rows {name}")
    assert got.rows[3] == rows[3] and rows[3]["n_rows"] > 0


def test_every_stage_off_is_traces_then_peaks(inp, clouds):
    cloud = _head(clouds[0], FEW)
    _, got = _chain(inp, OFF, clouds[0])
    traces, rows = _plain(inp, cloud)  # (every row through the peak restatement: the shortcut of ``possible`` left out)
    _assert_traces_and_rows(got, traces, rows)
    assert got.trigger is None and got.fired.all() and got.points is None and got.records is None


def test_one_stage_on_is_that_stage_alone(inp, clouds):
    """Straggling and the drift distortion only shape the cloud: on a given cloud the chain with either on is the chain
    with it off (what they do to the cloud is held to their restatements in tests/test_gpu_straggling.py and
    tests/test_gpu_distortion.py).  Every other stage on alone gives what its own restatement gives."""
    cloud = _head(clouds[0], FEW)
    offsets, points, labels = cloud
    resp = get_response(inp.config)
    at, thr = int(np.argmax(resp)), cc.TRACE_THRESHOLD
    plain_traces, plain_rows = _plain(inp, cloud)
    # gain
    s, got = _chain(inp, OFF._replace(gain=True), clouds[0])
    gain = gain_reference.Gain(1.0, normal_quantile_table(), cc.gain_map(), stream=1)
    want = gain_reference.traces_with_gain(offsets, points, labels, gain, cc.SEED, 0,
                                           lambda pts: trace_reference.traces(offsets, pts, labels, resp, thr, at, first_event=0))
    _assert_traces_and_rows(got, want, _rows(inp, want))
    assert want[4] != plain_traces[4]
    # pad noise and pedestals
    s, got = _chain(inp, OFF._replace(noise=True), clouds[0])
    from attpc_engine_amd.detector.traces import gaussian_noise_table
    noise = trace_noise_reference.Noise(*gaussian_noise_table(cc.NOISE_SIGMA), pedestals=cc.pedestals())
    want = trace_noise_reference.traces(offsets, points, labels, resp, thr, at, noise, cc.SEED, 0)
    _assert_traces_and_rows(got, want, _rows(inp, want, pedestals=cc.pedestals()))
    # common mode
    s, got = _chain(inp, OFF._replace(common=True), clouds[0])
    cm = s["common_mode"]
    common = common_mode_reference.CommonMode((cm.cdf, cm.min_level), cc.common_groups(), 2)
    want = common_mode_reference.traces(offsets, points, labels, resp, thr, at, None, common, cc.SEED, 0)
    _assert_traces_and_rows(got, want, _rows(inp, want))
    # partial readout (with the pad noise: alone it is no valid row)
    s, got = _chain(inp, OFF._replace(noise=True, readout="partial", n_events=2), clouds[0])
    from tests import readout_reference
    channels = np.zeros(10240, dtype=bool)
    channels[cc.readout_pads(inp.config)] = True
    two = _head(cloud, 2)
    want = readout_reference.traces(*two, resp, thr, at, noise, cc.SEED, 0, readout_reference.PARTIAL, channels)
    _assert_traces_and_rows(got, want, _rows(inp, want, pedestals=cc.pedestals()))
    assert (want[3] == -1).any()
    # baseline
    from tests import baseline_reference
    s, got = _chain(inp, OFF._replace(baseline=True), clouds[0])
    y = baseline_reference.remove(plain_traces[2], cc.BASELINE_SCALE)[0]
    _assert_traces_and_rows(got, plain_traces, _rows(inp, plain_traces[:2] + (y,) + plain_traces[3:]))
    assert got.rows[3] != plain_rows[3]
    # trigger, and its gate
    s, got = _chain(inp, OFF._replace(trigger="on"), clouds[0])
    records = trigger_reference.records(plain_traces[0], plain_traces[1], plain_traces[2], s["trigger"], None)
    _assert_traces_and_rows(got, plain_traces, plain_rows)
    assert got.trigger.tobytes() == records.tobytes() and got.fired.all()
    s, got = _chain(inp, OFF._replace(trigger="gate"), clouds[0])
    fired = records["fired"] != 0
    assert got.trigger.tobytes() == records.tobytes() and (got.fired == fired).all() and 0 < fired.sum() < FEW
    for e in range(FEW):
        lo, hi = got.rows[0][e], got.rows[0][e + 1]
        if fired[e]:
            np.testing.assert_array_equal(got.rows[1][lo:hi], plain_rows[1][plain_rows[0][e]:plain_rows[0][e + 1]])
        else:
            assert lo == hi
    # estimates of the rows, of the thinned points, and the circle fit behind either
    params = estimate_reference.Params(*cc.ESTIMATES["rows"], inp.config.det_params.bfield)
    s, got = _chain(inp, OFF._replace(estimates="rows"), clouds[0])
    _assert_traces_and_rows(got, plain_traces, plain_rows)
    estimate_reference.assert_same_records(got.records, estimate_reference.records(*plain_rows[:3], inp.indices, params))
    s, got = _chain(inp, OFF._replace(estimates="rows", circle=True), clouds[0])
    fitted = circle_reference.records(*plain_rows[:3], inp.indices, params, circle_reference.Settings())
    estimate_reference.assert_same_records(got.records, fitted)
    assert (fitted["reserved"] > 0).any() and got.points is None
    params = estimate_reference.Params(*cc.ESTIMATES["thinned"], inp.config.det_params.bfield)
    s, got = _chain(inp, OFF._replace(estimates="thinned"), clouds[0])
    thin_reference.assert_same_points(got.points, thin_reference.thin(*plain_rows[:3], inp.indices, cc.THIN_STEP))
    estimate_reference.assert_same_records(got.records, thin_reference.fused_records(*plain_rows[:3], inp.indices, cc.THIN_STEP, params))
    # straggling, the drift distortion: nothing of the chain of this cloud moves
    _, off = _chain(inp, OFF, clouds[0])
    for shaped in (OFF._replace(straggling=True), OFF._replace(distortion=True)):
        s, got = _chain(inp, shaped, clouds[0])
        assert s["straggling"] is not None or s["distortion"] is not None
        cr.assert_same(got, off)
    # the drift correction: the restatement on the plain rows; offsets, the number of rows and the checksum stay
    s, got = _chain(inp, OFF._replace(correction=True), clouds[0])
    drift = inp.config.elec_params
    settings = undistort_reference.Settings(distortion_cases.reference_map(distortion_cases.named_map(), inp.config),
                                            int(drift.windows_edge), int(drift.micromegas_edge), float(inp.config.det_params.length))
    fixed = undistort_reference.undistort(settings, *plain_rows[:3])
    _assert_traces_and_rows(got, plain_traces, (plain_rows[0], fixed[0], fixed[1], plain_rows[3]))
    # (rows that change places need more events: a condition of every table row with the stage, not of these six)
    assert got.correction == fixed[3] and fixed[3]["n_rows"] == len(plain_rows[1]) and not np.array_equal(fixed[0], plain_rows[1])
    assert got.records is None and got.fits is None and off.correction is None
    # the helix slope and the track fit, each alone behind the estimates of the raw rows
    params = estimate_reference.Params(*cc.ESTIMATES["rows"], inp.config.det_params.bfield)
    plain_records = estimate_reference.records(*plain_rows[:3], inp.indices, params)
    s, got = _chain(inp, OFF._replace(estimates="rows", helix=True), clouds[0])
    _assert_traces_and_rows(got, plain_traces, plain_rows)
    estimate_reference.assert_same_records(got.records, helix_reference.records(*plain_rows[:3], inp.indices, params,
                                                                                helix_reference.Settings()))
    assert (got.records["slope"] != plain_records["slope"]).any() and got.fits is None
    s, got = _chain(inp, OFF._replace(estimates="rows", fit=True), clouds[0])
    _assert_traces_and_rows(got, plain_traces, plain_rows)
    estimate_reference.assert_same_records(got.records, plain_records)
    fits = fit_reference.records(*plain_rows[:3], inp.indices, fit_reference.Model(inp.det, inp.layout), plain_records,
                                 fit_reference.Settings(**cc.FIT), cc.ESTIMATES["rows"][0])
    fit_reference.assert_same_records(got.fits, fits)
    assert (fits["evaluations"] >= 2).any()


# ---------------------------------------------------------------- 3. every row has something to show ----
@pytest.fixture(scope="module")
def all_on(inp, clouds):
    c = cc.case("all_on")
    s, got = _chain(inp, c, clouds[cc.first_event(c)])
    return c, s, got


@pytest.mark.parametrize("name", cc.CASE_IDS)
def test_settings_meet_the_non_vacuity_conditions(inp, clouds, all_on, name):
    c = cc.case(name)
    cloud = _head(clouds[cc.first_event(c)], c.n_events)
    s, got = all_on[1:] if name == "all_on" else _chain(inp, c, clouds[cc.first_event(c)])
    figures = cr.counts(s, inp.config, inp.indices, cloud, cc.SEED, cc.first_event(c), got)
    print(name, figures)
    cr.assert_not_vacuous(figures, c.n_events)


# ---------------------------------------------------------------- 4. a wrong composition is caught ----
def _wrong(inp, clouds, all_on, fault):
    """The all-on chain with one step out of place."""
    c, s, right = all_on
    config, indices, seed, first = inp.config, inp.indices, cc.SEED, cc.first_event(c)
    cloud = _head(clouds[first], c.n_events)
    tr = right.traces
    if fault == "gain after the noise":
        # the gain wrapped around the noiseless hit traces, the pedestal and both noise terms put on afterwards
        offsets, points, labels = cloud
        t = s["traces"]
        resp = get_response(config)
        bare = gain_reference.traces_with_gain(offsets, points, labels, cr.gain_of(s), seed, first,
                                               lambda pts: trace_reference.traces(offsets, pts, labels, resp, t["threshold"],
                                                                                  t["offset"], first_event=first))
        noise, common, samples = cr.noise_of(s), cr.common_of(s), []
        for e in range(c.n_events):
            pads = bare[1][bare[0][e]:bare[0][e + 1]]
            n = noise.values(seed, first + e, pads) + common.of_pads(seed, first + e, pads)
            samples.append(trace_noise_reference.noisy(bare[2][bare[0][e]:bare[0][e + 1]], noise.pedestals[pads][:, None], n))
        tr = (bare[0], bare[1], np.concatenate(samples).astype(np.int16), bare[3], bare[4])
    trigger = cr.trigger_of(s, tr)
    fired = cr.fired_of(s, trigger, c.n_events)
    early = fault != "the gate after the peaks"
    offsets, pads, samples, labels = cr.gated(tr[:4], fired) if early else tr[:4]
    y, pedestals = cr.y_of(s, samples)
    if fault == "the pedestal as well as the baseline":
        pedestals = cr.pedestals_of(s)
    rows = cr.rows_of(s, config, offsets, pads, y, labels, pedestals, seed, first)
    if not early:  # the rows of the events that did not fire dropped now: the sums are those of every event
        rows = cr.gated(rows[:3], fired) + (rows[3],)
    rows, correction = cr.corrected_of(s, config, rows)
    seen = rows
    if fault == "thinning of the ungated rows":
        ungated = cr.y_of(s, tr[2])
        seen = cr.corrected_of(s, config, cr.rows_of(s, config, tr[0], tr[1], ungated[0], tr[3], ungated[1], seed, first))[0]
    records = cr.records_of(s, config, seen, indices)
    return cr.Chain(tr, trigger, fired, rows, cr.points_of(s, seen, indices), records, correction, cr.fits_of(s, inp, seen, records))


def _wrong_behind_the_rows(inp, all_on, fault):
    """The all-on chain with one of the steps behind the trace rows out of place (the rows are the right chain's)."""
    c, s, right = all_on
    config, indices = inp.config, inp.indices
    if fault == "the correction after the thinning":
        # the uncorrected rows thinned, the points taken back through the map and sorted, then estimated and fitted
        point_offsets, points, point_labels, info = cr.points_of(s, right.uncorrected, indices)
        points, point_labels = cr.corrected_of(s, config, (point_offsets, points, point_labels, None))[0][1:3]
        unthinned = {**s, "thinning": None}
        records = cr.records_of(unthinned, config, (point_offsets, points, point_labels), indices)
        records["status"] |= np.where(info["n_dropped"] > 0, _abi.EST_RANGE, 0).astype(np.int32)
        fits = cr.fits_of(unthinned, inp, (point_offsets, points, point_labels), records)
        return right._replace(points=(point_offsets, points, point_labels, info), records=records, fits=fits)
    if fault == "the fit on the uncorrected rows":
        return right._replace(fits=cr.fits_of(s, inp, right.uncorrected, right.records))
    if fault == "the fit on the raw rows although thinning is on":
        return right._replace(fits=cr.fits_of({**s, "thinning": None}, inp, right.rows, right.records))
    assert fault == "the fit started from estimates without the helix slope"
    return right._replace(fits=cr.fits_of(s, inp, right.rows, cr.records_of({**s, "helix": None}, config, right.rows, indices)))


def test_the_steps_in_order_are_the_chain(inp, clouds, all_on):
    cr.assert_same(_wrong(inp, clouds, all_on, None), all_on[2])


@pytest.mark.parametrize("fault", ["the correction after the thinning", "the fit on the uncorrected rows",
                                   "the fit on the raw rows although thinning is on",
                                   "the fit started from estimates without the helix slope"])
def test_a_wrong_composition_behind_the_rows_is_caught(inp, all_on, fault):
    wrong = _wrong_behind_the_rows(inp, all_on, fault)
    with pytest.raises(AssertionError):
        cr.assert_same(wrong, all_on[2])


@pytest.mark.parametrize("fault", ["the pedestal as well as the baseline", "the gate after the peaks", "gain after the noise",
                                   "thinning of the ungated rows"])
def test_a_wrong_composition_is_caught(inp, clouds, all_on, fault):
    wrong = _wrong(inp, clouds, all_on, fault)
    with pytest.raises(AssertionError):
        cr.assert_same(wrong, all_on[2])
