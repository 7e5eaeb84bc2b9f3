"""The restatements of the single trace stages (tests/*_reference.py) composed in the order of the contract
(include/attpc_engine.h): gain -> traces (noise, pedestals, common mode, readout) -> trigger -> gate -> baseline or
pedestal subtraction -> peaks -> drift correction -> thinning -> estimates / circle fit / helix slope -> track fit.
``chain`` takes the stage settings of one case (``tests.chain_cases.settings``) and one run's cloud and returns what
every downstream output must be.  Straggling and the drift distortion act in front of the cloud: they shape it, and the
chain of a given cloud does not know of them.  No arithmetic of its own: every stage is a call of its restatement, a
stage that is off is passed by, and the steps are functions of their own so that tests/test_chain_cpu.py can put them
together wrongly on purpose."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from attpc_engine_amd._abi import EST_NO_HELIX, EST_RANGE, FIT_EMPTY
from attpc_engine_amd.detector.response import get_response
from attpc_engine_amd.detector.traces import gaussian_noise_table, normal_quantile_table, readout_mask
from tests import baseline_reference, circle_reference, common_mode_reference, estimate_reference, gain_reference
from tests import distortion_cases, fit_reference, helix_reference, peaks_reference, readout_reference, thin_reference
from tests import trace_noise_reference, trace_reference, trigger_reference, undistort_reference


class Chain(NamedTuple):
    """Every output of one case.  ``traces`` = (offsets, pads, samples, labels, sums) as ``run_traces`` delivers them;
    ``trigger`` the records [n] or None; ``fired`` bool [n] (all True without a gate); ``rows`` = (offsets, rows,
    labels, sums) as ``run_trace_rows`` delivers them (with the drift correction on: the corrected rows); ``points`` =
    what ``rows_to_points`` makes of the rows, or None; ``records`` the estimates [n, n_sim] or None; ``correction``
    the counts of the drift correction or None; ``fits`` the track-fit records [n, n_sim] or None."""
    traces: tuple
    trigger: np.ndarray | None
    fired: np.ndarray
    rows: tuple
    points: tuple | None
    records: np.ndarray | None
    correction: dict | None = None
    fits: np.ndarray | None = None
    uncorrected: tuple | None = None  # the rows in front of the drift correction (None without it); not an output


# ---------------------------------------------------------------- the settings, restated ----
def noise_of(s: dict):
    """The pad noise of the case's trace settings (None: no table and no pedestals)."""
    t = s["traces"]
    if not t.get("noise_sigma") and t.get("pedestals") is None:
        return None
    return _Noise(*gaussian_noise_table(t["noise_sigma"]), pedestals=t["pedestals"])


class _Noise(trace_noise_reference.Noise):
    """The pad noise with the draw of tests/readout_reference.py: one Philox call per counter instead of one per sample,
    the same numbers (tests/test_readout_cpu.py) in a quarter of the time."""

    def values(self, seed, event, pads):
        return readout_reference.values(self, seed, event, pads)


def pedestals_of(s: dict):
    return s["traces"].get("pedestals")


def common_of(s: dict):
    cm = s["common_mode"]
    return None if cm is None else common_mode_reference.CommonMode((cm.cdf, cm.min_level), cm.groups, cm.stream)


def gain_of(s: dict):
    g = s["gain"]
    return None if g is None else gain_reference.Gain(g.rel_variance, normal_quantile_table(), g.pad_gain, g.stream)


def peaks_of(s: dict):
    p = s["peaks"]
    return peaks_reference.Peaks(p.separation, p.prominence, p.min_width, p.max_width, p.rel_height, p.threshold)


def params_of(s: dict, config):
    e = s["estimates"]
    return estimate_reference.Params(e.beam_region_radius, e.min_points, config.det_params.bfield)


def circle_of(s: dict):
    c = s["circle"]
    return None if c is None else circle_reference.Settings(c.max_evaluations, c.tolerance)


def correction_of(s: dict, config):
    """The drift correction's descriptor: the map's three derived numbers as tests/distortion_cases.py writes them out,
    the drift of the config."""
    c = s["correction"]
    if c is None:
        return None
    return undistort_reference.Settings(distortion_cases.reference_map(c.map, config), int(config.elec_params.windows_edge),
                                        int(config.elec_params.micromegas_edge), float(config.det_params.length),
                                        c.iterations, c.tolerance_xy, c.tolerance_tb)


def helix_of(s: dict):
    return None if s["helix"] is None else helix_reference.Settings(s["helix"].regressor)


def fit_of(s: dict):
    f = s["fit"]
    return None if f is None else fit_reference.Settings(f.time_step, f.max_steps, f.max_evaluations, f.tolerance_momentum,
                                                         f.tolerance_position)


# ---------------------------------------------------------------- the steps ----
def traces_of(s: dict, config, cloud, seed: int, first: int, gain="from the settings"):
    """Steps 1 and 2: the traces of the cloud (offsets, points, labels), the gain wrapped around the trace restatement
    the settings call for."""
    offsets, points, labels = cloud
    t = s["traces"]
    response, threshold, offset = get_response(config), float(t["threshold"]), int(t["offset"])
    noise, common = noise_of(s), common_of(s)
    partial = t["readout"] == "partial"
    channels = readout_mask(t["readout_pads"]).astype(bool) if partial else None

    def inner(pts):
        if common is not None:
            mode = common_mode_reference.PARTIAL if partial else common_mode_reference.HIT
            return common_mode_reference.traces(offsets, pts, labels, response, threshold, offset, noise, common, seed, first,
                                                mode, channels)
        if partial:
            return readout_reference.traces(offsets, pts, labels, response, threshold, offset,
                                            trace_noise_reference.Noise() if noise is None else noise, seed, first,
                                            readout_reference.PARTIAL, channels)
        if noise is not None:
            return trace_noise_reference.traces(offsets, pts, labels, response, threshold, offset, noise, seed, first)
        return trace_reference.traces(offsets, pts, labels, response, threshold, offset, first_event=first)

    gain = gain_of(s) if isinstance(gain, str) else gain
    if gain is None:
        return inner(points)
    return gain_reference.traces_with_gain(offsets, points, labels, gain, seed, first, inner)


def trigger_of(s: dict, traces):
    """Step 3: the trigger records of the traces (None: no trigger)."""
    if s["trigger"] is None:
        return None
    return trigger_reference.records(traces[0], traces[1], traces[2], s["trigger"], pedestals_of(s))


def fired_of(s: dict, trigger, n: int) -> np.ndarray:
    if s["trigger"] is None or not s["trigger"].gate:
        return np.ones(n, dtype=bool)
    return trigger["fired"] != 0


def gated(csr, fired):
    """Step 4 on anything in CSR form (offsets, per-row arrays ...): the events that did not fire keep an empty range."""
    offsets = np.asarray(csr[0], dtype=np.int64)
    counts = np.diff(offsets)
    keep = np.repeat(fired, counts)
    return (np.concatenate([[0], np.cumsum(np.where(fired, counts, 0))]),) + tuple(np.asarray(a)[keep] for a in csr[1:])


def numpy_baseline(samples, scale):
    return baseline_reference.remove(samples, scale)[0]


def y_of(s: dict, samples, baseline=numpy_baseline):
    """Step 5 -> (the rows the peaks are looked for in, the pedestals the peak restatement still has to subtract):
    ``baseline(samples, window_scale)`` and nothing, or the samples as they are and the configured pedestals."""
    if s["baseline"] is None:
        return samples, pedestals_of(s)
    return baseline(samples, s["baseline"].window_scale), None


def possible(offsets, pads, y, labels, pedestals, pk):
    """The rows without those that cannot hold a point (step 6 of the trace-row contract needs y[k] > threshold): most
    noise-only rows end here instead of in the restatement's Python loops.  tests/test_gpu_baseline.py and
    tests/test_chain_cpu.py check that the rows left out give no row, offset or checksum term."""
    if not len(pads):
        return offsets, pads, y, labels
    top = y.max(axis=1).astype(np.int64) - (0 if pedestals is None else np.asarray(pedestals, dtype=np.int64)[pads])
    keep = top > pk.threshold
    new = np.concatenate([[0], np.cumsum(keep)])[np.asarray(offsets, dtype=np.int64)]
    return new, pads[keep], y[keep], labels[keep]


def rows_of(s: dict, config, offsets, pads, y, labels, pedestals, seed: int, first: int, shortcut: bool = True):
    """Step 6: the trace rows (offsets, rows, labels, sums)."""
    pk = peaks_of(s)
    if shortcut:
        offsets, pads, y, labels = possible(offsets, pads, y, labels, pedestals, pk)
    return peaks_reference.trace_rows(offsets, pads, y, labels, pk, peaks_reference.Geometry.of(config), seed, first, pedestals)


def corrected_of(s: dict, config, rows, mutant=None):
    """Step 6b -> (the rows every later step and the delivery see, the correction's counts or None): every gated row
    taken back through the map and every event's rows sorted again.  Offsets, n_rows and the row checksum (terms of
    event, pad and sample) stay."""
    settings = correction_of(s, config)
    if settings is None:
        return rows, None
    new_rows, new_labels, _, info = undistort_reference.undistort(settings, rows[0], rows[1], rows[2], mutant)
    return (rows[0], new_rows, new_labels, rows[3]), info


def points_of(s: dict, rows, indices):
    """Step 7 (None: no thinning)."""
    if s["estimates"] is None or s["thinning"] is None:
        return None
    return thin_reference.thin(rows[0], rows[1], rows[2], indices, s["thinning"].z_step)


def records_of(s: dict, config, rows, indices):
    """Step 8 (None: no estimates)."""
    if s["estimates"] is None:
        return None
    params, circle, helix = params_of(s, config), circle_of(s), helix_of(s)
    if helix is not None:  # (as tests/test_gpu_helix.py composes it)
        if s["thinning"] is None:
            return helix_reference.records(rows[0], rows[1], rows[2], indices, params, helix, circle)
        point_offsets, points, point_labels, info = thin_reference.thin(rows[0], rows[1], rows[2], indices, s["thinning"].z_step)
        records = helix_reference.records(point_offsets, points, point_labels, indices, params, helix, circle)
        records["status"] |= np.where(info["n_dropped"] > 0, EST_RANGE, 0).astype(np.int32)
        return records
    if s["thinning"] is not None:
        return thin_reference.fused_records(rows[0], rows[1], rows[2], indices, s["thinning"].z_step, params, circle)
    if circle is not None:
        return circle_reference.records(rows[0], rows[1], rows[2], indices, params, circle)
    return estimate_reference.records(rows[0], rows[1], rows[2], indices, params)


def fits_of(s: dict, inp, rows, records):
    """Step 9 (None: no track fit, or no estimates to start it from): the fit on what the estimates read -- the
    corrected rows, thinned if the thinning is on -- started from the restatement's own estimate records.  ``inp``: the
    workload's descriptors (``tests.helpers.Inputs``), whose detector and layout are the model."""
    if s["fit"] is None or s["estimates"] is None:
        return None
    assert inp is not None, "the track fit needs the workload's descriptors: chain(..., inp=)"
    seen = rows[:3]
    if s["thinning"] is not None:
        seen = thin_reference.thin(rows[0], rows[1], rows[2], inp.indices, s["thinning"].z_step)[:3]
    return fit_reference.records(*seen, inp.indices, fit_reference.Model(inp.det, inp.layout), records, fit_of(s),
                                 s["estimates"].beam_region_radius)


# ---------------------------------------------------------------- the composition ----
def chain(s: dict, config, indices, cloud, seed: int, first: int, baseline=numpy_baseline, traces=None, inp=None) -> Chain:
    """The steps in contract order.  ``baseline``: the operator of step 5 (the device tests pass the device's own,
    which they hold to ``baseline_reference`` under its ambiguity rule); ``traces``: step 1 and 2 if already made;
    ``inp``: the workload's descriptors, which the track fit needs."""
    tr = traces_of(s, config, cloud, seed, first) if traces is None else traces
    trigger = trigger_of(s, tr)
    fired = fired_of(s, trigger, len(tr[0]) - 1)
    offsets, pads, samples, labels = gated(tr[:4], fired)
    y, pedestals = y_of(s, samples, baseline)
    plain = rows_of(s, config, offsets, pads, y, labels, pedestals, seed, first)
    rows, correction = corrected_of(s, config, plain)
    records = records_of(s, config, rows, indices)
    return Chain(tr, trigger, fired, rows, points_of(s, rows, indices), records, correction, fits_of(s, inp, rows, records),
                 None if correction is None else plain)


def assert_same(got: Chain, want: Chain) -> None:
    """Every output of two chains: identical."""
    for k, name in enumerate(("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(got.traces[k], want.traces[k], err_msg=f"traces {name}")
    assert got.traces[4] == want.traces[4], (got.traces[4], want.traces[4])
    assert (got.trigger is None) == (want.trigger is None)
    if want.trigger is not None:
        assert got.trigger.tobytes() == want.trigger.tobytes(), trigger_reference.differing(got.trigger, want.trigger)
    np.testing.assert_array_equal(got.fired, want.fired, err_msg="fired")
    for k, name in enumerate(("offsets", "rows", "labels")):
        np.testing.assert_array_equal(got.rows[k], want.rows[k], err_msg=f"rows {name}")
    assert got.rows[3] == want.rows[3], (got.rows[3], want.rows[3])
    assert (got.points is None) == (want.points is None) and (got.records is None) == (want.records is None)
    if want.points is not None:
        thin_reference.assert_same_points(got.points, want.points)
    if want.records is not None:
        estimate_reference.assert_same_records(got.records, want.records)
    assert got.correction == want.correction, (got.correction, want.correction)
    assert (got.fits is None) == (want.fits is None)
    if want.fits is not None:
        fit_reference.assert_same_records(got.fits, want.fits)


# ---------------------------------------------------------------- what makes a case worth running ----
COMMON_EVENTS = 2  # the events on which ``counts`` makes the traces again without the common-mode term


def counts(s: dict, config, indices, cloud, seed: int, first: int, got: Chain, baseline=numpy_baseline) -> dict:
    """The figures of the non-vacuity conditions of one case, from the restatement's own outputs (``got`` = its chain):
    only the keys of the stages that are on."""
    out = {"trace_rows": got.traces[4]["n_rows"], "rows": got.rows[3]["n_rows"]}
    if s["traces"]["readout"] == "partial":
        out["noise_only_rows"] = int((got.traces[3] == -1).sum())
    if s["trigger"] is not None and s["trigger"].gate:
        out["fired"] = int(got.fired.sum())
    if s["gain"] is not None:  # dead pads that the cloud's own charge would have read out (noiseless, hit mode)
        offsets, points, labels = cloud
        on_dead = s["gain"].pad_gain[points[:, 0].astype(np.int64)] == 0.0
        dead_offsets = np.concatenate([[0], np.cumsum(on_dead)])[np.asarray(offsets, dtype=np.int64)]
        t = s["traces"]
        out["dead_pads_hit"] = trace_reference.traces(dead_offsets, points[on_dead], labels[on_dead], get_response(config),
                                                      float(t["threshold"]), int(t["offset"]), first)[4]["n_rows"]
    if s["common_mode"] is not None:  # verdicts and trigger records of the first events the common-mode term changes
        few = min(COMMON_EVENTS, len(cloud[0]) - 1)
        head = (cloud[0][:few + 1], cloud[1][:cloud[0][few]], cloud[2][:cloud[0][few]])
        without = {**s, "common_mode": None}
        plain, with_it = traces_of(without, config, head, seed, first), tuple(a[:got.traces[0][few]] for a in got.traces[1:4])
        with_it = (got.traces[0][:few + 1],) + with_it
        kept = lambda t: set(zip(np.repeat(np.arange(few), np.diff(t[0])).tolist(), t[1].tolist()))  # noqa: E731
        out["common_verdicts"] = len(kept(plain) ^ kept(with_it))
        if s["trigger"] is not None:
            out["common_trigger_records"] = int((trigger_of(without, plain) != got.trigger[:few]).sum())
    if s["baseline"] is not None:  # rows whose amplitude is not the pedestal-subtracted one
        plain = chain({**s, "baseline": None, "estimates": None}, config, indices, cloud, seed, first, traces=got.traces).rows
        amplitude = lambda r: {(int(e), int(p), int(c)): a for e, p, c, a in zip(  # noqa: E731
            np.repeat(np.arange(len(r[0]) - 1), np.diff(r[0])), r[1][:, 5], np.floor(r[1][:, 6]), r[1][:, 3])}
        a, b = amplitude(got.rows), amplitude(plain)
        out["baseline_amplitudes"] = sum(1 for key in a if key in b and a[key] != b[key])
    if got.points is not None:
        out["thinned_tracks"] = int((got.points[3]["n_points"] < got.points[3]["n_rows"]).sum())
    if got.records is not None:
        out["status_0"] = int((got.records["status"] == 0).sum())
        out["status_not_0"] = int((got.records["status"] != 0).sum())
        if s["circle"] is not None:
            out["circle_fits"] = int((got.records["reserved"] > 0).sum())
    if got.correction is not None:  # rows the re-sort moved, and events whose corrected rows would not be in ascending z
        out["rows_moved"] = got.correction["n_moved"]
        unsorted = undistort_reference.undistort(correction_of(s, config), *got.uncorrected[:3], "no_resort")[0]
        out["events_out_of_order"] = sum(bool((np.diff(unsorted[lo:hi, 2]) < 0.0).any())
                                         for lo, hi in zip(got.rows[0][:-1], got.rows[0][1:]))
    if got.records is not None and s["helix"] is not None:  # records the helix ran in, and those whose slope it moved
        ran = (got.records["n_fit"] > 0) & (got.records["status"] & EST_NO_HELIX == 0)
        without = records_of({**s, "helix": None}, config, got.rows, indices)
        out["helix_ran"] = int(ran.sum())
        out["helix_slopes_moved"] = int((got.records["slope"][ran] != without["slope"][ran]).sum())
    if got.fits is not None:
        ran = got.fits["evaluations"] >= 2
        out["fits_ran"] = int(ran.sum())
        if "fired" in out:  # behind a gate: fits that ran in events that fired, records of events that did not
            out["fits_ran_fired"] = int(ran[got.fired].sum())
            out["fits_not_fired"] = int((got.fits["status"][~got.fired] == FIT_EMPTY).sum())
    return out


def assert_not_vacuous(c: dict, n_events: int) -> None:
    """The conditions on the figures of ``counts``."""
    assert c["trace_rows"] > 0 and c["rows"] > 0, c
    assert c.get("noise_only_rows", 1) >= 1, c
    assert 0 < c.get("fired", 1) < (n_events if "fired" in c else 2), c
    assert c.get("dead_pads_hit", 1) >= 1, c
    if "common_verdicts" in c:
        assert c["common_verdicts"] + c.get("common_trigger_records", 0) >= 1, c
    assert c.get("baseline_amplitudes", 1) >= 1, c
    assert c.get("thinned_tracks", 1) >= 1, c
    assert c.get("status_0", 4) >= 4 and c.get("status_not_0", 1) >= 1, c
    assert c.get("circle_fits", 1) >= 1, c
    assert c.get("rows_moved", 1) >= 1 and c.get("events_out_of_order", 1) >= 1, c
    assert c.get("helix_ran", 2) >= 2 and c.get("helix_slopes_moved", 1) >= 1, c
    assert c.get("fits_ran", 2) >= 2, c
    assert c.get("fits_ran_fired", 1) >= 1 and c.get("fits_not_fired", 1) >= 1, c
