"""The fit hypotheses on the device (``fit_kernel<false, true>``, csrc/fit.hip, and ``hypothesis_selection_kernel``,
csrc/hypothesis.hip) against their restatement (tests/hypothesis_reference.py).  Needs a real MI355X: ``-m gpu``.

f is only compared and copied by the stage, and the fits are those of tests/fit_reference.py, so every comparison here
is exact, over every field of the hypothesis records, the chosen fits and the fits of every hypothesis: integers equal,
f64 bit for bit, NaN in the same places; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.clustering import ClusterSettings
from attpc_engine_amd.detector.estimate import EstimateSettings
from attpc_engine_amd.detector.fit import TrackFitSettings, rows_to_fit
from attpc_engine_amd.detector.hypothesis import (HYPOTHESIS_DTYPE, HypothesisSettings, hypothesis_fits_last,
                                                  rows_to_fit_hypotheses)
from attpc_engine_amd.detector.pid import PidSettings, estimates_to_pid
from attpc_engine_amd.detector.reaction import records_to_reaction
from tests import estimate_reference as est
from tests import fit_cases as cases
from tests import fit_reference as fref
from tests import hypothesis_cases as hc
from tests import hypothesis_reference as href
from tests import pid_reference as pref
from tests import reaction_reference as rref
from tests import thin_reference as thin
from tests.fit_cases import INDICES8
from tests.helpers import Inputs
from tests.test_gpu_estimate import _engine
from tests.test_gpu_fit import CIRCLE, ESTIMATES, FAR_FIRST, FAR_SEED, FUSED, HELIX, N, SEED, THINNING

pytestmark = pytest.mark.gpu

ESTIMATE = EstimateSettings(cases.BEAM_REGION, cases.MIN_POINTS, magnetic_field=hc.FIELD)
FIT = TrackFitSettings(**cases.SETTINGS)
FIT_REF = fref.Settings(**cases.SETTINGS)
EVERY = HypothesisSettings()


@pytest.fixture(scope="module")
def ctx():
    """A context with the detector of be10dp configured: its tables, masses, charges, fields and length are the model."""
    ctx = _abi.Context(0)
    _engine(Inputs("be10dp"), ctx)
    return ctx


def _restated(csr, indices, model, estimates, layout, settings=FIT_REF, beam=cases.BEAM_REGION, start=None, candidates=href.ALL,
              pid=None):
    """(records, chosen fits, the fits of every hypothesis) of the restatement."""
    tried = href.tried(layout, len(estimates), candidates, pid)
    fits = href.all_fits(*csr, indices, model, estimates, settings, beam, layout, tried, start=start)
    records, chosen = href.walk(fits, tried, layout, estimates)
    for array in (records, chosen, fits):
        array.setflags(write=False)
    return records, chosen, fits


def _assert_same(got, want, what=""):
    records, chosen, fits = got[:3]
    assert records.dtype == HYPOTHESIS_DTYPE, what
    href.assert_same(records, want[0])
    href.assert_same_fits(chosen, want[1])
    href.assert_same_fits(fits, want[2])


# ---------------------------------------------------------------- 1. the stage alone, hand-made rows ----
@pytest.fixture(scope="module")
def hand():
    """The hand-made events and what the restatement makes of them from the special starts and from the estimates."""
    model, events, csr, estimates, start, layout = hc.hand()
    want = {given: _restated(csr, INDICES8, model, estimates, layout, start=start if given else None) for given in (True, False)}
    return model, events, csr, estimates, start, layout, want


@pytest.mark.parametrize("given", [True, False], ids=["start=", "start from the estimates"])
def test_stage_alone_on_hand_made_rows(ctx, hand, given):
    model, events, csr, estimates, start, layout, want = hand
    got = rows_to_fit_hypotheses(*csr, cases.layout(), estimates, ctx, FIT, EVERY, start if given else None, estimate_settings=ESTIMATE)
    _assert_same(got, want[given], given)
    records, chosen, fits, species = got
    assert species.tolist() == [0, 1] == layout.hypothesis_species() and fits.shape == (len(events), 8, 2)
    # every hypothesis is the parent's kernel with every position forced to one of the species
    for h, first in enumerate(layout.first):
        forced = np.zeros(estimates.shape, dtype=_abi.PID_DTYPE)
        forced["position"] = first
        alone = rows_to_fit(*csr, cases.layout(), estimates, ctx, FIT, start if given else None, estimate_settings=ESTIMATE, pid=forced)
        assert alone.tobytes() == np.ascontiguousarray(fits[:, :, h]).tobytes(), h
    # the cases are there: the identity assignment of "eight" from the estimates, slots without a fit, a chosen copy
    names = list(events)
    e8, w = names.index("eight"), want[given][0]
    if not given:
        assert w["position"][e8].tolist() == list(range(8)) and (w["status"][e8] == 0).all()
    else:
        assert w["fitted"][e8, 0] == 0 and w["status"][e8, 0] == href.NO_FIT  # (the NaN start: NO_START for every species)
    assert (w["status"][names.index("empty")] == href.NO_FIT).all() and (w["position"][names.index("empty")] == -1).all()
    assert (chosen["status"][names.index("empty")] == href.FIT_NO_PID).all()
    assert (w["position"] >= 0).sum() >= 10 and np.isfinite(w["f_next"]).sum() >= 9
    # one event alone, and no event at all
    i = names.index("single")
    alone = rows_to_fit_hypotheses(*cases.csr([events["single"]]), cases.layout(), estimates[i:i + 1], ctx, FIT, EVERY,
                                   start[i:i + 1] if given else None, estimate_settings=ESTIMATE)
    _assert_same(alone, tuple(part[i:i + 1] for part in want[given]), "single")
    none = rows_to_fit_hypotheses([0], np.zeros((0, 8)), np.zeros(0), cases.layout(), np.zeros((0, 8), dtype=_abi.ESTIMATE_DTYPE), ctx,
                                  FIT, EVERY)
    assert none[0].shape == none[1].shape == (0, 8) and none[2].shape == (0, 8, 2) and none[3].tolist() == [0, 1]


# ---------------------------------------------------------------- 2. item counts that do not fill a wave ----
def _small(ctx, hand, names, indices, species, without=(), candidates=href.ALL):
    model, events, _, _, _, _, _ = hand
    lay = cases.layout(indices, species, without=without)
    csr = cases.csr([events[name] for name in names])
    estimates = est.records(*csr, indices, hc.PARAMS)
    small_model = fref.Model(Inputs("be10dp").det, lay)
    layout = href.Layout(href.species_of_positions(small_model))
    want = _restated(csr, indices, small_model, estimates, layout, candidates=candidates)
    got = rows_to_fit_hypotheses(*csr, lay, estimates, ctx, FIT, HypothesisSettings(candidates), estimate_settings=ESTIMATE)
    _assert_same(got, want, (names, indices))
    assert got[3].tolist() == layout.hypothesis_species()
    return want, layout


def test_item_counts_that_do_not_fill_a_wave(ctx, hand):
    three, species3 = [2, 5, 3], [0, 1, 1]  # the labels of the first three tracks of "eight": p, 11Be, 11Be
    want, layout = _small(ctx, hand, ["eight"], three, species3)  # 3 tracks x 2 hypotheses = 6 items: not a wave's eight
    assert layout.n == 2 and want[0]["position"][0].tolist() == [0, 1, 2] and want[2].shape == (1, 3, 2)
    want, _ = _small(ctx, hand, ["eight", "single", "eight"], three, species3)  # 18 items: two full groups of eight and two more
    assert want[2].shape == (3, 3, 2) and want[0]["position"][2].tolist() == [0, 1, 2]
    # a position without a species is no candidate; a label given twice; one hypothesis alone
    want, layout = _small(ctx, hand, ["eight", "same z"], cases.INDICES_TWICE, cases.SPECIES8, without=(4,))
    assert layout.of_position[7] == -1 and not (want[0]["tried"] & 0x80).any() and (want[0]["tried"] == 0x7F).all()
    # label 2 twice: the second slot of it is empty; the 11Be of the position without a species finds its best taken
    assert want[0]["position"][0].tolist() == [0, 1, 2, -1, 3, 5, 4, 6] and want[0]["status"][0, 3] == href.NO_FIT
    assert want[0]["status"][0, 7] == href.DISPLACED and (want[0]["status"][1] == href.NO_FIT).all()
    want, layout = _small(ctx, hand, ["eight"], [6, 7, 11], [0, 0, 0])
    assert layout.n == 1 and want[2].shape == (1, 3, 1) and want[0]["position"][0].tolist() == [0, 1, 2] and np.isnan(want[0]["f_next"]).all()
    want, _ = _small(ctx, hand, ["eight"], three, species3, candidates=0b010)  # the settings' mask: the 11Be of position 1 alone
    assert want[0]["position"][0].tolist() == [1, -1, -1] and (want[2]["status"][0, :, 0] == href.FIT_NO_PID).all()


# ---------------------------------------------------------------- 3. more groups of items than workgroups ----
def test_more_groups_of_items_than_workgroups(ctx, hand):
    """1 100 events of eight positions and two hypotheses are 2 200 groups of eight items for 1 024 workgroups."""
    _, events, _, estimates, start, _, want = hand
    names = list(events)
    small = [names.index(n) for n in ("single", "empty", "same z")]
    order = np.concatenate([np.random.default_rng(30).choice(small, size=1090), [names.index("eight")] * 4, small[:1] * 6])
    assert len(order) == 1100
    got = rows_to_fit_hypotheses(*cases.csr([events[names[i]] for i in order]), cases.layout(), estimates[order], ctx, FIT, EVERY,
                                 start[order], estimate_settings=ESTIMATE)
    _assert_same(got, tuple(part[order] for part in want[True]))


# ---------------------------------------------------------------- 4. behind the particle identification ----
def test_behind_the_particle_identification(ctx, hand):
    model, events, csr, estimates, _, layout, _ = hand
    pid = estimates_to_pid(estimates, PidSettings(list(hc.PID_GATES)), ctx)
    assert all(np.array_equal(pid[name], hc.hand_pid(estimates)[name]) for name in ("position", "held", "status"))
    before = pid.copy()
    e8 = list(events).index("eight")
    assert pid["held"][e8].tolist() == [1, 1, 2, 3, 2, 0, 2, 2]  # both species for slot 3, one for the others, none for slot 5
    for candidates in (href.ALL, 0b10):
        want = _restated(csr, INDICES8, model, estimates, layout, candidates=candidates, pid=pid)
        got = rows_to_fit_hypotheses(*csr, cases.layout(), estimates, ctx, FIT, HypothesisSettings(candidates), estimate_settings=ESTIMATE,
                                     pid=pid)
        _assert_same(got, want, candidates)
        records, chosen, fits, _ = got
        assert np.array_equal(records["tried"], pid["held"] & candidates)
        for h in range(layout.n):  # a (slot, species) pair outside it has the record without a fit
            positions = sum(1 << p for p in range(8) if layout.of_position[p] == h)
            outside = (records["tried"] & positions) == 0
            assert (fits["status"][:, :, h][outside] == href.FIT_NO_PID).all() and (fits["evaluations"][:, :, h][outside] == 0).all()
            assert not (fits["status"][:, :, h][~outside] & href.FIT_NO_PID).any()
        assert records["status"][e8, 5] == href.NO_CANDIDATE | href.NO_FIT and chosen["status"][e8, 5] == href.FIT_NO_PID
    assert pid.tobytes() == before.tobytes()  # the pid records are what the gates made them


# ---------------------------------------------------------------- 5. the argument checks ----
def test_the_library_checks_its_arguments(ctx):
    lay = cases.layout([2], [0])
    estimates = np.zeros((1, 1), dtype=_abi.ESTIMATE_DTYPE)
    estimates["status"] = _abi.EST_EMPTY
    offsets = np.array([0, 0], dtype=np.int64)
    records, fits = np.empty((1, 1), dtype=HYPOTHESIS_DTYPE), np.empty((1, 1), dtype=_abi.FIT_DTYPE)
    room = np.empty((1, 1, 8), dtype=_abi.FIT_DTYPE)
    good = _abi.HypothesisDesc(0xFF, 0)

    def call(c, desc=good, fit=FIT.desc(), out=records, chosen=fits, everything=room):
        return c.lib.attpc_rows_fit_hypotheses(
            c.handle, 1, _abi.iptr(offsets, _abi.C.c_int64), None, None, lay, _abi.EstimateDesc(25.0, hc.FIELD, 30, 0),
            _abi.iptr(estimates, _abi.TrackEstimate), None, fit, desc, None, _abi.iptr(out, _abi.FitHypothesis),
            _abi.iptr(chosen, _abi.TrackFit), _abi.iptr(everything, _abi.TrackFit), None, None)

    assert call(ctx) == _abi.OK and records["status"][0, 0] == href.NO_FIT and records["tried"][0, 0] == 1
    assert fits["status"][0, 0] == href.FIT_NO_PID and room["status"][0, 0, 0] == _abi.FIT_EMPTY
    assert call(ctx, everything=None) == _abi.OK  # the fits of every hypothesis are optional
    assert call(ctx, desc=None) == _abi.E_INVALID and call(ctx, fit=None) == _abi.E_INVALID
    assert call(ctx, out=None) == _abi.E_INVALID and call(ctx, chosen=None) == _abi.E_INVALID
    for bad in ((0, 0), (1 << 8, 0), (0x1FF, 0), (-1, 0), (1, 1)):
        assert call(ctx, desc=_abi.HypothesisDesc(*bad)) == _abi.E_INVALID, bad
        assert ctx.lib.attpc_trace_configure_hypotheses(ctx.handle, _abi.HypothesisDesc(*bad)) == _abi.E_INVALID, bad
    assert ctx.lib.attpc_trace_configure_hypotheses(ctx.handle, good) == _abi.OK
    assert ctx.lib.attpc_trace_configure_hypotheses(ctx.handle, None) == _abi.OK
    assert ctx.lib.attpc_hypotheses_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED  # no trace-row call has made records
    assert ctx.lib.attpc_hypothesis_fits_last(ctx.handle, 0, 0, None, None) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_hypotheses_last(None, 0, 0, None) == _abi.E_INVALID
    assert call(_abi.Context(0)) == _abi.E_NOTCONFIGURED  # no detector: no model


# ---------------------------------------------------------------- 6. fused ----
RANK = ClusterSettings(match="rank")


def _on(eng, hypotheses=EVERY):
    eng.configure_clustering(RANK)
    eng.configure_estimates(ESTIMATES)
    eng.configure_thinning(THINNING)
    eng.configure_circle_fit(CIRCLE)
    eng.configure_helix_slope(HELIX)
    eng.configure_track_fit(TrackFitSettings(**FUSED))
    eng.configure_fit_hypotheses(hypotheses)


def _off(eng):
    eng.configure_fit_hypotheses()
    eng.configure_track_fit()
    eng.configure_helix_slope()
    eng.configure_circle_fit()
    eng.configure_thinning()
    eng.configure_estimates()
    eng.configure_clustering()


def _want(res, inp):
    """The restatement on the thinned points of the delivered rows under their cluster labels, started from the delivered
    estimate records."""
    points = thin.thin(res["offsets"], res["rows"], res["cluster_labels"], inp.indices, THINNING.z_step)[:3]
    model = fref.Model(inp.det, inp.layout)
    layout = href.Layout(href.species_of_positions(model))
    return _restated(points, inp.indices, model, res["estimates"], layout, fref.Settings(**FUSED), ESTIMATES.beam_region_radius)


@pytest.fixture(scope="module")
def fused():
    """32 events of be10dp with noise and partial readout; clustering by rank, estimates, thinning at 5 mm, circle fit,
    helix slope, the track fit and the hypotheses on: (ctx, inp, the run before the stage was ever configured, the run
    with it, the restatement), read-only."""
    ctx = _abi.Context(0)
    inp = Inputs("be10dp")
    eng = _engine(inp, ctx)
    _on(eng, None)
    never = eng.run_trace_rows(N, seed=SEED)
    _on(eng)
    res = eng.run_trace_rows(N, seed=SEED)
    fits = hypothesis_fits_last(ctx, N, len(inp.indices))
    want = _want(res, inp)
    _off(eng)
    return ctx, inp, never, res, fits, want


def test_fused_records_equal_the_restatement_of_the_delivered_rows(fused):
    ctx, inp, never, res, fits, want = fused
    _assert_same((res["hypotheses"], res["fits"], fits), want, "fused")
    records = want[0]
    assert records.shape == (N, 2) and fits.shape == (N, 2, 2) and (records["position"] >= 0).sum() >= 10
    assert (records["position"] == 0).any() and np.isfinite(records["f_next"]).sum() >= 5
    print("positions by slot:", [np.bincount(records["position"][:, k] + 1, minlength=3).tolist() for k in range(2)],
          "status bits:", np.bincount(records["status"].ravel(), minlength=16).tolist())
    eng = _engine(inp, ctx)
    _on(eng)
    resident = eng.run_trace_rows(N, seed=SEED, fetch=False)
    _assert_same((resident["hypotheses"], resident["fits"], hypothesis_fits_last(ctx, N, 2)), want, "fetch=False")
    assert resident["trace_rows"] == res["trace_rows"] and "rows" not in resident
    alone = eng.run_estimates(N, seed=SEED)
    _assert_same((alone["hypotheses"], alone["fits"], hypothesis_fits_last(ctx, N, 2)), want, "run_estimates")
    _off(eng)


def test_fused_records_do_not_depend_on_calls_or_chunks(fused):
    ctx, inp, never, res, fits, want = fused
    eng = _engine(inp, ctx)
    _on(eng)
    half = N // 2
    halves, half_fits = [], []
    for i in range(2):
        halves.append(eng.run_estimates(half, seed=SEED, first_event=half * i))
        half_fits.append(hypothesis_fits_last(ctx, half, 2))
    _assert_same((np.concatenate([h["hypotheses"] for h in halves]), np.concatenate([h["fits"] for h in halves]),
                  np.concatenate(half_fits)), want, "two calls")
    for chunk in (5, 16):  # 7 chunks of the 32 events, and 2
        small = _engine(inp, ctx, chunk_events=chunk)
        try:
            _on(small)
            chunked = small.run_trace_rows(N, seed=SEED)
            _assert_same((chunked["hypotheses"], chunked["fits"], hypothesis_fits_last(ctx, N, 2)), want, chunk)
            np.testing.assert_array_equal(chunked["rows"], res["rows"])
        finally:
            ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
            _off(small)


def test_fused_at_event_ids_past_2_32(fused):
    ctx, inp = fused[:2]
    eng = _engine(inp, ctx)
    _on(eng)
    far = eng.run_trace_rows(12, seed=FAR_SEED, first_event=FAR_FIRST)
    far_fits = hypothesis_fits_last(ctx, 12, 2)
    want = _want(far, inp)
    _assert_same((far["hypotheses"], far["fits"], far_fits), want, "far")
    assert (want[0]["position"] >= 0).sum() >= 2
    halves = [eng.run_estimates(6, seed=FAR_SEED, first_event=FAR_FIRST + 6 * i) for i in range(2)]
    href.assert_same(np.concatenate([h["hypotheses"] for h in halves]), want[0])
    href.assert_same_fits(np.concatenate([h["fits"] for h in halves]), want[1])
    _off(eng)


# ---------------------------------------------------------------- 7. the reaction reconstruction ----
def test_reaction_reads_the_positions_of_the_stage(fused):
    ctx, inp, never, res, fits, want = fused
    eng = _engine(inp, ctx)
    _on(eng)
    try:
        eng.configure_reaction(track=0, source="fit", ex_range=(-4.0, 12.0), ex_bins=64, theta_bins=36)
        settings = eng._reaction
        on = eng.run_estimates(N, seed=SEED)
        href.assert_same(on["hypotheses"], want[0])
        position = on["hypotheses"]["position"]
        first = np.where((position == 0).any(axis=1), (position == 0).argmax(axis=1), -1)
        print("slot of the proton:", np.bincount(first + 1, minlength=3).tolist())
        assert np.array_equal(on["reaction"]["slot"], first) and (first >= 0).sum() >= 5
        assigned = np.zeros(position.shape, dtype=pref.PID_DTYPE)
        assigned["position"] = position
        restated = rref.records(rref.Settings.of(settings), on["p4"], on["vertex"], on["status"], fits=on["fits"], pid=assigned)
        assert on["reaction"].tobytes() == restated[0].tobytes() and np.array_equal(on["spectra"].cells, restated[1])
        alone = records_to_reaction(settings, on["p4"], on["vertex"], on["status"], fits=on["fits"], pid=assigned, ctx=ctx)
        assert alone[0].tobytes() == on["reaction"].tobytes() and alone[1] == on["spectra"]
        spectra = eng.run_spectra(N, seed=SEED)
        assert spectra["spectra"] == on["spectra"] and set(spectra) == {"spectra", "stats"}
        # a spectra-only call keeps the hypothesis records and the fits of every hypothesis on the device too
        records = np.zeros((1, 2), dtype=HYPOTHESIS_DTYPE)
        assert ctx.lib.attpc_hypotheses_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.FitHypothesis)) == _abi.E_NOTCONFIGURED
        assert ctx.lib.attpc_hypothesis_fits_last(ctx.handle, 0, 0, None, None) == _abi.E_NOTCONFIGURED
        fetched = eng.run_trace_rows(N, seed=SEED)
        assert fetched["reaction"].tobytes() == on["reaction"].tobytes() and fetched["spectra"] == on["spectra"]
    finally:
        eng.configure_reaction()
        _off(eng)


# ---------------------------------------------------------------- 8. off, nothing moves ----
def test_off_nothing_moves(fused):
    ctx, inp, never, res, fits, want = fused
    assert "hypotheses" not in never and "hypotheses" in res
    eng = _engine(inp, ctx)
    _on(eng)
    eng.configure_fit_hypotheses(None)  # on, then off again
    off = eng.run_trace_rows(N, seed=SEED)
    assert "hypotheses" not in off and set(off) == set(never)
    assert ctx.lib.attpc_hypotheses_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_hypothesis_fits_last(ctx.handle, 0, 0, None, None) == _abi.E_NOTCONFIGURED
    for key in ("rows", "labels", "cluster_labels", "offsets", "event_points", "p4", "vertex", "status", "estimates", "fits"):
        assert np.ascontiguousarray(off[key]).tobytes() == np.ascontiguousarray(never[key]).tobytes(), key
    for key in ("rows", "labels", "cluster_labels", "offsets", "event_points", "p4", "vertex", "status", "estimates"):
        assert np.ascontiguousarray(res[key]).tobytes() == np.ascontiguousarray(never[key]).tobytes(), key  # nor does the stage on
    assert off["trace_rows"] == never["trace_rows"] == res["trace_rows"]
    assert off["stats"]["key_checksum"] == never["stats"]["key_checksum"] == res["stats"]["key_checksum"]
    for a, b in zip(off["clusters"], never["clusters"]):
        assert a.tobytes() == b.tobytes()
    # behind the particle identification and the reaction reconstruction: pid and reaction are those of the parent too
    low = (1e-30, 1e30)
    from attpc_engine_amd.detector.pid import Gate

    try:
        eng.configure_pid([Gate.rectangle(low, low), Gate.rectangle(low, low)])
        eng.configure_reaction(track=0, source="fit", ex_range=(-4.0, 12.0), ex_bins=64, theta_bins=36)
        base = eng.run_estimates(N, seed=SEED)
        eng.configure_fit_hypotheses(EVERY)
        on = eng.run_estimates(N, seed=SEED)
        assert on["pid"].tobytes() == base["pid"].tobytes() and np.array_equal(on["hypotheses"]["tried"], on["pid"]["held"] & 3)
        eng.configure_fit_hypotheses(None)
        again = eng.run_estimates(N, seed=SEED)
        assert set(again) == set(base) and "hypotheses" not in again
        for key in ("fits", "pid", "reaction", "estimates"):
            assert again[key].tobytes() == base[key].tobytes(), key
        assert again["spectra"] == base["spectra"] and again["trace_rows"] == base["trace_rows"]
        # without the fit the stage is inert
        eng.configure_fit_hypotheses(EVERY)
        eng.configure_track_fit()
        bare = eng.run_estimates(N, seed=SEED)
        assert "hypotheses" not in bare and "fits" not in bare and bare["pid"].tobytes() == base["pid"].tobytes()
        assert ctx.lib.attpc_hypotheses_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED
    finally:
        eng.configure_pid()
        eng.configure_reaction()
        _off(eng)
    # the file-driven entry points do not take the stage and turn it off on their context
    from attpc_engine_amd.detector import hypothesis as hmod
    from attpc_engine_amd.detector import simulate_batch

    hmod.configure_fit_hypotheses(ctx, EVERY)
    simulate_batch(res["p4"][:2], res["vertex"][:2], inp.z, inp.a, inp.config, SEED, inp.indices, ctx=ctx)
    assert ctx._tokens["hypotheses"] is None
