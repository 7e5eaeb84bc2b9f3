"""The reaction reconstruction on the device (``reaction_kernel``, csrc/reaction.hip) against its restatement
(tests/reaction_reference.py).  Needs a real MI355X: run with ``-m gpu``.

The arithmetic is written operation by operation and the spectra are integer counts (include/attpc_engine.h, "reaction
reconstruction"), so every comparison here is exact: records byte for byte, NaN in the same places, every cell of the
spectra equal; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.clustering import ClusterSettings
from attpc_engine_amd.detector.fit import TrackFitSettings
from attpc_engine_amd.detector.pid import Gate
from attpc_engine_amd.detector.reaction import REACTION_DTYPE, ReactionSettings, ReactionSpectra, records_to_reaction
from tests import reaction_cases as rc
from tests import reaction_reference as pref
from tests.helpers import Inputs
from tests.test_gpu_join import ESTIMATES, PARTIAL, PEAKS, _stages

pytestmark = pytest.mark.gpu

EVENTS, SEED, FIRST = 256, 35, (1 << 32) - 100
FIT = dict(time_step=2e-9, max_steps=600, max_evaluations=3, tolerance_momentum=1e-3, tolerance_position=1e-3)


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.close()


def _same(got, want, what=""):
    records, spectra = got
    want_records, want_cells = want
    assert records.dtype == REACTION_DTYPE and records.shape == want_records.shape, what
    for name in REACTION_DTYPE.names:
        assert np.array_equal(records[name], want_records[name], equal_nan=True), (what, name, np.argwhere(records[name] != want_records[name])[:5].tolist())
    assert records.tobytes() == want_records.tobytes(), what
    assert np.array_equal(spectra.cells, want_cells), (what, np.argwhere(spectra.cells != want_cells)[:5].tolist())


def _device(case: rc.Case, ctx):
    return records_to_reaction(rc.to_settings(case.settings), case.p4, case.vertex, case.status, fits=case.fits,
                               estimates=case.estimates, pid=case.pid, ctx=ctx)


# 1 ------------------------------------------------------------------------------------------ the stage alone ----
@pytest.mark.parametrize("n", rc.EVENT_COUNTS)
def test_synthetic_records_equal_the_restatement(ctx, n):
    seen = 0
    for n_sim in (1, 8):
        for mode in rc.PID_MODES:
            for source in (pref.FROM_FIT, pref.FROM_ESTIMATE):
                for row in (2, 3):
                    case = rc.make(n, n_sim, source, mode, observed_row=row, track=0 if n_sim == 1 else 3)
                    want = rc.reference(case)
                    _same(_device(case, ctx), want, (n, n_sim, mode, source, row))
                    seen |= int(np.bitwise_or.reduce(want[0]["status"]))
    if n >= 63:
        assert seen == 15  # every status bit


def test_pid_absent_in_slot_seven_and_twice(ctx):
    for mode, slots in (("absent", {-1}), ("slot7", {7}), ("twice", set(range(7)))):
        case = rc.make(65, 8, pref.FROM_FIT, mode, track=2)
        got = _device(case, ctx)
        _same(got, rc.reference(case), mode)
        assert set(got[0]["slot"].tolist()) <= slots and (mode != "absent" or np.all(got[0]["status"] & pref.NO_TRACK)), mode
        if mode == "twice":  # the first of the two
            assert np.array_equal(got[0]["slot"], (case.pid["position"] == 2).argmax(axis=1))


def test_one_cell_and_own_cells(ctx):
    one = rc.make(130, 8, cells="one", flags=False)
    records, spectra = _device(one, ctx)
    _same((records, spectra), rc.reference(one), "one cell")
    assert spectra.truth.max() == spectra.truth_reconstructed.max() == spectra.reconstructed.max() == spectra.ex_response.max() == 130
    assert np.count_nonzero(spectra.cells) == 4
    own = rc.make(130, 8, cells="own", flags=False)
    records, spectra = _device(own, ctx)
    _same((records, spectra), rc.reference(own), "own cells")
    assert spectra.truth.max() == 1 and spectra.truth.sum() == 130 and np.array_equal(spectra.truth, spectra.reconstructed)
    assert np.all(spectra.efficiency()[spectra.truth > 0] == 1.0)


def test_values_on_the_edges_of_the_bins(ctx):
    for source in (pref.FROM_FIT, pref.FROM_ESTIMATE):
        case = rc.edge_case(source)
        records, spectra = _device(case, ctx)
        _same((records, spectra), rc.reference(case), ("edges", source))
        assert records["truth_theta_cm"][:3].tolist() == [0.0, pref.PI, 1.5707963267948966]
        assert spectra.truth[:, 0].sum() >= 1 and spectra.truth[:, 18].sum() >= 1 and spectra.outside[0] >= 1  # lo, an interior edge, hi
        if source == pref.FROM_FIT:
            assert records["theta_cm"][:3].tolist() == [0.0, pref.PI, 1.5707963267948966] and np.isnan(records["ex"][3])
        for variant in rc.edge_variants(case):  # Ex at lo, at hi, and at the largest double below hi
            _same(_device(variant, ctx), rc.reference(variant), ("edge bins", source, variant.settings.n_ex, variant.settings.ex_hi))
    for reaction, target in (("o16aa", "none"), ("o16aa", "two"), ("be10dp", "two")):
        case = rc.make(65, 2, reaction=reaction, target=target, track=1, ex_lo=-1.0, ex_hi=31.0, n_ex=256, n_theta=180)
        _same(_device(case, ctx), rc.reference(case), (reaction, target))


def test_the_library_checks_its_arguments(ctx):
    case = rc.make(8, 2)
    settings = rc.to_settings(case.settings)
    records = np.zeros(8, dtype=REACTION_DTYPE)
    cells = np.zeros(settings.n_cells, dtype=np.uint64)
    fits = np.ascontiguousarray(case.fits)

    def call(desc, n=8, n_sim=2, n_rows=4, fits_=fits, p4=case.p4, n_cells=settings.n_cells):
        return ctx.lib.attpc_reaction_records(ctx.handle, n, n_sim, n_rows, desc, _abi.iptr(fits_, _abi.TrackFit), None, None,
                                              _abi.dptr(p4), _abi.dptr(case.vertex), None, _abi.iptr(records, _abi.ReactionRecord),
                                              n_cells, _abi.iptr(cells, _abi.C.c_uint64))

    assert call(settings.desc()) == _abi.OK
    for field, value in (("observed_row", 1), ("observed_row", 4), ("source", 2), ("track", 8), ("n_ex", 257), ("n_theta", 181),
                         ("charge", 0), ("reserved", 1), ("ex_inv_width", 5.0), ("beam_energy", float("nan")), ("eloss_len", 1)):
        desc = settings.desc()
        setattr(desc, field, value)
        assert call(desc) == _abi.E_INVALID, (field, value)
        assert ctx.lib.attpc_reaction_configure(ctx.handle, desc) == _abi.E_INVALID, (field, value)
    assert call(None) == _abi.E_INVALID and call(settings.desc(), n=-1) == _abi.E_INVALID
    assert call(settings.desc(), n_sim=0) == _abi.E_INVALID and call(settings.desc(), n_sim=9) == _abi.E_INVALID
    assert call(settings.desc(), n_rows=3) == _abi.E_INVALID and call(settings.desc(), n_cells=settings.n_cells - 1) == _abi.E_INVALID
    assert call(settings.desc(), fits_=None) == _abi.E_INVALID and call(settings.desc(), p4=None) == _abi.E_INVALID
    far = rc.to_settings(rc.base_settings(track=2))
    assert call(far.desc()) == _abi.E_INVALID  # track 2 of two slots, without pid
    assert call(settings.desc(), n=0) == _abi.OK
    assert ctx.lib.attpc_reaction_last(ctx.handle, 0, 0, None) == _abi.E_NOTCONFIGURED  # no trace-row call has made records
    assert ctx.lib.attpc_reaction_spectra_last(ctx.handle, settings.n_cells, _abi.iptr(cells, _abi.C.c_uint64)) == _abi.E_NOTCONFIGURED


# 2 ------------------------------------------------------------------------------------------ in the run ----
@pytest.fixture(scope="module")
def run(ctx):
    """256 be10dp events, partial readout with noise, clustering in match="truth", thinning, estimates with circle fit
    and helix slope, and the track fit; the reconstruction reads the proton's fit.  (inp, eng, settings, the run with
    the stage off, the run with it on), read-only."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    inp = Inputs("be10dp")
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    eng.configure_traces(inp.config, offset=int(np.argmax(get_response(inp.config))), **PARTIAL)
    eng.configure_peaks(PEAKS)
    eng.configure_estimates(ESTIMATES)
    _stages(eng, True)
    eng.configure_clustering(ClusterSettings(match="truth"))
    eng.configure_track_fit(TrackFitSettings(**FIT))
    off = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)  # (this context has never configured the stage on)
    eng.configure_reaction(track=0, source="fit", ex_range=(-4.0, 12.0), ex_bins=64, theta_bins=36)
    on = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
    return inp, eng, eng._reaction, off, on


def _alone(settings, res, ctx, first=0, count=None, source="fit"):
    stop = None if count is None else first + count
    part = slice(first, stop)
    return records_to_reaction(settings, res["p4"][part], res["vertex"][part], res["status"][part],
                               fits=res["fits"][part] if source == "fit" else None,
                               estimates=res["estimates"][part] if source == "estimate" else None,
                               pid=res["pid"][part] if "pid" in res else None, ctx=ctx)


def _restated(settings, res, source="fit"):
    return pref.records(pref.Settings.of(settings), res["p4"], res["vertex"], res["status"], fits=res["fits"] if source == "fit" else None,
                        estimates=res["estimates"] if source == "estimate" else None, pid=res.get("pid"))


def test_end_to_end(run, ctx):
    inp, eng, settings, off, on = run
    assert settings.observed_row == 2 and settings.charge == 1 and settings.eloss is not None
    assert set(on) - set(off) == {"reaction", "spectra"} and on["reaction"].shape == (EVENTS,)
    for key in ("estimates", "fits", "p4", "vertex", "status"):
        assert on[key].tobytes() == off[key].tobytes(), key
    assert on["trace_rows"] == off["trace_rows"] and on["stats"]["key_checksum"] == off["stats"]["key_checksum"]
    got = (on["reaction"], on["spectra"])
    _same(got, _restated(settings, on), "restatement")
    alone = _alone(settings, on, ctx)
    _same(got, (alone[0], alone[1].cells), "stage alone")
    good = on["reaction"]["status"] == 0
    print("status 0:", int(good.sum()), "of", EVENTS, "statuses", np.bincount(on["reaction"]["status"], minlength=16).tolist())
    print("median Ex - truth:", float(np.median((on["reaction"]["ex"] - on["reaction"]["truth_ex"])[good])) if good.any() else None)
    assert good.sum() >= 1
    assert np.all(on["reaction"]["slot"] == 0) and on["spectra"].truth.sum() + on["spectra"].outside[0] == (on["status"] == 0).sum()
    # the truth beam energy is the one the kinematics used, up to the rounding of the look-up's last operation
    truth = on["reaction"]["truth_beam_ke"][on["status"] == 0]
    want = on["p4"][on["status"] == 0, 1, 3] - settings.masses[1]
    assert np.allclose(truth, want, rtol=0, atol=1e-11)


def test_chunks_resident_and_fetched_runs_give_the_same(run, ctx):
    inp, eng, settings, off, on = run
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 64), "attpc_set_chunk_events")
    try:
        chunked = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    assert chunked["reaction"].tobytes() == on["reaction"].tobytes() and chunked["spectra"] == on["spectra"]
    _same((chunked["reaction"], chunked["spectra"]), _restated(settings, chunked), "chunks of 64")
    # chunks of 16: a track batch holds 8 chunks, so the 256 events are two batches and the second batch's chunks read the
    # truth of the other track set at an offset of their own
    ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 16), "attpc_set_chunk_events")
    try:
        batches = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
    finally:
        ctx.check(ctx.lib.attpc_set_chunk_events(ctx.handle, 0), "attpc_set_chunk_events")
    assert batches["stats"]["launches_tracks"] >= 2, batches["stats"]
    assert batches["reaction"].tobytes() == on["reaction"].tobytes() and batches["spectra"] == on["spectra"]
    _same((batches["reaction"], batches["spectra"]), _restated(settings, batches), "two track batches")
    fetched = eng.run_trace_rows(64, seed=SEED, first_event=FIRST)
    assert "rows" in fetched and fetched["reaction"].tobytes() == on["reaction"][:64].tobytes()
    _same((fetched["reaction"], fetched["spectra"]), _restated(settings, fetched), "fetched")
    resident = eng.run_trace_rows(64, seed=SEED, first_event=FIRST, fetch=False)
    assert resident["reaction"].tobytes() == fetched["reaction"].tobytes() and resident["spectra"] == fetched["spectra"]
    # the range of the reader
    records = np.zeros(4, dtype=REACTION_DTYPE)
    ctx.check(ctx.lib.attpc_reaction_last(ctx.handle, 60, 4, _abi.iptr(records, _abi.ReactionRecord)), "attpc_reaction_last")
    assert records.tobytes() == on["reaction"][60:64].tobytes()
    assert ctx.lib.attpc_reaction_last(ctx.handle, 61, 4, _abi.iptr(records, _abi.ReactionRecord)) == _abi.E_INVALID
    cells = np.zeros(settings.n_cells + 1, dtype=np.uint64)
    assert ctx.lib.attpc_reaction_spectra_last(ctx.handle, settings.n_cells + 1, _abi.iptr(cells, _abi.C.c_uint64)) == _abi.E_INVALID


def test_spectra_of_disjoint_ranges_add(run, ctx):
    inp, eng, settings, off, on = run
    first, second = eng.run_spectra(128, seed=SEED, first_event=FIRST), eng.run_spectra(128, seed=SEED, first_event=FIRST + 128)
    assert set(first) == {"spectra", "stats"} and isinstance(first["spectra"], ReactionSpectra)
    assert first["spectra"] + second["spectra"] == on["spectra"]
    assert first["spectra"] != on["spectra"] and first["spectra"].cells.sum() > 0
    # a spectra-only call copies no record to the host: the readers have nothing of it, the spectra are the same
    whole = eng.run_spectra(EVENTS, seed=SEED, first_event=FIRST)
    assert whole["spectra"] == on["spectra"]
    n_sim = len(inp.indices)
    estimates, fits = np.zeros((1, n_sim), dtype=_abi.ESTIMATE_DTYPE), np.zeros((1, n_sim), dtype=_abi.FIT_DTYPE)
    records = np.zeros(1, dtype=REACTION_DTYPE)
    assert ctx.lib.attpc_estimates_last(ctx.handle, 0, 1, _abi.iptr(estimates, _abi.TrackEstimate)) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_fits_last(ctx.handle, 0, 1, _abi.iptr(fits, _abi.TrackFit)) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_reaction_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.ReactionRecord)) == _abi.E_NOTCONFIGURED
    assert ctx.lib.attpc_clusters_last(ctx.handle, 0, 0, None, None) == _abi.E_NOTCONFIGURED
    cells = np.zeros(settings.n_cells, dtype=np.uint64)
    ctx.check(ctx.lib.attpc_reaction_spectra_last(ctx.handle, settings.n_cells, _abi.iptr(cells, _abi.C.c_uint64)), "attpc_reaction_spectra_last")
    assert np.array_equal(cells, on["spectra"].cells)
    # ... and the option is the call's alone: the next run has its records again
    after = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
    for key in ("estimates", "fits", "reaction"):
        assert after[key].tobytes() == on[key].tobytes(), key
    assert after["spectra"] == on["spectra"] and after["clusters"][0].tobytes() == on["clusters"][0].tobytes()
    assert ctx.lib.attpc_set_option(ctx.handle, b"reaction_spectra_only", 1) == _abi.OK
    try:  # without the stage the option does nothing
        eng.configure_reaction()
        plain = eng.run_estimates(64, seed=SEED, first_event=FIRST)
        assert plain["estimates"].tobytes() == on["estimates"][:64].tobytes() and "reaction" not in plain
    finally:
        assert ctx.lib.attpc_set_option(ctx.handle, b"reaction_spectra_only", 0) == _abi.OK
        eng.configure_reaction(settings)


def test_estimate_source_and_rank_with_pid(run, ctx):
    inp, eng, settings, off, on = run
    try:
        eng.configure_reaction(track=0, source="estimate", ex_range=(-4.0, 12.0))
        res = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        _same((res["reaction"], res["spectra"]), _restated(eng._reaction, res, "estimate"), "estimate source")
        alone = _alone(eng._reaction, res, ctx, source="estimate")
        _same((res["reaction"], res["spectra"]), (alone[0], alone[1].cells), "estimate source alone")
        assert res["fits"].tobytes() == on["fits"].tobytes() and (res["reaction"]["status"] == 0).sum() >= 1
        # the same events label-free: clusters by rank, the species from two box gates
        eng.configure_reaction(settings)
        eng.configure_clustering(ClusterSettings(match="rank"))
        brho = on["estimates"]["brho"]
        cut = float(np.nanmedian(brho[:, 0]) + np.nanmedian(brho[:, 1])) / 2.0
        low, high = Gate.rectangle((1e-30, cut), (1e-30, 1e30)), Gate.rectangle((cut, 1e30), (1e-30, 1e30))
        proton_low = np.nanmedian(brho[:, 0]) < np.nanmedian(brho[:, 1])
        eng.configure_pid([low, high] if proton_low else [high, low])
        ranked = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        assert "pid" in ranked
        _same((ranked["reaction"], ranked["spectra"]), _restated(settings, ranked), "rank + pid")
        alone = _alone(settings, ranked, ctx)
        _same((ranked["reaction"], ranked["spectra"]), (alone[0], alone[1].cells), "rank + pid alone")
        slot = ranked["reaction"]["slot"]
        print("rank + pid: slots", np.bincount(slot + 1, minlength=3).tolist(), "status 0:", int((ranked["reaction"]["status"] == 0).sum()))
        assert (slot >= 0).sum() >= 1 and np.all(ranked["pid"]["position"][slot >= 0, slot[slot >= 0]] == 0)
        assert np.all((ranked["reaction"]["status"][slot < 0] & pref.NO_TRACK) != 0)
    finally:
        eng.configure_pid()
        eng.configure_clustering(ClusterSettings(match="truth"))
        eng.configure_reaction(settings)


def test_stage_off_and_without_its_source(run, ctx):
    inp, eng, settings, off, on = run
    records = np.zeros(1, dtype=REACTION_DTYPE)
    try:
        eng.configure_reaction()
        again = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
        assert set(again) == set(off) == {"indices", "vertex", "p4", "status", "stats", "trace_rows", "estimates", "thinning", "circle",
                                          "slope", "fits", "clusters"}, sorted(off)  # the parent's keys in this configuration
        for key in ("estimates", "fits", "p4", "vertex", "status"):
            assert again[key].tobytes() == off[key].tobytes(), key
        assert ctx.lib.attpc_reaction_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.ReactionRecord)) == _abi.E_NOTCONFIGURED
        with pytest.raises(RuntimeError):
            eng.run_spectra(8, seed=SEED, first_event=FIRST)
        # on, but the fit it reads is off: inert
        eng.configure_reaction(settings)
        eng.configure_track_fit()
        bare = eng.run_estimates(32, seed=SEED, first_event=FIRST)
        assert "reaction" not in bare and "spectra" not in bare and "fits" not in bare
        assert ctx.lib.attpc_reaction_last(ctx.handle, 0, 1, _abi.iptr(records, _abi.ReactionRecord)) == _abi.E_NOTCONFIGURED
        with pytest.raises(RuntimeError):
            eng.run_spectra(8, seed=SEED, first_event=FIRST)
        # a track that is not a position of the layout is refused by the run
        eng.configure_track_fit(TrackFitSettings(**FIT))
        far = ReactionSettings(settings.masses, 1, settings.beam_energy, (settings.z_min, settings.z_max, settings.eloss), track=5)
        with pytest.raises(ValueError, match="track 5"):
            eng.configure_reaction(far)  # (the engine knows its indices)
        eng._reaction = far  # ... and the library refuses the run of whoever does not
        with pytest.raises(ValueError, match="track"):
            eng.run_estimates(8, seed=SEED, first_event=FIRST)
        # position 0 is the proton, row 2: settings that call it row 3 would read its fit with the 11Be's mass
        wrong = ReactionSettings(settings.masses, 4, settings.beam_energy, (settings.z_min, settings.z_max, settings.eloss), track=0,
                                 observed_row=3)
        with pytest.raises(ValueError, match="row 3"):
            eng.configure_reaction(wrong)
        eng._reaction = wrong
        with pytest.raises(ValueError, match="observed_row"):
            eng.run_estimates(8, seed=SEED, first_event=FIRST)
        estimates = np.zeros((1, len(inp.indices)), dtype=_abi.ESTIMATE_DTYPE)
        assert ctx.lib.attpc_estimates_last(ctx.handle, 0, 1, _abi.iptr(estimates, _abi.TrackEstimate)) == _abi.E_NOTCONFIGURED
    finally:
        eng.configure_track_fit(TrackFitSettings(**FIT))
        eng.configure_reaction(settings)


def test_the_context_holds_this_engines_settings_for_its_runs(run, ctx):
    """Another owner of the context may replace or remove the stage; a run of the engine applies its own again, and the
    file-driven entry points, which do not take the stage, turn it off."""
    from attpc_engine_amd.detector import reaction as rmod
    from attpc_engine_amd.detector import simulate_batch

    inp, eng, settings, off, on = run
    rmod.configure_reaction(ctx, None)
    again = eng.run_estimates(EVENTS, seed=SEED, first_event=FIRST)
    assert again["reaction"].tobytes() == on["reaction"].tobytes() and again["spectra"] == on["spectra"]
    other = ReactionSettings(settings.masses, 1, settings.beam_energy, None, ex_range=(0.0, 1.0), ex_bins=3, theta_bins=5)
    rmod.configure_reaction(ctx, other)
    again = eng.run_trace_rows(64, seed=SEED, first_event=FIRST, fetch=False)
    assert again["reaction"].tobytes() == on["reaction"][:64].tobytes() and again["spectra"].settings is settings
    assert ctx._tokens["reaction"] == settings.token()
    simulate_batch(on["p4"][:2], on["vertex"][:2], inp.z, inp.a, inp.config, SEED, inp.indices, ctx=ctx)
    assert ctx._tokens["reaction"] is None
