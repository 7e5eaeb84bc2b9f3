"""The track straggling on the device (``track_kernel<*, true>``, csrc/tracks.hip) against its restatement
(tests/straggle_reference.py), sample by sample, through ``attpc_det_tracks`` unless said.  Needs a real MI355X: run
with ``-m gpu``.

The rule for one track is that of tests/test_gpu_track_paths.py: ``n_steps`` and ``counts`` equal the reference's,
electrons equal except for at most ``1 + samples // 10_000_000`` samples of a test that differ by exactly one primary
electron x gain, positions and time buckets within a tolerance that is measured, not assumed: four times the largest
|device - reference| seen on an MI355X over the five passes of ``test_samples_against_the_reference`` (tests/
straggle_cases.py), the clamp and the id case.

Measured on an MI355X (260 tracks per pass; largest |d x, y| in m, largest |d time bucket|; no Fano flip anywhere):
  angular 1.50e-14, 4.04e-12; energy 1.12e-14, 2.67e-12; both 1.17e-14, 4.41e-12; substeps2 1.63e-14, 3.78e-12;
  path_step (170 518 samples, tracks of up to 4911 rows) 1.08e-13, 1.45e-11; the clamp 3.47e-17, 1.14e-13; the ids
  4.08e-15, 6.75e-13.
Asserted: ``XY_TOL`` = 4 x 1.08e-13 m and ``TB_TOL`` = 4 x 1.45e-11, more than three orders of magnitude below the
1e-9 m of test_tracks_vs_oracle.  The unkicked tracks of tests/test_gpu_track_paths.py differ by 1.31e-14 m and
1.94e-12; with the kick the differences of the grid passes are of that size, those of the path-length pass (three
times the samples and the kicks per track) eight times larger."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import straggle_cases as sc
from tests import straggle_reference as sr
from tests import track_cases as tc
from tests.helpers import Inputs, id_case, sort_cloud

pytestmark = pytest.mark.gpu

MEASURED_XY, MEASURED_TB = 1.08e-13, 1.45e-11  # see above
XY_TOL, TB_TOL = 4.0 * MEASURED_XY, 4.0 * MEASURED_TB


@pytest.fixture(scope="module")
def ctx():
    context = _abi.Context(0)
    yield context
    context.check(context.lib.attpc_det_configure_straggling(context.handle, None), "attpc_det_configure_straggling")
    context.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _desc(settings: sr.Settings):
    return _abi.StraggleDesc(settings.angular_scale, settings.energy_scale, settings.radiation_length,
                             settings.electron_density, settings.stream)


def _straggling(ctx, settings):
    """``attpc_det_configure_straggling`` through the C ABI directly (None: NULL, the stage off)."""
    ctx.forget("straggling")
    ctx.check(ctx.lib.attpc_det_configure_straggling(ctx.handle, None if settings is None else _desc(settings)),
              "attpc_det_configure_straggling")


def _device_tracks(ctx, inp, p4, vertex, seed, first, max_samples):
    """(samples [tracks, max_samples, 4], counts, n_steps) of ``attpc_det_tracks``."""
    ctx.forget("det")
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, inp.det), "det_configure")
    n = len(p4)
    nt = n * inp.layout.n_sim
    samples = np.zeros((nt, max(1, max_samples), 4))
    counts = np.empty(nt, dtype=np.int32)
    steps = np.empty(nt, dtype=np.int32)
    ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, seed, first, n, inp.layout, _abi.dptr(np.ascontiguousarray(p4)),
                                       _abi.dptr(np.ascontiguousarray(vertex)), max(1, max_samples), _abi.dptr(samples),
                                       _abi.iptr(counts, _abi.C.c_int32), _abi.iptr(steps, _abi.C.c_int32)), "tracks")
    return samples, counts, steps


def _compare(what, gain, device, refs):
    """The rule of the module docstring over all tracks of a launch -> (samples compared, max |d xy|, max |d tb|);
    every figure is printed before anything is asserted."""
    samples, counts, steps = device
    assert len(refs) == len(counts)
    worst_xy = worst_tb = 0.0
    flips = compared = 0
    wrong = []
    for t, (ref, ref_rows, _) in enumerate(refs):
        if steps[t] != ref_rows or counts[t] != len(ref):
            wrong.append((t, int(steps[t]), ref_rows, int(counts[t]), len(ref)))
            continue
        mine = samples[t, :counts[t]]
        worst_xy = max(worst_xy, float(np.abs(mine[:, :2] - ref[:, :2]).max(initial=0.0)))
        worst_tb = max(worst_tb, float(np.abs(mine[:, 2] - ref[:, 2]).max(initial=0.0)))
        differ = mine[:, 3] != ref[:, 3]
        assert (np.abs(mine[differ, 3] - ref[differ, 3]) == float(gain)).all(), (what, t, mine[differ, 3], ref[differ, 3])
        flips += int(differ.sum())
        compared += int(counts[t])
    print(f"{what}: tracks {len(refs)}, samples compared {compared}, Fano flips {flips}, max |d xy| {worst_xy:.3g} m, "
          f"max |d tb| {worst_tb:.3g}, tracks of another length {wrong}")
    assert not wrong, (what, wrong)
    assert flips <= 1 + compared // 10_000_000, (what, flips, compared)
    assert worst_xy <= XY_TOL and worst_tb <= TB_TOL, (what, worst_xy, worst_tb)
    return compared, worst_xy, worst_tb


# 1 ------------------------------------------------------------------------------------------ off is off ----
def test_both_scales_zero_and_null_equal_unconfigured(ctx, orc):
    inp = Inputs("be10dp")
    seed, first, n = 13, 5, 8
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    gas = sc.settings_of(inp, (1.0, 1.0))
    _straggling(ctx, None)
    plain = _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)
    assert plain[1].sum() > 100
    _straggling(ctx, sr.Settings(0.0, 0.0, gas.radiation_length, gas.electron_density, 7))
    for a, b in zip(plain, _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)):
        np.testing.assert_array_equal(a, b)
    _straggling(ctx, gas)
    on = _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)
    assert not np.array_equal(on[0], plain[0])
    # reconfiguring the detector keeps the stage (_device_tracks does), NULL drops it
    again = _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)
    for a, b in zip(on, again):
        np.testing.assert_array_equal(a, b)
    _straggling(ctx, None)
    for a, b in zip(plain, _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)):
        np.testing.assert_array_equal(a, b)
    for bad in (sr.Settings(-1.0, 1.0, 1.0, 1.0), sr.Settings(1.0, np.nan, 1.0, 1.0), sr.Settings(1.0, 1.0, 0.0, 1.0),
                sr.Settings(1.0, 1.0, 1.0, np.inf), sr.Settings(1.0, 1.0, 1.0, 1.0, 65536)):
        assert ctx.lib.attpc_det_configure_straggling(ctx.handle, _desc(bad)) == _abi.E_INVALID, bad


# 2 ------------------------------------------------------------------------------------------ samples ----
@pytest.mark.parametrize("name", list(sc.PASSES))
def test_samples_against_the_reference(ctx, orc, name):
    """260 tracks of be10dp, the kick's parts alone and together, two substeps and the path-length step."""
    inp, settings, p4, vertex, refs = sc.pass_references(orc, name)
    margin = min(info["margin"] for _, _, info in refs)
    print(name, "smallest margin to a terminal event", margin)
    assert margin > sc.MIN_MARGIN  # (tests/test_straggling_cpu.py: no track may legitimately end a step apart)
    _straggling(ctx, settings)
    device = _device_tracks(ctx, inp, p4, vertex, sc.SEED, sc.FIRST, max(len(ref) for ref, _, _ in refs))
    compared, _, _ = _compare(name, inp.config.det_params.mpgd_gain, device, refs)
    assert compared > 10000
    # the kick is not a no-op: the lengths of the unkicked tracks are not these
    _straggling(ctx, None)
    _, _, plain_steps = _device_tracks(ctx, inp, p4, vertex, sc.SEED, sc.FIRST, 1)
    assert (plain_steps != device[2]).sum() > 20


# 3 ------------------------------------------------------------------------------------------ the clamp ----
def test_clamp_ends_the_track_through_the_ke_event(ctx, orc):
    inp, p4, vertex = sc.clamp_event()
    settings = sc.settings_of(inp, (1.0, sc.CLAMP_ENERGY_SCALE))
    refs = sr.reference_tracks(orc, inp, p4, vertex, sc.CLAMP_SEED, sc.CLAMP_EVENT, settings)
    be11 = inp.indices.index(tc.ROW["be11"])
    _, rows, info = refs[be11]
    unkicked = orc.point_cloud_samples(inp.det_raw, inp.layout.species_of_row[tc.ROW["be11"]], p4[0, tc.ROW["be11"]],
                                       vertex[0], sc.CLAMP_SEED, sc.CLAMP_EVENT, tc.ROW["be11"])[1]
    assert info["clamped"] == rows - 1 and info["events"] == ["ke"] and rows < unkicked, (info, rows, unkicked)
    _straggling(ctx, settings)
    device = _device_tracks(ctx, inp, p4, vertex, sc.CLAMP_SEED, sc.CLAMP_EVENT, max(len(ref) for ref, _, _ in refs))
    _compare("clamp", inp.config.det_params.mpgd_gain, device, refs)
    assert device[2][be11] == rows
    np.testing.assert_allclose(device[0][be11, device[1][be11] - 1, :3], refs[be11][0][-1, :3], rtol=0, atol=TB_TOL)


# 4 ------------------------------------------------------------------------------------------ ids and seeds ----
def test_high_words_of_ids_and_seeds(ctx, orc):
    """8 events from 2^32 - 4 with a seed whose high word is set: the high words reach the new domain's counters."""
    case = id_case("u32_wrap")
    seed, first, n = case.seed, (1 << 32) - 4, 8
    assert seed >> 32
    inp = sc.pass_inputs("both")
    settings = sc.settings_of(inp, (1.0, 1.0))
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    assert (status == 0).all()
    refs = sr.reference_tracks(orc, inp, p4, vertex, seed, first, settings)
    _straggling(ctx, settings)
    device = _device_tracks(ctx, inp, p4, vertex, seed, first, max(len(ref) for ref, _, _ in refs))
    _compare("ids", inp.config.det_params.mpgd_gain, device, refs)
    # (the events from 2^32 on would repeat those from 0 on, and the seed be another, if a high word were dropped: the
    #  reference above has both; and the seed's high word does reach the kick)
    other = _device_tracks(ctx, inp, p4, vertex, seed & 0xffffffff, first, device[0].shape[1])
    assert not np.array_equal(other[0], device[0])


# 5 ------------------------------------------------------------------------------------------ streams ----
def test_streams_differ_and_repeat(ctx, orc):
    inp = sc.pass_inputs("both")
    seed, first, n = 13, 5, 8
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    runs = {}
    for stream in (0, 1, 0, 1):
        _straggling(ctx, sc.settings_of(inp, (1.0, 1.0), stream))
        got = _device_tracks(ctx, inp, p4, vertex, seed, first, tc.TIME_SAMPLES)
        if stream in runs:
            for a, b in zip(runs[stream], got):
                np.testing.assert_array_equal(a, b)
        runs[stream] = got
    assert not np.array_equal(runs[0][0], runs[1][0])


# 6 ------------------------------------------------------------------------------------------ the full path ----
def _sorted_events(res):
    return [sort_cloud(res["points"][lo:hi], res["labels"][lo:hi]) for lo, hi in zip(res["offsets"][:-1], res["offsets"][1:])]


def test_full_path_is_a_pure_function_of_the_event():
    """``Engine.run(fetch=True)`` with the stage on, 24 events of o16aa: one call, two calls of 12 and chunks of 5
    events give the same clouds and checksums bit for bit; ``run_trace_rows`` with the estimates and the thinning on
    gives the same records across the split."""
    from attpc_engine_amd.engine import Engine
    inp = Inputs("o16aa")
    seed, first, n = 17, (1 << 32) - 10, 24
    fresh = _abi.Context(0)
    try:
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=fresh)
        off = eng.run(n, seed=seed, first_event=first, fetch=True)
        eng.configure_straggling(stream=3)
        whole = eng.run(n, seed=seed, first_event=first, fetch=True)
        assert whole["stats"]["key_checksum"] != off["stats"]["key_checksum"]
        resident = eng.run(n, seed=seed, first_event=first)["stats"]
        halves = [eng.run(12, seed=seed, first_event=first + lo, fetch=True) for lo in (0, 12)]
        fresh.check(fresh.lib.attpc_set_chunk_events(fresh.handle, 5), "attpc_set_chunk_events")
        chunked = eng.run(n, seed=seed, first_event=first, fetch=True)
        fresh.check(fresh.lib.attpc_set_chunk_events(fresh.handle, 0), "attpc_set_chunk_events")
        events = _sorted_events(whole)
        assert sum(len(p) for p, _ in events) > 1000
        for other in (_sorted_events(chunked), _sorted_events(halves[0]) + _sorted_events(halves[1])):
            assert len(other) == n
            for (pa, la), (pb, lb) in zip(events, other):
                np.testing.assert_array_equal(pa, pb)
                np.testing.assert_array_equal(la, lb)
        mask = (1 << 64) - 1
        for key in ("charge_checksum", "key_checksum"):
            assert whole["stats"][key] == resident[key] == chunked["stats"][key], key
            assert whole["stats"][key] == (halves[0]["stats"][key] + halves[1]["stats"][key]) & mask, key
        for key in ("n_points", "n_track_samples"):
            assert whole["stats"][key] == resident[key] == chunked["stats"][key] == halves[0]["stats"][key] + halves[1]["stats"][key]
        # trace rows with estimates and thinning
        eng.configure_estimates(min_points=10)
        eng.configure_thinning(z_step=10)
        rows = eng.run_trace_rows(n, seed=seed, first_event=first)
        parts = [eng.run_trace_rows(12, seed=seed, first_event=first + lo) for lo in (0, 12)]
        assert rows["estimates"].shape == (n, len(inp.indices)) and rows["trace_rows"]["n_rows"] > 100
        assert rows["estimates"].tobytes() == np.concatenate([p["estimates"] for p in parts]).tobytes()
        np.testing.assert_array_equal(rows["rows"], np.concatenate([p["rows"] for p in parts]))
        eng.configure_straggling()
        assert eng.run_trace_rows(n, seed=seed, first_event=first)["estimates"].tobytes() != rows["estimates"].tobytes()
        # the file-driven form: the same kinematics through simulate_batch(straggling=) give the same clouds, and a
        # call without the keyword runs with the stage off again
        from attpc_engine_amd.detector.simulator import simulate_batch
        from attpc_engine_amd.detector.straggling import StragglingSettings
        args = (whole["p4"], whole["vertex"], inp.z, inp.a, inp.config, seed, inp.indices)
        for want, settings in ((whole, StragglingSettings(stream=3)), (off, None), (off, StragglingSettings(0.0, 0.0))):
            offsets, points, labels, stats = simulate_batch(*args, first_event=first, ctx=fresh, straggling=settings)
            np.testing.assert_array_equal(offsets, want["offsets"])
            got = {"offsets": offsets, "points": points, "labels": labels}
            for (pa, la), (pb, lb) in zip(_sorted_events(want), _sorted_events(got)):
                np.testing.assert_array_equal(pa, pb)
                np.testing.assert_array_equal(la, lb)
            assert stats["key_checksum"] == want["stats"]["key_checksum"]
    finally:
        fresh.close()
