"""``track_kernel`` (csrc/tracks.hip) against the CPU oracle, sample by sample, on the paths that a launch of one wave
never takes: lanes that take a second and a tenth track, batches of track ids and pools of arena blocks that run out in
the middle of a request, real second batches, ``ode_substeps > 1``, every way a track ends (tests/track_cases.py,
proven on the oracle alone by tests/test_track_cases_cpu.py), the arena's grow-and-rerun and a fused run that mixes good
events with events at the sample limit.  Needs a real MI355X: run with ``-m gpu``.

The rule for one track: ``n_steps`` and ``counts`` equal the oracle's; x, y within 1e-9 m and the
time bucket within 1e-7; electrons equal, except that over a whole test at most ``1 + samples // 10_000_000`` samples may
differ by exactly one primary electron x gain (the Fano draw truncates ``mu + sigma z``, and device log / sincos differ
from glibc in the last bit of z about once in 1e7..1e8 samples).

Tracks of more than 2000 rows accumulate the rounding differences of up to 10^4 RK4 steps (the device contracts
a * b + c into one fma and takes rsqrt where the oracle rounds every operation and divides by a square root), so their
position tolerance is measured, not assumed.  On an MI355X, over the three 10001-row tracks of tests/track_cases.py,
the 18 trapped protons of ``test_long_track_among_short_ones`` (2383 .. 10001 rows) and the 5 path-step tracks of
``test_substeps_vs_oracle`` (2323 .. 5241 rows): largest |device - oracle| of x, y 1.31e-14 m (``path_cap``), of the
time bucket 1.94e-12 -- the differences do not grow along a track.  Asserted: four times that, 5.24e-14 m and 7.76e-12
(``LONG_XY_TOL``, ``LONG_TB_TOL``), with the row counts exact.  The tracks of up to 2000 rows stayed below 6.2e-15 m
and 4.9e-12."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import track_cases as tc
from tests.helpers import Inputs, compare_clouds, sort_cloud

pytestmark = pytest.mark.gpu

XY_TOL, TB_TOL = 1.0e-9, 1.0e-7
LONG_ROWS = 2000
LONG_MEASURED_XY, LONG_MEASURED_TB = 1.31e-14, 1.94e-12  # see above
LONG_XY_TOL, LONG_TB_TOL = 4.0 * LONG_MEASURED_XY, 4.0 * LONG_MEASURED_TB


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _oracle_tracks(orc, inp, p4, vertex, seed, first):
    """[(kept samples [m, 4], ODE rows)] of every track, in the device's order (event, simulated nucleus)."""
    out = []
    for e in range(len(p4)):
        for row in inp.indices:
            sp = inp.layout.species_of_row[row]
            out.append(orc.point_cloud_samples(inp.det_raw, sp, p4[e, row], vertex[e], seed, first + e, row))
    return out


def _device_tracks(ctx, inp, p4, vertex, seed, first, max_samples):
    """(samples [tracks, max_samples, 4], counts, n_steps) of ``attpc_det_tracks``; ``max_samples`` the largest oracle
    count of the test (it only limits the copy)."""
    ctx.forget("det")  # configured through the C ABI directly: the shim's cache no longer describes the device
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


class Tally:
    """What a test compared: printed at its end, and the bound on the Fano flips of the whole test."""

    def __init__(self, what, gain):
        self.what, self.gain = what, float(gain)
        self.tracks = self.samples = self.flips = self.long_tracks = 0
        self.xy = self.tb = self.long_xy = self.long_tb = 0.0

    def track(self, where, mine, count, steps, ref, ref_rows):
        assert steps == ref_rows, (self.what, where, "n_steps", steps, ref_rows)
        assert count == len(ref), (self.what, where, "counts", count, len(ref))
        mine = mine[:count]
        d_xy = float(np.abs(mine[:, :2] - ref[:, :2]).max(initial=0.0))
        d_tb = float(np.abs(mine[:, 2] - ref[:, 2]).max(initial=0.0))
        if ref_rows > LONG_ROWS:
            self.long_tracks += 1
            self.long_xy, self.long_tb = max(self.long_xy, d_xy), max(self.long_tb, d_tb)
            print(self.what, where, "rows", ref_rows, "kept", count, "max |d xy|", d_xy, "max |d tb|", d_tb)
            assert d_xy <= LONG_XY_TOL and d_tb <= LONG_TB_TOL, (self.what, where, ref_rows, d_xy, d_tb)
        else:
            self.xy, self.tb = max(self.xy, d_xy), max(self.tb, d_tb)
            assert d_xy <= XY_TOL and d_tb <= TB_TOL, (self.what, where, ref_rows, d_xy, d_tb)
        differ = mine[:, 3] != ref[:, 3]
        assert (np.abs(mine[differ, 3] - ref[differ, 3]) == self.gain).all(), (self.what, where, mine[differ, 3], ref[differ, 3])
        self.flips += int(differ.sum())
        self.tracks += 1
        self.samples += count

    def all_tracks(self, samples, counts, steps, refs):
        assert len(refs) == len(counts)
        for t, (ref, ref_rows) in enumerate(refs):
            self.track(t, samples[t], counts[t], steps[t], ref, ref_rows)

    def close(self):
        print(f"{self.what}: tracks {self.tracks}, samples compared {self.samples}, Fano flips {self.flips}, "
              f"max |d xy| {self.xy:.3g} m, max |d tb| {self.tb:.3g}; tracks of more than {LONG_ROWS} rows {self.long_tracks}: "
              f"max |d xy| {self.long_xy:.3g} m, max |d tb| {self.long_tb:.3g}")
        assert self.flips <= 1 + self.samples // 10_000_000, (self.what, self.flips, self.samples)


def _gain(inp):
    return int(inp.config.det_params.mpgd_gain)


def _most(refs):
    return max(len(ref) for ref, _ in refs)


# ------------------------------------------------------------------------------------------ one workgroup ----
def test_track_workgroups_option_takes_0_to_65536(ctx):
    for bad in (-1, 65537):
        with pytest.raises(ValueError, match="track_workgroups must be 0..65536"):
            ctx.set_option("track_workgroups", bad)
    for good in (65536, 1, 0):  # (0 last: the default launch for the tests behind this one)
        ctx.set_option("track_workgroups", good)


@pytest.mark.parametrize("name,seed,first,n", tc.REFILL_RUNS, ids=[r[0] for r in tc.REFILL_RUNS])
def test_lanes_refill_and_batches_and_pools_cross(orc, name, seed, first, n):
    """704 and more tracks through ONE workgroup: its 4 waves take 5.5 and more batches of 128 ids (real second batches,
    requests that straddle two batches since tracks end at different steps), every lane takes several tracks, and
    every wave refills its pool of 64 arena blocks more than once.  Nucleus by nucleus and event by event; then the
    default grid, bit for bit."""
    inp = Inputs(name)
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    assert (status == 0).all()
    refs = _oracle_tracks(orc, inp, p4, vertex, seed, first)
    assert len(refs) >= 704
    assert sum(-(-len(ref) // 128) for ref, _ in refs) >= tc.REFILL_MIN_BLOCKS  # twice the 4 x 64 blocks of the first pools
    fresh = _abi.Context(0)
    try:
        fresh.set_option("track_workgroups", 1)
        runs = {}
        for species_major in (1, 0):
            fresh.set_option("track_species_major", species_major)
            runs[species_major] = _device_tracks(fresh, inp, p4, vertex, seed, first, _most(refs))
            tally = Tally(f"{name} one workgroup, species major {species_major}", _gain(inp))
            tally.all_tracks(*runs[species_major], refs)
            tally.close()
        fresh.set_option("track_workgroups", 0)
        for species_major in (1, 0):
            fresh.set_option("track_species_major", species_major)
            default_grid = _device_tracks(fresh, inp, p4, vertex, seed, first, _most(refs))
            for one, many in zip(runs[species_major], default_grid):
                np.testing.assert_array_equal(one, many)
    finally:
        fresh.close()


def test_long_track_among_short_ones(orc):
    """The full-window track and the trapped 3 MeV spiral of test_long_and_degenerate_tracks at events 0, 63 and 200 of
    300 ordinary events, one launch of one workgroup: lanes that start their tenth track run beside lanes at sample
    several thousand (the Fano pairs of a wave are shared among lanes whose sample numbers differ in parity)."""
    inp = tc.inputs("thin")
    n, seed, first = 300, 31, 7
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    assert (status == 0).all()
    full = tc.case("full_window")
    for e, (ke, polar) in ((0, (full.ke, full.polar)), (63, (3.0, np.pi / 2)), (200, (full.ke, full.polar))):
        p4[e, 2] = tc.momentum(tc.MASS["p"], ke, polar, 0.0)
        vertex[e] = full.vertex
    refs = _oracle_tracks(orc, inp, p4, vertex, seed, first)
    assert refs[0][1] == tc.TIME_SAMPLES and refs[200 * 2][1] == tc.TIME_SAMPLES and refs[63 * 2][1] > 1000
    fresh = _abi.Context(0)
    try:
        fresh.set_option("track_workgroups", 1)
        tally = Tally("long tracks among short ones", _gain(inp))
        tally.all_tracks(*_device_tracks(fresh, inp, p4, vertex, seed, first, _most(refs)), refs)
        tally.close()
        assert tally.long_tracks >= 3
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------ endings ----
@pytest.mark.parametrize("detector", sorted({c.detector for c in tc.CASES}))
def test_every_way_a_track_ends(ctx, orc, detector):
    """The cases of tests/track_cases.py, one launch per detector description: against the oracle sample by sample, and
    against the endings written in the table (a device and an oracle that are wrong together at >= versus > still fail
    the table)."""
    inp = tc.inputs(detector)
    cases, p4, vertex = tc.events_of(detector)
    refs = _oracle_tracks(orc, inp, p4, vertex, tc.SEED, 0)
    samples, counts, steps = _device_tracks(ctx, inp, p4, vertex, tc.SEED, 0, _most(refs))
    tally = Tally(f"endings on the {detector} detector", _gain(inp))
    tally.all_tracks(samples, counts, steps, refs)
    tally.close()
    for e, c in enumerate(cases):
        t = e * inp.layout.n_sim + inp.indices.index(c.row)
        assert steps[t] == c.expected[0], (c.name, steps[t], c.expected)
        assert (c.expected[2] == "first") == (steps[t] == 1) and (c.expected[2] == "last") == (steps[t] == tc.TIME_SAMPLES)
        if c.expected[2] == "first":
            assert counts[t] == 0  # the vertex row makes no electrons
    if detector == "thin":
        t = [c.name for c in cases].index("full_window") * inp.layout.n_sim + inp.indices.index(2)
        assert counts[t] > 78 * 128  # the 79th entry of the block table


@pytest.mark.parametrize("name,nsub,path_step,n", tc.SUBSTEP_RUNS)
def test_substeps_vs_oracle(ctx, orc, name, nsub, path_step, n):
    """``ode_substeps`` 2 and 4: tracks whose stop falls in a substep that is not the last are among them
    (tests/test_track_cases_cpu.py::test_some_track_stops_in_a_middle_substep)."""
    inp = Inputs(name, ode_substeps=nsub, **({"path_step": path_step} if path_step else {}))
    vertex, p4, _, _ = orc.kin_batch(inp.kin, tc.SUBSTEP_SEED, tc.SUBSTEP_FIRST, n, threads=8)
    refs = _oracle_tracks(orc, inp, p4, vertex, tc.SUBSTEP_SEED, tc.SUBSTEP_FIRST)
    tally = Tally(f"{name}, {nsub} substeps, path step {path_step}", _gain(inp))
    tally.all_tracks(*_device_tracks(ctx, inp, p4, vertex, tc.SUBSTEP_SEED, tc.SUBSTEP_FIRST, _most(refs)), refs)
    tally.close()
    assert tally.samples > 1000


@pytest.mark.parametrize("detector", ["thin_path_window", "path_cap"])
def test_path_step_window_end_and_cap(ctx, orc, detector):
    """The two path-length tracks that reach the sample cap -- at the end of the 1 us window and after a third of it
    (tests/track_cases.py on why the window cannot end a track earlier) -- through ``attpc_det_tracks`` and through the
    fused tracks + scatter run: ``n_tracks_capped`` counts them, and the cloud is the oracle's."""
    from attpc_engine_amd.detector.simulator import simulate_batch
    inp = tc.inputs(detector)
    cases, p4, vertex = tc.events_of(detector)
    refs = _oracle_tracks(orc, inp, p4, vertex, tc.SEED, 0)
    capped = sum(1 for _, rows in refs if rows == tc.TIME_SAMPLES)
    assert 1 <= capped < len(refs)
    tally = Tally(f"path step on the {detector} detector", _gain(inp))
    tally.all_tracks(*_device_tracks(ctx, inp, p4, vertex, tc.SEED, 0, _most(refs)), refs)
    tally.close()
    offsets, points, labels, stats = simulate_batch(p4, vertex, inp.z, inp.a, inp.config, tc.SEED, inp.indices,
                                                    first_event=0, ctx=ctx)
    assert stats["n_tracks_capped"] == capped, (stats["n_tracks_capped"], capped)
    assert stats["n_failed"] == 0
    for e in range(len(p4)):
        ref_pts, ref_lab, _ = orc.simulate(inp.det_raw, inp.layout, tc.SEED, e, p4[e], vertex[e], capacity=1 << 19)
        compare_clouds(*sort_cloud(points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]),
                       *sort_cloud(ref_pts, ref_lab))
    print(detector, "capped tracks", capped, "of", len(refs), "cloud points", int(offsets[-1]))


# ------------------------------------------------------------------------------------------ arena, dead events ----
def test_arena_grows_under_det_tracks(orc):
    """``tiny_buffers``: the first launch has an arena of 4 blocks, counts the blocks it would have needed with no block
    to write to, and is repeated; the repeated launch is the oracle's, and so is a second call."""
    inp = Inputs("be10dp")
    n, seed, first = 100, 41, 3
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    refs = _oracle_tracks(orc, inp, p4, vertex, seed, first)
    assert sum(-(-len(ref) // 128) for ref, _ in refs) > 4
    fresh = _abi.Context(0)
    try:
        fresh.set_option("tiny_buffers", 1)
        once = _device_tracks(fresh, inp, p4, vertex, seed, first, _most(refs))
        tally = Tally("arena of 4 blocks, grown", _gain(inp))
        tally.all_tracks(*once, refs)
        tally.close()
        again = _device_tracks(fresh, inp, p4, vertex, seed, first, _most(refs))
        for a, b in zip(once, again):
            np.testing.assert_array_equal(a, b)
    finally:
        fresh.close()


def test_fused_run_with_events_at_the_sample_limit(orc):
    """``event_sample_limit = 1`` and an excitation that is forbidden half of the time: the events that hit the limit are
    dead tracks between live ones in every chunk of 64.  They deliver no rows and are counted; the others are the
    oracle's, cloud by cloud and in the sums."""
    from attpc_engine_amd.engine import Engine
    inp = Inputs(tc.sample_limit_workload)
    n, seed, first = tc.LIMIT_EVENTS, tc.LIMIT_SEED, tc.LIMIT_FIRST
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=seed, first=first, n=n, capacity=1 << 22, threads=8)
    failed = ref["status"] != 0
    assert 0.2 * n <= failed.sum() <= 0.8 * n
    fresh = _abi.Context(0)
    try:
        fresh.set_option("deliver_chunk_events", tc.LIMIT_CHUNK)
        eng = Engine(inp.pipeline, inp.config, inp.indices, context=fresh, chunk_events=tc.LIMIT_CHUNK)
        res = eng.run(n, seed=seed, first_event=first, fetch=True)
        resident = eng.run(n, seed=seed, first_event=first)["stats"]
    finally:
        fresh.close()
    st = res["stats"]
    np.testing.assert_array_equal(res["status"] != 0, failed)
    assert st["n_sample_limit"] == failed.sum() == resident["n_sample_limit"]
    sizes = np.diff(res["offsets"])
    assert (sizes[failed] == 0).all()
    np.testing.assert_array_equal(res["offsets"], ref["offsets"])
    for e in np.flatnonzero(~failed):
        lo, hi = ref["offsets"][e], ref["offsets"][e + 1]
        np.testing.assert_allclose(res["p4"][e], ref["p4"][e], rtol=0, atol=1e-9)
        compare_clouds(*sort_cloud(res["points"][lo:hi], res["labels"][lo:hi]),
                       *sort_cloud(ref["points"][lo:hi], ref["labels"][lo:hi]))
    for stats in (st, resident):
        assert stats["n_points"] == ref["stats"][0] and stats["n_track_samples"] == ref["stats"][1]
        assert stats["key_checksum"] == ref["stats"][3] % (1 << 64)
        assert stats["n_failed"] == 0
    print("events", n, "at the sample limit", int(failed.sum()), "cloud points", st["n_points"], "track samples",
          st["n_track_samples"])
