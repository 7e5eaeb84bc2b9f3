"""The laws of the device's random draws, from what a user gets back: the runs of tests/law_cases.py through the
analysis of tests/law_analysis.py, exactly as tests/test_laws_cpu.py holds the oracle to them (and shows, with one law
broken at a time, that each check can fail).  An unmutated law asserts p >= 1e-6, an independence check |corr_z| <= 5
(tests/law_checks.py).  No scipy here, and nothing but numpy between the device's arrays and the statistic; the Fano
means come from the oracle's trajectory rows, which no draw enters.  Figures and wall times: profiles/r25_draw_laws.md
(``-s`` prints them).  Needs a real MI355X: run with ``-m gpu``."""
import time

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.simulator import simulate_batch
from attpc_engine_amd.engine import Engine
from tests import law_analysis as la
from tests import law_cases as cases
from tests import law_checks as lc
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


class _Clock:
    def __init__(self, what):
        self.what, self.t0 = what, time.perf_counter()

    def lap(self, stage):
        print(f"  [{self.what}] {stage}: {time.perf_counter() - self.t0:.2f} s since the test began")


def _run(inp, n, seed, first=0):
    vertex, p4, status, attempts = inp.pipeline.run_many(n, first_event=first, seed=seed, return_status=True)
    assert (status == 0).all()
    return vertex, p4, attempts


def test_k1_o16aa_as_the_workload_defines_it(ctx):
    clock = _Clock("K1")
    inp = Inputs("o16aa", context=ctx)
    m = cases.masses_of(inp.kin)
    cols = []
    for seed in (cases.K1_SEED, cases.K1_SEED + cases.HI):
        vertex, p4, _ = _run(inp, cases.K1_N, seed)
        cols.append(la.k1_columns(vertex, p4, m, **cases.K1_LAW))
    clock.lap("two device runs and their columns")
    ks = la.ks_all(cols[0])
    off = lc.corr_matrix_z(cols[0])
    lag = la.lag1(cols[0])
    cross = la.cross(*cols)
    print(f"\nK1 device: n {cases.K1_N}")
    for k, (n, d, p) in ks.items():
        print(f"  {k}: D {d:.3g} p {p:.3g}")
    worst_lag = max(abs(v) for v in lag.values())
    print(f"  largest off-diagonal |corr_z| {off[0]:.3g} {off[1]}; lag-1 max {worst_lag:.3g}; seed vs seed + 2^32 max "
          f"{cross[0]:.3g} {cross[1]}")
    clock.lap("done")
    assert all(p >= lc.P_PASS for _, _, p in ks.values()), ks
    assert off[0] <= lc.Z_PASS and worst_lag <= lc.Z_PASS and cross[0] <= lc.Z_PASS, (off, lag, cross)


def test_k2_tabulated_and_binned_samplers(ctx):
    """(test_laws_cpu.py::test_k2_table_error_is_below_the_ks_resolution holds the table's own error to a tenth of the
    resolution of this size.)"""
    clock = _Clock("K2")
    inp = Inputs(cases.k2, context=ctx)
    _, p4, attempts = _run(inp, cases.K2_N, cases.K2_SEED)
    clock.lap("device run")
    out = la.k2_checks(p4, attempts, cases.masses_of(inp.kin), cases.K2_BEAM, cases.k2_bw(), cases.K2_ANGLES,
                       cases.K2_PROBS, cases.K2_BIN_WIDTH, cases.K2_PIT_SEED)
    print(f"\nK2 device: n {len(p4)}; ex D {out['ex'][1]:.3g} p {out['ex'][2]:.3g}; attempts chi2 {out['attempts'][0]:.3g} "
          f"dof {out['attempts'][1]} p {out['attempts'][2]:.3g} (mean {out['mean_attempts'][0]:.6f}, 1/F {out['mean_attempts'][1]:.6f}); "
          f"bin chi2 {out['bin'][0]:.3g} dof {out['bin'][1]} p {out['bin'][2]:.3g}; offset D {out['offset'][1]:.3g} "
          f"p {out['offset'][2]:.3g}; bin vs offset corr_z {out['bin_offset_z']:.3g}")
    clock.lap("done")
    assert min(out["ex"][2], out["attempts"][2], out["bin"][2], out["offset"][2]) >= lc.P_PASS, out
    assert abs(out["bin_offset_z"]) <= lc.Z_PASS, out


def test_k3_the_rejection_loop_keeps_the_shape(ctx):
    """(test_laws_cpu.py::test_k3_ranges_make_both_steps_refuse shows the conditions on the ranges.)  An engine that
    resampled only the failed step would pass every invariant and fail the marginal of ex0."""
    clock = _Clock("K3")
    inp = Inputs(cases.k3, context=ctx)
    law = la.K3Law(cases.masses_of(inp.kin), cases.K3_BEAM, cases.K3_RANGE0, cases.K3_RANGE1)
    _, p4, attempts = _run(inp, cases.K3_N, cases.K3_SEED)
    clock.lap("device run")
    out = law.checks(p4, attempts)
    print(f"\nK3 device: n {len(p4)}, outside the allowed set {out['outside_allowed_set']}")
    for k, (n, d, p) in out["ks"].items():
        print(f"  {k}: D {d:.3g} p {p:.3g}")
    print(f"  attempts chi2 {out['attempts'][0]:.4g} dof {out['attempts'][1]} p {out['attempts'][2]:.3g} (mean "
          f"{np.mean(attempts):.5f}, 1/p {1 / law.p_accept:.5f}); angles among attempts >= 2: smallest KS p {min(p for _, _, p in out['ks_retried'].values()):.3g}, vs ex: n "
          f"{out['angles_vs_ex_retried'][0]} max |corr_z| {out['angles_vs_ex_retried'][1]:.3g} {out['angles_vs_ex_retried'][2]}; "
          f"PIT(ex0) vs PIT(ex1 | ex0) corr_z {out['ex0_ex1_z']:.3g}")
    clock.lap("done")
    assert out["outside_allowed_set"] == 0
    assert all(p >= lc.P_PASS for _, _, p in out["ks"].values()) and out["attempts"][2] >= lc.P_PASS, out
    assert all(p >= lc.P_PASS for _, _, p in out["ks_retried"].values()), out["ks_retried"]
    assert out["angles_vs_ex_retried"][1] <= lc.Z_PASS and abs(out["ex0_ex1_z"]) <= lc.Z_PASS, out


K3_SMALL_LIMIT = 8  # as test_laws_cpu.py::test_k3_attempt_number_enters_the_counter


def test_k3_attempts_at_a_small_sample_limit(ctx):
    """``attempts`` = 1 .. 7 and >= 8 (the events that exhaust the limit report it) against the geometric law: with the
    attempt left out of the draw's counter they would all be 1 or 8."""
    inp = Inputs(cases.k3, context=ctx, event_sample_limit=K3_SMALL_LIMIT)
    law = la.K3Law(cases.masses_of(inp.kin), cases.K3_BEAM, cases.K3_RANGE0, cases.K3_RANGE1)
    _, p4, status, attempts = inp.pipeline.run_many(cases.K3_N, first_event=0, seed=cases.K3_SEED, return_status=True)
    chi2, dof, p = la.geometric_chi2(attempts, law.p_accept, K3_SMALL_LIMIT)
    print(f"\nK3 device, limit {K3_SMALL_LIMIT}: attempts chi2 {chi2:.4g} dof {dof} p {p:.3g}; exhausted {int((status != 0).sum())}")
    assert p >= lc.P_PASS and np.isnan(p4[status != 0]).all() and np.isfinite(p4[status == 0]).all()


def _device_kept(ctx, inp, det, p4, vertex, seed, first, max_samples=4096):
    """attpc_det_tracks in calls of at most F_CALL events -> {(event index, isim): kept samples [m, 4]}."""
    ctx.forget("det")  # configured through the C ABI directly: the shim's cache no longer describes the device
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, det), "det_configure")
    kept = {}
    n_sim = inp.layout.n_sim
    for lo in range(0, len(p4), cases.F_CALL):
        n = min(cases.F_CALL, len(p4) - lo)
        samples = np.zeros((n * n_sim, max_samples, 4))
        counts = np.empty(n * n_sim, dtype=np.int32)
        steps = np.empty(n * n_sim, dtype=np.int32)
        ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, seed, first + lo, n, inp.layout,
                                           _abi.dptr(np.ascontiguousarray(p4[lo:lo + n])),
                                           _abi.dptr(np.ascontiguousarray(vertex[lo:lo + n])), max_samples,
                                           _abi.dptr(samples), _abi.iptr(counts, _abi.C.c_int32),
                                           _abi.iptr(steps, _abi.C.c_int32)), "tracks")
        assert counts.max() <= max_samples
        for e in range(n):
            for i in range(n_sim):
                kept[(lo + e, i)] = samples[e * n_sim + i, :counts[e * n_sim + i]].copy()
    return kept


def test_fano_draws(ctx, orc):
    clock = _Clock("F")
    inp = Inputs("o16aa", context=ctx)
    assert inp.det.fano_factor == 0.2
    vertex, p4, _ = _run(inp, cases.F_EVENTS, cases.F_SEED)
    rows = cases.fano_rows(orc, inp, inp.det_raw, p4, vertex)  # det_raw: the oracle's descriptor of the same detector
    gain = inp.det.mpgd_gain
    # the alignment proves itself: at Fano factor 0 every kept sample carries exactly trunc(mu)
    kept0 = _device_kept(ctx, inp, cases.with_field(inp.det, fano_factor=0.0), p4, vertex, cases.F_SEED, 0)
    cases.fano_samples(rows, inp, gain, lambda e, i: kept0[(e, i)], expect_trunc=True)
    clock.lap("Fano 0 run, aligned")
    kept = _device_kept(ctx, inp, inp.det, p4, vertex, cases.F_SEED, 0)
    out = la.fano_checks(cases.fano_samples(rows, inp, gain, lambda e, i: kept[(e, i)]), 0.2, cases.F_PIT_SEED)
    far = _device_kept(ctx, inp, inp.det, p4, vertex, cases.F_SEED, cases.HI)  # the same tracks as events e + 2^32
    out_far = la.fano_checks(cases.fano_samples(rows, inp, gain, lambda e, i: far[(e, i)]), 0.2, cases.F_PIT_SEED + 1)
    n_far, z_far = la.fano_same_samples_z(out, out_far)
    ctx.forget("det")
    n, d, p = out["ks"]
    names = ("lag1_shared_call", "lag1_other", "nuclei_equal_k", "events_equal_row_k")
    print(f"\nF device: tracks {len(kept)}, usable samples {n}, KS D {d:.3g} p {p:.3g}; "
          + "; ".join(f"{k} n {out[k][0]} corr_z {out[k][1]:.3g}" for k in names)
          + f"; events e vs e + 2^32 n {n_far} corr_z {z_far:.3g}")
    clock.lap("done")
    assert p >= lc.P_PASS and n >= 100_000
    for k in names:
        assert out[k][0] >= cases.J_MIN_PAIRS and abs(out[k][1]) <= lc.Z_PASS, (k, out[k])
    assert n_far >= 100_000 and abs(z_far) <= lc.Z_PASS


def test_time_bucket_jitter(ctx):
    """The law and the pairs inside an event on the fetched run; equal keys between event ids e and e + 1 and between
    seeds 7 and 7 + 2^32 on the same kinematics run again at the other id or seed (two runs of different tracks share
    too few keys to have 10 000 pairs; the jitter is a function of seed, event id and key alone)."""
    clock = _Clock("J")
    inp = Inputs("o16aa", context=ctx)
    eng = Engine(inp.pipeline, inp.config, inp.indices, context=ctx)
    base = eng.run(cases.J_EVENTS, seed=cases.J_SEED, first_event=0, fetch=True)
    clouds = []
    for seed, first in ((cases.J_SEED, 1), (cases.J_SEED + cases.HI, 0)):
        offsets, points, _, _ = simulate_batch(base["p4"], base["vertex"], inp.z, inp.a, inp.config, seed, inp.indices,
                                               first_event=first, ctx=ctx)
        clouds.append((offsets, points))
    clock.lap("three device runs")
    out = la.jitter_within(base["offsets"], base["points"])
    out["event_next"] = la.jitter_equal_keys(*clouds[0], base["offsets"], base["points"])
    out["seed_hi"] = la.jitter_equal_keys(*clouds[1], base["offsets"], base["points"])
    n, d, p = out["ks"]
    names = ("tb_next", "pad_next", "event_next", "seed_hi")
    print(f"\nJ device: points {n}, KS D {d:.3g} p {p:.3g}; " + "; ".join(
        f"{k} n {out[k][0]} corr_z {out[k][1]:.3g}" for k in names))
    clock.lap("done")
    assert p >= lc.P_PASS
    for k in names:
        assert out[k][0] >= cases.J_MIN_PAIRS and abs(out[k][1]) <= lc.Z_PASS, (k, out[k])


def test_monte_carlo_diffusion(ctx):
    """40 samples of 10 000 primaries at one centre: every pad stays far below 2^32 electrons, so the default build of
    the scatter kernel is the one under test."""
    from tests.test_gpu_scatter_fixtures import device_scatter

    clock = _Clock("M")
    mc = cases.McSetup()
    ctx.forget("det")  # configured through the C ABI directly: the shim's cache no longer describes the device
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, mc.det), "attpc_det_configure")
    try:
        (cloud,), stats = device_scatter(ctx, [[(mc.xyt, mc.electrons, 2)]], seed=cases.M_SEED, first_event=cases.M_EVENT)
    finally:
        ctx.forget("det")
    clock.lap("device run")
    points = cloud[0]
    assert stats["n_failed"] == 0 and points[:, 2].max() < 2 ** 32
    expect, lost = mc.expected()
    out = la.mc_checks(mc.observed(points[:, 0], points[:, 2]), expect, lost, mc.total)
    chi2, dof, p = out["chi2"]
    print(f"\nM device: primaries {mc.total}, pads hit {out['pads_hit']}, unexpected {out['unexpected']}, lost "
          f"{out['lost_fraction']:.4f}; chi2 {chi2:.4g} dof {dof} p {p:.3g}")
    clock.lap("done")
    assert out["unexpected"] == [] and p >= lc.P_PASS


def test_monte_carlo_diffusion_past_the_u32_sums():
    """One sample of 400 000 primaries: pads collect more than 2^32 electrons, which the u32 sums of the default table
    cannot hold.  The wide build (u64 sums) delivers it: the default build meets a sum past 2^31 and marks its window
    dangerous, and with more than one such window per 64 events the launch is repeated with the wide build
    (``n_lone_buckets`` 0 on an MI355X: nothing went to lone_bucket_kernel); the law is the same.  A context of its
    own: the switch to the wide build is for good."""
    from tests.test_gpu_scatter_fixtures import device_scatter

    own = _abi.Context(0)
    mc = cases.McSetup(n_samples=1, n_primary=400_000)
    own.check(own.lib.attpc_det_configure(own.handle, mc.det), "attpc_det_configure")
    (cloud,), stats = device_scatter(own, [[(mc.xyt, mc.electrons, 2)]], seed=cases.M_SEED, first_event=cases.M_EVENT)
    points = cloud[0]
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0 and points[:, 2].max() >= 2 ** 32
    expect, lost = mc.expected()
    out = la.mc_checks(mc.observed(points[:, 0], points[:, 2]), expect, lost, mc.total)
    chi2, dof, p = out["chi2"]
    print(f"\nM device, one sample of {mc.total} primaries: lone time buckets {stats['n_lone_buckets']}, pads hit "
          f"{out['pads_hit']}, unexpected {out['unexpected']}, lost {out['lost_fraction']:.4f}; chi2 {chi2:.4g} dof {dof} p {p:.3g}")
    assert out["unexpected"] == [] and p >= lc.P_PASS
