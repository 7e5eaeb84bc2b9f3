"""The laws of the engine's random draws, on the CPU: the statistics of tests/law_checks.py against scipy, the numpy
restatement of the samplers (tests/law_reference.py) tied to the oracle, every law check of tests/law_analysis.py passed
by the oracle's output at the sizes and seeds of tests/law_cases.py, and every mutant of the restatement failing its
check by the margin of law_checks (p < 1e-12 or |corr_z| > 8 where the unmutated run has p >= 1e-6, |corr_z| <= 5).
tests/test_gpu_laws.py runs the same analysis on the device's output.  Figures: profiles/r25_draw_laws.md (``-s`` prints
them)."""
import math

import numpy as np
import pytest

from tests import law_analysis as la
from tests import law_cases as cases
from tests import law_checks as lc
from tests import law_reference as ref
from tests.helpers import Inputs

THREADS = 16


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


# ------------------------------------------------------------------------------- the statistics vs scipy ----
def test_statistics_against_scipy():
    st = pytest.importorskip("scipy.stats")
    sp = pytest.importorskip("scipy.special")
    worst = 0.0
    for x in np.concatenate([np.linspace(0.05, 1.2, 60), np.linspace(1.2, 8.4, 100)]):
        want = float(sp.kolmogorov(x))
        if want >= 1e-30:
            worst = max(worst, abs(lc.kolmogorov_sf(float(x)) - want) / want)
    assert worst <= 1e-3, worst
    print(f"\nKolmogorov series vs scipy.special.kolmogorov, p >= 1e-30: relative {worst:.2e}")
    u = np.random.default_rng(1).random(50_000) ** 1.01
    d, p = lc.ks_uniform(u)
    want = st.kstest(u, "uniform", method="asymp")
    assert d == pytest.approx(want.statistic, rel=1e-12) and p == pytest.approx(want.pvalue, rel=1e-3)
    worst = worst_wh = 0.0
    for dof in (1, 2, 3, 5, 17, 38, 100, 400):
        for p in 10.0 ** -np.arange(0.0, 31.0):
            chi2 = float(st.chi2.isf(p, dof))
            want = float(st.chi2.sf(chi2, dof))
            worst = max(worst, abs(lc.chi2_sf(chi2, dof) - want) / want)
            if p >= 1e-6:
                worst_wh = max(worst_wh, abs(lc.wilson_hilferty_sf(chi2, dof) - want) / want)
    assert worst <= 1e-3, worst
    print(f"chi-square tail vs scipy, p 1 .. 1e-30: relative {worst:.2e}; Wilson-Hilferty down to 1e-6: {worst_wh:.2e}")
    obs = np.array([30, 25, 41, 3, 2, 9.0])
    exp = np.array([28, 30, 35, 4, 5, 8.0])
    chi2, dof, p = lc.chi2_p(obs, exp)  # the three cells below 20 pooled into one
    pooled_obs, pooled_exp = np.array([30, 25, 41, 14.0]), np.array([28, 30, 35, 17.0])
    assert dof == 3 and chi2 == pytest.approx(((pooled_obs - pooled_exp) ** 2 / pooled_exp).sum())
    assert p == pytest.approx(st.chi2.sf(chi2, 3), rel=1e-3)
    x = np.linspace(-9.0, 9.0, 2001)
    assert np.abs(lc.ndtr(x) - sp.ndtr(x)).max() <= 1e-15
    q = np.concatenate([10.0 ** -np.arange(1.0, 16.0), np.linspace(0.001, 0.999, 999)])
    assert np.abs(lc.ndtri(q) - sp.ndtri(q)).max() <= 1e-12
    assert np.abs(lc.halfnormal_cdf(np.abs(x)) - st.halfnorm.cdf(np.abs(x))).max() <= 1e-15
    worst = 0.0
    for rho in (0.5, 3.0, 36.0, (cases.k2_bw()[0] + cases.K2_CENTROID) / cases.K2_WIDTH):
        x = np.concatenate([np.linspace(0.0, 2.0 * rho + 5.0, 200_001), rho + np.linspace(-50.0, 50.0, 100_001)])
        worst = max(worst, float(np.abs(lc.rel_breitwigner_cdf(x, rho) - st.rel_breitwigner.cdf(x, rho)).max()))
    assert worst <= 1e-12, worst
    print(f"Breit-Wigner CDF vs scipy: {worst:.2e}")
    # corr_z and the randomised PIT
    rng = np.random.default_rng(2)
    a, b = rng.random(10_000), rng.random(10_000)
    r = st.pearsonr(sp.ndtri(a), sp.ndtri(b)).statistic
    assert lc.corr_z(a, b) == pytest.approx(r * 100.0, rel=1e-9)
    k = rng.poisson(30.0, 20_000)
    pit = lc.pit_discrete(k, st.poisson.cdf(k - 1, 30.0), st.poisson.cdf(k, 30.0), rng.random(20_000))
    assert st.kstest(pit, "uniform").pvalue > 1e-3 and lc.ks_uniform(pit)[1] > 1e-3


# ------------------------------------------------------------------------ the restatement is the oracle ----
@pytest.mark.parametrize("name,n", [("o16aa", 4000), ("k2", 4000), ("k3", 4000)])
def test_restatement_kinematics_equal_the_oracle(orc, name, n):
    inp = Inputs({"k2": cases.k2, "k3": cases.k3}.get(name, name))
    seed, first = 11 + cases.HI, (1 << 32) - n // 2  # the high word of the seed and of the event id in play
    vertex, p4, status, attempts = orc.kin_batch(inp.kin, seed, first, n, threads=THREADS)
    v2, q4, s2, a2 = ref.kin_run(ref.KinModel(inp.kin), seed, first, n)
    np.testing.assert_array_equal(status, s2)
    np.testing.assert_array_equal(attempts, a2)
    assert (status == 0).all()
    assert np.abs(vertex - v2).max() <= 1e-9 and np.abs(p4 - q4).max() <= 1e-9
    if name == "k3":
        assert attempts.max() >= 10  # the rejection loop in play


def _oracle_tracks(orc, inp, det, n, seed, first=0):
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=THREADS)
    assert (status == 0).all()
    kept = {(e, i): orc.point_cloud_samples(det, inp.layout.species_of_row[row], p4[e, row], vertex[e], seed, first + e, row)[0]
            for e in range(n) for i, row in enumerate(inp.indices)}
    return vertex, p4, kept


def test_restatement_fano_jitter_mc_equal_the_oracle(orc):
    inp = Inputs("o16aa")
    det = inp.det_raw
    seed, first, n = 21 + cases.HI, (1 << 32) - 8, 16
    vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, first, n, threads=THREADS)
    total = 0
    for e in range(n):
        for row in inp.indices:
            sp = inp.layout.species_of_row[row]
            track = orc.trajectory(det, sp, vertex[e], p4[e, row])
            want = orc.electrons(det, sp, track, seed, first + e, 1 + row)
            mu = ref.fano_mu(track, det.species[sp].mass, det.w_value)
            got = ref.fano_electrons(mu, np.arange(len(mu)), seed, first + e, 1 + row, det.fano_factor)
            np.testing.assert_array_equal(got, want)
            total += len(mu)
    assert total >= 3000, total
    rng = np.random.default_rng(3)
    pad, tb = rng.integers(0, 10240, 3000), rng.integers(0, 512, 3000)
    for s, ev in ((7, 0), (7 + cases.HI, 5), (cases.HI * 77 + 1, (1 << 39) + 3)):
        want = np.array([orc.jitter_uniform(s, ev, (int(t) << 14) | int(p)) for p, t in zip(pad, tb)])
        np.testing.assert_array_equal(ref.jitter(s, ev, pad, tb), want)
    mc = cases.McSetup(n_samples=3, n_primary=2000)
    keys, charge, _ = orc.transport(mc.det_raw, [(mc.xyt, mc.electrons, 2)], seed=cases.M_SEED, event=cases.M_EVENT)
    want = {}
    for key, q in zip(keys, charge):
        t, p = orc.unpair(int(key))
        want[(t, p)] = int(q)
    got = {}
    for i in range(3):
        counts = ref.mc_pad_counts(mc.plane, *cases.M_CENTRE, mc.sigmas[i], mc.n_primary, cases.M_SEED, cases.M_EVENT, i)
        got.update({(int(mc.xyt[i, 2]), p): c * mc.gain for p, c in counts.items()})
    assert got == want and len(got) > 30


# ------------------------------------------------------------------------------------------------- K1 ----
def _k1_report(cols_a, cols_b, mutant=None):
    """-> (ks, largest off-diagonal, lag-1, cross) of a K1 run and the same run one seed high word further."""
    ks = la.ks_all(cols_a)
    off = lc.corr_matrix_z(cols_a)
    lag = la.lag1(cols_a)
    cross = la.cross(cols_a, cols_b)
    print(f"\nK1{' mutant ' + mutant if mutant else ''}: n {len(cols_a['rho'])}")
    for k, (n, d, p) in ks.items():
        print(f"  {k}: D {d:.3g} p {p:.3g}")
    print(f"  largest off-diagonal |corr_z| {off[0]:.3g} {off[1]}; lag-1 max {max(abs(v) for v in lag.values()):.3g}; "
          f"seed vs seed + 2^32 max {cross[0]:.3g} {cross[1]}")
    return ks, off, lag, cross


def _k1_assert_passes(report):
    ks, off, lag, cross = report
    assert all(p >= lc.P_PASS for _, _, p in ks.values()), ks
    assert off[0] <= lc.Z_PASS and cross[0] <= lc.Z_PASS and max(abs(v) for v in lag.values()) <= lc.Z_PASS


def test_k1_oracle(orc):
    inp = Inputs("o16aa")
    m = cases.masses_of(inp.kin)
    cols = []
    for seed in (cases.K1_SEED, cases.K1_SEED + cases.HI):
        vertex, p4, status, _ = orc.kin_batch(inp.kin, seed, 0, cases.K1_N, threads=THREADS)
        assert (status == 0).all()
        cols.append(la.k1_columns(vertex, p4, m, **cases.K1_LAW))
    _k1_assert_passes(_k1_report(*cols))


@pytest.mark.parametrize("mutant", [None, "sigma_fwhm", "theta_uniform", "rho_rayleigh", "azimuth_z_same"])
def test_k1_restatement_and_mutants(mutant):
    inp = Inputs("o16aa")
    model, m = ref.KinModel(inp.kin), cases.masses_of(inp.kin)
    cols = []
    for seed in (cases.K1_SEED, cases.K1_SEED + cases.HI):
        vertex, p4, status, _ = ref.kin_run(model, seed, 0, cases.K1_N, mutant)
        cols.append(la.k1_columns(vertex, p4, m, **cases.K1_LAW))
    ks, off, lag, cross = report = _k1_report(*cols, mutant=mutant)
    if mutant is None:
        _k1_assert_passes(report)
    elif mutant == "azimuth_z_same":
        assert off[0] > lc.Z_MUTANT and set(off[1]) == {"azimuth", "z"}, off
    else:
        column = {"sigma_fwhm": "ex0", "theta_uniform": "cos0", "rho_rayleigh": "rho"}[mutant]
        assert ks[column][2] < lc.P_MUTANT, ks[column]


# ------------------------------------------------------------------------------------------------- K2 ----
def test_k2_table_error_is_below_the_ks_resolution():
    """sup |F_table - F_exact| of the device's Breit-Wigner table (linear in x between its nodes, normalised over the
    table's span) at the nodes and midpoints, and the two tails the table cuts off."""
    inp = Inputs(cases.k2)
    model = ref.KinModel(inp.kin)
    x, cdf = model.excitation[0]["x"], model.excitation[0]["cdf"]
    bw = cases.k2_bw()
    mid = 0.5 * (x[1:] + x[:-1])
    f_mid = 0.5 * (cdf[1:] + cdf[:-1])
    err = max(float(np.abs(f_mid - la.bw_cdf(mid - bw[0], *bw)).max()), float(np.abs(cdf - la.bw_cdf(x - bw[0], *bw)).max()))
    low, high = float(la.bw_cdf(x[0] - bw[0], *bw)), 1.0 - float(la.bw_cdf(x[-1] - bw[0], *bw))
    print(f"\nBreit-Wigner table: {len(x)} nodes, sup |F_table - F_exact| {err:.3g}; tails cut {low:.3g} and {high:.3g}")
    assert err < 0.1 * 1.36 / math.sqrt(cases.K2_N), err


def _k2_report(name, p4, attempts, masses):
    out = la.k2_checks(p4, attempts, masses, cases.K2_BEAM, cases.k2_bw(), cases.K2_ANGLES, cases.K2_PROBS,
                       cases.K2_BIN_WIDTH, cases.K2_PIT_SEED)
    print(f"\nK2 {name}: n {len(p4)}; ex D {out['ex'][1]:.3g} p {out['ex'][2]:.3g}; attempts chi2 {out['attempts'][0]:.3g} "
          f"dof {out['attempts'][1]} p {out['attempts'][2]:.3g} (mean {out['mean_attempts'][0]:.6f}, 1/F {out['mean_attempts'][1]:.6f}); "
          f"bin chi2 {out['bin'][0]:.3g} dof {out['bin'][1]} p {out['bin'][2]:.3g}; offset D {out['offset'][1]:.3g} "
          f"p {out['offset'][2]:.3g}; bin vs offset corr_z {out['bin_offset_z']:.3g}")
    return out


def _k2_assert_passes(out):
    assert min(out["ex"][2], out["attempts"][2], out["bin"][2], out["offset"][2]) >= lc.P_PASS
    assert abs(out["bin_offset_z"]) <= lc.Z_PASS


def test_k2_oracle(orc):
    inp = Inputs(cases.k2)
    _, p4, status, attempts = orc.kin_batch(inp.kin, cases.K2_SEED, 0, cases.K2_N, threads=THREADS)
    assert (status == 0).all()
    _k2_assert_passes(_k2_report("oracle", p4, attempts, cases.masses_of(inp.kin)))


@pytest.mark.parametrize("mutant", [None, "offset_from_bin"])
def test_k2_restatement_and_mutant(mutant):
    inp = Inputs(cases.k2)
    _, p4, status, attempts = ref.kin_run(ref.KinModel(inp.kin), cases.K2_SEED, 0, cases.K2_N, mutant)
    out = _k2_report(f"restatement {mutant}", p4, attempts, cases.masses_of(inp.kin))
    if mutant is None:
        _k2_assert_passes(out)
    else:
        assert abs(out["bin_offset_z"]) > lc.Z_MUTANT


# ------------------------------------------------------------------------------------------------- K3 ----
def _k3_law(inp):
    return la.K3Law(cases.masses_of(inp.kin), cases.K3_BEAM, cases.K3_RANGE0, cases.K3_RANGE1)


def test_k3_ranges_make_both_steps_refuse(orc):
    """Shown with the oracle's own step functions on proposals drawn here: step 0 refuses 20-70 % of the proposals,
    step 1 20-70 % of those that pass step 0, and whether step 1 passes depends on ex0."""
    inp = Inputs(cases.k3)
    law = _k3_law(inp)
    rng = np.random.default_rng(0)
    n = 20_000
    ex0, ex1 = rng.uniform(*cases.K3_RANGE0, n), rng.uniform(*cases.K3_RANGE1, n)
    th = np.arccos(rng.uniform(-1.0, 1.0, (n, 2)))
    ph = rng.uniform(0.0, 2.0 * np.pi, (n, 2))
    _, status = orc.kin_calculate(inp.kin, np.full(n, cases.K3_BEAM), np.column_stack([ex0, ex1]), th, ph)
    refused0 = np.isin(status, (1, -1))
    refused1 = status == 2
    f0, f1 = refused0.mean(), refused1.sum() / (~refused0).sum()
    print(f"\nK3 ranges: step 0 refuses {f0:.3f} (law {1 - law.p_step0:.3f}), step 1 {f1:.3f} of the rest "
          f"(law {1 - law.p_step1:.3f}); ex_max0 {law.ex_max0:.4f} MeV, q1 {law.q1:.4f} MeV")
    assert 0.2 <= f0 <= 0.7 and 0.2 <= f1 <= 0.7
    assert abs(f0 - (1 - law.p_step0)) < 0.02 and abs(f1 - (1 - law.p_step1)) < 0.02
    np.testing.assert_array_equal(status == 0, law.allowed(ex0, ex1))  # the allowed set as law_analysis writes it
    passed0 = ~refused0
    low = passed0 & (ex0 < np.median(ex0[passed0]))
    high = passed0 & ~low
    assert refused1[low].mean() > refused1[high].mean() + 0.2  # step 1 passes far more often at a large ex0


def _k3_report(name, law, p4, attempts, n_cells=41):
    out = law.checks(p4, attempts, n_cells)
    print(f"\nK3 {name}: n {len(p4)}, outside the allowed set {out['outside_allowed_set']}")
    for k, (n, d, p) in out["ks"].items():
        print(f"  {k}: D {d:.3g} p {p:.3g}")
    print(f"  attempts chi2 {out['attempts'][0]:.4g} dof {out['attempts'][1]} p {out['attempts'][2]:.3g} (mean "
          f"{np.mean(attempts):.5f}, 1/p {1 / law.p_accept:.5f}); angles among attempts >= 2: smallest KS p {min(p for _, _, p in out['ks_retried'].values()):.3g}, vs ex: n "
          f"{out['angles_vs_ex_retried'][0]} max |corr_z| {out['angles_vs_ex_retried'][1]:.3g} {out['angles_vs_ex_retried'][2]}; "
          f"PIT(ex0) vs PIT(ex1 | ex0) corr_z {out['ex0_ex1_z']:.3g}")
    return out


def _k3_assert_passes(out):
    assert out["outside_allowed_set"] == 0
    assert all(p >= lc.P_PASS for _, _, p in out["ks"].values()) and out["attempts"][2] >= lc.P_PASS
    assert all(p >= lc.P_PASS for _, _, p in out["ks_retried"].values()), out["ks_retried"]
    assert out["angles_vs_ex_retried"][1] <= lc.Z_PASS and abs(out["ex0_ex1_z"]) <= lc.Z_PASS


def test_k3_oracle(orc):
    inp = Inputs(cases.k3)
    _, p4, status, attempts = orc.kin_batch(inp.kin, cases.K3_SEED, 0, cases.K3_N, threads=THREADS)
    assert (status == 0).all()
    _k3_assert_passes(_k3_report("oracle", _k3_law(inp), p4, attempts))


@pytest.mark.parametrize("mutant", [None, "resample_failed_step", "ex1_slot0"])
def test_k3_restatement_and_mutants(mutant):
    inp = Inputs(cases.k3)
    _, p4, status, attempts = ref.kin_run(ref.KinModel(inp.kin), cases.K3_SEED, 0, cases.K3_N, mutant)
    good = status == 0  # (resampling step 1 alone exhausts the limit where ex0 leaves it next to no room)
    assert good.all() or (mutant == "resample_failed_step" and good.mean() > 0.99)
    out = _k3_report(f"restatement {mutant}", _k3_law(inp), p4[good], attempts[good])
    if mutant is None:
        _k3_assert_passes(out)
    else:  # an engine that resamples the failed step alone keeps every invariant and loses the shape of ex0
        assert out["outside_allowed_set"] == 0
        assert out["ks"]["ex0"][2] < lc.P_MUTANT, out["ks"]["ex0"]


K3_SMALL_LIMIT = 8


@pytest.mark.parametrize("mutant", [None, "attempt_not_in_counter"])
def test_k3_attempt_number_enters_the_counter(mutant):
    """With the attempt left out of the counter every retry redraws the same proposal: ``attempts`` is 1 or the
    limit.  A sample limit of 8 shows it on the counts of attempts = 1 .. 7 and >= 8 (exhausted events included:
    they report the limit)."""
    inp = Inputs(cases.k3)
    model = ref.KinModel(inp.kin)
    model.sample_limit = K3_SMALL_LIMIT
    _, p4, status, attempts = ref.kin_run(model, cases.K3_SEED, 0, cases.K3_N, mutant)
    chi2, dof, p = la.geometric_chi2(attempts, _k3_law(inp).p_accept, K3_SMALL_LIMIT)
    print(f"\nK3 limit {K3_SMALL_LIMIT} {mutant}: attempts chi2 {chi2:.4g} dof {dof} p {p:.3g}; exhausted {int((status != 0).sum())}")
    if mutant is None:
        assert p >= lc.P_PASS
    else:
        assert p < lc.P_MUTANT and set(np.unique(attempts)) == {1, K3_SMALL_LIMIT}


# ------------------------------------------------------------------------------------------------ Fano ----
@pytest.fixture(scope="module")
def fano_tracks(orc):
    """The F run on the oracle: kinematics, and per track (trajectory rows k, mu) of the kept samples."""
    inp = Inputs("o16aa")
    det = inp.det_raw
    assert det.fano_factor == 0.2
    vertex, p4, kept = _oracle_tracks(orc, inp, det, cases.F_EVENTS, cases.F_SEED)
    rows = cases.fano_rows(orc, inp, det, p4, vertex)
    samples = cases.fano_samples(rows, inp, det.mpgd_gain, lambda e, i: kept[(e, i)])
    _, _, kept0 = _oracle_tracks(orc, inp, cases.with_field(det, fano_factor=0.0), cases.F_EVENTS, cases.F_SEED)
    cases.fano_samples(rows, inp, det.mpgd_gain, lambda e, i: kept0[(e, i)], expect_trunc=True)
    return inp, det, vertex, p4, samples


def _fano_report(name, out):
    n, d, p = out["ks"]
    print(f"\nF {name}: usable samples {n}, KS D {d:.3g} p {p:.3g}; " + "; ".join(
        f"{k} n {out[k][0]} corr_z {out[k][1]:.3g}" for k in ("lag1_shared_call", "lag1_other", "nuclei_equal_k", "events_equal_row_k")))
    return out


def _fano_assert_passes(out):
    assert out["ks"][2] >= lc.P_PASS
    for k in ("lag1_shared_call", "lag1_other", "nuclei_equal_k", "events_equal_row_k"):
        assert out[k][0] >= cases.J_MIN_PAIRS and abs(out[k][1]) <= lc.Z_PASS, (k, out[k])


def test_fano_oracle(fano_tracks):
    inp, det, vertex, p4, samples = fano_tracks
    _fano_assert_passes(_fano_report("oracle", la.fano_checks(samples, det.fano_factor, cases.F_PIT_SEED)))


def _restated(samples, fano, mutant, event_offset=0):
    event, row, k, mu, _ = samples.arrays()
    out = la.FanoSamples()
    n = ref.fano_electrons(mu, k, cases.F_SEED, event + event_offset, 1 + row, fano, mutant)
    out.parts.append((event, row, k, mu, n))
    return out


@pytest.mark.parametrize("mutant", [None] + list(ref.FANO_MUTANTS))
def test_fano_restatement_and_mutants(fano_tracks, mutant):
    """The restatement's draws on the oracle's means (its unmutated counts are the oracle's: the tie above)."""
    inp, det, vertex, p4, samples = fano_tracks
    fano = det.fano_factor
    out = _fano_report(f"restatement {mutant}", la.fano_checks(_restated(samples, fano, mutant), fano, cases.F_PIT_SEED))
    far = la.fano_checks(_restated(samples, fano, mutant, event_offset=cases.HI), fano, cases.F_PIT_SEED + 1)
    n_far, z_far = la.fano_same_samples_z(out, far)
    print(f"  events e vs e + 2^32: n {n_far} corr_z {z_far:.3g}")
    if mutant is None:
        np.testing.assert_array_equal(_restated(samples, fano, None).arrays()[4], samples.arrays()[4])
        _fano_assert_passes(out)
        assert abs(z_far) <= lc.Z_PASS
    elif mutant in ("round", "sigma_sqrt_mu", "sigma_f_sqrt_mu"):
        assert out["ks"][2] < lc.P_MUTANT
    else:
        z = {"odd_reuses_even": out["lag1_shared_call"][1], "one_domain": out["nuclei_equal_k"][1],
             "event_hi_ignored": z_far}[mutant]
        assert abs(z) > lc.Z_MUTANT, z


# ---------------------------------------------------------------------------------------------- jitter ----
@pytest.fixture(scope="module")
def jitter_clouds(orc):
    """The J run on the oracle, and the same kinematics one event id later and one seed high word further (the
    jitter is a function of seed, event id and (pad, tb): equal tracks give equal keys to compare it at)."""
    inp = Inputs("o16aa")
    kw = dict(n=cases.J_EVENTS, capacity=1 << 21, threads=THREADS)
    base = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=cases.J_SEED, first=0, **kw)
    again = dict(p4_in=base["p4"], vertex_in=base["vertex"], **kw)
    later = orc.sim_batch(None, inp.det_raw, inp.layout, seed=cases.J_SEED, first=1, **again)
    other = orc.sim_batch(None, inp.det_raw, inp.layout, seed=cases.J_SEED + cases.HI, first=0, **again)
    return base, later, other


def _jitter_report(name, base, later, other):
    out = la.jitter_within(base["offsets"], base["points"])
    out["event_next"] = la.jitter_equal_keys(later["offsets"], later["points"], base["offsets"], base["points"])
    out["seed_hi"] = la.jitter_equal_keys(other["offsets"], other["points"], base["offsets"], base["points"])
    n, d, p = out["ks"]
    print(f"\nJ {name}: points {n}, KS D {d:.3g} p {p:.3g}; " + "; ".join(
        f"{k} n {out[k][0]} corr_z {out[k][1]:.3g}" for k in ("tb_next", "pad_next", "event_next", "seed_hi")))
    return out


def _jitter_assert_passes(out):
    assert out["ks"][2] >= lc.P_PASS
    for k in ("tb_next", "pad_next", "event_next", "seed_hi"):
        assert out[k][0] >= cases.J_MIN_PAIRS and abs(out[k][1]) <= lc.Z_PASS, (k, out[k])


def test_jitter_oracle(jitter_clouds):
    _jitter_assert_passes(_jitter_report("oracle", *jitter_clouds))


def _rejittered(cloud, seed, first, mutant):
    """The cloud with its jitter drawn again by the restatement."""
    points = cloud["points"].copy()
    pad, tb, _ = la.split_cloud(points)
    for e in range(len(cloud["offsets"]) - 1):
        s = slice(cloud["offsets"][e], cloud["offsets"][e + 1])
        points[s, 1] = tb[s] + ref.jitter(seed, first + e, pad[s], tb[s], mutant)
    return {"offsets": cloud["offsets"], "points": points}


@pytest.mark.parametrize("mutant", [None] + list(ref.JITTER_MUTANTS))
def test_jitter_restatement_and_mutants(jitter_clouds, mutant):
    base, later, other = jitter_clouds
    clouds = [_rejittered(base, cases.J_SEED, 0, mutant), _rejittered(later, cases.J_SEED, 1, mutant),
              _rejittered(other, cases.J_SEED + cases.HI, 0, mutant)]
    out = _jitter_report(f"restatement {mutant}", *clouds)
    if mutant is None:
        for mine, theirs in zip(clouds, jitter_clouds):
            np.testing.assert_array_equal(mine["points"], theirs["points"])
        _jitter_assert_passes(out)
    else:
        z = out[{"no_tb": "tb_next", "no_pad": "pad_next", "no_seed_hi": "seed_hi"}[mutant]][1]
        assert abs(z) > lc.Z_MUTANT, z


# --------------------------------------------------------------------------------- Monte-Carlo diffusion ----
def _mc_report(name, mc, observed):
    expect, lost = mc.expected()
    out = la.mc_checks(observed, expect, lost, mc.total)
    chi2, dof, p = out["chi2"]
    print(f"\nM {name}: primaries {mc.total}, pads hit {out['pads_hit']}, unexpected {out['unexpected']}, lost "
          f"{out['lost_fraction']:.4f}; chi2 {chi2:.4g} dof {dof} p {p:.3g}")
    return out


@pytest.mark.parametrize("n_samples,n_primary", [(cases.M_SAMPLES, cases.M_PRIMARIES), (1, 400_000)])
def test_mc_oracle(orc, n_samples, n_primary):
    """The device's two cases: 40 samples of 10 000 primaries, and one sample of 400 000 (pads above 2^32 electrons:
    on the device the wide build of the scatter kernel)."""
    mc = cases.McSetup(n_samples, n_primary)
    keys, charge, _ = orc.transport(mc.det_raw, [(mc.xyt, mc.electrons, 2)], seed=cases.M_SEED, event=cases.M_EVENT)
    pad = np.array([orc.unpair(int(k))[1] for k in keys])
    out = _mc_report("oracle", mc, mc.observed(pad, charge))
    assert out["unexpected"] == [] and out["chi2"][2] >= lc.P_PASS


@pytest.mark.parametrize("mutant", [None] + list(ref.MC_MUTANTS))
def test_mc_restatement_and_mutants(mutant):
    mc = cases.McSetup()
    observed: dict = {}
    for i in range(len(mc.xyt)):
        counts = ref.mc_pad_counts(mc.plane, *cases.M_CENTRE, mc.sigmas[i], mc.n_primary, cases.M_SEED, cases.M_EVENT, i, mutant)
        for p, c in counts.items():
            observed[p] = observed.get(p, 0) + c
    out = _mc_report(f"restatement {mutant}", mc, observed)
    assert out["unexpected"] == []
    if mutant is None:
        assert out["chi2"][2] >= lc.P_PASS
    else:
        assert out["chi2"][2] < lc.P_MUTANT
