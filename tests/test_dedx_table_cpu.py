"""The stopping-power table against the function it samples -- on the CPU alone (numpy, scipy, mpmath and the oracle).

* the restated lookup equals ``orc_dedx_lookup`` bit for bit; the restated right-hand side equals the reference's own
  ``equation_of_motion`` run on the smooth ``GasTarget`` (tests/golden/dedx_smooth.npz) to 1e-13
* |lookup - function| at the quarter points of every sub-bin stays under a bound computed from the function alone, for
  every table the workloads build; the only bins named as not twice differentiable are the predicted seams
* ``sample_dedx_table``'s clamp, a deliberately rough target, the range by two quadratures
* the oracle's tracks of tests/dedx_cases.py against the table-side reference track (1e-7 m, 2e-6 MeV, equal rows) and
  against the smooth track under the rule of tests/dedx_check.py; the fixture's smooth tracks regenerate
* five wrong tables / lookups, each of which must break that rule on at least one case

Figures: profiles/r27_dedx_table.md."""
import sys
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, nuclear_map
from attpc_engine_amd.detector.luts import dedx_node_energies, sample_dedx_table
from tests import dedx_cases as dc
from tests import dedx_check as chk
from tests import dedx_reference as dr

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_dedx_smooth as mk  # noqa: E402  (the generator's own functions; its main() needs the reference tree)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def fx():
    return chk.Fixture(GOLDEN / "dedx_smooth.npz")


def _nucleus(species):
    return nuclear_map.get_data(*dc.NUCLEUS[species])


def _function(gas, nuc):
    return lambda ke: gas.get_dedx(nuc, ke)


# ------------------------------------------------------------------------------------------------ restatements ----
def test_lookup_restatement_equals_the_oracle_bit_for_bit(orc):
    gas = mk.gas_of("he")
    tab = sample_dedx_table(gas, _nucleus("c12"))
    nodes = dedx_node_energies()
    np.testing.assert_array_equal(nodes, dr.node_energies())
    a, b = nodes[:-1], nodes[1:]
    probes = np.concatenate([nodes, a + 0.25 * (b - a), a + 0.5 * (b - a), a + 0.75 * (b - a), np.nextafter(b, 0.0),
                             [0.0, -1.0, 5e-324, 2.2e-308, np.nextafter(nodes[0], 0.0), nodes[-1], 1e9, np.inf, np.nan]])
    L = orc.lib()
    want = np.array([L.orc_dedx_lookup(_abi.dptr(tab), float(e)) for e in probes])
    got = dr.lookup(tab, probes)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:len(nodes)], tab)
    read = dr.scalar_lookup(tab)
    assert all(read(float(e)) == w for e, w in zip(probes, want))
    assert dr.lookup(tab, float("nan")) == tab[0] and dr.lookup(tab, 0.0) == tab[0]
    # the mutants' lookups are other functions
    inner = probes[len(nodes):4 * len(nodes) - 3]
    for mode in ("nearest", "weight48"):
        assert (dr.lookup(tab, inner, mode) != dr.lookup(tab, inner)).mean() > 0.5, mode
    # 16 sub-bins written on the fine grid: the engine's lookup of it is the coarse lookup
    coarse = dr.sample(_function(gas, _nucleus("c12")), dr.node_energies(16))
    np.testing.assert_allclose(dr.lookup(dr.coarse_as_fine(coarse), inner), dr.lookup(coarse, inner), rtol=4e-16)


def test_right_hand_side_equals_the_reference_on_the_smooth_target(fx):
    g = fx.g
    species, gases = [str(s) for s in g["species_names"]], [str(s) for s in g["gas_names"]]
    assert len(g["eom_states"]) >= 190 and set(g["eom_species"].tolist()) == set(range(len(species)))
    ke = np.array([dr.kinetic_energy(s[3:6], dc.MASS[species[i]]) for s, i in zip(g["eom_states"], g["eom_species"])])
    assert ke.min() < 1e-4 and ke.max() > 50.0
    worst = 0.0
    for state, want, si, gi in zip(g["eom_states"], g["eom_results"], g["eom_species"], g["eom_gas"]):
        gas, nuc = mk.gas_of(gases[gi]), _nucleus(species[si])
        got = np.array(dr.equation_of_motion(state.tolist(), -float(g["bfield"]), -float(g["efield"]), _function(gas, nuc),
                                             gas.density, nuc.Z, nuc.mass))
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
    print("restated right-hand side against the reference's: largest relative difference", worst)
    assert worst <= 1e-13


# ------------------------------------------------------------------------------------------------ the profile ----
# the species of every table that be10dp, o16aa and b10chain build (their simulated rows) and the 13 of
# tests/test_gpu_layout_limits.py::test_thirteen_stopping_power_tables (OTHER_SPECIES + chain8's), written out: building
# the workloads themselves costs their kinematics' energy-loss tables, 40 s of pure Python
WORKLOAD_TABLES = {
    "be10dp": ("d2", [(1, 1), (4, 11)]),
    "o16aa": ("he", [(2, 4), (6, 12)]),
    "b10chain": ("he", [(2, 4), (1, 1)]),
    "chain8": ("he", [(1, 3), (2, 3), (3, 6), (5, 10), (6, 12), (8, 16),
                      (4, 8), (13, 26), (2, 4), (1, 2), (10, 20), (1, 1), (12, 25)]),
    # the tables the tracks of tests/dedx_cases.py are integrated on (d in D2 and 16O in He are in no workload's default
    # indices), and the rest of the survey of profiles/r27_dedx_table.md: p, d, alpha, 10Be, 11Be, 12C, 16O in both gases
    "cases he": ("he", [dc.NUCLEUS[s] for s in dc.GASES["he"][1]]),
    "cases d2": ("d2", [dc.NUCLEUS[s] for s in dc.GASES["d2"][1]]),
    "survey he": ("he", [(1, 1), (1, 2), (2, 4), (4, 10), (4, 11), (6, 12), (8, 16)]),
    "survey d2": ("d2", [(1, 1), (1, 2), (2, 4), (4, 10), (4, 11), (6, 12), (8, 16)]),
}


def _workload_tables():
    out, seen = [], set()
    for name, (gas_name, species) in WORKLOAD_TABLES.items():
        gas = mk.gas_of(gas_name)
        for z, a in species:
            if (gas_name, z, a) not in seen:
                seen.add((gas_name, z, a))
                out.append((f"{name}:{z}-{a}", gas, nuclear_map.get_data(z, a)))
    return out


def test_the_thirteen_tables_are_those_of_the_layout_limit_launch():
    from tests.test_gpu_layout_limits import OTHER_SPECIES
    thirteen = WORKLOAD_TABLES["chain8"][1]
    assert thirteen[:6] == OTHER_SPECIES and len(set(thirteen)) == 13
    assert mk.gas_of("he").compound_key == ((2, 4, 1),) and mk.gas_of("d2").compound_key == ((1, 2, 2),)


def test_every_workload_table_is_inside_the_bound_of_its_function():
    tables = _workload_tables()
    assert len(tables) == 22   # 15 of the workloads, d in D2 and 16O in He of the cases, 5 more of the survey
    for label, gas, nuc in tables:
        pr = dr.profile(_function(gas, nuc), sample_dedx_table(gas, nuc))
        w = pr.worst()
        print(f"{label}: median {np.median(pr.rel_all):.2e} max {pr.rel[w]:.2e} at {pr.at[w]:.4g} MeV; named bins "
              f"{[(int(i), float(pr.a[pr.index == i][0])) for i in pr.named]}; largest error / bound "
              f"{(pr.err / pr.bound).max():.4f}")
        assert pr.over_bound().size == 0, (label, pr.over_bound())
        seams = dr.seam_energies(gas, nuc)
        assert len(pr.named) <= len(seams), (label, pr.named)
        for i in pr.named:  # a named bin holds a predicted seam, one bin per (species, element) pair
            a, b = pr.a[pr.index == i][0], pr.b[pr.index == i][0]
            assert sum(a <= s < b for s in seams) == 1, (label, i, a, b, seams)


def test_seam_is_where_the_formula_says():
    from attpc_engine_amd.target import _elemental_stopping
    gas, nuc = mk.gas_of("he"), _nucleus("c12")
    (seam,) = dr.seam_energies(gas, nuc)
    (zt, at_u, _), = gas._elements
    below, above = _elemental_stopping(6, nuc.mass, seam * (1 - 1e-9), zt, at_u), _elemental_stopping(6, nuc.mass, seam * (1 + 1e-9), zt, at_u)
    near = _elemental_stopping(6, nuc.mass, seam * (1 - 3e-9), zt, at_u)
    assert abs(above - below) > 1e4 * abs(below - near) > 0.0   # a jump, not a slope


class _Rough:
    """Piecewise constant dE/dx: the model's value at the last quarter decade."""
    density, compound_key = 1.0e-4, None

    def __init__(self, gas):
        self.gas = gas

    def get_dedx(self, nuc, ke):
        return self.gas.get_dedx(nuc, 10.0 ** (np.floor(4.0 * np.log10(ke)) / 4.0))


def test_a_rough_target_is_named_not_passed():
    gas, nuc = _Rough(mk.gas_of("d2")), _nucleus("p")
    f = _function(gas, nuc)
    pr = dr.profile(f, sample_dedx_table(gas, nuc), e_min=1e-3, e_max=10.0)
    steps = 10.0 ** (np.arange(-12, 5) / 4.0)
    holding = {int(pr.index[(pr.a < s) & (s <= pr.b)][0]) for s in steps}
    assert len(holding) == len(steps)
    assert set(pr.named.tolist()) == holding                      # every bin with a step is named, and no other
    assert len(pr.named) > 1                                      # ... so the one-seam condition fails for this target
    assert (pr.err[~pr.rough] == 0.0).all() and (pr.err[pr.rough] > 0.0).all()
    assert pr.over_bound().size == 0 and (pr.jump[pr.rough] >= pr.err[pr.rough]).all()


# ------------------------------------------------------------------------------------------------ the clamp ----
class _Window:
    """Valid between ``lo`` and ``hi`` only; outside NaN, negative, or infinite."""
    density = 1.0e-4

    def __init__(self, lo, hi, bad):
        self.lo, self.hi, self.bad = lo, hi, bad

    def get_dedx(self, nuc, ke):
        return 100.0 + ke if self.lo <= ke <= self.hi else self.bad


@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("inf"), -0.5])
def test_clamp_takes_the_nearest_valid_node_and_moves_no_valid_value(bad):
    nodes = dedx_node_energies()
    lo, hi = 600, 900
    tab = sample_dedx_table(_Window(nodes[lo], nodes[hi], bad), _nucleus("p"))
    np.testing.assert_array_equal(tab[lo:hi + 1], 100.0 + nodes[lo:hi + 1])   # valid values stay
    assert (tab[:lo] == 100.0 + nodes[lo]).all() and (tab[hi + 1:] == 100.0 + nodes[hi]).all()


def test_clamp_ties_and_no_valid_value():
    nodes = dedx_node_energies()

    class Holes:
        density = 1.0e-4

        def get_dedx(self, nuc, ke):
            i = int(np.searchsorted(nodes, ke))
            return float("nan") if 700 < i < 704 or i == 710 else float(i)   # 701..703 and 710 invalid

    tab = sample_dedx_table(Holes(), _nucleus("p"))
    assert tab[701] == 700.0 and tab[703] == 704.0 and tab[710] in (709.0, 711.0)
    assert tab[702] == 700.0   # equally far from 700 and 704: the lower node (argmin takes the first)
    assert tab[710] == 709.0
    assert tab[0] == 0.0 and tab[-1] == float(len(nodes) - 1)   # zero is a valid value

    class Nothing:
        density = 1.0e-4

        def get_dedx(self, nuc, ke):
            return float("nan")

    with pytest.raises(ValueError, match="no valid value"):
        sample_dedx_table(Nothing(), _nucleus("p"))


# ------------------------------------------------------------------------------------------------ the range ----
@pytest.mark.parametrize("name", [c.name for c in dc.CASES if c.along_z])
def test_range_quadrature_by_two_methods_and_against_the_track(fx, name):
    c, f = dc.case(name), fx.case(name)
    gas, nuc = mk.gas_of(c.gas), _nucleus(c.species)
    force = dr.stopping_force(_function(gas, nuc), nuc.Z, gas.density, mk.EFIELD)
    seams = dr.seam_energies(gas, nuc)
    ke = f["track"][:, 3]
    k = len(ke) - 1
    whole = dr.range_quadrature(force, ke[0], ke[k], seams)
    halved = dr.range_quadrature(force, ke[0], ke[k], seams, halve=1)
    other = dr.range_quadrature_mp(force, ke[0], ke[k], seams)
    print(name, "range", whole, "halved", halved - whole, "mpmath", other - whole, "stored", f["range"][k] - whole,
          "track", f["track"][k, 2] - c.vertex[2] - whole)
    assert abs(halved - whole) <= 1e-9 * whole and abs(other - whole) <= 1e-9 * whole
    assert abs(f["range"][k] - whole) <= 1e-9 * whole
    # the ODE and the integral are two statements of one track: the smooth track's z agrees at every grid time
    assert np.abs(f["track"][:, 2] - c.vertex[2] - f["range"]).max() <= 1e-9
    assert seams[0] < ke[0]   # the seam is inside the integral


# ------------------------------------------------------------------------------------------------ the tracks ----
_TRACKS: dict = {}


_RUNS = {name: (c, path_step) for name, c, path_step in dc.RUNS}


def _reference_tracks(name):
    if name not in _TRACKS:
        _TRACKS[name] = mk.case_tracks(*_RUNS[name])
    return _TRACKS[name]


def _oracle(orc, c, table=None, path_step=0.0):
    """(ODE rows, kept samples, n_steps) of the oracle, on the engine's table or on ``table``."""
    inp = dc.inputs(c.gas, path_step=path_step)
    assert inp.det_raw.path_step == path_step
    sp = inp.layout.species_of_row[c.row]
    det = inp.det_raw
    p4 = c.p4()
    old = det.species[sp].dedx
    try:
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float64)
            det.species[sp].dedx = _abi.dptr(table)
        track = orc.trajectory(det, sp, c.vertex, p4[:3])
        kept, rows = orc.point_cloud_samples(det, sp, p4, c.vertex, dc.SEED, 0, c.row)
    finally:
        det.species[sp].dedx = old
    return track, kept, rows, det


@pytest.mark.parametrize("name", list(_RUNS))
def test_oracle_track_against_table_side_and_smooth_reference(orc, fx, name):
    """Every case on the time grid, and ``dc.PATH_NAME``: one of them recorded by path length (the oracle, the
    table-side and the smooth solution each at its own sample times; rows compared at equal sample number)."""
    (c, path_step), f = _RUNS[name], fx.case(name)
    mass = dc.MASS[c.species]
    smooth, event, tabled, tab_event = _reference_tracks(name)
    # the fixture regenerates: the smooth track, its ending and the table's deviations
    assert event == f["event"] == c.event and len(smooth) == f["rows"] < dc.MAX_ROWS and len(tabled) == f["table_rows"]
    np.testing.assert_allclose(smooth[:, :3], f["track"][:, :3], rtol=0, atol=1e-11)
    np.testing.assert_allclose(dr.kinetic_energy(smooth[:, 3:6], mass), f["track"][:, 3], rtol=0, atol=1e-10)
    d_tab, e_tab = dr.table_deviation(smooth, tabled, mass)
    assert abs(d_tab - f["d_tab"]) <= 1e-3 * f["d_tab"] + 1e-11 and abs(e_tab - f["e_tab"]) <= 1e-3 * f["e_tab"] + 1e-10
    np.testing.assert_array_equal(f["p4"], c.p4())
    # the oracle against the converged solution ON THE TABLE: the rule of test_tracks_vs_converged_reference_ode
    track, kept, rows, det = _oracle(orc, c, path_step=path_step)
    assert len(track) == len(tabled) == rows and tab_event == c.event
    pos = float(np.abs(track[:, :3] - tabled[:, :3]).max())
    ke = float(np.abs(dr.kinetic_energy(track[:, 3:6], mass) - dr.kinetic_energy(tabled[:, 3:6], mass)).max())
    assert pos < 1e-7 and ke < 2e-6, (pos, ke)
    # ... and against the smooth track
    np.testing.assert_array_equal(chk.kept_from_track(track, mass, det), kept)
    fig = chk.check_track(f, kept, rows, det, along_z=c.along_z and not path_step,
                          min_electrons_per_row=0.0 if name == dc.WORST_BIN_CASE else 100.0)
    print(name, "vs table-side", pos, ke, "| vs smooth", fig)


def test_the_path_step_run_differs_from_the_time_grid(fx):
    """The path-length case really is another recording: more rows than on the grid while the proton is fast, the
    1e-10 s grid below the speed at which the path step takes longer than that."""
    grid, path = fx.case(dc.PATH_CASE), fx.case(dc.PATH_NAME)
    assert path["rows"] > 1.15 * grid["rows"]
    step = np.sqrt((np.diff(path["track"][:, :3], axis=0) ** 2).sum(axis=1))
    assert abs(step[0] - dc.PATH_STEP) < 1e-2 * dc.PATH_STEP   # (the chord; the proton slows down within the step)
    assert (step < dc.PATH_STEP * (1 + 1e-9)).all()
    assert (step < 0.5 * dc.PATH_STEP).sum() > 20   # the tail on the time grid


def test_launch_rows_are_the_workloads_rows():
    """``dedx_cases.Launch`` writes the Z and A of the workloads' rows out (it skips their kinematics pipelines)."""
    from attpc_engine_amd import workloads
    for gas, (workload, rows) in dc.GASES.items():
        pipeline, config, _ = workloads.WORKLOADS[workload]()
        launch = dc.inputs(gas)
        assert list(pipeline.get_proton_numbers()) == launch.z and list(pipeline.get_mass_numbers()) == launch.a, gas
        mine, theirs = launch.config.det_params, config.det_params
        assert mine.gas_target.compound_key == theirs.gas_target.compound_key and mine.gas_target.density == theirs.gas_target.density
        for field in ("length", "efield", "bfield", "mpgd_gain", "diffusion", "w_value"):
            assert getattr(mine, field) == getattr(theirs, field), (gas, field)
        for name, row in rows.items():
            assert (launch.z[row], launch.a[row]) == dc.NUCLEUS[name], (gas, name)


def test_worst_bin_case_starts_in_the_worst_bin():
    worst = None
    for gas_name, (_, rows) in dc.GASES.items():
        for species in rows:
            gas, nuc = mk.gas_of(gas_name), _nucleus(species)
            pr = dr.profile(_function(gas, nuc), sample_dedx_table(gas, nuc))
            w = pr.worst()
            if worst is None or pr.rel[w] > worst[0]:
                worst = (pr.rel[w], gas_name, species, pr.a[w], pr.b[w])
    c = dc.case(dc.WORST_BIN_CASE)
    assert (worst[1], worst[2]) == (c.gas, c.species) and worst[3] <= c.ke < worst[4], worst


# ------------------------------------------------------------------------------------------------ mutants ----
def _mutant_track(orc, c, mutant):
    """(kept, n_steps, det) of the oracle's integrator on a wrong table or with a wrong lookup."""
    gas, nuc = mk.gas_of(c.gas), _nucleus(c.species)
    f = _function(gas, nuc)
    if mutant == "sub16":
        table = dr.coarse_as_fine(dr.sample(f, dr.node_energies(16)))
    elif mutant == "per_nucleon":
        table = dr.sample(lambda e: f(e / nuc.A), dr.node_energies())
    elif mutant == "isotope":
        z, a = dc.NUCLEUS[c.species]
        other = nuclear_map.get_data(z, a + 1)
        table = sample_dedx_table(gas, other)
    else:
        inp = dc.inputs(c.gas)
        det = inp.det_raw
        read = dr.scalar_lookup(sample_dedx_table(gas, nuc), mutant)
        track, _ = dr.rk4_track(read, nuc.Z, nuc.mass, gas.density, det.bfield, det.efield, c.vertex, c.p4()[:3])
        return chk.kept_from_track(track, nuc.mass, det), len(track), det
    _, kept, rows, det = _oracle(orc, c, table)
    return kept, rows, det


def test_python_rk4_is_the_oracles(orc):
    c = dc.case("p_stops")
    gas, nuc = mk.gas_of(c.gas), _nucleus(c.species)
    track, _, rows, det = _oracle(orc, c)
    mine, event = dr.rk4_track(dr.scalar_lookup(sample_dedx_table(gas, nuc)), nuc.Z, nuc.mass, gas.density, det.bfield,
                               det.efield, c.vertex, c.p4()[:3])
    assert event == "ke" and len(mine) == rows
    np.testing.assert_allclose(mine, track, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("mutant", ["sub16", "nearest", "per_nucleon", "weight48", "isotope"])
def test_every_mutant_breaks_the_rule(orc, fx, mutant):
    broken = {}
    for c in dc.CASES:
        kept, rows, det = _mutant_track(orc, c, mutant)
        try:
            chk.check_track(fx.case(c.name), kept, rows, det, along_z=c.along_z)
        except AssertionError as err:
            broken[c.name] = err.args[0][:3] if err.args and isinstance(err.args[0], tuple) else str(err)[:80]
    print(mutant, "breaks", len(broken), "of", len(dc.CASES), "cases:", broken)
    assert broken, mutant
    if mutant == "sub16":   # the coarsest mutant: the factor 2 of the position rule is below its factor 4
        assert any(v[0] == "position" for v in broken.values()), broken
