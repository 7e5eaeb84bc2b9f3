"""Generate tests/golden/dedx_smooth.npz: what the stopping-power FUNCTION gives, with no table anywhere.

Run in the build container only (the reference tree never travels):

    python3 -B tests/golden/make_dedx_smooth.py

Two parts, data only:

* the tie to the reference: ``make_golden.py``'s stand-ins with the smooth ``GasTarget`` of this repository in place
  of ``TableGasTarget``, and the reference's unmodified ``solver.equation_of_motion`` on ``N_STATES`` states (every
  species of tests/dedx_cases.py, kinetic energies from 1e-5 to 100 MeV, random directions and positions).
  tests/dedx_reference.py's restatement of the right-hand side must equal these to 1e-13 relative
  (tests/test_dedx_table_cpu.py);
* per case of tests/dedx_cases.py: the initial conditions, the smooth track (the restated right-hand side with
  ``get_dedx`` called live, DOP853 at rtol 1e-12) on the 1e-10 s grid as (x, y, z, KE), its row count and terminal
  event, ``D_tab`` and ``E_tab`` (largest position and energy difference at equal grid time to the same ODE
  integrated on the restated table), and for the tracks along +z the range by quadrature from the start energy down
  to the smooth track's energy at every grid time;
* one of the cases again, recorded by path length (``dedx_cases.PATH_CASE`` at ``PATH_STEP``): each of the two
  solutions at its own sample times, D_tab and E_tab at equal sample number.

The grid is stored whole (no thinning); the file is smaller than kin_exact.npz.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(OUT))

from attpc_engine_amd import GasTarget, nuclear_map  # noqa: E402
from attpc_engine_amd.detector.luts import sample_dedx_table  # noqa: E402
from tests import dedx_cases as dc  # noqa: E402
from tests import dedx_reference as dr  # noqa: E402

N_STATES = 192
COMPOUND = {"he": [(2, 4, 1)], "d2": [(1, 2, 2)]}
PRESSURE = 600.0
BFIELD, EFIELD = 2.85, 45000.0   # workloads.detector_config


def gas_of(name: str) -> GasTarget:
    return GasTarget(COMPOUND[name], PRESSURE, nuclear_map)


def case_tracks(c, path_step: float = 0.0):
    """-> (smooth rows, event, table rows, table event) of one case, both by DOP853 and without the engine; on the time
    grid, or recorded by path length (each solution at its own sample times)."""
    gas = gas_of(c.gas)
    nuc = nuclear_map.get_data(*dc.NUCLEUS[c.species])
    p4 = c.p4()
    smooth, event = dr.integrate_track(lambda ke: gas.get_dedx(nuc, ke), nuc.Z, nuc.mass, gas.density, BFIELD, EFIELD,
                                       c.vertex, p4[:3], path_step=path_step)
    table = sample_dedx_table(gas, nuc)
    tabled, tab_event = dr.integrate_track(dr.scalar_lookup(table), nuc.Z, nuc.mass, gas.density, BFIELD, EFIELD,
                                           c.vertex, p4[:3], path_step=path_step)
    return smooth, event, tabled, tab_event


def reference_states(rng):
    """States for the reference's equation_of_motion -> (gas index, species index, state [n, 6])."""
    species = list(dc.NUCLEUS)
    gas_i = np.empty(N_STATES, dtype=np.int64)
    sp_i = np.empty(N_STATES, dtype=np.int64)
    states = np.empty((N_STATES, 6))
    for n in range(N_STATES):
        sp_i[n] = n % len(species)
        gas_i[n] = (n // len(species)) % 2
        mass = dc.MASS[species[sp_i[n]]]
        ke = 10.0 ** rng.uniform(-5.0, 2.0)
        gv = np.sqrt(ke * (ke + 2.0 * mass)) / mass
        direction = rng.normal(size=3)
        direction /= np.linalg.norm(direction)
        states[n, :3] = rng.uniform(-0.2, 0.2, 3) + [0.0, 0.0, 0.5]
        states[n, 3:] = gv * direction
    return gas_i, sp_i, states


def main() -> None:
    sys.dont_write_bytecode = True  # never leave __pycache__ under the reference tree
    import make_golden
    make_golden.install_standins()
    sys.modules["spyral_utils.nuclear.target"].GasTarget = GasTarget   # the smooth model, not TableGasTarget
    sys.path.insert(0, str(make_golden.REF_SRC))
    import attpc_engine  # noqa: F401  the reference package, unmodified
    from attpc_engine.detector import solver

    out = {}
    rng = np.random.default_rng(20261020)
    gas_names = ["he", "d2"]
    gas_i, sp_i, states = reference_states(rng)
    results = np.empty_like(states)
    for n in range(N_STATES):
        nuc = nuclear_map.get_data(*dc.NUCLEUS[list(dc.NUCLEUS)[sp_i[n]]])
        results[n] = solver.equation_of_motion(0.0, states[n], -BFIELD, -EFIELD, gas_of(gas_names[gas_i[n]]), nuc)
    out.update(eom_gas=gas_i, eom_species=sp_i, eom_states=states, eom_results=results,
               species_names=np.array(list(dc.NUCLEUS)), gas_names=np.array(gas_names),
               bfield=BFIELD, efield=EFIELD, pressure=PRESSURE)

    out["case_names"] = np.array([name for name, _, _ in dc.RUNS])
    for i, (name, c, path_step) in enumerate(dc.RUNS):
        gas = gas_of(c.gas)
        nuc = nuclear_map.get_data(*dc.NUCLEUS[c.species])
        smooth, event, tabled, tab_event = case_tracks(c, path_step)
        ke = dr.kinetic_energy(smooth[:, 3:6], nuc.mass)
        d_tab, e_tab = dr.table_deviation(smooth, tabled, nuc.mass)
        out[f"p4_{i}"] = np.array(c.p4())
        out[f"vertex_{i}"] = np.array(c.vertex)
        out[f"track_{i}"] = np.column_stack([smooth[:, :3], ke])
        out[f"rows_{i}"] = len(smooth)
        out[f"event_{i}"] = event
        out[f"table_rows_{i}"] = len(tabled)
        out[f"d_tab_{i}"] = d_tab
        out[f"e_tab_{i}"] = e_tab
        if c.along_z and not path_step:
            force = dr.stopping_force(lambda e: gas.get_dedx(nuc, e), nuc.Z, gas.density, EFIELD)
            seams = dr.seam_energies(gas, nuc)
            # R(KE_0 -> KE_k) = sum of the pieces between neighbouring grid energies
            pieces = [dr.range_quadrature(force, ke[k], ke[k + 1], seams) for k in range(len(ke) - 1)]
            out[f"range_{i}"] = np.concatenate([[0.0], np.cumsum(pieces)])
        print(f"{name}: rows {len(smooth)} ({event}), on the table {len(tabled)} ({tab_event}), D_tab {d_tab:.3e} m, "
              f"E_tab {e_tab:.3e} MeV")
    np.savez_compressed(OUT / "dedx_smooth.npz", **out)
    print("wrote", OUT / "dedx_smooth.npz", (OUT / "dedx_smooth.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
