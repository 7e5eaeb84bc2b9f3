"""``track_kernel`` (csrc/tracks.hip) against what the stopping-power FUNCTION gives -- not against the table it reads.

The single tracks of tests/dedx_cases.py, one launch per gas, under the rule of tests/dedx_check.py against the smooth
tracks of tests/golden/dedx_smooth.npz (``get_dedx`` called in every right-hand side, DOP853 at rtol 1e-12; no table on
that side): positions within ``2 D_tab + 1e-7 m`` and within 0.5 mm, rows within max(3, 2 %) and the same ending, the
range of the tracks along +z against a quadrature over the energy, and the running sum of electrons inside
``Q_k - k - q <= S_k <= Q_k + q``.  The stage switches: the same launches at two substeps, and one case recorded by
path length against fixture rows of its own.  tests/test_dedx_table_cpu.py shows on the CPU that the oracle passes this rule and
that a table of 16 sub-bins, a nearest-node lookup, nodes at the per-nucleon energy, a 48-bit weight and the
neighbouring isotope's table each break it.  Reads only the fixture and numpy on the reference side.  Needs a real
MI355X: run with ``-m gpu``.

Measured on an MI355X: profiles/r27_dedx_table.md."""
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import dedx_cases as dc
from tests import dedx_check as chk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def fx():
    return chk.Fixture(Path(__file__).resolve().parent / "golden" / "dedx_smooth.npz")


def _device_tracks(ctx, inp, p4, vertex, max_samples=dc.MAX_ROWS):
    ctx.forget("det")  # configured through the C ABI directly
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, inp.det), "det_configure")
    n = len(p4)
    nt = n * inp.layout.n_sim
    samples = np.zeros((nt, max_samples, 4))
    counts = np.empty(nt, dtype=np.int32)
    steps = np.empty(nt, dtype=np.int32)
    ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, dc.SEED, 0, n, inp.layout, _abi.dptr(np.ascontiguousarray(p4)),
                                       _abi.dptr(np.ascontiguousarray(vertex)), max_samples, _abi.dptr(samples),
                                       _abi.iptr(counts, _abi.C.c_int32), _abi.iptr(steps, _abi.C.c_int32)), "tracks")
    return samples, counts, steps


def _check_launch(ctx, fx, gas, ode_substeps=1, path_step=0.0, only=None, fixture_name=None):
    inp = dc.inputs(gas, ode_substeps=ode_substeps, path_step=path_step)
    assert inp.det.fano_factor == 0.0 and inp.det.ode_substeps == ode_substeps and inp.det.path_step == path_step
    cases, p4, vertex = dc.events_of(gas, only)
    assert cases
    samples, counts, steps = _device_tracks(ctx, inp, p4, vertex)
    for e, c in enumerate(cases):
        ref = fx.case(fixture_name or c.name)
        np.testing.assert_array_equal(ref["p4"], p4[e, c.row])
        for isim, row in enumerate(inp.indices):
            t = e * inp.layout.n_sim + isim
            if row != c.row:   # no momentum: one row, no electrons
                assert steps[t] == 1 and counts[t] == 0, (c.name, row, steps[t], counts[t])
                continue
            assert 0 < counts[t] < dc.MAX_ROWS
            fig = chk.check_track(ref, samples[t, :counts[t]], int(steps[t]), inp.det, along_z=c.along_z and not path_step,
                                  min_electrons_per_row=0.0 if c.name == dc.WORST_BIN_CASE else 100.0)
            print(f"{fixture_name or c.name} substeps {ode_substeps}: rows {fig['rows']} (smooth {fig['smooth_rows']}), kept {fig['kept']}, "
                  f"left out {fig['left_out']}, ends by {fig['event']}, position {fig['position']:.3e} m of "
                  f"{fig['position_bound']:.3e}, range {fig.get('range_difference', float('nan')):.3e} m, electrons over "
                  f"{fig['electrons_over']:.2f} under {fig['electrons_under']:.2f} of q {fig['electrons_q']:.2f}")


@pytest.mark.parametrize("gas", sorted(dc.GASES))
def test_device_tracks_against_the_smooth_function(ctx, fx, gas):
    _check_launch(ctx, fx, gas)


@pytest.mark.parametrize("gas", sorted(dc.GASES))
def test_two_substeps_read_the_table_at_other_energies(ctx, fx, gas):
    """``ode_substeps = 2``: the same launch on steps of 5e-11 s, against the same fixture rows."""
    _check_launch(ctx, fx, gas, ode_substeps=2)


def test_path_step_records_at_another_spacing(ctx, fx):
    """``path_step`` set on one ranging-out case (``dedx_cases.PATH_CASE``): samples every 0.6 mm of arc length while
    that is finer than the 1e-10 s grid, against the fixture's smooth track recorded the same way at its own speeds."""
    _check_launch(ctx, fx, dc.case(dc.PATH_CASE).gas, path_step=dc.PATH_STEP, only=dc.PATH_CASE, fixture_name=dc.PATH_NAME)
