"""The layout limits of the C ABI on the CPU side: ATTPC_MAX_STEPS = 8 kinematic steps (18 rows) and ATTPC_MAX_SIM = 8
simulated nuclei.  The two long decay chains of tests/helpers.py (``chain7``, ``chain8``) are pinned here on the oracle:
their layouts, that every event is allowed, and that their clouds reach what the device tests at the limits rely on
(labels 14..17, every charged position 0..7 the last writer of some key, keys lit by three and more nuclei).  The
oracle's kinematics on an 8-step chain is pinned against the reference in test_oracle_golden.py."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.luts import build_layout, species_for
from attpc_engine_amd.detector.simulator import default_indices
from oracle import pyoracle as orc
from tests.helpers import CHAIN8_INDICES, LONG_CHAINS, Inputs, chain7, chain8, overlap_counts


def test_chain_layouts_reach_the_limits():
    a = Inputs(chain7)
    assert a.n_rows == 16 and a.kin.n_steps == 7
    assert a.indices == [2, 4, 6, 8, 10, 12, 14, 15] and a.layout.n_sim == _abi.MAX_SIM
    assert a.species == [(1, 2), (1, 1), (2, 4), (1, 3), (6, 12)]
    assert a.z[6] == 0 and a.layout.species_of_row[6] == -1  # the neutron: a dead track at isim 2
    b = Inputs(chain8)
    assert b.n_rows == _abi.MAX_ROWS == 18 and b.kin.n_steps == _abi.MAX_STEPS
    assert b.indices == CHAIN8_INDICES and sorted(b.indices) != b.indices and b.layout.n_sim == _abi.MAX_SIM
    assert len(b.species) == 7 and {(13, 26), (12, 25), (10, 20), (4, 8)} <= set(b.species)
    assert (b.z[16], b.a[16], b.z[17], b.a[17]) == (2, 4, 4, 8)
    for row in b.indices:
        assert b.species[b.layout.species_of_row[row]] == (b.z[row], b.a[row])


def test_default_indices_of_18_rows_are_refused():
    """The reference's default indices for 18 rows name 9 nuclei; the layout holds 8."""
    b = Inputs(chain8)
    idx = default_indices(18)
    assert len(idx) == 9
    with pytest.raises(ValueError, match="at most 8 simulated nuclei per event"):
        build_layout(b.z, b.a, idx, species_for(b.z, b.a, idx))
    build_layout(b.z, b.a, idx[:8], species_for(b.z, b.a, idx[:8]))  # eight of them are fine


@pytest.mark.parametrize("name", ["chain7", "chain8"])
def test_long_chain_kinematics_on_the_oracle(name):
    inp = Inputs(LONG_CHAINS[name])
    vertex, p4, status, attempts = orc.kin_batch(inp.kin, 11, 0, 2000, threads=8)
    assert (status == 0).all()
    if name == "chain7":
        assert 0.005 < (attempts > 1).mean() < 0.05  # the whole-event rejection loop runs
    np.testing.assert_allclose(p4[:, 0] + p4[:, 1], p4[:, 2] + p4[:, 3], atol=1e-9)
    for s in range(1, inp.kin.n_steps):  # every decay conserves its parent's (the previous residual's) 4-momentum
        np.testing.assert_allclose(p4[:, 1 + 2 * s], p4[:, 2 + 2 * s] + p4[:, 3 + 2 * s], atol=1e-8)


@pytest.mark.parametrize("name", ["chain7", "chain8"])
def test_long_chain_clouds_overlap_and_every_position_wins(name):
    inp = Inputs(LONG_CHAINS[name])
    vertex, p4, _, _ = orc.kin_batch(inp.kin, 77, 5, 12, threads=4)
    wins, shared3, labels = overlap_counts(orc, inp, p4, vertex, 77, 5)
    charged = [inp.layout.species_of_row[row] >= 0 for row in inp.indices]
    print(name, "points won per isim", wins.tolist(), "keys lit by >= 3 nuclei", shared3, "labels", sorted(labels))
    assert all(w > 0 for w, c in zip(wins, charged) if c) and all(w == 0 for w, c in zip(wins, charged) if not c)
    assert shared3 > 20
    assert {14, 15} <= labels if name == "chain7" else {16, 17} <= labels
