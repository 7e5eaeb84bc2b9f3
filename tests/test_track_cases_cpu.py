"""The inputs of tests/test_gpu_track_paths.py do what that file assumes -- on the CPU oracle alone, no device.

Every entry of tests/track_cases.py ends the way it says: the oracle's row count is the entry's, and one more oracle
step from the last kept state (classical RK4 on the oracle's own right-hand side, tests/track_cases.py::next_sample)
fires the named terminal event and no other.  The runs that the GPU file sizes by a property of the oracle's output --
arena blocks of the one-workgroup runs, the share of events at the sample limit, a stop in a middle substep -- have
that property."""
import math

import numpy as np
import pytest

from tests import track_cases as tc
from tests.helpers import Inputs


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _oracle(orc, c):
    inp = tc.inputs(c.detector)
    sp = inp.layout.species_of_row[c.row]
    p4 = c.p4()
    track = orc.trajectory(inp.det_raw, sp, c.vertex, p4[:3])
    kept, rows = orc.point_cloud_samples(inp.det_raw, sp, p4, c.vertex, tc.SEED, 0, c.row)
    assert rows == len(track)
    return inp, sp, track, kept, rows


@pytest.mark.parametrize("c", tc.CASES, ids=tc.CASE_IDS)
def test_case_ends_as_its_entry_says(orc, c):
    inp, sp, track, kept, rows = _oracle(orc, c)
    n_steps, event, where = c.expected
    mass = tc.MASS[c.species]
    assert rows == n_steps, (c.name, rows, n_steps)
    assert where == ("first" if rows == 1 else "last" if rows == tc.TIME_SAMPLES else "middle")
    g_last = tc.event_functions(track[-1], mass)
    if where == "last":
        # alive at the last sample: no event function has reached its limit
        assert event == "none"
        assert g_last[0] > 0.0 and g_last[1] < 0.0 and g_last[2] > 0.0 and g_last[3] < 0.0, g_last
    else:
        nxt, events, _, _ = tc.next_sample(orc, inp.det_raw, sp, track[-1])
        assert events == [event], (c.name, events, g_last, tc.event_functions(nxt, mass))
    print(c.name, "rows", rows, "kept", len(kept), "ends by", event, "g at the last row", g_last)


def test_the_full_window_track_fills_the_block_table(orc):
    _, _, _, kept, rows = _oracle(orc, tc.case("full_window"))
    assert rows == tc.TIME_SAMPLES and len(kept) > 78 * 128  # the 79th block-table entry is written


@pytest.mark.parametrize("name", ["ranges_out", "leaves_forward", "leaves_backward", "leaves_cage"])
def test_each_event_alone_ends_a_track_past_one_wave_of_rows(orc, name):
    assert tc.case(name).expected[0] > 64


@pytest.mark.parametrize("name,index", [("on_window_forward", 1), ("on_window_backward", 1), ("on_cathode_backward", 2),
                                        ("on_cathode_forward", 2), ("on_cage_outward", 3), ("on_cage_inward", 3)])
def test_the_event_function_is_exactly_zero_at_the_vertex(name, index):
    c = tc.case(name)
    state = np.array([*c.vertex, *(np.array(c.p4()[:3]) / tc.MASS[c.species])])
    assert tc.event_functions(state, tc.MASS[c.species])[index] == 0.0
    # the device's form of the cage test, rounded product by product or fused
    x, y = c.vertex[0], c.vertex[1]
    assert index != 3 or (x * x + y * y - tc.RHO_MAX * tc.RHO_MAX == 0.0 and y == 0.0)
    # ... and the stopping direction is the one the name says
    moving = {1: c.p4()[2], 2: -c.p4()[2], 3: c.p4()[0]}[index]
    assert (moving > 0.0) == (c.expected[2] == "first")


def test_hair_above_the_ke_limit(orc):
    c = tc.case("hair_above_ke_limit")
    ke = float(tc.kinetic_energy(np.array(c.p4()[:3]) / tc.MASS["p"], tc.MASS["p"]))
    assert tc.KE_LIMIT * 1.005 < ke < tc.KE_LIMIT * 1.015  # above the limit by far more than the 2e-4 of its rounding


def test_dedx_table_ends(orc):
    inp, sp, track, _, _ = _oracle(orc, tc.case("dedx_last_node"))
    assert tc.kinetic_energy(track[:, 3:6], tc.MASS["be11"]).min() >= 16384.0  # the last node on every row
    for name, node in (("dedx_above_node_4mev", 4.0), ("dedx_below_node_4mev", 4.0), ("dedx_above_node_1kev", 2.0 ** -10)):
        c = tc.case(name)
        ke = float(tc.kinetic_energy(np.array(c.p4()[:3]) / tc.MASS["p"], tc.MASS["p"]))
        # the neighbour of the node on the grid of m (gamma - 1): a few times m 2^-52 away, on the side named
        assert 0.0 <= (ke - node) * c.node_side < 4.0 * tc.MASS["p"] * 2.0 ** -52 and (ke >= node) == (c.node_side > 0), (name, ke)
        table = np.ctypeslib.as_array(inp.det_raw.species[inp.layout.species_of_row[2]].dedx, shape=(1409,))
        e, m = math.frexp(node)[1] - 1, 0
        node_value = table[(e + 30) * 32 + m]
        got = orc.lib().orc_dedx_lookup(inp.det_raw.species[inp.layout.species_of_row[2]].dedx, ke)
        assert abs(got - node_value) <= 1e-9 * node_value, (name, got, node_value)


def _accumulated_time(inp, track):
    gv2 = (track[:-1, 3:6] ** 2).sum(axis=1)
    h = np.minimum(inp.det_raw.path_step / (tc.C_LIGHT * np.sqrt(gv2 / (1.0 + gv2))), tc.H_GRID)
    return float(h.sum()), h


def test_path_cases_are_told_apart_by_the_accumulated_time(orc):
    inp, _, track, _, rows = _oracle(orc, tc.case("path_window"))
    t, h = _accumulated_time(inp, track)
    assert rows == tc.TIME_SAMPLES and (h == tc.H_GRID).all() and abs(t - 1.0e-6) < 1e-15  # ends AT the window's end
    same, _, grid_track, _, _ = _oracle(orc, tc.case("full_window"))
    np.testing.assert_array_equal(track, grid_track)  # (5 mm steps are the time grid)
    inp, _, track, _, rows = _oracle(orc, tc.case("path_cap"))
    t, h = _accumulated_time(inp, track)
    assert rows == tc.TIME_SAMPLES and h.max() < 0.5 * tc.H_GRID and t < 0.5e-6  # the cap came first


def test_path_window_cannot_end_a_track_before_the_cap():
    """A step is at most 1e-10 s: after the 9999 steps that come before the last one allowed, the window test
    ``t + h > 1e-6 (1 + 1e-9)`` is still false, in the arithmetic of the oracle and the device (a running sum)."""
    t = 0.0
    for _ in range(tc.TIME_SAMPLES - 2):
        t += tc.H_GRID
    assert not t + tc.H_GRID > 1.0e-6 * (1.0 + 1.0e-9)
    assert t + tc.H_GRID - 1.0e-6 < 1e-17


@pytest.mark.parametrize("name,nsub,path_step,n", tc.SUBSTEP_RUNS)
def test_some_track_stops_in_a_middle_substep(orc, name, nsub, path_step, n):
    """The oracle does not say in which substep a track stopped; one more step from its last kept state does.  A track
    that stops in a substep that is not the last must not run the substeps behind it (the ``&& !stop`` of the loop)."""
    kw = {"path_step": path_step} if path_step else {}
    inp = Inputs(name, ode_substeps=nsub, **kw)
    assert inp.det_raw.ode_substeps == nsub
    vertex, p4, _, _ = orc.kin_batch(inp.kin, tc.SUBSTEP_SEED, tc.SUBSTEP_FIRST, n, threads=4)
    stopped_in = np.zeros(nsub, dtype=np.int64)
    for e in range(n):
        for row in inp.indices:
            sp = inp.layout.species_of_row[row]
            track = orc.trajectory(inp.det_raw, sp, vertex[e], p4[e, row, :3])
            if len(track) < tc.TIME_SAMPLES:
                _, events, sub, _ = tc.next_sample(orc, inp.det_raw, sp, track[-1])
                assert events and 0 <= sub < nsub, (e, row, events, sub)
                stopped_in[sub] += 1
    print(name, "substeps", nsub, "path step", path_step, "tracks stopped in substep", stopped_in.tolist())
    assert stopped_in[:-1].sum() >= 1, stopped_in


@pytest.mark.parametrize("name,seed,first,n", tc.REFILL_RUNS)
def test_one_workgroup_runs_need_more_than_two_pools_per_wave(orc, name, seed, first, n):
    inp = Inputs(name)
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=4)
    blocks = 0
    for e in range(n):
        for row in inp.indices:
            kept, _ = orc.point_cloud_samples(inp.det_raw, inp.layout.species_of_row[row], p4[e, row], vertex[e], seed, first + e, row)
            blocks += -(-len(kept) // 128)
    print(name, "tracks", n * len(inp.indices), "arena blocks", blocks)
    assert n * len(inp.indices) >= 704 and blocks >= tc.REFILL_MIN_BLOCKS


def test_a_share_of_the_events_hits_the_sample_limit(orc):
    inp = Inputs(tc.sample_limit_workload)
    _, _, status, attempts = orc.kin_batch(inp.kin, tc.LIMIT_SEED, tc.LIMIT_FIRST, tc.LIMIT_EVENTS, threads=4)
    failed = int((status != 0).sum())
    print("events at the sample limit", failed, "of", tc.LIMIT_EVENTS)
    assert 0.2 * tc.LIMIT_EVENTS <= failed <= 0.8 * tc.LIMIT_EVENTS and (attempts == 1).all()
    for lo in range(0, tc.LIMIT_EVENTS, tc.LIMIT_CHUNK):  # every chunk of the fused run mixes good and failed events
        part = status[lo: lo + tc.LIMIT_CHUNK]
        assert (part != 0).any() and (part == 0).any(), lo
