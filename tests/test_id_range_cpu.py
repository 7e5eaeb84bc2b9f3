"""The id / seed cases of tests/helpers.py discriminate: with the oracle only, a device that narrowed the event id or the
seed in any of the ways of ``NARROWINGS`` would compute other kinematics, other electron counts or another jitter at
these cases -- so tests/test_gpu_id_range.py, which compares the device with the oracle there, would fail.  And the
documented design limit of the jitter: events 2^40 apart share their jitter and nothing else.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import ID_CASES, ID_CASE_IDS, NARROWINGS, U64, Inputs

JITTER_KEYS = [(tb << 14) | pad for tb, pad in ((0, 0), (37, 1234), (200, 5000), (511, 10239))]
ROW = 2  # the alpha of o16aa: the first simulated row
JITTER_EVENT_MASK = (1 << 40) - 1


def _key_word(seed: int) -> int:
    """seed[31:0] ^ rotl(seed[63:32], 13) ^ 0x100 (csrc/common.hpp jitter_key_word)."""
    hi = seed >> 32
    return (seed & 0xFFFFFFFF) ^ (((hi << 13) | (hi >> 19)) & 0xFFFFFFFF) ^ 0x100


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def inp():
    return Inputs("o16aa")


def _p4(orc, inp, seed, event):
    vertex, p4, status, attempts = orc.kin_batch(inp.kin, seed, event, 1)
    return np.concatenate([p4.ravel(), vertex.ravel(), attempts.astype(np.float64)])


def _track(orc, inp):
    """One fixed 8 MeV alpha track across the chamber: the electron counts along it depend on (seed, event) alone."""
    sp = inp.layout.species_of_row[ROW]
    mass = inp.det_raw.species[sp].mass
    ke, polar = 8.0, 1.2
    p = np.sqrt(ke * (ke + 2.0 * mass))
    momentum = [p * np.sin(polar), 0.0, p * np.cos(polar), ke + mass]
    return sp, orc.trajectory(inp.det_raw, sp, [0.0, 0.0, 0.3], momentum)


def _electrons(orc, inp, sp, track, seed, event):
    return orc.electrons(inp.det_raw, sp, track, seed, event, 1 + ROW)


def _jitter(orc, seed, event):
    return np.array([orc.jitter_uniform(seed, event, k) for k in JITTER_KEYS])


def test_every_case_is_reached_by_an_event_and_a_seed_narrowing():
    """Each case crosses a boundary of the event id that some narrowing model trips over, with a seed whose high
    word matters; and every model is tripped by some case.  (A case below 2^24 with a 32-bit seed fails here.)"""
    hit = set()
    for case in ID_CASES:
        changed = [m for m in NARROWINGS if any(m(case.seed, e) != (case.seed, e) for e in case.ids())]
        assert any(m.on == "event" for m in changed), (case, "no event narrowing changes this case's ids")
        assert any(m.on == "seed" for m in changed), (case, "no seed narrowing changes this case's seed")
        hit.update(m.name for m in changed)
    assert hit == {m.name for m in NARROWINGS}, hit


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_narrowed_ids_and_seeds_give_other_numbers(orc, inp, case):
    """For every narrowing model that changes this case's (seed, event) pairs: the kinematics (p4, vertex, attempts)
    and the Fano electron counts along a track differ at every changed event, and the jitter differs at one event of
    the range at least (a jitter-only model: at every event)."""
    sp, track = _track(orc, inp)
    assert len(track) > 100
    checked = 0
    for model in NARROWINGS:
        changed = [e for e in case.ids() if model(case.seed, e) != (case.seed, e)]
        if not changed:
            continue
        for ev in changed:
            s2, e2 = model(case.seed, ev)
            if model.scope == "all":
                assert not np.array_equal(_p4(orc, inp, case.seed, ev), _p4(orc, inp, s2, e2)), (case, model, ev)
                assert not np.array_equal(_electrons(orc, inp, sp, track, case.seed, ev),
                                          _electrons(orc, inp, sp, track, s2, e2)), (case, model, ev)
            # the jitter sees the key word and event[39:0] only: it changes exactly where those do
            inputs_differ = _key_word(s2) != _key_word(case.seed) or (e2 ^ ev) & JITTER_EVENT_MASK != 0
            jitter_differs = not np.array_equal(_jitter(orc, case.seed, ev), _jitter(orc, s2, e2))
            assert jitter_differs == inputs_differ, (case, model, ev)
        checked += 1
    assert checked >= 3, case


def test_every_narrowing_changes_the_jitter_at_some_case(orc):
    """Each model changes the jitter of some event of the table: a device with the narrowing in its flush loop alone
    (the Philox4x32 draws right) still fails the cloud comparison."""
    hits = set()
    for case in ID_CASES:
        for model in NARROWINGS:
            for ev in case.ids():
                s2, e2 = model(case.seed, ev)
                if not np.array_equal(_jitter(orc, case.seed, ev), _jitter(orc, s2, e2)):
                    hits.add(model.name)
    assert hits == {m.name for m in NARROWINGS}, hits


@pytest.mark.parametrize("case", ID_CASES, ids=ID_CASE_IDS)
def test_the_case_values_are_exact_in_the_oracle_call(orc, inp, case):
    """The oracle itself takes full-width ids: a batch from first_event equals event-by-event calls (the ids reach
    orc_kin_event as u64, not through a float or a signed type)."""
    vertex, p4, status, attempts = orc.kin_batch(inp.kin, case.seed, case.first_event, case.n, threads=4)
    for e in (0, case.n // 2, case.n - 1):
        one = orc.kin_batch(inp.kin, case.seed, case.first_event + e, 1)
        np.testing.assert_array_equal(p4[e], one[1][0])
        np.testing.assert_array_equal(vertex[e], one[0][0])


def test_events_2_pow_40_apart_share_the_jitter_and_nothing_else(orc, inp):
    """The jitter's counter holds event[39:0] (csrc/common.hpp): events k and k + 2^40 have the
    same jitter for every key -- and different Philox4x32 draws, hence different kinematics and electron counts."""
    L = orc.lib()
    for seed in (0, 0xFEDCBA9876543210 & ((1 << 63) - 1), U64 - 1):
        for k in (0, 17, (1 << 40) - 1, (1 << 33) + 5, U64 - (1 << 40) - 3):
            far = (k + (1 << 40)) % U64
            np.testing.assert_array_equal(_jitter(orc, seed, k), _jitter(orc, seed, far))
            a = (C.c_double(), C.c_double())
            b = (C.c_double(), C.c_double())
            L.orc_rng_pair(seed, k, 0, 0, C.byref(a[0]), C.byref(a[1]))
            L.orc_rng_pair(seed, far, 0, 0, C.byref(b[0]), C.byref(b[1]))
            assert (a[0].value, a[1].value) != (b[0].value, b[1].value)
            assert not np.array_equal(_p4(orc, inp, seed, k), _p4(orc, inp, seed, far))
    sp, track = _track(orc, inp)
    assert not np.array_equal(_electrons(orc, inp, sp, track, 5, 100), _electrons(orc, inp, sp, track, 5, 100 + (1 << 40)))
    assert orc.jitter_uniform(5, 100, 77) != orc.jitter_uniform(5, 101, 77)  # (the event does enter the jitter)


def test_ids_and_seeds_that_would_wrap_are_rejected_before_the_c_abi():
    """ctypes wraps a u64 argument silently (seed=-1 -> 2^64 - 1, seed=2^64 + 5 -> 5); the package refuses such values
    (like numpy's default_rng refuses a negative seed) before any native call."""
    from attpc_engine_amd._abi import check_id_range
    assert check_id_range(U64 - 1, U64 - 10, 10) == (U64 - 1, U64 - 10, 10)
    assert check_id_range(0, 0, 0) == (0, 0, 0)
    assert check_id_range(np.uint64(5), np.int64(7), 3) == (5, 7, 3)
    for seed, first, n in ((-1, 0, 1), (U64, 0, 1), (U64 + 5, 0, 1), (0, -3, 1), (0, U64 - 10, 11), (0, 1, U64),
                           (0, 0, -1), (0, U64, 1)):
        with pytest.raises(ValueError):
            check_id_range(seed, first, n)
