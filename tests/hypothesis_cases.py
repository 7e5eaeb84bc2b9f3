"""Cases of the fit hypotheses (include/attpc_engine.h, "fit hypotheses"), shared by tests/test_hypothesis_cpu.py (the
host C++ and the mutants against the restatement) and tests/test_gpu_hypothesis.py (the device against the restatement).

``hand()``: the hand-made events of tests/fit_cases.py in the layout ``INDICES8`` / ``SPECIES8`` (two hypotheses: the
proton and the 11Be), with their estimate records and their special starts.  ``walk_cases()``: events whose f tables
are written by hand -- no fit is needed to say what the walk must make of them --, name -> ``WalkCase``.
``PID_GATES``: two gates in the plane of the hand-made events' own (B rho, dE/dx) that hold both species for some
slots of the event "eight", one for others and none for one."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from attpc_engine_amd._abi import ESTIMATE_DTYPE, FIT_DTYPE, FIT_NO_START
from tests import estimate_reference as est
from tests import fit_cases as cases
from tests import hypothesis_reference as href
from tests import pid_cases
from tests import pid_reference as pref

NAN = float("nan")
FIELD = 2.85
PARAMS = est.Params(cases.BEAM_REGION, cases.MIN_POINTS, FIELD)
# position 0 (a proton position) has the gate "wide" of tests/pid_cases.py, which holds the slots of "eight" whose dE/dx
# is below 4 (slots 0, 1 and 3); position 1 (an 11Be position) a box that holds dE/dx 2.75 .. 70 at B rho 0.1 .. 0.7
# (slots 2, 3, 4, 6 and 7).  Slot 3 is held by both, slots 0 and 1 by the proton's alone, 2, 4, 6 and 7 by the 11Be's
# alone, slot 5 (dE/dx 74) by none; the other events' tracks by the 11Be's or by none.
PID_GATES = (pid_cases.GATES["wide"], np.array([(0.1, 2.75), (0.7, 2.75), (0.7, 70.0), (0.1, 70.0)])) + (None,) * 6


@functools.lru_cache(maxsize=None)
def hand():
    """(model, events, csr, estimates, start, layout): read-only."""
    model = cases.model()
    events = cases.hand_cases(model)
    csr = cases.csr(events)
    estimates = est.records(*csr, cases.INDICES8, PARAMS)
    start = cases.special_starts(events)
    for array in (*csr, estimates, start):
        array.setflags(write=False)
    return model, events, csr, estimates, start, href.Layout(href.species_of_positions(model))


def hand_pid(estimates):
    """The pid records of the hand-made events behind ``PID_GATES``."""
    return pref.records(estimates, PID_GATES, pref.ANY, species=cases.SPECIES8)


class WalkCase(NamedTuple):
    species: tuple      # the detector species of every position, -1: none
    candidates: int     # the settings' mask
    held: tuple | None  # pid.held of every slot, or None: no particle identification
    f: tuple            # [n_sim][H]
    status: tuple       # [n_sim][H] the fit records' status
    want: dict          # field -> [n_sim]: what the contract says of the event, worked by hand


def _case(species, f, want, candidates=href.ALL, held=None, status=None):
    status = status or tuple(tuple(0 for _ in row) for row in f)
    return WalkCase(tuple(species), candidates, held, tuple(map(tuple, f)), tuple(map(tuple, status)), want)


D, T, NC, NF = href.DISPLACED, href.TAKEN, href.NO_CANDIDATE, href.NO_FIT


@functools.lru_cache(maxsize=None)
def walk_cases() -> dict:
    return {
        # both slots are better as species 0: the first takes its position, the second is displaced to the other
        "two slots prefer one position": _case([10, 11], [(1.0, 5.0), (2.0, 3.0)],
                                               dict(position=[0, 1], status=[0, D], f_next=[5.0, 2.0], fitted=[3, 3])),
        "three slots for two fitted positions": _case([10, 11, -1], [(1.0, 5.0), (7.0, 3.0), (2.0, 2.5)],
                                                      dict(position=[0, 1, -1], status=[0, 0, T], tried=[3, 3, 3])),
        # an exact tie goes to the lowest position; the free position of the same f is no displacement
        "an exact tie between two species": _case([10, 11], [(4.0, 4.0), (4.0, 4.0)],
                                                  dict(position=[0, 1], status=[0, 0], f_next=[4.0, 4.0])),
        "two positions of one species": _case([10, 10, 11], [(1.0, 9.0), (2.0, 9.0), (8.0, 3.0)],
                                              dict(position=[0, 1, 2], status=[0, 0, 0], species=[10, 10, 11], f_next=[9.0, 9.0, 8.0])),
        "a NaN f": _case([10, 11], [(NAN, 6.0), (1.0, NAN)], dict(position=[1, 0], status=[0, 0], fitted=[2, 1], f_next=[NAN, NAN])),
        "nothing fitted": _case([10, 11], [(NAN, NAN), (1.0, 2.0)], dict(position=[-1, 0], status=[NF, 0])),
        "tried == 0": _case([10, 11], [(1.0, 2.0), (1.0, 2.0)], dict(position=[-1, 0], status=[NC | NF, 0], tried=[0, 3]),
                            held=(0, 3)),
        "a pid mask that leaves one candidate": _case([10, 11], [(1.0, 2.0), (1.0, 2.0)],
                                                      dict(position=[1, 0], status=[0, 0], tried=[2, 3], f_next=[NAN, 2.0]),
                                                      held=(2, 7)),
        "candidates leave one species": _case([10, 11, 10], [(1.0, 2.0), (1.0, 2.0), (1.0, 2.0)],
                                              dict(position=[1, -1, -1], status=[0, T, T], tried=[2, 2, 2]), candidates=2),
        # a record with NO_START is not fitted even if its f is a number
        "NO_START beside a finite f": _case([10, 11], [(1.0, 2.0), (3.0, 4.0)], dict(position=[1, 0], status=[0, 0], fitted=[2, 3]),
                                            status=((FIT_NO_START, 0), (0, 0))),
        "the best is taken, an equal and a worse are free": _case(
            [10, 10, 11], [(1.0, 9.0), (1.0, 9.0), (1.0, 9.0)], dict(position=[0, 1, 2], status=[0, 0, D], f_next=[9.0, 9.0, 1.0])),
    }


def walk_arrays(case: WalkCase):
    """(layout, tried [1, n_sim], fits [1, n_sim, H], estimates [1, n_sim], pid [1, n_sim] or None) of a walk case."""
    layout = href.Layout(case.species)
    n_sim = len(case.species)
    fits = np.zeros((1, n_sim, layout.n), dtype=FIT_DTYPE)
    fits["f"][0], fits["status"][0] = np.array(case.f), np.array(case.status)
    fits["n_points"], fits["ke"] = 7, np.arange(n_sim * layout.n).reshape(1, n_sim, layout.n)  # (which record was copied)
    estimates = np.zeros((1, n_sim), dtype=ESTIMATE_DTYPE)
    estimates["n_used"] = 7
    pid = None
    if case.held is not None:
        pid = np.zeros((1, n_sim), dtype=pref.PID_DTYPE)
        pid["held"][0] = case.held
    return layout, href.tried(layout, 1, case.candidates, pid), fits, estimates, pid


def check_walk_cases() -> None:
    """The restatement gives what every case says by hand, and the set holds every status bit."""
    seen = 0
    for name, case in walk_cases().items():
        layout, tried, fits, estimates, _ = walk_arrays(case)
        records, chosen = href.walk(fits, tried, layout, estimates)
        for field, want in case.want.items():
            got = records[field][0]
            assert href.same_f64(got, want) if field == "f_next" else got.tolist() == list(want), (name, field, got, want)
        for k, position in enumerate(records["position"][0]):
            if position >= 0:
                assert chosen["ke"][0, k] == fits["ke"][0, k, layout.of_position[position]], name
            else:
                assert chosen["status"][0, k] == href.FIT_NO_PID and chosen["n_points"][0, k] == 7 and np.isnan(chosen["f"][0, k]), name
        seen |= int(np.bitwise_or.reduce(records["status"][0]))
    assert seen == NC | NF | T | D
