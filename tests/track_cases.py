"""Single tracks that end in every way ``track_kernel`` (csrc/tracks.hip) can end a track, defined once:
tests/test_track_cases_cpu.py checks on the CPU oracle alone that every case ends the way its entry says, and
tests/test_gpu_track_paths.py runs the same entries on the device.

A case is one nucleus of a 10Be(d,p)11Be event (``workloads.be10dp``: row 2 the proton, row 3 the 11Be) with its
momentum and vertex written down, on one of the detector descriptions of ``DETECTORS``.  The other nucleus of the event
is ``COMPANION``, an ordinary short track.  ``expected`` = (ODE rows, the terminal event that ended the track, where):

* rows   ``n_steps`` as the oracle gives it, a literal: a case that drifts shows up as a failing CPU test
* event  "ke" | "z_forward" | "z_backward" | "rho" (solver.py:80-240), or "none": the track is alive at the last of the
         10001 samples
* where  "first": the event fires in the first step (one row, the vertex);  "middle";  "last": row 10001 is recorded

The four event functions are tested like scipy tests them: an event with direction -1 fires where ``g_old >= 0 and
g_new <= 0``, one with direction +1 where ``g_old <= 0 and g_new >= 0``.  The ``*_on_*`` cases start with g exactly 0
at the vertex, once moving in the stopping direction (the first step fires: one row) and once in the other (it does
not).  The oracle's cage test is ``sqrt(x^2 + y^2) - 0.292``, the device's ``x^2 + y^2 - 0.292^2``; both are exactly
0 at (0.292, 0, z), which is the vertex used (a point within a rounding error of the circle at another azimuth may
legitimately differ and is not a case).

The path-length cases: recording in that mode ends with the 1 us window (``t + h > 1e-6 (1 + 1e-9)``) or with the cap of
10000 steps.  A step is never longer than the 1e-10 s of the reference grid, so 9999 steps reach 0.9999 us at the most
and the 10000th ends at 1 us or before: the window test cannot fire before the cap does, in the oracle or on the device
(tests/test_track_cases_cpu.py::test_path_window_cannot_end_a_track_before_the_cap).  ``path_window`` is therefore the
track that the cap ends exactly AT the end of the window (every step 1e-10 s, accumulated time 1 us), ``path_cap`` the one
it ends before (steps of 1 mm, about a third of the window); both have 10001 rows.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from attpc_engine_amd import GasTarget, nuclear_map, workloads

SEED = 5
KE_LIMIT = 1.0e-6   # MeV, solver.py:14
RHO_MAX = 0.292     # m, the field cage
TIME_SAMPLES = 10001
H_GRID = 1.0e-10    # s
C_LIGHT = 299792458.0
ROW = {"p": 2, "be11": 3}
MASS = {"p": nuclear_map.get_data(1, 1).mass, "be11": nuclear_map.get_data(4, 11).mass}

# name -> what differs from workloads.be10dp's detector (D2 at 600 Torr, 45 kV/m): gas pressure [Torr], electric field
# [V/m], path_step [m]
DETECTORS = {
    "default": {},
    # thin gas and a weak field: a 6 MeV proton at 90 degrees circles inside the cage for the whole microsecond, drifts
    # 2 cm along z and still loses 170 eV and more per sample (>= 5 primary electrons: every sample is kept)
    "thin": {"pressure": 60.0, "efield": 500.0},
    "thin_path_window": {"pressure": 60.0, "efield": 500.0, "path_step": 5.0e-3},  # 5 mm / v > 1e-10 s: the time grid
    "path_cap": {"pressure": 100.0, "efield": 500.0, "path_step": 1.0e-3},
}


def builder(pressure: float = 600.0, efield: float | None = None, **_):
    """A workload builder (tests.helpers.Inputs takes one): be10dp with another gas pressure / electric field."""
    def build(**kw):
        pipeline, config, indices = workloads.be10dp(**kw)
        if pressure != 600.0:
            config.det_params.gas_target = GasTarget([(1, 2, 2)], pressure, nuclear_map)
        if efield is not None:
            config.det_params.efield = efield
        return pipeline, config, indices
    return build


_INPUTS: dict = {}


def inputs(detector: str):
    """``tests.helpers.Inputs`` of a ``DETECTORS`` entry (built once per process)."""
    from tests.helpers import Inputs
    if detector not in _INPUTS:
        d = DETECTORS[detector]
        kw = {"path_step": d["path_step"]} if "path_step" in d else {}
        _INPUTS[detector] = Inputs(builder(**d), **kw)
    return _INPUTS[detector]


def momentum(mass: float, ke: float, polar: float, azimuth: float) -> list:
    p = math.sqrt(ke * (ke + 2.0 * mass))
    return [p * math.sin(polar) * math.cos(azimuth), p * math.sin(polar) * math.sin(azimuth), p * math.cos(polar), ke + mass]


def kinetic_energy(gv, mass: float):
    """solver.py:116-119 as the oracle computes it, every operation rounded (``gv``: gamma beta, [..., 3])."""
    g = np.sqrt((np.asarray(gv, dtype=np.float64) ** 2).sum(axis=-1))
    beta = np.sqrt(g * g / (1.0 + g * g))
    return mass * (g / beta - 1.0)


def pz_near_kinetic_energy(mass: float, ke: float, side: int) -> float:
    """A momentum along z whose ``kinetic_energy`` is the smallest one >= ``ke`` (``side`` > 0) or the largest one
    < ``ke`` (``side`` < 0) that a momentum gives.  KE = m (gamma - 1) comes on a grid of m 2^-52 = 2e-13 MeV, a thousand
    times coarser than the doubles near 4 MeV, so a node of the dE/dx table is hit exactly by no momentum of this mass;
    these are its two neighbours (the doubles within 4000 ulp of the analytic momentum are tried)."""
    p = math.sqrt(ke * (ke + 2.0 * mass))
    cands = np.array([p + k * math.ulp(p) for k in range(-4000, 4001)])
    gv = np.zeros((len(cands), 3))
    gv[:, 2] = cands / mass
    got = kinetic_energy(gv, mass)
    ok = got >= ke if side > 0 else got < ke
    best = got[ok].min() if side > 0 else got[ok].max()
    return float(cands[ok & (got == best)][0])


@dataclass
class TrackCase:
    name: str
    species: str            # "p" or "be11"
    ke: float               # MeV at the vertex
    polar: float
    azimuth: float
    vertex: tuple
    expected: tuple         # (n_steps, terminal event, "first" | "middle" | "last")
    detector: str = "default"
    node_side: int = 0      # != 0: the momentum is along z and chosen by pz_near_kinetic_energy(mass, ke, node_side)
    note: str = field(default="", compare=False)

    @property
    def row(self) -> int:
        return ROW[self.species]

    def p4(self) -> list:
        mass = MASS[self.species]
        if self.node_side:
            return [0.0, 0.0, pz_near_kinetic_energy(mass, self.ke, self.node_side), self.ke + mass]
        return momentum(mass, self.ke, self.polar, self.azimuth)


HALF_PI = math.pi / 2.0
# the nucleus beside the case's: short, ordinary, far from every limit
COMPANION = {"p": ("be11", 40.0, 0.1, 0.0), "be11": ("p", 0.3, 0.4, 1.0)}

CASES = [
    TrackCase("full_window", "p", 6.0, HALF_PI, 0.0, (0.0, 0.0, 0.5), (10001, "none", "last"), "thin",
              note="10000 kept samples: the 79th entry of the block table is written"),
    # each terminal event alone, after more than one wave's worth of rows
    TrackCase("ranges_out", "p", 0.5, 0.3, 2.0, (0.001, 0.002, 0.2), (121, "ke", "middle")),
    TrackCase("leaves_forward", "p", 2.0, 0.1, 0.0, (0.0, 0.0, 0.7), (177, "z_forward", "middle")),
    TrackCase("leaves_backward", "p", 2.0, math.pi - 0.1, 0.0, (0.0, 0.0, 0.3), (176, "z_backward", "middle")),
    TrackCase("leaves_cage", "p", 12.0, HALF_PI, 0.0, (0.0, 0.0, 0.5), (73, "rho", "middle")),
    # an event function exactly 0 at the vertex: in the stopping direction and in the other one
    TrackCase("on_window_forward", "p", 2.0, 0.1, 0.0, (0.0, 0.0, 1.0), (1, "z_forward", "first")),
    TrackCase("on_window_backward", "p", 2.0, math.pi - 0.1, 0.0, (0.0, 0.0, 1.0), (392, "ke", "middle")),
    TrackCase("on_cathode_backward", "p", 2.0, math.pi - 0.1, 0.0, (0.0, 0.0, 0.0), (1, "z_backward", "first")),
    TrackCase("on_cathode_forward", "p", 2.0, 0.1, 0.0, (0.0, 0.0, 0.0), (384, "ke", "middle")),
    TrackCase("on_cage_outward", "p", 2.0, HALF_PI, 0.0, (RHO_MAX, 0.0, 0.5), (1, "rho", "first")),
    TrackCase("on_cage_inward", "p", 2.0, HALF_PI, math.pi, (RHO_MAX, 0.0, 0.5), (102, "rho", "middle")),
    TrackCase("hair_above_ke_limit", "p", 1.01e-6, 0.3, 0.0, (0.0, 0.0, 0.5), (1, "ke", "first"),
              note="1 % above: KE = m (gamma - 1) at gamma - 1 = 1e-12 carries a relative error of 2e-4 in any arithmetic"),
    # the ends of the dE/dx table
    TrackCase("dedx_last_node", "be11", 20000.0, 0.05, 0.0, (0.0, 0.0, 0.2), (29, "z_forward", "middle"),
              note="KE >= 2^14 MeV on every row: the last node"),
    TrackCase("dedx_above_node_4mev", "p", 4.0, 0.0, 0.0, (0.0, 0.0, 0.2), (319, "z_forward", "middle"), node_side=+1),
    TrackCase("dedx_below_node_4mev", "p", 4.0, 0.0, 0.0, (0.0, 0.0, 0.2), (319, "z_forward", "middle"), node_side=-1),
    TrackCase("dedx_above_node_1kev", "p", 2.0 ** -10, 0.0, 0.0, (0.0, 0.0, 0.2), (17, "ke", "middle"), node_side=+1),
    # path-length sampling (see the module docstring)
    TrackCase("path_window", "p", 6.0, HALF_PI, 0.0, (0.0, 0.0, 0.5), (10001, "none", "last"), "thin_path_window"),
    TrackCase("path_cap", "p", 6.0, HALF_PI, 0.0, (0.0, 0.0, 0.5), (10001, "none", "last"), "path_cap"),
]
CASE_IDS = [c.name for c in CASES]
LONG_CASES = ("full_window", "path_window", "path_cap")  # more than 2000 rows: their own position tolerance

# ode_substeps > 1: workload, substeps, path_step, events (from SUBSTEP_FIRST at SUBSTEP_SEED)
SUBSTEP_SEED, SUBSTEP_FIRST = 21, 1000
SUBSTEP_RUNS = [("o16aa", 2, 0.0, 40), ("o16aa", 4, 0.0, 40), ("be10dp", 2, 0.0, 40), ("be10dp", 4, 0.0, 40),
                ("be10dp", 2, 2.5e-4, 8)]

# one workgroup for several hundred tracks: workload, seed, first event (one past 2^32), events.  704 tracks are 5.5
# batches of 128 ids for the 4 waves, and their arena blocks more than twice the 4 x 64 of the waves' first pools
REFILL_RUNS = [("be10dp", 21, 1000, 352), ("o16aa", 22, (1 << 32) + 5, 352)]
REFILL_MIN_BLOCKS = 512

# a fused run in which a share of the events hits event_sample_limit = 1 (tests/test_gpu_parity.py::
# test_kin_sample_limit_and_samplers' reaction: most of ExcitationUniform(0, 60) is forbidden at 24 MeV)
LIMIT_SEED, LIMIT_FIRST, LIMIT_EVENTS, LIMIT_CHUNK = 9, 0, 200, 64


def sample_limit_workload(seed: int = LIMIT_SEED, **kw):
    """10B(3He,a)9B at 24 MeV in He at 600 Torr with a uniform excitation of 0..60 MeV and one attempt per event."""
    from attpc_engine_amd.detector.simulator import default_indices
    from attpc_engine_amd.kinematics import (ExcitationUniform, KinematicsPipeline, KinematicsTargetMaterial, PolarUniform,
                                             Reaction)
    nm = nuclear_map
    gas = GasTarget([(2, 4, 1)], 600.0, nm)
    rxn = Reaction(nm.get_data(5, 10), nm.get_data(2, 3), nm.get_data(2, 4))
    pipeline = KinematicsPipeline([rxn], [ExcitationUniform(0.0, 60.0)], [PolarUniform(0.0, math.pi)], 24.0,
                                  target_material=KinematicsTargetMaterial(gas, (0.0, 1.0), 0.007), event_sample_limit=1,
                                  seed=seed, **kw)
    return pipeline, workloads.detector_config(gas), default_indices(4)


def case(name: str) -> TrackCase:
    return next(c for c in CASES if c.name == name)


def events_of(detector: str):
    """The cases of one detector description as one launch -> (cases, p4 [n, 4, 4], vertex [n, 3])."""
    cases = [c for c in CASES if c.detector == detector]
    p4 = np.zeros((len(cases), 4, 4))
    vertex = np.zeros((len(cases), 3))
    for e, c in enumerate(cases):
        other, ke, polar, azimuth = COMPANION[c.species]
        p4[e, c.row] = c.p4()
        p4[e, ROW[other]] = momentum(MASS[other], ke, polar, azimuth)
        vertex[e] = c.vertex
    return cases, p4, vertex


# ---------------------------------------------------------------------------- one more step of the oracle ----
def event_functions(state, mass: float):
    """(g_ke, g_z_forward, g_z_backward, g_rho) of a state (x, y, z, gamma beta), as the oracle computes them."""
    return (float(kinetic_energy(state[3:6], mass)) - KE_LIMIT, state[2] - 1.0, state[2],
            math.sqrt(state[0] * state[0] + state[1] * state[1]) - RHO_MAX)


EVENT_NAMES = ("ke", "z_forward", "z_backward", "rho")
_DIRECTION = (-1, +1, -1, +1)


def fired(g_old, g_new) -> list:
    """Names of the terminal events scipy's sign-change test finds between two sets of event functions."""
    out = []
    for name, direction, a, b in zip(EVENT_NAMES, _DIRECTION, g_old, g_new):
        if (direction < 0 and a >= 0.0 and b <= 0.0) or (direction > 0 and a <= 0.0 and b >= 0.0):
            out.append(name)
    return out


def next_sample(orc, det, species_index: int, state, g_old=None):
    """The oracle's next sample after ``state`` (classical RK4 on the oracle's own right-hand side, ``ode_substeps``
    substeps, the step of the path-length mode where it is on) -> (state, events fired, substep in which they fired or
    -1, step [s]).  ``g_old``: the event functions carried over from the step before (default: those of ``state``)."""
    import ctypes as C
    L = orc.lib()
    dp = C.POINTER(C.c_double)
    L.orc_equation_of_motion.argtypes = [dp, C.c_double, C.c_double, C.c_void_p, C.c_void_p, dp]
    L.orc_equation_of_motion.restype = None
    sp = det.species[species_index]
    mass = float(sp.mass)
    nsub = max(1, int(det.ode_substeps))
    s = np.array(state, dtype=np.float64)
    h_sample = H_GRID
    if det.path_step > 0.0:
        gv2 = float((s[3:6] ** 2).sum())
        h_sample = min(det.path_step / (C_LIGHT * math.sqrt(gv2 / (1.0 + gv2))), H_GRID)
    h = h_sample / nsub
    g = event_functions(s, mass) if g_old is None else g_old

    def rhs(y):
        r = np.empty(6)
        L.orc_equation_of_motion(y.ctypes.data_as(dp), -det.bfield, -det.efield, C.byref(det), C.byref(sp), r.ctypes.data_as(dp))
        return r

    for sub in range(nsub):
        k1 = rhs(s)
        k2 = rhs(s + 0.5 * h * k1)
        k3 = rhs(s + 0.5 * h * k2)
        k4 = rhs(s + h * k3)
        s = s + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        g_new = event_functions(s, mass)
        events = fired(g, g_new)
        if events or not g_new[0] == g_new[0]:
            return s, events, sub, h_sample
        g = g_new
    return s, [], -1, h_sample
