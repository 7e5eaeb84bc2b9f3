"""Hand-made tracks for the track fit, shared by tests/test_fit_cpu.py (the host C++ against the restatement) and
tests/test_gpu_fit.py (the device against the restatement).  The tracks are made by the restatement's own integrator
(tests/fit_reference.py) at known parameters in the detector of the be10dp workload (protons and 11Be), sampled in z
and quantised to 1/16 mm, so the truth of every track is known: ``Case.truth`` beside its rows."""
import numpy as np

from tests import estimate_reference as est
from tests import fit_reference as ref
from tests.helpers import Inputs

INDICES8 = [2, 5, 3, 6, 7, 9, 11, 4]       # n_sim = 8: the eight track slots of a wave
SPECIES8 = [0, 1, 1, 0, 0, 1, 0, 1]        # the species of every position: 0 = proton, 1 = 11Be
INDICES_TWICE = [2, 5, 3, 2, 7, 9, 11, 4]  # label 2 is given twice; row 4 has no species here
BEAM_REGION = 10.0                          # mm: the first rows of a track from the axis are not used
MIN_POINTS = 3
# (time_step 4e-10 s: a track of these takes 20 .. 130 steps; the longest, the 11Be that stops, runs into max_steps)
SETTINGS = dict(time_step=4e-10, max_steps=100, max_evaluations=8, tolerance_momentum=1e-3, tolerance_position=1e-3)
LONG = ref.Settings(time_step=4e-10, max_steps=2000)


def layout(indices=INDICES8, species=SPECIES8, without=()):
    from attpc_engine_amd import _abi

    lay = _abi.EventLayout()
    lay.n_rows, lay.n_sim = _abi.MAX_ROWS, len(indices)
    for row in range(_abi.MAX_ROWS):
        lay.species_of_row[row] = -1
    for s, row in enumerate(indices):
        lay.indices[s] = row
        if row not in without:
            lay.species_of_row[row] = species[s]
    return lay


def model(lay=None):
    return ref.Model(Inputs("be10dp").det, lay or layout())


def momentum(sp, kinetic, polar, azimuth):
    g = np.sqrt((1.0 + kinetic / float(sp.mass)) ** 2 - 1.0)
    return [g * np.sin(polar) * np.cos(azimuth), g * np.sin(polar) * np.sin(azimuth), g * np.cos(polar)]


class Case:
    """One track: ``rows`` [n, 8] in ascending z, its ``truth`` q [6] and how the true track ended."""

    def __init__(self, sp, kinetic, polar, azimuth, vertex, n, span=(0.02, 0.98), length=1.0, same_z=False, unused=2):
        self.truth = np.array(momentum(sp, kinetic, polar, azimuth) + list(vertex), dtype=np.float64)
        samples, self.end = ref.trajectory(sp, self.truth, length, LONG)
        z = samples[:, 2]
        keep = len(z)
        turn = np.flatnonzero(np.diff(z) * np.sign(z[1] - z[0]) <= 0.0)
        if len(turn):
            keep = turn[0] + 1  # the monotone part
        order = slice(None) if z[1] > z[0] else slice(None, None, -1)
        zs, xs, ys = z[:keep][order], samples[:keep, 0][order], samples[:keep, 1][order]
        lo, hi = (zs[0] + f * (zs[-1] - zs[0]) for f in span)
        # a dense grid along the track, quantised; n of its USED points, evenly, and the first unused ones in front
        dense = np.linspace(lo, hi, 8 * n + 64)
        units = np.rint(16000.0 * np.stack([np.interp(dense, zs, xs), np.interp(dense, zs, ys), dense], axis=1))
        rb = np.rint(16.0 * BEAM_REGION)
        used = np.flatnonzero(units[:, 0] ** 2 + units[:, 1] ** 2 >= rb * rb)
        take = used[np.rint(np.linspace(0, len(used) - 1, n)).astype(np.int64)]
        assert len(np.unique(take)) == n
        units = np.concatenate([units[np.flatnonzero(units[:, 0] ** 2 + units[:, 1] ** 2 < rb * rb)[:unused]], units[take]])
        if same_z:  # neighbours share their z
            units[1::2, 2] = units[0:-1:2, 2][:len(units[1::2])]
        units = units[np.argsort(units[:, 2], kind="stable")]
        self.rows = est.spyral_rows(units[:, 0], units[:, 1], units[:, 2])
        self.steps = len(samples) - 1


def event(tracks):
    """[(Case or rows, label)] -> (rows, labels) in ascending z."""
    rows = np.concatenate([getattr(t, "rows", t) for t, _ in tracks]) if tracks else np.zeros((0, 8))
    labels = np.concatenate([np.full(len(getattr(t, "rows", t)), label, dtype=np.int64) for t, label in tracks]) if tracks else np.zeros(0, dtype=np.int64)
    order = np.argsort(rows[:, 2], kind="stable")
    return rows[order], labels[order]


def hand_cases(m=None):
    """name -> [(Case, label)]: the events.  Every label of ``INDICES8`` has its species (``SPECIES8``)."""
    m = m or model()
    p, be = m.species
    v = (0.002, -0.001, 0.4)
    eight = [
        (Case(p, 3.0, 0.6, 0.3, v, 3), 2),                         # forward, leaves through the end
        (Case(be, 40.0, 1.0, 1.3, v, 7), 5),                       # leaves through the wall
        (Case(be, 15.0, 0.8, 2.0, v, 8, span=(0.02, 1.0)), 3),     # stops inside (the true track takes more than max_steps)
        (Case(p, 3.0, 2.4, 4.0, v, 9), 6),                         # backward, leaves through z = 0
        (Case(p, 20.0, 1.2, 5.0, v, 63), 7),                       # leaves through the wall
        (Case(be, 5.0, 1.9, 0.1, v, 64, span=(0.02, 1.0)), 9),     # backward, stops inside: the range constrains it
        (Case(p, 1.0, 1.0, 2.5, v, 65, span=(0.02, 1.0)), 11),     # forward, stops inside
        (Case(be, 30.0, 2.0, 3.0, (0.0, 0.003, 0.7), 129), 4),     # backward
    ]
    return {
        "eight": eight,
        # one track alone, every other label is empty; its first points are at the vertex, which lies off the axis
        "single": [(Case(p, 0.3, 1.0, 0.7, (0.03, 0.0, 0.4), 40, span=(0.0, 1.0)), 7)],
        "capped": [(Case(p, 3.0, 0.5, 1.0, v, 2049), 11)],
        "same z": [(Case(p, 2.0, 1.45, 0.2, v, 31, same_z=True), 6), (Case(be, 20.0, 1.2, 3.3, v, 2), 5)],  # and a FEW
        "collinear": [(est.spyral_rows(480 + 9 * np.arange(45), 12 * np.arange(45), 300 + 21 * np.arange(45)), 9)],  # no circle: no start
        "empty": [],
    }


def csr(events):
    events = [event(tracks) for tracks in (events.values() if isinstance(events, dict) else events)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in events])])
    return offsets, np.concatenate([r for r, _ in events]), np.concatenate([l for _, l in events])


def starts(events, indices=INDICES8, scale=1.0):
    """start [n_events, n_sim, 6]: the truth of every track, perturbed by ``scale`` x (0.5 % of the momentum, in a
    fixed pattern, and 0.3 mm of the vertex); NaN where there is no track."""
    out = np.full((len(events), len(indices), 6), np.nan)
    for e, tracks in enumerate(events.values()):
        for case, label in tracks:
            if not isinstance(case, Case):
                continue
            s = list(indices).index(label)
            sign = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0]) * (1.0 if (e + s) % 2 else -1.0)
            out[e, s] = case.truth + scale * sign * np.concatenate([0.005 * np.abs(case.truth[:3]) + 1e-5, np.full(3, 3e-4)])
    return out


def special_starts(events):
    """The starts of the failure cases: a NaN, a vertex past the first points (near side), all points behind the
    vertex (singular) -- on the tracks of the event "eight"."""
    start = starts(events)
    e = list(events).index("eight")
    start[e, 0, 1] = np.nan                      # NO_START
    start[e, 4, 5] += 0.02                       # the first points lie on the near side of the vertex
    start[e, 7, 5] = 0.05                        # a backward track that starts below all of its points: J of g vanishes
    return start


def truths(events, indices=INDICES8):
    out = np.full((len(events), len(indices), 6), np.nan)
    for e, tracks in enumerate(events.values()):
        for case, label in tracks:
            if isinstance(case, Case):
                out[e, list(indices).index(label)] = case.truth
    return out
