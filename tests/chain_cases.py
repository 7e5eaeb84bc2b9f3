"""The combinations of opt-in stages that tests/test_gpu_chain.py runs on the device and tests/test_chain_cpu.py checks
without one, as data: the factors and their levels, which assignments are valid, the committed ``TABLE`` of cases in
which every valid pair of levels of two factors occurs, the seeded greedy generator that made it (``generate``: the
table's first generation of 12 factors, ``generate_base``, extended to the 16 without changing a column of it), and the
one set of stage settings every case draws from (``settings``).  The table is a literal so that a reader sees what runs;
tests/test_chain_cpu.py recomputes its pair coverage from the rows and does not trust the generator."""
from __future__ import annotations

import itertools
from typing import NamedTuple

import numpy as np

from attpc_engine_amd import _abi

# ---------------------------------------------------------------- factors and levels ----
# (the first level of every factor is its "off", the last its "most on")
FACTORS = {
    "straggling": (False, True),
    "gain": (False, True),
    "noise": (False, True),            # pad noise AND pedestals
    "common": (False, True),
    "readout": ("hit", "partial"),
    "baseline": (False, True),
    "trigger": ("off", "on", "gate"),
    "estimates": ("off", "rows", "thinned"),
    "circle": (False, True),
    "chunks": (1, 3),                  # one chunk, or chunk_events = CHUNK_EVENTS: 5 + 5 + 2 events
    "first": ("zero", "straddle"),     # first_event 0, or FIRST_STRADDLE: the middle chunk crosses 2^32
    "delivery": ("resident", "fetch"),  # fetch=False: records and checksums only
    "distortion": (False, True),       # the named map of tests/distortion_cases.py on the track samples
    "correction": (False, True),       # the same map taken back on the trace rows, the rows sorted again
    "helix": (False, True),
    "fit": (False, True),
}
NAMES = tuple(FACTORS)
N_BASE = 12  # the factors of the table's first generation: ``BASE_NAMES``, whose columns ``generate`` never changes
BASE_NAMES = NAMES[:N_BASE]


class Case(NamedTuple):
    name: str
    straggling: bool
    gain: bool
    noise: bool
    common: bool
    readout: str
    baseline: bool
    trigger: str
    estimates: str
    circle: bool
    chunks: int
    first: str
    delivery: str
    distortion: bool = False
    correction: bool = False
    helix: bool = False
    fit: bool = False
    packed: bool = False   # also run_traces(packed=True) (not a factor: the packing sees samples, whatever made them)
    n_events: int = 12     # (raised for a row only if a non-vacuity condition cannot be met at 12; none needed it)

    def levels(self) -> tuple:
        return tuple(getattr(self, f) for f in NAMES)


def valid(levels) -> bool:
    """The two rules: the circle fit, the helix slope and the track fit need the estimates; a partial readout needs a
    noise source (without one no pad of the set beyond the hit ones can cross the threshold: not a valid row of the
    table).  ``levels``: of all the factors, or of the first ``N_BASE`` (the later ones then off)."""
    a = {**dict(zip(NAMES, ALL_OFF)), **dict(zip(NAMES, levels))}
    if (a["circle"] or a["helix"] or a["fit"]) and a["estimates"] == "off":
        return False
    if a["readout"] == "partial" and not (a["noise"] or a["common"]):
        return False
    return True


RULED = ("noise", "common", "readout", "estimates", "circle", "helix", "fit")  # the factors the rules speak of


def pairs_of(levels) -> set:
    """{((factor, level), (factor, level))} of one assignment, the factors in the order of NAMES."""
    tagged = list(zip(NAMES, levels))
    return set(itertools.combinations(tagged, 2))


def valid_pairs(names=None) -> set:
    """Every pair of levels of two different factors (of ``names``: all of them) that some valid assignment holds: the
    pairs of every valid assignment of the factors the rules speak of, each of them with every level of every other
    factor, and every pair of levels of two other factors (147 456 assignments are too many to walk through;
    tests/test_chain_cpu.py counts the pairs its own way)."""
    names = NAMES if names is None else tuple(names)
    ruled = [f for f in names if f in RULED]
    free = [(f, level) for f in names if f not in RULED for level in FACTORS[f]]
    place = {f: k for k, f in enumerate(names)}
    ordered = lambda p, q: (p, q) if place[p[0]] < place[q[0]] else (q, p)  # noqa: E731
    out = {ordered(p, q) for p, q in itertools.combinations(free, 2) if p[0] != q[0]}
    for levels in itertools.product(*(FACTORS[f] for f in ruled)):
        tagged = list(zip(ruled, levels))
        if valid(tuple(dict(tagged).get(f, FACTORS[f][0]) for f in NAMES)):
            out |= {ordered(p, q) for p, q in itertools.combinations(tagged, 2)}
            out |= {ordered(p, q) for p in tagged for q in free}
    return out


ALL_OFF = tuple(v[0] for v in FACTORS.values())
ALL_ON = tuple(v[-1] for v in FACTORS.values())


def _random_rows(rows, missing, names, rng, candidates):
    """Rows of ``names`` appended until nothing is missing: each the best of ``candidates`` random valid assignments
    (most uncovered pairs; the first on a tie)."""
    pairs = lambda levels: set(itertools.combinations(zip(names, levels), 2))  # noqa: E731
    while missing:
        best, gain = None, 0
        for _ in range(candidates):
            levels = tuple(FACTORS[f][int(rng.integers(len(FACTORS[f])))] for f in names)
            if valid(levels) and len(pairs(levels) & missing) > gain:
                best, gain = levels, len(pairs(levels) & missing)
        if best is not None:
            rows.append(best)
            missing -= pairs(best)
    return rows


def generate_base(seed: int = 32, candidates: int = 400) -> list[tuple]:
    """The first generation of the table, over ``BASE_NAMES``: the all-on and the all-off assignment, then, until every
    valid pair of those factors is covered, the best of ``candidates`` random valid assignments."""
    on, off = ALL_ON[:N_BASE], ALL_OFF[:N_BASE]
    pairs = lambda levels: set(itertools.combinations(zip(BASE_NAMES, levels), 2))  # noqa: E731
    return _random_rows([on, off], valid_pairs(BASE_NAMES) - pairs(on) - pairs(off), BASE_NAMES, np.random.default_rng(seed),
                        candidates)


def generate(seed: int = 1, candidates: int = 400) -> list[tuple]:
    """The generator of the table: the rows of ``generate_base`` with their columns as they are -- the all-on row gets
    every later factor on, the all-off row every one off, every other row in turn the levels of the later factors that
    cover the most pairs still uncovered (the first of ``itertools.product`` on a tie) --, then rows over all the
    factors as in ``generate_base`` until every valid pair is covered."""
    base = generate_base()
    later = [FACTORS[f] for f in NAMES[N_BASE:]]
    rows = [base[0] + ALL_ON[N_BASE:], base[1] + ALL_OFF[N_BASE:]]
    missing = valid_pairs() - pairs_of(rows[0]) - pairs_of(rows[1])
    for old in base[2:]:
        best, gain = None, -1
        for new in itertools.product(*later):
            if valid(old + new) and len(pairs_of(old + new) & missing) > gain:
                best, gain = old + new, len(pairs_of(old + new) & missing)
        rows.append(best)
        missing -= pairs_of(best)
    return _random_rows(rows, missing, NAMES, np.random.default_rng(seed), candidates)


# ---------------------------------------------------------------- the table ----
# generate(): the first twelve columns of the first eleven rows are generate_base(seed=32), as committed with the table's
# first generation; the later factors are given by name (one not named is off); the names of the rows, the packed marks
# and the event counts added by hand
TABLE = (
    Case("all_on", True, True, True, True, "partial", True, "gate", "thinned", True, 3, "straddle", "fetch", packed=True,
         distortion=True, correction=True, helix=True, fit=True),
    Case("all_off", False, False, False, False, "hit", False, "off", "off", False, 1, "zero", "resident"),
    Case("noise_partial_trigger_rows", True, False, True, False, "partial", False, "on", "rows", False, 1, "straddle", "fetch",
         packed=True, helix=True, fit=True),
    Case("gain_common_gate_circle", False, True, False, True, "hit", False, "gate", "rows", True, 3, "zero", "resident",
         distortion=True, correction=True),
    Case("common_baseline_thinned_circle", False, False, False, True, "hit", True, "on", "thinned", True, 1, "straddle",
         "resident", fit=True),
    Case("gain_common_partial_baseline", True, True, False, True, "partial", True, "off", "off", False, 3, "zero", "resident",
         correction=True),
    Case("noise_hit_thinned_circle", True, False, True, False, "hit", False, "off", "thinned", True, 3, "zero", "fetch",
         distortion=True, helix=True),
    Case("noise_partial_baseline_gate", False, False, True, False, "partial", True, "gate", "off", False, 1, "straddle",
         "resident", distortion=True, correction=True),
    Case("gain_common_trigger", False, True, False, True, "hit", False, "on", "off", False, 1, "zero", "fetch", packed=True,
         distortion=True),
    Case("straggle_gain_baseline_rows", True, True, False, False, "hit", True, "off", "rows", False, 3, "straddle", "resident",
         helix=True, fit=True),
    Case("noise_trigger_thinned", True, False, True, False, "hit", False, "on", "thinned", False, 3, "zero", "resident",
         correction=True, fit=True),
    Case("common_gate_circle_helix", False, False, False, True, "hit", False, "gate", "rows", True, 3, "straddle", "resident",
         helix=True),
)

CASE_IDS = [c.name for c in TABLE]


def case(name: str) -> Case:
    return next(c for c in TABLE if c.name == name)


# ---------------------------------------------------------------- the workload and the settings ----
WORKLOAD, SEED = "be10dp", 29
CHUNK_EVENTS = 5
FIRST_STRADDLE = (1 << 32) - 7   # 12 events in chunks of 5: the middle chunk holds 2^32 - 2 .. 2^32 + 2
# The readout threshold, in ADC counts above the pedestal: low enough for the pad noise alone (sigma 2: a sample above 8
# is 4.5 sigma, 3.4e-6 a sample, some 200 pads of the set in 12 events) to read out a pad without charge; with the
# common-mode term on top (sigma 3.6 together) nearly every pad of the set crosses it.
TRACE_THRESHOLD = 8.0
NOISE_SIGMA, COMMON_SIGMA = 2.0, 3.0
PEAKS = dict(prominence=10.0, threshold=15.0)
ESTIMATES = {"rows": (20.0, 15), "thinned": (20.0, 10)}
THIN_STEP = 10.0
BASELINE_SCALE = 20.0
# The track fit as tests/test_gpu_fit.py runs it fused: a coarse step and few evaluations keep the restatement short.
FIT = dict(time_step=2e-9, max_steps=600, max_evaluations=6, tolerance_momentum=1e-3, tolerance_position=1e-3)
# The windowed sums of the 12 events reach 470 .. 2 200 with every hit pad read out and 0 .. 26 000 in the sector: 600
# lets 10 and 6 of them fire.
TRIGGER = dict(threshold=25, window=50, group_multiplicity=600)


def first_event(c: Case) -> int:
    return 0 if c.first == "zero" else FIRST_STRADDLE


def pedestals() -> np.ndarray:
    return np.random.default_rng(3).integers(200, 401, size=_abi.NUM_PADS).astype(np.int16)


def gain_map() -> np.ndarray:
    """1.0, with one pad in 16 dead (0) and one in 8 at 1.25."""
    g = np.ones(_abi.NUM_PADS)
    pick = np.random.default_rng(8).integers(0, 16, size=_abi.NUM_PADS)
    g[pick == 0] = 0.0
    g[(pick == 1) | (pick == 2)] = 1.25
    return g


def common_groups() -> np.ndarray:
    """Four groups, one pad in 11 without a common-mode term."""
    g = (np.arange(_abi.NUM_PADS) * 7 % 4).astype(np.uint8)
    g[5::11] = 255
    return g


def readout_pads(config) -> np.ndarray:
    """The readout set of the partial rows: the pads whose centre lies in a fixed sector of the pad plane, 120 degrees
    about -y out to the rim (the beam pads left out): 3 377 pads.  The tracks of be10dp leave the vertex in every
    direction and a thinned fit needs 10 bins of 10 mm: a smaller set leaves fewer than 4 records of status 0 in 12
    events (a 170 mm sector of 2 221 pads: 1), and this one keeps the restatement of the all-on row at 5 s."""
    from attpc_engine_amd.detector.beam_pads import BEAM_PADS_ARRAY

    centres = np.asarray(config.pad_centers, dtype=np.float64)
    r = np.hypot(centres[:, 0], centres[:, 1])
    inside = (r < READOUT_RADIUS_MM) & (centres[:, 0] * READOUT_AXIS[0] + centres[:, 1] * READOUT_AXIS[1] > READOUT_COS * r)
    inside[BEAM_PADS_ARRAY] = False
    return np.flatnonzero(inside)


READOUT_RADIUS_MM, READOUT_AXIS, READOUT_COS = 280.0, (0.0, -1.0), 0.5


def settings(c: Case, config) -> dict:
    """What ``Engine.configure_*`` takes for the case, by stage (None: the stage off) -- and what
    tests/chain_reference.py restates."""
    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.correction import CorrectionSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings
    from attpc_engine_amd.detector.fit import TrackFitSettings
    from attpc_engine_amd.detector.helix import HelixSlopeSettings
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.detector.straggling import StragglingSettings
    from attpc_engine_amd.detector.thinning import ThinSettings
    from attpc_engine_amd.detector.traces import (BaselineSettings, CommonModeSettings, GainSettings, PeakSettings,
                                                  TriggerSettings)
    from tests.distortion_cases import named_map

    traces = {"threshold": TRACE_THRESHOLD, "offset": int(np.argmax(get_response(config))), "readout": c.readout}
    if c.noise:
        traces.update(noise_sigma=NOISE_SIGMA, pedestals=pedestals())
    if c.readout == "partial":
        traces["readout_pads"] = readout_pads(config)
    return {
        "straggling": StragglingSettings(stream=3) if c.straggling else None,
        "gain": GainSettings(rel_variance=1.0, pad_gain=gain_map(), stream=1) if c.gain else None,
        "traces": traces,
        "common_mode": CommonModeSettings(sigma=COMMON_SIGMA, groups=common_groups(), stream=2) if c.common else None,
        "peaks": PeakSettings(**PEAKS),
        "baseline": BaselineSettings(BASELINE_SCALE) if c.baseline else None,
        "trigger": None if c.trigger == "off" else TriggerSettings(**TRIGGER, gate=c.trigger == "gate"),
        "estimates": None if c.estimates == "off" else EstimateSettings(*ESTIMATES[c.estimates]),
        "thinning": ThinSettings(THIN_STEP) if c.estimates == "thinned" else None,
        "circle": CircleFitSettings() if c.circle else None,
        "distortion": named_map() if c.distortion else None,
        # (the correction is run whether or not the tracks were distorted: its map need not be the tracks')
        "correction": CorrectionSettings(named_map()) if c.correction else None,
        "helix": HelixSlopeSettings() if c.helix else None,
        "fit": TrackFitSettings(**FIT) if c.fit else None,
    }
