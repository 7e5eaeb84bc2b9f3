"""The fit hypotheses restated in numpy (include/attpc_engine.h, "fit hypotheses"): the hypotheses of a layout, the
candidates of a slot, the fit of every (slot, hypothesis) pair -- ``tests/fit_reference.py`` once per species, which is
``pid_reference.fit_with_pid`` with every position forced to one of that species --, and the walk over the slots of an
event in plain Python.  f is only compared and copied, so every comparison against this file is exact.  ``mutant=``
names one deliberate mistake; each of them must fail the comparison on the case set (tests/hypothesis_cases.py)."""
import numpy as np

from attpc_engine_amd._abi import FIT_DTYPE, FIT_EMPTY, FIT_FEW, FIT_MAX_POINTS, FIT_NO_START
from tests import fit_reference as fref

MAX_SIM = 8
NO_CANDIDATE, NO_FIT, TAKEN, DISPLACED = 1, 2, 4, 8
FIT_NO_PID = 256
ALL = (1 << MAX_SIM) - 1
HYPOTHESIS_DTYPE = np.dtype([("position", "<i4"), ("species", "<i4"), ("tried", "<i4"), ("fitted", "<i4"), ("status", "<i4"),
                             ("reserved", "<i4"), ("f", "<f8", (MAX_SIM,)), ("f_next", "<f8")])
MUTANTS = ("tie_highest", "no_uniqueness", "not_strict", "fitted_ignores_no_start", "held_ignored")


def desc_error(candidates, reserved=0):
    """What is wrong with the settings, or None."""
    if candidates == 0 or candidates < 0 or candidates >> MAX_SIM:
        return "candidates"
    return "reserved" if reserved != 0 else None


class Layout:
    """The hypotheses of the positions whose detector species are ``species`` (-1: none): ``first[h]`` the first
    position of hypothesis h, ``of_position[p]`` the hypothesis of position p (-1: none), in the order of their first
    position."""

    def __init__(self, species):
        self.species = [int(s) for s in species]
        self.first, self.of_position = [], []
        for p, sp in enumerate(self.species):
            if sp < 0:
                self.of_position.append(-1)
                continue
            known = [h for h, q in enumerate(self.first) if self.species[q] == sp]
            if not known:
                self.first.append(p)
            self.of_position.append(known[0] if known else len(self.first) - 1)
        self.n = len(self.first)
        self.with_species = sum(1 << p for p, sp in enumerate(self.species) if sp >= 0)

    def hypothesis_species(self):
        return [self.species[p] for p in self.first]


def species_of_positions(model):
    """The detector species (the index of the model's table) of every position of a ``fit_reference.Model``."""
    return [-1 if sp is None else next(i for i, known in enumerate(model.species) if known is sp) for sp in model.position]


def tried(layout, n_events, candidates=ALL, pid=None, mutant=None):
    """[n_events, n_sim] the candidate positions of every slot."""
    n_sim = len(layout.species)
    out = np.full((n_events, n_sim), candidates & layout.with_species, dtype=np.int64)
    if pid is not None and mutant != "held_ignored":
        out &= np.asarray(pid["held"], dtype=np.int64)
    return out


class _Forced:
    """A model in which every position has the nucleus ``sp``."""

    def __init__(self, model, sp):
        self.length, self.species, self.position = model.length, model.species, [sp] * len(model.position)


def no_fit(estimates, status):
    """Records without a fit, one per estimate record."""
    out = np.zeros(estimates.shape, dtype=FIT_DTYPE)
    flat = out.reshape(-1)
    for i, est in enumerate(estimates.reshape(-1)):
        flat[i] = fref._empty_record(status, min(int(est["n_used"]), FIT_MAX_POINTS))
    return out


def all_fits(offsets, rows, labels, indices, model, estimates, settings, beam_region_radius, layout, tried_masks, start=None):
    """[n_events, n_sim, H]: ``fit_reference.records`` with every position taken for the nucleus of hypothesis h, and the
    record without a fit with NO_PID alone where no position of h is a candidate of the slot."""
    n_events, n_sim = estimates.shape
    out = np.zeros((n_events, n_sim, layout.n), dtype=FIT_DTYPE)
    none = no_fit(estimates, FIT_NO_PID)
    for h, first in enumerate(layout.first):
        positions = sum(1 << p for p in range(n_sim) if layout.of_position[p] == h)
        forced = fref.records(offsets, rows, labels, indices, _Forced(model, model.position[first]), estimates, settings,
                              beam_region_radius, start=start)
        candidate = (tried_masks & positions) != 0
        out[:, :, h] = np.where(candidate, forced, none)
    return out


def fitted_test(record, mutant=None):
    bad = FIT_EMPTY | FIT_FEW | (0 if mutant == "fitted_ignores_no_start" else FIT_NO_START)
    return not (int(record["status"]) & bad) and bool(np.isfinite(record["f"]))


def walk(fits, tried_masks, layout, estimates, mutant=None):
    """(records [n, n_sim] HYPOTHESIS_DTYPE, chosen fits [n, n_sim]) of the fit records ``fits`` [n, n_sim, H]."""
    n_events, n_sim = tried_masks.shape
    records = np.zeros((n_events, n_sim), dtype=HYPOTHESIS_DTYPE)
    chosen = no_fit(estimates, FIT_NO_PID)
    less = (lambda a, b: a <= b) if mutant == "not_strict" else (lambda a, b: a < b)
    order = range(MAX_SIM - 1, -1, -1) if mutant == "tie_highest" else range(MAX_SIM)
    for e in range(n_events):
        taken = 0
        for k in range(n_sim):
            r = records[e, k]
            r["position"], r["species"], r["tried"], r["f"], r["f_next"] = -1, -1, tried_masks[e, k], np.nan, np.nan
            best = choice = -1
            fitted = 0
            for p in order:
                if not (int(r["tried"]) >> p) & 1:
                    continue
                rec = fits[e, k, layout.of_position[p]]
                r["f"][p] = rec["f"]
                if not fitted_test(rec, mutant):
                    continue
                fitted |= 1 << p
                if best < 0 or less(rec["f"], r["f"][best]):
                    best = p
                free = mutant == "no_uniqueness" or not (taken >> p) & 1
                if free and (choice < 0 or less(rec["f"], r["f"][choice])):
                    choice = p
            r["fitted"] = fitted
            status = (NO_CANDIDATE if r["tried"] == 0 else 0) | (NO_FIT if fitted == 0 else 0)
            if fitted and choice < 0:
                status |= TAKEN
            if choice >= 0:
                taken |= 1 << choice
                r["position"], r["species"] = choice, layout.species[choice]
                if less(r["f"][best], r["f"][choice]):
                    status |= DISPLACED
                others = [r["f"][p] for p in range(MAX_SIM)
                          if (fitted >> p) & 1 and layout.of_position[p] != layout.of_position[choice]]
                if others:
                    r["f_next"] = min(others)
                chosen[e, k] = fits[e, k, layout.of_position[choice]]
            r["status"] = status
    return records, chosen


def same_f64(a, b) -> bool:
    """Bit for bit, a NaN in the same places."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def same(got, want) -> bool:
    """Every field of the hypothesis records."""
    if got.shape != want.shape:
        return False
    return all(same_f64(got[name], want[name]) if HYPOTHESIS_DTYPE[name].base.kind == "f" else np.array_equal(got[name], want[name])
               for name in HYPOTHESIS_DTYPE.names)


def assert_same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for name in HYPOTHESIS_DTYPE.names:
        if HYPOTHESIS_DTYPE[name].base.kind == "f":
            assert same_f64(got[name], want[name]), (name, got[name], want[name])
        else:
            np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def assert_same_fits(got, want):
    """Fit records of any shape, as ``fit_reference.assert_same_records``."""
    assert got.shape == want.shape, (got.shape, want.shape)
    fref.assert_same_records(np.ascontiguousarray(got).reshape(-1, 1), np.ascontiguousarray(want).reshape(-1, 1))
