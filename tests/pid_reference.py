"""The particle identification restated in numpy (include/attpc_engine.h, "particle identification"): the inside test
with its written edge rule, the assignment walk, the records, and the track fit behind them (``fit_with_pid``, composed
of tests/fit_reference.py's per-track functions).  Every operation of the edge rule is one f64 rounding in numpy as on
the device, so every comparison against this file is exact.  ``mutant=`` names one deliberate mistake; each of them must
fail the comparison on the case set (tests/pid_cases.py)."""
import numpy as np

from tests import fit_reference as fref

MAX_SIM, MAX_VERTICES = 8, 32
ANY, OWN = 0, 1
NO_ESTIMATE, NONE, TAKEN, AMBIGUOUS = 1, 2, 4, 8
FIT_NO_PID = 256
PID_DTYPE = np.dtype([("position", "<i4"), ("species", "<i4"), ("held", "<i4"), ("status", "<i4")])
MUTANTS = ("side_not_strict", "d_zero_counts", "no_closing_edge", "highest_free", "taken_ignored", "own_is_any",
           "swapped_axes", "zero_accepted")


def desc_error(gates, mode, reserved=0):
    """What is wrong with the gates ([8] of None or arrays [n, 2]) and the mode, or None."""
    if mode not in (ANY, OWN):
        return "mode"
    if reserved != 0:
        return "reserved"
    for gate in gates:
        if gate is None:
            continue
        v = np.asarray(gate, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 2 or not 3 <= len(v) <= MAX_VERTICES:
            return "n_vertices"
        if not np.isfinite(v).all():
            return "vertices"
    return None


def testable(x, y, mutant=None):
    """The points that are tested at all: both coordinates finite and > 0."""
    with np.errstate(invalid="ignore"):
        if mutant == "zero_accepted":
            return np.isfinite(x) & np.isfinite(y)
        return np.isfinite(x) & np.isfinite(y) & (x > 0.0) & (y > 0.0)


def inside(vertices, x, y, mutant=None):
    """The crossing number of the polygon ``vertices`` [n, 2] for the points (x, y), arrays of one shape -> bool."""
    v = np.asarray(vertices, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    odd = np.zeros(x.shape, dtype=bool)
    edges = len(v) - 1 if mutant == "no_closing_edge" else len(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(edges):
            (x0, y0), (x1, y1) = v[i], v[(i + 1) % len(v)]
            if mutant == "side_not_strict":
                straddles = (y0 >= y) != (y1 >= y)
            else:
                straddles = (y0 > y) != (y1 > y)
            d = (x1 - x0) * (y - y0) - (x - x0) * (y1 - y0)
            if mutant == "d_zero_counts":
                counts = straddles & ((d >= 0.0) == (y1 > y0))
            else:
                counts = straddles & (d != 0.0) & ((d > 0.0) == (y1 > y0))
            odd ^= counts
    return odd


def records(estimates, gates, mode, species=None, mutant=None):
    """Records [n, n_sim] (PID_DTYPE) of the estimate records [n, n_sim] (anything with "brho" and "dedx"); ``gates`` [8]
    of None or vertex arrays, ``species`` [n_sim] the detector species of every position (None: -1 throughout)."""
    x = np.asarray(estimates["brho"], dtype=np.float64)
    y = np.asarray(estimates["dedx"], dtype=np.float64)
    if mutant == "swapped_axes":
        x, y = y, x
    n, n_sim = x.shape
    ok = testable(x, y, mutant)
    held = np.zeros((n, n_sim), dtype=np.int64)
    for p in range(n_sim):
        if gates[p] is None:
            continue
        holds = inside(gates[p], x, y, mutant) & ok  # [n, n_sim]: slot k against gate p
        if mode == OWN and mutant != "own_is_any":
            holds = holds & (np.arange(n_sim)[None, :] == p)
        held |= holds.astype(np.int64) << p
    out = np.zeros((n, n_sim), dtype=PID_DTYPE)
    out["position"], out["species"] = -1, -1
    taken = np.zeros(n, dtype=np.int64)
    for k in range(n_sim):
        mask = held[:, k]
        free = mask if mutant == "taken_ignored" else mask & ~taken
        position = np.full(n, -1, dtype=np.int64)
        for p in (range(n_sim) if mutant == "highest_free" else range(n_sim - 1, -1, -1)):
            position = np.where((free >> p) & 1 == 1, p, position)  # (the last p written wins: the lowest, or the highest)
        got = position >= 0
        taken |= np.where(got, 1 << np.maximum(position, 0), 0)
        many = (mask & (mask - 1)) != 0
        status = np.where(~ok[:, k], NO_ESTIMATE,
                          np.where(mask == 0, NONE, np.where(got, 0, TAKEN) | np.where(many, AMBIGUOUS, 0)))
        out["held"][:, k] = np.where(ok[:, k], mask, 0)
        out["status"][:, k] = status
        out["position"][:, k] = np.where(ok[:, k], position, -1)
        if species is not None:
            table = np.asarray(list(species) + [-1], dtype=np.int64)
            out["species"][:, k] = table[np.where(ok[:, k], position, -1)]
    return out


def same(got, want) -> bool:
    return got.shape == want.shape and all(np.array_equal(got[name], want[name]) for name in PID_DTYPE.names)


def fit_with_pid(offsets, rows, labels, indices, model, estimates, pid, settings, beam_region_radius):
    """``fit_reference.records`` behind the identification: slot k is fitted as the nucleus of position
    ``pid["position"][e, k]`` (its rows, its estimate record as the start), and a slot without a position gets the
    record without a fit, NO_PID."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 8)
    labels = np.asarray(labels, dtype=np.int64)
    n_events, n_sim = len(offsets) - 1, len(indices)
    out = np.zeros((n_events, n_sim), dtype=fref.FIT_DTYPE)
    todo = []
    for e in range(n_events):
        ev_rows, ev_labels = rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        for s, index in enumerate(indices):
            est, at = estimates[e, s], int(pid["position"][e, s])
            n_points = min(int(est["n_used"]), fref.FIT_MAX_POINTS)
            if at < 0 or at >= n_sim:
                out[e, s] = fref._empty_record(FIT_NO_PID, n_points)
                continue
            sp = model.position[at]
            if est["status"] & (fref.EST_EMPTY | fref.EST_FEW):
                out[e, s] = fref._empty_record(fref.FIT_EMPTY if est["status"] & fref.EST_EMPTY else fref.FIT_FEW, n_points)
                continue
            if sp is None:
                out[e, s] = fref._empty_record(fref.FIT_NO_START, n_points)
                continue
            q, ok = fref.start_from(est, sp)
            if not ok:
                out[e, s] = fref._empty_record(fref.FIT_NO_START, n_points)
                continue
            points, n_used = fref.used_points(ev_rows[ev_labels == index], beam_region_radius)
            todo.append(((e, s), sp, points, q, n_used > fref.FIT_MAX_POINTS))
    fitted = fref.fit_tracks([t[1] for t in todo], [t[2] for t in todo], [t[3] for t in todo], model.length, settings,
                             [t[4] for t in todo])
    for t, rec in zip(todo, fitted):
        out[t[0]] = rec
    return out
