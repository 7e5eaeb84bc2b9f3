"""The selection predicate of include/attpc_engine.h restated independently of ``detector.selection``: plain loops
over the records, one event and one track at a time, Python ints and floats only.

``passes(events, tracks, cuts)``: ``cuts`` is a dict with the names of ``attpc_select_desc`` without _lo / _hi mapped to
(lo, hi) pairs (None = that end open), plus "track_mask" and "min_tracks".  ``records`` builds the structured arrays
from short hand-made descriptions, ``hand_made_cases`` is a list of (description, events, tracks, cuts, expected) with
the answers written out.
"""
import math

import numpy as np

from attpc_engine_amd import _abi

U32 = (0, (1 << 32) - 1)
I64 = (-(1 << 63), (1 << 63) - 1)
F64 = (-math.inf, math.inf)
OPEN = {"n_kept": U32, "n_pads": U32, "tb_span": U32, "charge": I64, "track_n_kept": U32, "track_n_pads": U32,
        "track_n_samples": U32, "track_rho2_max": F64, "track_end_tb": F64, "track_end_rho2": F64}


def _range(cuts, name):
    lo, hi = cuts.get(name) or (None, None)
    return (OPEN[name][0] if lo is None else lo), (OPEN[name][1] if hi is None else hi)


def _holds(cuts, name, value):
    lo, hi = _range(cuts, name)
    if (lo, hi) == OPEN[name]:
        return True  # not evaluated: whatever the value is, NaN included
    return lo <= value and value <= hi  # false for NaN


def passes(events, tracks, cuts) -> np.ndarray:
    mask, min_tracks = int(cuts.get("track_mask", 0)), int(cuts.get("min_tracks", 0))
    out = []
    for e in range(len(events)):
        ev = events[e]
        span = int(ev["tb_max"]) - int(ev["tb_min"]) + 1 if int(ev["n_kept"]) > 0 else 0
        ok = (_holds(cuts, "n_kept", int(ev["n_kept"])) and _holds(cuts, "n_pads", int(ev["n_pads"]))
              and _holds(cuts, "tb_span", span) and _holds(cuts, "charge", int(ev["charge"])))
        good = 0
        for s in range(tracks.shape[1]):
            if not (mask >> s) & 1:
                continue
            t = tracks[e, s]
            x, y = float(t["end_x"]), float(t["end_y"])
            xx = x * x
            yy = y * y
            end_rho2 = xx + yy
            if (_holds(cuts, "track_n_kept", int(t["n_kept"])) and _holds(cuts, "track_n_pads", int(t["n_pads"]))
                    and _holds(cuts, "track_n_samples", int(t["n_samples"]))
                    and _holds(cuts, "track_rho2_max", float(t["rho2_max"])) and _holds(cuts, "track_end_tb", float(t["end_tb"]))
                    and _holds(cuts, "track_end_rho2", end_rho2)):
                good += 1
        out.append(ok and good >= min_tracks)
    return np.array(out, dtype=bool)


def selection_of(cuts):
    """The ``Selection`` of a cuts dict (min_tracks explicit: the restatement's default is 0)."""
    from attpc_engine_amd.detector.selection import Selection

    cuts = dict(cuts)
    return Selection(track_mask=cuts.pop("track_mask", 0), min_tracks=cuts.pop("min_tracks", 0), **cuts)


EMPTY_TRACK = dict(n_points=0, n_kept=0, n_pads=0, tb_min=-1, tb_max=-1, charge=0, rho2_max=-1.0, n_steps=0, n_samples=0,
                   electrons=0, end_x=math.nan, end_y=math.nan, end_tb=math.nan)
EMPTY_EVENT = dict(n_points=0, n_kept=0, n_pads=0, tb_min=-1, tb_max=-1, charge=0)


def records(events, tracks):
    """events: list of dicts (fields left out: the empty record's); tracks: list (per event) of lists of dicts."""
    n, n_sim = len(events), len(tracks[0]) if tracks else 0
    ev = np.zeros(n, dtype=_abi.EVENT_SUMMARY_DTYPE)
    tr = np.zeros((n, n_sim), dtype=_abi.TRACK_SUMMARY_DTYPE)
    for e in range(n):
        for key, value in {**EMPTY_EVENT, **events[e]}.items():
            ev[e][key] = value
        for s in range(n_sim):
            for key, value in {**EMPTY_TRACK, **tracks[e][s]}.items():
                tr[e, s][key] = value
    return ev, tr


def hand_made_cases():
    nan = math.nan
    cases = []
    # a NaN end point under an absent and under a present cut (one masked position, all of them must pass)
    ev, tr = records([dict(n_kept=5, n_pads=4, tb_min=10, tb_max=12)] * 2,
                     [[dict(end_x=nan, end_y=nan, end_tb=nan)], [dict(end_x=0.3, end_y=0.4, end_tb=100.0, n_samples=7)]])
    cases.append(("NaN end, cut absent", ev, tr, dict(track_mask=1, min_tracks=1), [True, True]))
    cases.append(("NaN end, end_tb cut present", ev, tr, dict(track_mask=1, min_tracks=1, track_end_tb=(None, 500.0)), [False, True]))
    cases.append(("NaN end, end_rho2 cut present", ev, tr, dict(track_mask=1, min_tracks=1, track_end_rho2=(0.0, None)), [False, True]))
    # end_rho2 = fl(fl(0.3 * 0.3) + fl(0.4 * 0.4)), hit exactly and missed by one ulp
    r2 = 0.3 * 0.3 + 0.4 * 0.4
    cases.append(("end_rho2 hit exactly", ev, tr, dict(track_mask=1, min_tracks=1, track_end_rho2=(r2, r2)), [False, True]))
    cases.append(("end_rho2 one ulp below", ev, tr, dict(track_mask=1, min_tracks=1, track_end_rho2=(None, math.nextafter(r2, 0.0))),
                  [False, False]))
    # rho2_max = -1.0 (no kept row) compares as -1.0
    ev, tr = records([dict(n_kept=3, n_pads=3, tb_min=1, tb_max=1)] * 3,
                     [[dict(rho2_max=-1.0)], [dict(rho2_max=0.0, n_kept=1)], [dict(rho2_max=2500.0, n_kept=3)]])
    cases.append(("rho2_max -1 under [0, inf)", ev, tr, dict(track_mask=1, min_tracks=1, track_rho2_max=(0.0, None)), [False, True, True]))
    cases.append(("rho2_max -1 under (-inf, 0]", ev, tr, dict(track_mask=1, min_tracks=1, track_rho2_max=(None, 0.0)), [True, True, False]))
    cases.append(("rho2_max -1 under [-1, -1]", ev, tr, dict(track_mask=1, min_tracks=1, track_rho2_max=(-1.0, -1.0)), [True, False, False]))
    # min_tracks 0 / 1 / all over three positions of which two are masked
    ev, tr = records([dict(n_kept=9, n_pads=9, tb_min=0, tb_max=8)] * 4,
                     [[dict(n_pads=5), dict(n_pads=5), dict(n_pads=0)], [dict(n_pads=5), dict(n_pads=0), dict(n_pads=0)],
                      [dict(n_pads=0), dict(n_pads=9), dict(n_pads=5)], [dict(n_pads=0), dict(n_pads=9), dict(n_pads=0)]])
    cut = dict(track_mask=0b101, track_n_pads=(5, 5))
    cases.append(("min_tracks 0", ev, tr, dict(cut, min_tracks=0), [True, True, True, True]))
    cases.append(("min_tracks 1 (any)", ev, tr, dict(cut, min_tracks=1), [True, True, True, False]))
    cases.append(("min_tracks 2 (all)", ev, tr, dict(cut, min_tracks=2), [False, False, False, False]))
    cases.append(("min_tracks all, position 0 and 1", ev, tr, dict(track_mask=0b011, min_tracks=2, track_n_pads=(5, 9)),
                  [True, False, False, False]))
    # an empty mask: the track cuts decide nothing, whatever they say
    cases.append(("empty mask", ev, tr, dict(track_mask=0, min_tracks=0, track_n_pads=(1000, 2000)), [True] * 4))
    # bounds hit exactly, and the span of an event without a kept row
    ev, tr = records([dict(n_kept=10, n_pads=7, tb_min=100, tb_max=109, charge=5000), dict(n_kept=11, n_pads=8, tb_min=100, tb_max=110, charge=5001),
                      dict(n_kept=0, n_pads=0, tb_min=-1, tb_max=-1, charge=12), dict(n_kept=1, n_pads=1, tb_min=7, tb_max=7, charge=-3)],
                     [[{}]] * 4)
    cases.append(("n_kept [10, 10]", ev, tr, dict(n_kept=(10, 10)), [True, False, False, False]))
    cases.append(("n_pads [7, 8]", ev, tr, dict(n_pads=(7, 8)), [True, True, False, False]))
    cases.append(("span [10, 10]", ev, tr, dict(tb_span=(10, 10)), [True, False, False, False]))
    cases.append(("span [0, 0]: no kept row", ev, tr, dict(tb_span=(0, 0)), [False, False, True, False]))
    cases.append(("span [1, 1]", ev, tr, dict(tb_span=(1, 1)), [False, False, False, True]))
    cases.append(("span [1, inf)", ev, tr, dict(tb_span=(1, None)), [True, True, False, True]))
    cases.append(("charge [5001, 5001]", ev, tr, dict(charge=(5001, 5001)), [False, True, False, False]))
    cases.append(("charge (-inf, 12]", ev, tr, dict(charge=(None, 12)), [False, False, True, True]))
    cases.append(("conjunction", ev, tr, dict(n_pads=(7, None), charge=(None, 5000)), [True, False, False, False]))
    cases.append(("no cuts", ev, tr, dict(), [True] * 4))
    return cases
