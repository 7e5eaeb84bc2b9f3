"""Cost and yield of the track fit (attpc_trace_configure_fit): one GPU, o16aa and be10dp in partial
readout with sigma = 5, pedestals and threshold 20; estimates with ``--min-points`` points, thinning at ``--thinning``
mm, geometric circle fit and helix slope on in every leg.

Rates: per workload one engine in this process; ``run_estimates`` of ``--events`` events with the fit off and on,
alternating, ``--reps`` timed calls each behind one warm-up call of each kind.  A leg's figure is the median of its
timed calls, its spread their minimum and maximum; the stage's cost per fitted track is (1 / rate(on) - 1 / rate(off))
x events / tracks with a fit.
Yield: ``--stats-events`` events through ``run_estimates`` in calls of ``--events`` (fewer if ``--budget`` seconds run
out first; the line says how many): the share of tracks per status bit and per end of the final trial, and per position
the median and half the 16 .. 84 % range of brho / true - 1, polar - true and ke / true - 1 against the kinematics of
the same call, BEFORE (the estimate record) and AFTER (the fit record) on the tracks that have both.
Lanes: the share of the 64 lanes of a wave that integrate, estimated from the records of eight consecutive tracks (a
wave): sum over its tracks of 7 x steps x evaluations over 64 x the largest steps x evaluations among them.
Reported values for the settings used, no limits.

    python tools/fit_rate.py [--events N] [--reps K] [--stats-events M] [--budget S] [--workloads o16aa,be10dp]
                             [--time-step T] [--max-steps N] [--max-evaluations N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

PARTIAL = {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"}


def _engine(name: str, args):
    import numpy as np

    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    eng = Engine(pipeline, config, indices, context=_abi.Context(0))
    eng.configure_traces(config, offset=int(np.argmax(get_response(config))), **PARTIAL)
    eng.configure_estimates(min_points=args.min_points)
    eng.configure_thinning(z_step=args.thinning)
    eng.configure_circle_fit()
    eng.configure_helix_slope()
    return eng, pipeline, indices


def _fit(args):
    from attpc_engine_amd.detector.fit import TrackFitSettings

    return TrackFitSettings(time_step=args.time_step, max_steps=args.max_steps, max_evaluations=args.max_evaluations)


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def rates(eng, args) -> dict:
    legs = {"off": [], "on": []}
    fitted = 0

    def call(on: bool):
        eng.configure_track_fit(_fit(args) if on else None)
        t0 = time.perf_counter()
        res = eng.run_estimates(args.events, seed=1)
        return args.events / (time.perf_counter() - t0), res

    call(False), call(True)
    for _ in range(args.reps):
        for on in (False, True):
            rate, res = call(on)
            legs["on" if on else "off"].append(rate)
            if on:
                fitted = int((res["fits"]["evaluations"] > 0).sum())
    eng.configure_track_fit()
    out = {k: [_median(v), min(v), max(v)] for k, v in legs.items()}
    out["fitted_tracks_per_call"] = fitted
    out["seconds_per_fitted_track"] = (1.0 / out["on"][0] - 1.0 / out["off"][0]) * args.events / max(fitted, 1)
    return out


def _spread(values):
    import numpy as np

    values = values[np.isfinite(values)]
    if len(values) == 0:
        return [0, None, None]
    lo, mid, hi = np.percentile(values, [16.0, 50.0, 84.0])
    return [int(len(values)), float(mid), float(0.5 * (hi - lo))]


def physics(eng, pipeline, indices, args) -> dict:
    import numpy as np

    from attpc_engine_amd import nuclear_map
    from attpc_engine_amd.detector import estimate, fit

    eng.configure_track_fit(_fit(args))
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    mass = np.array([nuclear_map.get_data(int(z[i]), int(a[i])).mass for i in indices])
    charge = np.array([float(z[i]) for i in indices])
    est, fits, truth, ke_true = [], [], {"brho": [], "polar": []}, []
    t0, done = time.perf_counter(), 0
    while done < args.stats_events and (done == 0 or time.perf_counter() - t0 < args.budget):
        res = eng.run_estimates(args.events, seed=2, first_event=done)
        est.append(res["estimates"])
        fits.append(res["fits"])
        t = estimate.truth_tracks(res["p4"], indices, z)
        truth["brho"].append(t["brho"])
        truth["polar"].append(t["polar"])
        p4 = res["p4"][:, [int(i) for i in indices]]
        ke_true.append(p4[..., 3] - np.sqrt(np.maximum(p4[..., 3] ** 2 - (p4[..., :3] ** 2).sum(axis=-1), 0.0)))
        done += args.events
    eng.configure_track_fit()
    est, fits, ke_true = np.concatenate(est), np.concatenate(fits), np.concatenate(ke_true)
    truth = {k: np.concatenate(v) for k, v in truth.items()}
    out = {"events": done, "seconds": time.perf_counter() - t0, "positions": []}
    tracks = fits.size
    out["status_share"] = {name: float((fits["status"] & bit != 0).sum() / tracks) for name, bit in fit.STATUS_BITS.items()}
    out["status_share"]["clean"] = float((fits["status"] == 0).sum() / tracks)
    ran = fits["evaluations"] > 0
    out["end_share_of_fitted"] = {name: float((fits["end"][ran] == code).sum() / max(ran.sum(), 1)) for name, code in fit.ENDS.items()}
    out["evaluations_mean"] = float(fits["evaluations"][ran].mean()) if ran.any() else None
    out["steps_mean"] = float(fits["steps"][ran].mean()) if ran.any() else None
    # the lanes of a wave: eight consecutive tracks in the call's order
    work = (fits["steps"].astype(np.float64) * fits["evaluations"]).reshape(-1)
    work = work[:len(work) // 8 * 8].reshape(-1, 8)
    busy = work.max(axis=1) > 0
    out["active_lane_share"] = float((7.0 * work[busy].sum(axis=1) / (64.0 * work[busy].max(axis=1))).mean()) if busy.any() else None
    for s in range(len(indices)):
        e, f = est[:, s], fits[:, s]
        both = (f["evaluations"] > 0) & np.isfinite(e["brho"]) & np.isfinite(e["slope"]) & np.isfinite(truth["brho"][:, s])
        p_before = estimate.C_MEV_PER_TM * charge[s] * e["brho"][both]
        ke_before = np.sqrt(p_before * p_before + mass[s] * mass[s]) - mass[s]
        row = {"position": s, "row": int(indices[s]), "Z": int(charge[s]), "mass": float(mass[s]), "tracks": int(both.sum()),
               "converged": int((both & (f["status"] & (fit.FIT_NOT_CONVERGED | fit.FIT_SINGULAR) == 0)).sum()),
               "before": {"brho": _spread(e["brho"][both] / truth["brho"][both, s] - 1.0),
                          "polar": _spread(estimate.polar(e)[both] - truth["polar"][both, s]),
                          "ke": _spread(ke_before / ke_true[both, s] - 1.0)},
               "after": {"brho": _spread(f["brho"][both] / truth["brho"][both, s] - 1.0),
                         "polar": _spread(fit.polar(f)[both] - truth["polar"][both, s]),
                         "ke": _spread(f["ke"][both] / ke_true[both, s] - 1.0)}}
        out["positions"].append(row)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=100000)
    ap.add_argument("--budget", type=float, default=1.0e9)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--min-points", type=int, default=10)
    ap.add_argument("--thinning", type=float, default=5.0)
    ap.add_argument("--time-step", type=float, default=1.0e-10)
    ap.add_argument("--max-steps", type=int, default=10000)
    ap.add_argument("--max-evaluations", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.workloads.split(","):
        eng, pipeline, indices = _engine(name, args)
        settings = {k: getattr(args, k) for k in ("events", "min_points", "thinning", "time_step", "max_steps", "max_evaluations")}
        if args.reps > 0:
            lines.append({"workload": name, "kind": "rates", **settings, **rates(eng, args)})
            print(json.dumps(lines[-1]), flush=True)
        if args.stats_events > 0:
            lines.append({"workload": name, "kind": "physics", **settings, **physics(eng, pipeline, indices, args)})
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        Path(args.out).write_text("".join(json.dumps(line) + "\n" for line in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
