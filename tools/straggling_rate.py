"""Cost of the track straggling (attpc_det_configure_straggling) and what it does to the track estimates:
one GPU, o16aa and be10dp.

Rates: per workload one engine in this process; ``run(fetch=False)`` of ``--events`` events with the stage off and on,
alternating, ``--reps`` timed calls each behind one warm-up call of each kind (buffers settle).  A leg's figure is the
median of its timed calls, its spread their minimum and maximum; beside the rate the track kernels' own time per event
(``ms_tracks`` of the run's statistics).  ``--plain-only`` times the stage-off leg alone: what a library without the
entry point (``ATTPC_HIP_LIBRARY``, a build of the parent commit) can run, to set beside the same leg of this build in
the same session, the two processes alternating.
Resolution: ``--stats-events`` events through ``run_estimates`` (``min_points`` 10, thinning at 10 mm) and through
``run_summary`` in calls of ``--events``, with the stage off and on: per track position the median and the 16 .. 84 %
half-width of brho / brho_true - 1 and of polar - polar_true, and of the end point of the track (x, y in mm, time
bucket) with the stage on minus the same event's with it off.  Reported values for the settings used, no limits.
``--profile WORKLOAD`` runs two ``run(fetch=False)`` calls with the stage on and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/straggling_rate.py --profile o16aa`` (a run of its own).

    python tools/straggling_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
                                    [--plain-only] [--angular-scale A] [--energy-scale E]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _engine(name: str):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    return Engine(pipeline, config, indices, context=_abi.Context(0))


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def _stage(eng, on: bool, args) -> None:
    if on:
        eng.configure_straggling(angular_scale=args.angular_scale, energy_scale=args.energy_scale)
    elif hasattr(eng.ctx.lib, "attpc_det_configure_straggling"):
        eng.configure_straggling()


def rates(eng, args) -> dict:
    kinds = (False,) if args.plain_only else (False, True)
    legs = {on: {"rate": [], "track_us": []} for on in kinds}

    def call(on: bool):
        _stage(eng, on, args)
        t0 = time.perf_counter()
        stats = eng.run(args.events, seed=1)["stats"]
        return args.events / (time.perf_counter() - t0), 1.0e3 * stats["ms_tracks"] / args.events

    for on in kinds:
        call(on)
    for _ in range(args.reps):
        for on in kinds:
            rate, track_us = call(on)
            legs[on]["rate"].append(rate)
            legs[on]["track_us"].append(track_us)
    _stage(eng, False, args)
    return {("on" if on else "off"): {k: [_median(v), min(v), max(v)] for k, v in leg.items()} for on, leg in legs.items()}


def resolution(eng, args) -> dict:
    import numpy as np

    from attpc_engine_amd.detector.estimate import EstimateSettings, polar, truth_tracks

    def widths(delta):
        lo, mid, hi = np.percentile(delta, [16.0, 50.0, 84.0])
        return {"median": float(mid), "half_width_16_84": float((hi - lo) / 2.0), "n": int(len(delta))}

    eng.configure_estimates(EstimateSettings(min_points=10))
    eng.configure_thinning(z_step=10)
    out = {"indices": list(eng.indices), "nuclei": [(int(eng.z[i]), int(eng.a[i])) for i in eng.indices], "estimates": {},
           "end_point_shift": []}
    ends = {}
    for on in (False, True):
        _stage(eng, on, args)
        est, truth, tracks = [], [], []
        for first in range(0, args.stats_events, args.events):
            n = min(args.events, args.stats_events - first)
            res = eng.run_estimates(n, seed=1, first_event=first)
            est.append(res["estimates"])
            truth.append(truth_tracks(res["p4"], res["indices"], eng.z))
            tracks.append(eng.run_summary(n, seed=1, first_event=first)["tracks"])
        est = np.concatenate(est)
        truth = {k: np.concatenate([t[k] for t in truth]) for k in truth[0]}
        ends[on] = np.concatenate(tracks)
        legs = []
        for s in range(est.shape[1]):
            e = est[:, s]
            good = np.isfinite(e["brho"]) & np.isfinite(e["slope"]) & np.isfinite(truth["brho"][:, s])
            pos = {"estimated": float(good.mean())}
            if good.sum() >= 10:
                pos["brho_rel"] = widths(e["brho"][good] / truth["brho"][good, s] - 1.0)
                pos["polar"] = widths(polar(e)[good] - truth["polar"][good, s])
            legs.append(pos)
        out["estimates"]["on" if on else "off"] = legs
    _stage(eng, False, args)
    eng.configure_estimates()
    eng.configure_thinning()
    for s in range(ends[True].shape[1]):
        a, b = ends[False][:, s], ends[True][:, s]
        both = (a["n_samples"] > 0) & (b["n_samples"] > 0)
        out["end_point_shift"].append({
            "tracks": int(both.sum()),
            "x_mm": widths(1.0e3 * (b["end_x"][both] - a["end_x"][both])),
            "y_mm": widths(1.0e3 * (b["end_y"][both] - a["end_y"][both])),
            "tb": widths(b["end_tb"][both] - a["end_tb"][both]),
            "n_steps": widths((b["n_steps"][both].astype(np.int64) - a["n_steps"][both].astype(np.int64)).astype(float)),
        })
    return out


def _print_resolution(r: dict) -> None:
    for s, nucleus in enumerate(r["nuclei"]):
        print(f"  position {s} (row {r['indices'][s]}, Z {nucleus[0]} A {nucleus[1]}):")
        for leg in ("off", "on"):
            pos = r["estimates"][leg][s]
            line = f"    stage {leg:3s} estimated {100 * pos['estimated']:.1f} %"
            for key in ("brho_rel", "polar"):
                if key in pos:
                    line += f"; {key} median {pos[key]['median']:+.4f} half-width {pos[key]['half_width_16_84']:.4f}"
            print(line)
        shift = r["end_point_shift"][s]
        print(f"    end point on - off over {shift['tracks']} tracks: half-width x {shift['x_mm']['half_width_16_84']:.3f} mm, "
              f"y {shift['y_mm']['half_width_16_84']:.3f} mm, time bucket {shift['tb']['half_width_16_84']:.3f}, "
              f"ODE rows {shift['n_steps']['half_width_16_84']:.1f} (median {shift['n_steps']['median']:+.1f})")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile")
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=100000)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--angular-scale", type=float, default=1.0)
    ap.add_argument("--energy-scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.profile:
        eng = _engine(args.profile)
        _stage(eng, True, args)
        eng.run(args.events, seed=1)
        eng.run(args.events, seed=1)
        return
    for name in args.workloads.split(","):
        eng = _engine(name)
        line = {"workload": name, "events": args.events}
        if args.reps > 0:
            r = line["rates"] = rates(eng, args)
            print(f"## {name}: run(fetch=False) of {args.events} events", flush=True)
            for leg, v in r.items():
                print(f"  stage {leg:3s} {v['rate'][0]:12.0f} events/s  ({v['rate'][1]:.0f} .. {v['rate'][2]:.0f}); "
                      f"track kernels {v['track_us'][0]:.3f} us per event ({v['track_us'][1]:.3f} .. {v['track_us'][2]:.3f})")
            if "on" in r:
                print(f"  cost of the stage: {100.0 * (1.0 - r['on']['rate'][0] / r['off']['rate'][0]):.1f} % of the stage-off rate, "
                      f"{100.0 * (r['on']['track_us'][0] / r['off']['track_us'][0] - 1.0):.1f} % more track time")
        if args.stats_events > 0 and not args.plain_only:
            line["resolution"] = resolution(eng, args)
            print(f"## {name}: {args.stats_events} events, min_points 10, thinning 10 mm", flush=True)
            _print_resolution(line["resolution"])
        eng.ctx.close()
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
