"""Cost and yield of the track estimates of the trace rows (attpc_trace_configure_estimates): one GPU,
o16aa and be10dp, two trace modes -- hit mode without noise, partial readout with sigma = 5, pedestals and
threshold 20.

Rates: per (workload, mode) one engine in this process; ``run_trace_rows(fetch=False)`` of ``--events`` events with
the stage off and on, alternating, ``--reps`` timed calls each behind one warm-up call of each kind (buffers settle).
A leg's figure is the median of its timed calls, its spread their minimum and maximum; the stage's cost per event is
1 / rate(on) - 1 / rate(off).
Yield: ``--stats-events`` events through ``run_estimates`` in calls of ``--events``: the share of tracks per status
bit, and for the tracks with B rho and slope the median and the 16 .. 84 % half-width of brho / brho_true - 1 and of
polar - polar_true against ``truth_tracks`` of the same call -- and, to tell the two factors of B rho apart, of
radius / radius_true - 1 and of the cumulated distance over twice the chord vertex -> segment mean (1 for a thin
straight segment; the zig-zag of neighbouring pads raises it).  Reported values for the settings used, no limits.
Thinning (attpc_trace_configure_thinning): ``--thinning Z`` times the estimates without and with
thinning at a z step of Z mm in the place of stage off / on (both legs have the estimates on, ``--min-points`` points),
and ``--thin-steps 2,5,10`` repeats the yield at these steps beside the unthinned one.  ``--estimates-only`` times the
estimates leg alone: what a library without the thinning entry points (``ATTPC_HIP_LIBRARY``, a build of the parent
commit by tools/build_variant.sh) can run, to set beside the same leg of this build in the same session.
Geometric circle fit (attpc_trace_configure_circle): ``--circle`` times the estimates with the Kasa circle
against the estimates with the geometric fit behind it, alternating (both legs on raw rows, or with ``--thinning Z`` on
the points of that z step), and repeats the yield with the Kasa circle and with the geometric fit -- on the raw rows, or
at every step of ``--thin-steps`` if given -- with the distribution of the evaluations made (``reserved``) beside it.
Helix slope (attpc_trace_configure_helix): ``--helix`` times the estimates with the zig-zag slope against
the estimates with the helix slope, alternating (both legs with ``--thinning Z`` and ``--circle`` as given), and repeats
the yield with the stage off and on at every step of ``--thin-steps`` -- with the share of NO_HELIX and the share of
tracks for which regressor "auto" took the path against z (the records of three runs, one per regressor, compared)
beside it.  ``--helix-off-only`` times the stage-off leg alone: what a library without the helix entry points
(``ATTPC_HIP_LIBRARY``, a build of the parent commit) can run, to set beside the same leg of this build.
``--profile WORKLOAD`` runs two ``run_estimates`` calls in partial readout and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/estimate_rate.py --profile o16aa`` (a run of its own).

    python tools/estimate_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
                                  [--thinning Z | --estimates-only] [--thin-steps 2,5,10] [--min-points P] [--circle]
                                  [--helix | --helix-off-only]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

MODES = {
    "hit": {},
    "partial": {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"},
}


def _engine(name: str, mode: str):
    import numpy as np

    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    eng = Engine(pipeline, config, indices, context=_abi.Context(0))
    eng.configure_traces(config, offset=int(np.argmax(get_response(config))), **MODES[mode])
    return eng


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def rates(eng, events: int, reps: int) -> dict:
    from attpc_engine_amd.detector.estimate import EstimateSettings

    legs = {"off": [], "on": []}

    def call(on: bool):
        eng.configure_estimates(EstimateSettings() if on else None)
        t0 = time.perf_counter()
        res = eng.run_trace_rows(events, seed=1, fetch=False)
        return events / (time.perf_counter() - t0), res

    call(False), call(True)
    rows = 0
    for _ in range(reps):
        for on in (False, True):
            rate, res = call(on)
            legs["on" if on else "off"].append(rate)
            rows = res["trace_rows"]["n_rows"]
    eng.configure_estimates()
    return {"rows_per_event": rows / events, **{k: [_median(v), min(v), max(v)] for k, v in legs.items()}}


def thinning_rates(eng, events: int, reps: int, z_step, min_points: int) -> dict:
    """The estimates alone against the estimates of thinned points (``z_step`` None: the first leg only)."""
    from attpc_engine_amd.detector.estimate import EstimateSettings

    kinds = ("estimates",) if z_step is None else ("estimates", "thinned")
    legs = {kind: [] for kind in kinds}
    eng.configure_estimates(EstimateSettings(min_points=min_points))

    def call(kind: str):
        if z_step is not None:
            eng.configure_thinning(**({"z_step": z_step} if kind == "thinned" else {}))
        t0 = time.perf_counter()
        res = eng.run_trace_rows(events, seed=1, fetch=False)
        return events / (time.perf_counter() - t0), res

    for kind in kinds:
        call(kind)
    rows = 0
    for _ in range(reps):
        for kind in kinds:
            rate, res = call(kind)
            legs[kind].append(rate)
            rows = res["trace_rows"]["n_rows"]
    eng.configure_estimates()
    if z_step is not None:
        eng.configure_thinning()
    return {"rows_per_event": rows / events, **{k: [_median(v), min(v), max(v)] for k, v in legs.items()}}


def circle_rates(eng, events: int, reps: int, z_step, min_points: int) -> dict:
    """The estimates with the Kasa circle against the estimates with the geometric fit behind it (``z_step``: both on
    the thinned points of that step, None: on the raw rows)."""
    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings

    kinds = ("kasa", "geometric")
    legs = {kind: [] for kind in kinds}
    eng.configure_estimates(EstimateSettings(min_points=min_points))
    if z_step is not None:
        eng.configure_thinning(z_step=z_step)

    def call(kind: str):
        eng.configure_circle_fit(CircleFitSettings() if kind == "geometric" else None)
        t0 = time.perf_counter()
        res = eng.run_trace_rows(events, seed=1, fetch=False)
        return events / (time.perf_counter() - t0), res

    for kind in kinds:
        call(kind)
    rows = 0
    for _ in range(reps):
        for kind in kinds:
            rate, res = call(kind)
            legs[kind].append(rate)
            rows = res["trace_rows"]["n_rows"]
    eng.configure_estimates()
    eng.configure_thinning()
    eng.configure_circle_fit()
    return {"rows_per_event": rows / events, "z_step": z_step, **{k: [_median(v), min(v), max(v)] for k, v in legs.items()}}


def helix_rates(eng, events: int, reps: int, z_step, min_points: int, circle: bool, off_only: bool = False) -> dict:
    """The estimates with the zig-zag slope against the estimates with the helix slope (``z_step``: both on the thinned
    points of that step; ``circle``: both behind the geometric circle fit; ``off_only``: the first leg alone)."""
    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings

    kinds = ("zigzag",) if off_only else ("zigzag", "helix")
    legs = {kind: [] for kind in kinds}
    eng.configure_estimates(EstimateSettings(min_points=min_points))
    if z_step is not None:
        eng.configure_thinning(z_step=z_step)
    if circle:
        eng.configure_circle_fit(CircleFitSettings())

    def call(kind: str):
        if not off_only:
            eng.configure_helix_slope(**({"regressor": "auto"} if kind == "helix" else {}))
        t0 = time.perf_counter()
        res = eng.run_trace_rows(events, seed=1, fetch=False)
        return events / (time.perf_counter() - t0), res

    for kind in kinds:
        call(kind)
    rows = 0
    for _ in range(reps):
        for kind in kinds:
            rate, res = call(kind)
            legs[kind].append(rate)
            rows = res["trace_rows"]["n_rows"]
    eng.configure_estimates()
    eng.configure_thinning()
    eng.configure_circle_fit()
    if not off_only:
        eng.configure_helix_slope()
    return {"rows_per_event": rows / events, "z_step": z_step, "circle": circle, **{k: [_median(v), min(v), max(v)] for k, v in legs.items()}}


def yield_(eng, events: int, total: int, z_step=None, min_points: int = 30, circle: bool = False, helix: bool = False) -> dict:
    import numpy as np

    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings, polar, truth_tracks
    from attpc_engine_amd.detector.helix import STATUS_BITS

    eng.configure_estimates(EstimateSettings(min_points=min_points))
    if z_step is not None:
        eng.configure_thinning(z_step=z_step)
    eng.configure_circle_fit(CircleFitSettings() if circle else None)
    est, truth, fixed = [], [], {"z_on_path": [], "path_on_z": []}
    for regressor in (("auto", "z_on_path", "path_on_z") if helix else (None,)):
        if helix:
            eng.configure_helix_slope(regressor=regressor)
        for first in range(0, total, events):
            res = eng.run_estimates(min(events, total - first), seed=1, first_event=first)
            if regressor in fixed:
                fixed[regressor].append(res["estimates"])
                continue
            est.append(res["estimates"])
            truth.append(truth_tracks(res["p4"], res["indices"], eng.z))
    eng.configure_estimates()
    if z_step is not None:
        eng.configure_thinning()
    eng.configure_circle_fit()
    if helix:
        eng.configure_helix_slope()
    est = np.concatenate(est)
    field = float(eng.config.det_params.bfield)
    truth = {k: np.concatenate([t[k] for t in truth]) for k in truth[0]}
    out = {"tracks": int(est.size), "indices": list(eng.indices), "z_step": z_step, "min_points": min_points,
           "circle": "geometric" if circle else "kasa", "slope": "helix" if helix else "zigzag", "positions": []}
    if helix:
        fixed = {k: np.concatenate(v) for k, v in fixed.items()}
    for s in range(est.shape[1]):
        e = est[:, s]
        pos = {"status": {name: float((e["status"] & bit != 0).mean()) for name, bit in STATUS_BITS.items()},
               "clean": float((e["status"] == 0).mean())}
        good = np.isfinite(e["brho"]) & np.isfinite(e["slope"]) & np.isfinite(truth["brho"][:, s])
        pos["estimated"] = float(good.mean())
        if helix:  # which regressor "auto" took: its slope is bit for bit the one of that regressor's run
            ran_helix = np.isfinite(e["slope"]) & (e["status"] & STATUS_BITS["NO_HELIX"] == 0) & (e["n_fit"] > 0)
            same = {k: e["slope"].view(np.int64) == v[:, s]["slope"].view(np.int64) for k, v in fixed.items()}
            if ran_helix.any():
                pos["auto"] = {"path_on_z": float((same["path_on_z"] & ~same["z_on_path"])[ran_helix].mean()),
                               "z_on_path": float((same["z_on_path"] & ~same["path_on_z"])[ran_helix].mean()),
                               "either": float((same["z_on_path"] & same["path_on_z"])[ran_helix].mean())}
            fitted = e["n_fit"] > 0
            pos["no_helix_of_fitted"] = float((e["status"][fitted] & STATUS_BITS["NO_HELIX"] != 0).mean()) if fitted.any() else 0.0
        ran = e["reserved"] > 0
        if ran.any():  # the geometric circle fit: the evaluations of the records it ran on
            pos["evaluations"] = {"share": float(ran.mean()), "median": float(np.median(e["reserved"][ran])),
                                  "p90": float(np.percentile(e["reserved"][ran], 90.0)), "max": int(e["reserved"][ran].max()),
                                  "histogram": np.bincount(e["reserved"][ran], minlength=65).tolist()}
        if good.sum() >= 10:
            # the two factors of brho apart: the circle against R = B rho sin(theta) / B of the truth, and the
            # cumulated pad-plane distance against the straight chord of the same segment (zig-zag: above 1)
            radius_true = truth["brho"][good, s] * np.sin(truth["polar"][good, s]) / field * 1.0e3
            chord = 16.0 * np.hypot(e["x_mean"][good] - e["vx"][good], e["y_mean"][good] - e["vy"][good])
            for name, delta in (("brho_rel", e["brho"][good] / truth["brho"][good, s] - 1.0),
                                ("polar", polar(e)[good] - truth["polar"][good, s]),
                                ("radius_rel", e["radius"][good] / radius_true - 1.0),
                                ("arc_over_2chord_to_mean", e["arc"][good] / (2.0 * chord))):
                lo, mid, hi = np.percentile(delta, [16.0, 50.0, 84.0])
                pos[name] = {"median": float(mid), "half_width_16_84": float((hi - lo) / 2.0)}
        out["positions"].append(pos)
    return out


def _print_yield(y: dict) -> None:
    for s, pos in enumerate(y["positions"]):
        shares = ", ".join(f"{k} {100 * v:.1f} %" for k, v in pos["status"].items())
        print(f"  position {s} (nucleus {y['indices'][s]}): clean {100 * pos['clean']:.1f} %, estimated"
              f" {100 * pos['estimated']:.1f} %; {shares}")
        for key in ("brho_rel", "polar", "radius_rel", "arc_over_2chord_to_mean"):
            if key in pos:
                print(f"    {key}: median {pos[key]['median']:+.4f}, 16 .. 84 % half-width {pos[key]['half_width_16_84']:.4f}")
        if "auto" in pos:
            print(f"    NO_HELIX {100 * pos['no_helix_of_fitted']:.2f} % of the fitted tracks; auto took the path against z for "
                  f"{100 * pos['auto']['path_on_z']:.1f} %, z against the path for {100 * pos['auto']['z_on_path']:.1f} %")
        if "evaluations" in pos:
            ev = pos["evaluations"]
            print(f"    evaluations (fit ran on {100 * ev['share']:.1f} %): median {ev['median']:.0f}, 90 % {ev['p90']:.0f}, max {ev['max']}")


def thinning_main(args) -> None:
    steps = [float(z) for z in args.thin_steps.split(",") if z]
    for name in args.workloads.split(","):
        for mode in MODES:
            eng = _engine(name, mode)
            line = {"workload": name, "mode": mode, "events": args.events, "min_points": args.min_points}
            if args.reps > 0:
                r = line["rates"] = thinning_rates(eng, args.events, args.reps, args.thinning, args.min_points)
                print(f"## {name} / {mode}: {r['rows_per_event']:.1f} trace rows per event, min_points {args.min_points}", flush=True)
                for leg in ("estimates", "thinned"):
                    if leg in r:
                        print(f"  run_trace_rows(fetch=False), {leg:9s} {r[leg][0]:12.0f} events/s  ({r[leg][1]:.0f} .. {r[leg][2]:.0f})")
                if "thinned" in r:
                    cost = 1.0 / r["thinned"][0] - 1.0 / r["estimates"][0]
                    print(f"  cost of thinning at {args.thinning} mm: {cost * 1e9:.0f} ns per event, "
                          f"{100.0 * (1.0 - r['thinned'][0] / r['estimates'][0]):.2f} % of the rate without it")
            line["yield"] = []
            for z_step in ([None] + steps if steps and args.stats_events > 0 else []):
                y = yield_(eng, args.events, args.stats_events, z_step, args.min_points)
                line["yield"].append(y)
                print(f"## {name} / {mode}: records of {args.stats_events} events, " + ("raw rows" if z_step is None else f"z step {z_step} mm"), flush=True)
                _print_yield(y)
            eng.ctx.close()
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


def circle_main(args) -> None:
    steps = [float(z) for z in args.thin_steps.split(",") if z] or [None]
    for name in args.workloads.split(","):
        for mode in MODES:
            eng = _engine(name, mode)
            line = {"workload": name, "mode": mode, "events": args.events, "min_points": args.min_points}
            if args.reps > 0:
                r = line["rates"] = circle_rates(eng, args.events, args.reps, args.thinning, args.min_points)
                where = "raw rows" if args.thinning is None else f"points of {args.thinning} mm"
                print(f"## {name} / {mode}: {r['rows_per_event']:.1f} trace rows per event, min_points {args.min_points}, {where}", flush=True)
                for leg in ("kasa", "geometric"):
                    print(f"  run_trace_rows(fetch=False), {leg:9s} {r[leg][0]:12.0f} events/s  ({r[leg][1]:.0f} .. {r[leg][2]:.0f})")
                cost = 1.0 / r["geometric"][0] - 1.0 / r["kasa"][0]
                print(f"  cost of the geometric fit: {cost * 1e9:.0f} ns per event, "
                      f"{100.0 * (1.0 - r['geometric'][0] / r['kasa'][0]):.2f} % of the rate without it")
            line["yield"] = []
            for z_step in (steps if args.stats_events > 0 else []):
                for circle in (False, True):
                    y = yield_(eng, args.events, args.stats_events, z_step, args.min_points, circle)
                    line["yield"].append(y)
                    print(f"## {name} / {mode}: records of {args.stats_events} events, " + ("raw rows" if z_step is None else f"z step {z_step} mm")
                          + f", {y['circle']} circle", flush=True)
                    _print_yield(y)
            eng.ctx.close()
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


def helix_main(args) -> None:
    steps = [float(z) for z in args.thin_steps.split(",") if z] or [None]
    for name in args.workloads.split(","):
        for mode in MODES:
            eng = _engine(name, mode)
            line = {"workload": name, "mode": mode, "events": args.events, "min_points": args.min_points}
            if args.reps > 0:
                r = line["rates"] = helix_rates(eng, args.events, args.reps, args.thinning, args.min_points, args.circle, args.helix_off_only)
                where = "raw rows" if args.thinning is None else f"points of {args.thinning} mm"
                print(f"## {name} / {mode}: {r['rows_per_event']:.1f} trace rows per event, min_points {args.min_points}, {where}, "
                      f"{'geometric' if args.circle else 'kasa'} circle", flush=True)
                for leg in ("zigzag", "helix"):
                    if leg in r:
                        print(f"  run_trace_rows(fetch=False), {leg:9s} {r[leg][0]:12.0f} events/s  ({r[leg][1]:.0f} .. {r[leg][2]:.0f})")
                if "helix" in r:
                    cost = 1.0 / r["helix"][0] - 1.0 / r["zigzag"][0]
                    print(f"  cost of the helix slope: {cost * 1e9:.0f} ns per event, "
                          f"{100.0 * (1.0 - r['helix'][0] / r['zigzag'][0]):.2f} % of the rate without it")
            line["yield"] = []
            for z_step in (steps if args.stats_events > 0 and not args.helix_off_only else []):
                for helix in (False, True):
                    y = yield_(eng, args.events, args.stats_events, z_step, args.min_points, args.circle, helix)
                    line["yield"].append(y)
                    print(f"## {name} / {mode}: records of {args.stats_events} events, " + ("raw rows" if z_step is None else f"z step {z_step} mm")
                          + f", {y['circle']} circle, {y['slope']} slope", flush=True)
                    _print_yield(y)
            eng.ctx.close()
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


def profile(name: str, events: int, z_step=None, min_points: int = 30, circle: bool = False, helix: bool = False) -> None:
    from attpc_engine_amd.detector.estimate import EstimateSettings

    eng = _engine(name, "partial")
    eng.configure_estimates(EstimateSettings(min_points=min_points))
    if z_step is not None:
        eng.configure_thinning(z_step=z_step)
    if circle:
        eng.configure_circle_fit(max_evaluations=32)
    if helix:
        eng.configure_helix_slope(regressor="auto")
    eng.run_estimates(events, seed=1)
    eng.run_estimates(events, seed=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile")
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=100000)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out")
    ap.add_argument("--thinning", type=float)
    ap.add_argument("--estimates-only", action="store_true")
    ap.add_argument("--thin-steps", default="")
    ap.add_argument("--min-points", type=int, default=30)
    ap.add_argument("--circle", action="store_true")
    ap.add_argument("--helix", action="store_true")
    ap.add_argument("--helix-off-only", action="store_true")
    args = ap.parse_args()
    if args.profile:
        return profile(args.profile, args.events, args.thinning, args.min_points, args.circle, args.helix)
    if args.helix or args.helix_off_only:
        return helix_main(args)
    if args.circle:
        return circle_main(args)
    if args.thinning is not None or args.estimates_only or args.thin_steps:
        return thinning_main(args)
    for name in args.workloads.split(","):
        for mode in MODES:
            eng = _engine(name, mode)
            line = {"workload": name, "mode": mode, "events": args.events, "rates": rates(eng, args.events, args.reps)}
            if args.stats_events > 0:
                line["yield"] = yield_(eng, args.events, args.stats_events)
            eng.ctx.close()
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            r = line["rates"]
            cost = 1.0 / r["on"][0] - 1.0 / r["off"][0]
            print(f"## {name} / {mode}: {r['rows_per_event']:.1f} trace rows per event", flush=True)
            for leg in ("off", "on"):
                print(f"  run_trace_rows(fetch=False), estimates {leg:3s} {r[leg][0]:12.0f} events/s  ({r[leg][1]:.0f} .. {r[leg][2]:.0f})")
            print(f"  cost of the stage: {cost * 1e6:.3f} us per event, {100.0 * (1.0 - r['on'][0] / r['off'][0]):.1f} % of the stage-off rate")
            if "yield" in line:
                _print_yield(line["yield"])


if __name__ == "__main__":
    main()
