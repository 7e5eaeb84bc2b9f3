"""Cost of the drift distortion (attpc_det_configure_distortion) and what it does to the track estimates:
one GPU, o16aa and be10dp.  The map is M of the tests: ``linear_radial_field(0.05, 2.0)`` on 33 x 41 nodes with the time
table 4 (rho / rho_max)^2 d / length time buckets.

Rates: per workload one engine in this process; ``run(fetch=False)`` of ``--events`` events with the stage off and on,
alternating, ``--reps`` timed calls each behind one warm-up call of each kind (buffers settle).  A leg's figure is the
median of its timed calls, its spread their minimum and maximum; beside the rate the track stage's own time per event
(``ms_tracks`` of the run's statistics: the track kernel and, with the stage on, the distortion pass behind it).
``--plain-only`` times the stage-off leg alone: what a library without the entry point (``ATTPC_HIP_LIBRARY``, a build of
the parent commit) can run, to set beside the same leg of this build in the same session, the two processes alternating.
Effect: ``--stats-events`` events through ``run_estimates`` (``min_points`` 10, thinning at 10 mm, geometric circle fit,
helix slope) in calls of ``--events``, with the stage off and on: per track position the median of the same event's
brho_on / brho_off - 1, polar_on - polar_off and vertex_on - vertex_off.  Then ``--rows-events`` events through
``run_trace_rows`` with the stage off and on, the delivered rows of the latter through ``undistort_rows`` and all three
through ``rows_to_estimates`` (circle fit and helix slope, no thinning): what the distortion does to these estimates and
what is left of it after the correction.  Reported values for the map used, no limits.
``--profile WORKLOAD`` runs two ``run(fetch=False)`` calls with the stage on and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/distortion_rate.py --profile o16aa`` (a run of its own); it prints
the records of one call, so that distort_kernel's time gives the achieved GB/s of the pass against 64 B x records.

    python tools/distortion_rate.py [--events N] [--reps K] [--stats-events M] [--rows-events R] [--workloads o16aa,be10dp]
                                    [--out FILE] [--plain-only]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def named_map():
    import numpy as np

    from attpc_engine_amd.detector.distortion import DistortionMap

    field = DistortionMap.linear_radial_field(0.05, 2.0, 33, 41, 0.292, 1.0)
    rho = np.arange(33) * 0.292 / 32
    d = np.arange(41) / 40.0
    return DistortionMap(field.radial, field.azimuthal, 4.0 * (rho[:, None] / 0.292) ** 2 * d[None, :], rho_max=0.292, length=1.0)


def _engine(name: str):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    return Engine(pipeline, config, indices, context=_abi.Context(0))


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def _stage(eng, on: bool) -> None:
    if on:
        eng.configure_distortion(named_map())
    elif hasattr(eng.ctx.lib, "attpc_det_configure_distortion"):
        eng.configure_distortion()


def rates(eng, args) -> dict:
    kinds = (False,) if args.plain_only else (False, True)
    legs = {on: {"rate": [], "track_us": []} for on in kinds}
    samples = {}

    def call(on: bool):
        _stage(eng, on)
        t0 = time.perf_counter()
        stats = eng.run(args.events, seed=1)["stats"]
        samples[on] = int(stats["n_track_samples"])
        return args.events / (time.perf_counter() - t0), 1.0e3 * stats["ms_tracks"] / args.events

    for on in kinds:
        call(on)
    for _ in range(args.reps):
        for on in kinds:
            rate, track_us = call(on)
            legs[on]["rate"].append(rate)
            legs[on]["track_us"].append(track_us)
    _stage(eng, False)
    out = {("on" if on else "off"): {k: [_median(v), min(v), max(v)] for k, v in leg.items()} for on, leg in legs.items()}
    out["track_samples"] = samples[False]
    return out


def _widths(delta):
    import numpy as np

    if len(delta) == 0:
        return {"n": 0}
    lo, mid, hi = np.percentile(delta, [16.0, 50.0, 84.0])
    return {"median": float(mid), "half_width_16_84": float((hi - lo) / 2.0), "n": int(len(delta))}


def _compare(a, b) -> list:
    """Per track position: the records ``b`` against the same events' records ``a`` where both are estimated."""
    import numpy as np

    from attpc_engine_amd.detector.estimate import polar

    out = []
    for s in range(a.shape[1]):
        x, y = a[:, s], b[:, s]
        both = np.isfinite(x["brho"]) & np.isfinite(y["brho"]) & np.isfinite(x["slope"]) & np.isfinite(y["slope"])
        out.append({"estimated_both": float(both.mean()),
                    "brho_rel": _widths(y["brho"][both] / x["brho"][both] - 1.0),
                    "polar_mrad": _widths(1.0e3 * (polar(y)[both] - polar(x)[both])),
                    "vertex_xy_mm": _widths(np.hypot(y["vx"][both] - x["vx"][both], y["vy"][both] - x["vy"][both])),
                    "vertex_z_mm": _widths(y["vz"][both] - x["vz"][both])})
    return out


def _corrected(res, config):
    """The delivered rows of a distorted run through ``undistort_rows``, every event in ascending z again (as the
    estimates read them) -> (rows, labels)."""
    import numpy as np

    rows = named_map().undistort_rows(res["rows"], config)
    labels = np.array(res["labels"])
    for lo, hi in zip(res["offsets"][:-1], res["offsets"][1:]):
        order = np.argsort(rows[lo:hi, 2], kind="stable")
        rows[lo:hi], labels[lo:hi] = rows[lo:hi][order], labels[lo:hi][order]
    return rows, labels


def effect(eng, args) -> dict:
    import numpy as np

    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
    from attpc_engine_amd.detector.helix import HelixSlopeSettings

    settings = EstimateSettings(min_points=10)
    eng.configure_estimates(settings)
    eng.configure_thinning(z_step=10)
    eng.configure_circle_fit(CircleFitSettings())
    eng.configure_helix_slope(HelixSlopeSettings())
    out = {"indices": list(eng.indices), "nuclei": [(int(eng.z[i]), int(eng.a[i])) for i in eng.indices]}
    est = {}
    for on in (False, True):
        _stage(eng, on)
        est[on] = np.concatenate([eng.run_estimates(min(args.events, args.stats_events - first), seed=1, first_event=first)["estimates"]
                                  for first in range(0, args.stats_events, args.events)])
    out["device"] = _compare(est[False], est[True])
    eng.configure_thinning()
    if args.rows_events > 0:
        rows = {}
        for on in (False, True):
            _stage(eng, on)
            rows[on] = eng.run_trace_rows(args.rows_events, seed=1, first_event=0)
        host = {}
        for key, res, fix in (("off", rows[False], False), ("on", rows[True], False), ("corrected", rows[True], True)):
            r, labels = _corrected(res, eng.config) if fix else (res["rows"], res["labels"])
            host[key] = rows_to_estimates(res["offsets"], r, labels, eng.indices, settings, eng.ctx, eng.config,
                                          circle=CircleFitSettings(), helix=HelixSlopeSettings())
        out["host_on"] = _compare(host["off"], host["on"])
        out["host_corrected"] = _compare(host["off"], host["corrected"])
    _stage(eng, False)
    eng.configure_estimates()
    eng.configure_circle_fit()
    eng.configure_helix_slope()
    return out


def _print_effect(r: dict) -> None:
    for s, nucleus in enumerate(r["nuclei"]):
        print(f"  position {s} (row {r['indices'][s]}, Z {nucleus[0]} A {nucleus[1]}):")
        for key in ("device", "host_on", "host_corrected"):
            if key not in r:
                continue
            pos = r[key][s]
            if not pos["brho_rel"]["n"]:
                print(f"    {key:14s} no track estimated in both legs")
                continue
            print(f"    {key:14s} tracks {pos['brho_rel']['n']:6d}  brho median {100 * pos['brho_rel']['median']:+.3f} % "
                  f"(half-width {100 * pos['brho_rel']['half_width_16_84']:.3f}); polar {pos['polar_mrad']['median']:+.3f} mrad "
                  f"({pos['polar_mrad']['half_width_16_84']:.3f}); vertex xy {pos['vertex_xy_mm']['median']:.3f} mm, "
                  f"z {pos['vertex_z_mm']['median']:+.3f} mm ({pos['vertex_z_mm']['half_width_16_84']:.3f})")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile")
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=32768)
    ap.add_argument("--rows-events", type=int, default=2048)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    if args.profile:
        eng = _engine(args.profile)
        _stage(eng, True)
        eng.run(args.events, seed=1)
        stats = eng.run(args.events, seed=1)["stats"]
        print(json.dumps({"workload": args.profile, "events": args.events, "track_samples": int(stats["n_track_samples"]),
                          "bytes_moved": 64 * int(stats["n_track_samples"]), "launches_tracks": int(stats["launches_tracks"])}))
        return
    for name in args.workloads.split(","):
        eng = _engine(name)
        line = {"workload": name, "events": args.events}
        if args.reps > 0:
            r = line["rates"] = rates(eng, args)
            print(f"## {name}: run(fetch=False) of {args.events} events, {r['track_samples']} track samples", flush=True)
            for leg in ("off", "on"):
                if leg in r:
                    v = r[leg]
                    print(f"  stage {leg:3s} {v['rate'][0]:12.0f} events/s  ({v['rate'][1]:.0f} .. {v['rate'][2]:.0f}); "
                          f"track stage {v['track_us'][0]:.3f} us per event ({v['track_us'][1]:.3f} .. {v['track_us'][2]:.3f})")
            if "on" in r:
                extra_us = r["on"]["track_us"][0] - r["off"]["track_us"][0]
                print(f"  cost of the stage: {100.0 * (1.0 - r['on']['rate'][0] / r['off']['rate'][0]):.1f} % of the stage-off rate, "
                      f"{extra_us:.3f} us more track time per event"
                      + (f" = {64.0e-3 * r['track_samples'] / args.events / extra_us:.0f} GB/s over 64 B x records" if extra_us > 0 else ""))
        if args.stats_events > 0 and not args.plain_only:
            line["effect"] = effect(eng, args)
            print(f"## {name}: {args.stats_events} events, min_points 10, thinning 10 mm, circle fit, helix slope; host rows: "
                  f"{args.rows_events} events, no thinning", flush=True)
            _print_effect(line["effect"])
        eng.ctx.close()
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
