"""Cost of the drift correction (attpc_trace_configure_correction) and the closure of distortion and
correction at the resident rate: one GPU, o16aa and be10dp.  The map is M of the tests (tools/distortion_rate.py), for
the distortion and for the correction alike.

Rates: per workload one engine in this process; ``run_estimates`` of ``--events`` events (estimates with ``min_points``
10, thinning at 10 mm, geometric circle fit, helix slope; the distortion on in both legs) with the correction off and on,
alternating, ``--reps`` timed calls each behind one warm-up call of each kind.  A leg's figure is the median of its timed
calls, its spread their minimum and maximum.  ``--plain-only`` times the correction-off leg alone, without the
distortion: what a library without either entry point (``ATTPC_HIP_LIBRARY``, a build of the parent commit) can run, to
set beside the same leg of this build in the same session, the two processes alternating.
Closure: ``--stats-events`` events through ``run_estimates`` in calls of ``--events`` with the distortion off, on, and on
with the correction: per track position the median of the same event's brho / brho_off - 1, polar - polar_off and
vertex - vertex_off, and the correction's counts.  Reported values for the map used, no limits.
``--profile WORKLOAD`` runs two ``run_estimates`` calls with distortion and correction on and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/correction_rate.py --profile o16aa`` (a run of its own); it prints the
rows of one call, so that undistort_kernel's time is set against 72 B in and 72 B out per row.

    python tools/correction_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
                                    [--plain-only]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from distortion_rate import _compare, _engine, _median, _print_effect, named_map  # noqa: E402


def _estimates(eng) -> None:
    from attpc_engine_amd.detector.circle import CircleFitSettings
    from attpc_engine_amd.detector.estimate import EstimateSettings
    from attpc_engine_amd.detector.helix import HelixSlopeSettings

    eng.configure_estimates(EstimateSettings(min_points=10))
    eng.configure_thinning(z_step=10)
    eng.configure_circle_fit(CircleFitSettings())
    eng.configure_helix_slope(HelixSlopeSettings())


def _stages(eng, distortion: bool, correction: bool) -> None:
    if hasattr(eng.ctx.lib, "attpc_det_configure_distortion"):
        eng.configure_distortion(named_map() if distortion else None)
    if hasattr(eng.ctx.lib, "attpc_trace_configure_correction"):
        from attpc_engine_amd.detector.correction import CorrectionSettings

        eng.configure_correction(CorrectionSettings(named_map()) if correction else None)


def rates(eng, args) -> dict:
    kinds = (False,) if args.plain_only else (False, True)
    legs = {on: [] for on in kinds}
    counts = {}

    def call(on: bool) -> float:
        _stages(eng, not args.plain_only, on)
        t0 = time.perf_counter()
        res = eng.run_estimates(args.events, seed=1)
        rate = args.events / (time.perf_counter() - t0)
        counts["rows"] = int(res["trace_rows"]["n_rows"])
        if "correction" in res:
            counts["correction"] = res["correction"]
        return rate

    for on in kinds:
        call(on)
    for _ in range(args.reps):
        for on in kinds:
            legs[on].append(call(on))
    _stages(eng, False, False)
    out = {("on" if on else "off"): [_median(v), min(v), max(v)] for on, v in legs.items()}
    out.update(counts)
    return out


def closure(eng, args) -> dict:
    import numpy as np

    out = {"indices": list(eng.indices), "nuclei": [(int(eng.z[i]), int(eng.a[i])) for i in eng.indices], "correction": {}}
    est = {}
    for key, distortion, correction in (("off", False, False), ("on", True, False), ("corrected", True, True)):
        _stages(eng, distortion, correction)
        parts = [eng.run_estimates(min(args.events, args.stats_events - first), seed=1, first_event=first)
                 for first in range(0, args.stats_events, args.events)]
        est[key] = np.concatenate([p["estimates"] for p in parts])
        if correction:
            out["correction"] = {k: sum(p["correction"][k] for p in parts) for k in parts[0]["correction"]}
    out["host_on"] = _compare(est["off"], est["on"])
    out["host_corrected"] = _compare(est["off"], est["corrected"])
    _stages(eng, False, False)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile")
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=32768)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out")
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    if args.profile:
        eng = _engine(args.profile)
        _estimates(eng)
        _stages(eng, True, True)
        eng.run_estimates(args.events, seed=1)
        res = eng.run_estimates(args.events, seed=1)
        print(json.dumps({"workload": args.profile, "events": args.events, "rows": int(res["trace_rows"]["n_rows"]),
                          "bytes_moved": 144 * int(res["trace_rows"]["n_rows"]), "correction": res["correction"]}))
        return
    for name in args.workloads.split(","):
        eng = _engine(name)
        _estimates(eng)
        line = {"workload": name, "events": args.events}
        if args.reps > 0:
            r = line["rates"] = rates(eng, args)
            print(f"## {name}: run_estimates of {args.events} events, {r['rows']} rows", flush=True)
            for leg in ("off", "on"):
                if leg in r:
                    print(f"  correction {leg:3s} {r[leg][0]:12.0f} events/s  ({r[leg][1]:.0f} .. {r[leg][2]:.0f})")
            if "on" in r:
                print(f"  cost of the stage: {100.0 * (1.0 - r['on'][0] / r['off'][0]):.1f} % of the stage-off rate; counts {r.get('correction')}")
        if args.stats_events > 0 and not args.plain_only:
            line["closure"] = closure(eng, args)
            print(f"## {name}: {args.stats_events} events at the resident rate, min_points 10, thinning 10 mm, circle fit, helix slope; "
                  f"host_on = distortion on, host_corrected = on + corrected, both against distortion off; counts "
                  f"{line['closure']['correction']}", flush=True)
            _print_effect(line["closure"])
        eng.ctx.close()
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
