"""Rate of the multiplicity trigger on the pad traces (attpc_trace_configure_trigger) against a yardstick
build of the library (the parent commit's, built beside this one with tools/build_variant.sh): one GPU, o16aa and
be10dp, two trace modes -- hit mode without noise, partial readout with sigma = 5, pedestals and threshold 20.

The method is tools/trace_rows_rate.py's: every (library, workload) measurement runs in a child process of its own
(the library is chosen once per process, ATTPC_HIP_LIBRARY); the children of the two libraries alternate, ``--reps``
times, so that drift of the machine hits both alike.  A child warms every leg up with one call (buffers settle) and
times the next one; a leg's figure is the median of the ``--reps`` timed calls, its spread their minimum and maximum.
Legs, all of ``--events`` events device-resident unless named delivered:
  traces / rows                  run_traces(fetch=False) / run_trace_rows(fetch=False), no trigger configured (both libraries)
  traces_delivered               run_traces into page-locked arrays, ``--deliver-events`` events (both libraries)
  trigger                        run_trigger: the traces stay on the device, 32 B per event come back
  rows_trigger                   run_trace_rows with the trigger on, gate off
  rows_gate_half / rows_gate_tenth   ... gated at a multiplicity about a half / a tenth of the events reach
The driver prints, per workload and mode: (i) traces and rows of this build without a trigger inside the yardstick's
spread; the cost of the stage per event, 1 / rate(on) - 1 / rate(off), for the traces and the rows; run_trigger against
the yardstick's delivered run_traces; the gated rows against the ungated ones; and the bytes of kept rows the stage
reads per second of its own cost.  ``--profile WORKLOAD`` runs one run_trigger call in partial readout and nothing
else, for ``rocprofv3 --kernel-trace --stats -- python tools/trigger_rate.py --profile o16aa`` (a run of its own).

    python tools/trigger_rate.py [--yardstick attpc_engine_amd/_lib/libattpc_parent.so] [--events N] [--deliver-events M]
                                 [--reps K] [--workloads o16aa,be10dp] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

MODES = {
    "hit": {},
    "partial": {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"},
}
TRACE_ROW_BYTES = 512 * 2
TRIGGER = {"threshold": 25, "window": 50}


def _engine(name: str):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    return Engine(pipeline, config, indices, context=_abi.Context(0)), config


def _reach(records, fraction: float) -> int:
    """A group multiplicity that about ``fraction`` of the events reach (one group: fired iff peak_group_sum >= it)."""
    import numpy as np

    reach = np.sort(records["peak_group_sum"])[::-1]
    return max(1, int(reach[max(0, int(fraction * len(reach)) - 1)]))


def child(name: str, events: int, deliver_events: int) -> None:
    from attpc_engine_amd import _abi
    from attpc_engine_amd.outputs import TraceArrays

    eng, config = _engine(name)
    ctx, seed = eng.ctx, 1
    has_trigger = all(hasattr(ctx.lib, s) for s in _abi.TRIGGER_SYMBOLS)
    out = {"workload": name, "library": os.environ.get("ATTPC_HIP_LIBRARY", "own"), "events": events,
           "deliver_events": deliver_events, "modes": {}}

    def timed(fn, n):
        fn()
        t0 = time.perf_counter()
        res = fn()
        return n / (time.perf_counter() - t0), res

    for mode, kw in MODES.items():
        eng.configure_traces(config, **kw)
        if has_trigger:
            eng.configure_trigger()
        legs = {}
        legs["traces"], res = timed(lambda: eng.run_traces(events, seed=seed, fetch=False), events)
        rows_per_event = res["trace"]["n_rows"] / events
        legs["rows"], _ = timed(lambda: eng.run_trace_rows(events, seed=seed, fetch=False), events)
        pinned = TraceArrays(deliver_events, int(rows_per_event * deliver_events * 1.3) + 4096, ctx.pinned_empty)
        stats = _abi.RunStats()

        def delivered():
            ctx.check(ctx.lib.attpc_sim_run_traces(ctx.handle, seed, 0, deliver_events, eng.layout, None, None, None, pinned.out,
                                                   stats), "attpc_sim_run_traces")

        legs["traces_delivered"], _ = timed(delivered, deliver_events)
        del pinned
        extra = {"rows_per_event": rows_per_event}
        if has_trigger:
            eng.configure_trigger(group_multiplicity=1, **TRIGGER)
            legs["trigger"], res = timed(lambda: eng.run_trigger(events, seed=seed), events)
            legs["rows_trigger"], _ = timed(lambda: eng.run_trace_rows(events, seed=seed, fetch=False), events)
            for leg, fraction in (("rows_gate_half", 0.5), ("rows_gate_tenth", 0.1)):
                mg = _reach(res["trigger"], fraction)
                eng.configure_trigger(group_multiplicity=mg, gate=True, **TRIGGER)
                legs[leg], gated = timed(lambda: eng.run_trace_rows(events, seed=seed, fetch=False), events)
                extra[leg] = {"group_multiplicity": mg, "fired": float((gated["trigger"]["fired"] != 0).mean())}
            eng.configure_trigger()
        out["modes"][mode] = {"rates": legs, **extra}
    print(json.dumps(out), flush=True)


def profile(name: str, events: int) -> None:
    eng, config = _engine(name)
    eng.configure_traces(config, **MODES["partial"])
    eng.configure_trigger(group_multiplicity=1, **TRIGGER)
    eng.run_trigger(events, seed=1)
    eng.run_trigger(events, seed=1)


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--profile")
    ap.add_argument("--yardstick", default=str(ROOT / "attpc_engine_amd" / "_lib" / "libattpc_parent.so"))
    ap.add_argument("--events", type=int, default=65536)
    ap.add_argument("--deliver-events", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.events, args.deliver_events)
    if args.profile:
        return profile(args.profile, args.events)
    results = {}
    for name in args.workloads.split(","):
        for rep in range(args.reps):
            for library in ("yardstick", "own"):
                env = dict(os.environ)
                env.pop("ATTPC_HIP_LIBRARY", None)
                if library == "yardstick":
                    env["ATTPC_HIP_LIBRARY"] = args.yardstick
                cmd = [sys.executable, __file__, "--child", name, "--events", str(args.events), "--deliver-events",
                       str(args.deliver_events)]
                proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if proc.returncode != 0:  # a fault ends the measurement: nothing more is started on the device
                    sys.exit(f"child {library} {name} rep {rep} ended with {proc.returncode}:\n{proc.stderr[-2000:]}")
                line = json.loads(proc.stdout.strip().splitlines()[-1])
                line["rep"], line["which"] = rep, library
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                for mode, m in line["modes"].items():
                    for leg, rate in m["rates"].items():
                        results.setdefault((name, mode, library, leg), []).append(rate)
                    results[(name, mode, library, "info")] = m
    for name in args.workloads.split(","):
        for mode in MODES:
            def fig(library, leg):
                v = results.get((name, mode, library, leg))
                return (_median(v), min(v), max(v)) if v else None

            info = results[(name, mode, "own", "info")]
            print(f"## {name} / {mode}: {info['rows_per_event']:.1f} kept rows per event")
            for leg in ("traces", "rows", "traces_delivered", "trigger", "rows_trigger", "rows_gate_half", "rows_gate_tenth"):
                for library in ("yardstick", "own"):
                    f = fig(library, leg)
                    if f:
                        print(f"  {leg:18s} {library:9s} {f[0]:12.0f} events/s  ({f[1]:.0f} .. {f[2]:.0f})")
            for leg in ("traces", "rows"):
                own, yard = fig("own", leg), fig("yardstick", leg)
                print(f"  (i) {leg} without a trigger inside the yardstick's spread: {yard[1] <= own[0] <= yard[2]}"
                      f"  (own median {own[0]:.0f}, yardstick {yard[1]:.0f} .. {yard[2]:.0f})")
            cost_t = 1.0 / fig("own", "trigger")[0] - 1.0 / fig("own", "traces")[0]
            cost_r = 1.0 / fig("own", "rows_trigger")[0] - 1.0 / fig("own", "rows")[0]
            bytes_per_event = info["rows_per_event"] * TRACE_ROW_BYTES
            print(f"  cost of the stage per event: {cost_t * 1e6:.3f} us behind the traces, {cost_r * 1e6:.3f} us in the trace rows;"
                  f" one read of the kept rows is {bytes_per_event / 1e3:.1f} KB per event"
                  + (f" -> {bytes_per_event / cost_t / 1e12:.2f} TB/s over that cost" if cost_t > 0 else ""))
            print(f"  run_trigger against the yardstick's delivered run_traces: "
                  f"{fig('own', 'trigger')[0] / fig('yardstick', 'traces_delivered')[0]:.1f} x")
            for leg in ("rows_gate_half", "rows_gate_tenth"):
                print(f"  {leg} (Mg {info[leg]['group_multiplicity']}, {100 * info[leg]['fired']:.0f} % fire) against ungated rows with the"
                      f" trigger on: {fig('own', leg)[0] / fig('own', 'rows_trigger')[0]:.2f} x")


if __name__ == "__main__":
    main()
