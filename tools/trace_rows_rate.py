"""Rate of the trace rows (attpc_sim_run_trace_rows) against the pad traces they are made of (attpc_sim_run_traces) at
identical settings, and of the traces against a yardstick build of the library (the parent commit's, built beside
this one with tools/build_variant.sh): one GPU, o16aa and be10dp, three trace modes -- hit mode without noise, hit mode
with sigma = 5 and pedestals, partial readout (sigma = 5, threshold 20) -- device-resident and delivered into
page-locked host arrays.

Every (library, workload) measurement runs in a child process of its own (the library is chosen once per process,
ATTPC_HIP_LIBRARY); the children of the two libraries alternate, ``--reps`` times, so that drift of the machine hits
both alike.  Each child warms every leg up with one call (buffers settle) and times the next one: a leg's figure is
the median of ``--reps`` single timed calls, its spread their minimum and maximum.  The driver prints,
per workload and mode, the median and the spread (min .. max) of every leg and the two verdicts:
  (i)  run_traces of this build stays within the spread of the yardstick's, resident and delivered;
  (ii) run_trace_rows delivered is faster than the yardstick's run_traces delivered by more than the spread.
A library with the Fourier baseline (attpc_trace_configure_baseline) gets one more leg: run_trace_rows resident with
the stage on (``--baseline-scale``), beside the same call with it off: off before on in the even repeats, on before
off in the odd ones (``--baseline-first``), so that order, clock and warm-up do not all fall on one side.  When the yardstick has the trace rows too
(the parent commit of the baseline stage) the driver adds
  (iii) run_trace_rows resident with the stage off stays within the spread of the yardstick's;
  and the cost of the stage per event, 1 / rate(on) - 1 / rate(off), from the medians.
A library with the micromegas gain (attpc_trace_configure_gain) gets two more legs: run_traces and run_trace_rows
resident with the stage on (``--gain-theta``, a Polya gain with a gain map of its own), after the legs with it off in
the even repeats and before them in the odd ones, as the baseline leg; the driver prints the cost of the stage per
event from the medians.  (i) and (iii) are the verdicts on the stage being off.
``--modes`` picks the trace modes, ``--resident-only`` leaves the delivered legs out.
``--out FILE`` appends the children's JSON lines.

    python tools/trace_rows_rate.py [--yardstick attpc_engine_amd/_lib/libattpc_parent.so] [--events N]
                                    [--deliver-events M] [--reps K] [--workloads o16aa,be10dp] [--out FILE]
                                    [--modes hit,partial] [--resident-only] [--baseline-scale S] [--gain-theta T]
    python tools/trace_rows_rate.py --child WORKLOAD   (one measurement of the library ATTPC_HIP_LIBRARY names, or of
                                                        the package's own without it)
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
    "hit_noise": {"noise_sigma": 5.0, "pedestals": 300},
    "partial": {"noise_sigma": 5.0, "pedestals": 300, "threshold": 20.0, "readout": "partial"},
}
TRACE_ROW_BYTES = 512 * 2 + 4 + 8
ROW_BYTES = 8 * 8 + 8


def child(name: str, events: int, deliver_events: int, modes, resident_only: bool, baseline_scale: float,
          baseline_first: bool, gain_theta: float) -> None:
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine
    from attpc_engine_amd.outputs import RowArrays, TraceArrays

    ctx = _abi.Context(0)
    lib, seed = ctx.lib, 1
    # (the yardstick is a build of the same ABI version from before the trace rows: the binding loads it without them)
    has_rows = all(hasattr(lib, name) for name in _abi.TRACE_ROW_SYMBOLS)
    has_baseline = has_rows and all(hasattr(lib, name) for name in _abi.BASELINE_SYMBOLS)
    has_gain = has_rows and all(hasattr(lib, name) for name in _abi.GAIN_SYMBOLS)
    pipeline, config, indices = workloads.WORKLOADS[name]()
    eng = Engine(pipeline, config, indices, context=ctx)
    if has_rows:
        eng.configure_spyral(config)
        eng.configure_peaks()

    def timed(call, n):
        """One warm-up call, one timed call on other ids -> (seconds, what the timed call returned)."""
        call(0, n)
        t0 = time.perf_counter()
        result = call(n, n)
        return time.perf_counter() - t0, result

    for mode in modes:
        kw = MODES[mode]
        eng.configure_traces(config, **kw)
        line = {"library": _abi.library_path().name, "workload": name, "mode": mode,
                "resident_events": events, "delivered_events": deliver_events}

        def traces_resident(first, n):
            out, stats = _abi.TraceOut(), _abi.RunStats()
            ctx.check(lib.attpc_sim_run_traces(ctx.handle, seed, first, n, eng.layout, None, None, None, out, stats),
                      "attpc_sim_run_traces")
            return int(out.n_rows)

        def gain_leg(call, key):  # the same call with the micromegas gain on, then off again for what follows
            import numpy as np

            pad_gain = np.random.default_rng(1).uniform(0.8, 1.2, size=_abi.NUM_PADS)
            eng.configure_gain(theta=gain_theta, pad_gain=pad_gain)
            t, rows = timed(call, events)
            eng.configure_gain()
            line.update({f"{key}_gain_resident_events_per_s": events / t, f"{key}_gain_per_event": rows / events,
                         "gain_theta": gain_theta, "gain_first": baseline_first})

        if has_gain and baseline_first:
            gain_leg(traces_resident, "traces")
        t, rows = timed(traces_resident, events)
        if has_gain and not baseline_first:
            gain_leg(traces_resident, "traces")
        per_event = rows / events
        line.update(traces_resident_events_per_s=events / t, trace_rows_per_event=per_event,
                    trace_bytes_per_event=per_event * TRACE_ROW_BYTES)
        if not resident_only:
            arrays = TraceArrays(deliver_events, int(per_event * deliver_events * 1.3) + 4096, ctx.pinned_empty)

            def traces_delivered(first, n):
                stats = _abi.RunStats()
                ctx.check(lib.attpc_sim_run_traces(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats),
                          "attpc_sim_run_traces")
                return int(arrays.out.n_rows)

            t, rows = timed(traces_delivered, deliver_events)
            line.update(traces_delivered_events_per_s=deliver_events / t,
                        traces_delivered_GB_per_s=rows * TRACE_ROW_BYTES / t / 1e9)
            del arrays
        if has_rows:
            def rows_resident(first, n):
                out, stats = _abi.CloudOut(), _abi.RunStats()
                ctx.check(lib.attpc_sim_run_trace_rows(ctx.handle, seed, first, n, eng.layout, None, None, None, out, stats),
                          "attpc_sim_run_trace_rows")
                return int(stats.n_points)

            def baseline_leg():  # the same call with the Fourier baseline on, then off again for what follows
                eng.configure_baseline(window_scale=baseline_scale)
                t, rows = timed(rows_resident, events)
                eng.configure_baseline(None)
                line.update(rows_baseline_resident_events_per_s=events / t, rows_baseline_per_event=rows / events,
                            baseline_scale=baseline_scale, baseline_first=baseline_first)

            if has_baseline and baseline_first:
                baseline_leg()
            if has_gain and baseline_first:
                gain_leg(rows_resident, "rows")
            t, rows = timed(rows_resident, events)
            per_event = rows / events
            line.update(rows_resident_events_per_s=events / t, rows_per_event=per_event,
                        row_bytes_per_event=per_event * ROW_BYTES)
            if has_baseline and not baseline_first:
                baseline_leg()
            if has_gain and not baseline_first:
                gain_leg(rows_resident, "rows")
            if not resident_only:
                row_arrays = RowArrays(deliver_events, int(per_event * deliver_events * 1.3) + 4096, ctx.pinned_empty, width=8)

                def rows_delivered(first, n):
                    stats = _abi.RunStats()
                    ctx.check(lib.attpc_sim_run_trace_rows(ctx.handle, seed, first, n, eng.layout, None, None, None,
                                                           row_arrays.out, stats), "attpc_sim_run_trace_rows")
                    return int(stats.n_points)

                t, rows = timed(rows_delivered, deliver_events)
                line.update(rows_delivered_events_per_s=deliver_events / t, rows_delivered_GB_per_s=rows * ROW_BYTES / t / 1e9)
                del row_arrays
        print(json.dumps(line), flush=True)
    ctx.close()


def _spread(values):
    values = sorted(values)
    return values[len(values) // 2], values[0], values[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--yardstick", default=str(ROOT / "attpc_engine_amd" / "_lib" / "libattpc_parent.so"))
    ap.add_argument("--events", type=int, default=131072, help="events per device-resident call")
    ap.add_argument("--deliver-events", type=int, default=16384, help="events per delivered call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--resident-only", action="store_true")
    ap.add_argument("--baseline-scale", type=float, default=20.0)
    ap.add_argument("--baseline-first", action="store_true", help="child: the baseline leg before the leg without it")
    ap.add_argument("--gain-theta", type=float, default=0.5, help="Polya parameter of the legs with the micromegas gain on")
    args = ap.parse_args()
    modes = args.modes.split(",")
    if any(m not in MODES for m in modes):
        raise SystemExit(f"--modes takes {list(MODES)}")
    if args.child:
        child(args.child, args.events, args.deliver_events, modes, args.resident_only, args.baseline_scale,
              args.baseline_first, args.gain_theta)
        return

    new = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
    libraries = [Path(args.yardstick).resolve(), new]
    for lib in libraries:
        if not lib.exists():
            raise SystemExit(f"{lib} is missing (tools/build_variant.sh builds a yardstick from another checkout)")
    lines = []
    for rep in range(args.reps):
        for lib in libraries:
            for name in args.workloads.split(","):
                env = dict(os.environ, ATTPC_HIP_LIBRARY=str(lib))
                proc = subprocess.run([sys.executable, __file__, "--child", name, "--events", str(args.events),
                                       "--deliver-events", str(args.deliver_events), "--modes", args.modes,
                                       "--baseline-scale", str(args.baseline_scale), "--gain-theta", str(args.gain_theta)]
                                      + (["--resident-only"] if args.resident_only else [])
                                      + (["--baseline-first"] if rep % 2 else []), env=env, capture_output=True,
                                      text=True, timeout=300)
                if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                    sys.stderr.write(proc.stdout + proc.stderr)
                    raise SystemExit(f"{lib.name} / {name} ended with status {proc.returncode}")
                for text in proc.stdout.splitlines():
                    if text.startswith("{"):
                        # (the side, not the file name, tells the libraries apart: both may be a libattpc_hip.so)
                        line = dict(json.loads(text), rep=rep, side="yardstick" if lib is libraries[0] else "new")
                        lines.append(line)
                        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    yard = libraries[0].name
    print(f"\nmedian (min .. max) of {args.reps} alternating repeats, events/s; yardstick = {yard}")
    for name in args.workloads.split(","):
        for mode in modes:
            def leg(lib, key):
                return [ln[key] for ln in lines if (ln["side"], ln["workload"], ln["mode"]) == (lib, name, mode)
                        and key in ln]

            some = next(ln for ln in lines if (ln["side"], ln["workload"], ln["mode"]) == ("new", name, mode))
            print(f"{name} / {mode}: {some['trace_rows_per_event']:.1f} trace rows = {some['trace_bytes_per_event'] / 1e3:.1f} KB"
                  f" per event; {some['rows_per_event']:.1f} rows = {some['row_bytes_per_event'] / 1e3:.1f} KB per event")
            verdicts = []
            for what in ("resident",) if args.resident_only else ("resident", "delivered"):
                key = f"traces_{what}_events_per_s"
                (ym, ylo, yhi), (nm, nlo, nhi) = _spread(leg("yardstick", key)), _spread(leg("new", key))
                rm, rlo, rhi = _spread(leg("new", f"rows_{what}_events_per_s"))
                print(f"  {what:9s} traces yardstick {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   traces {nm:10.0f} ({nlo:.0f} .. {nhi:.0f})"
                      f"   rows {rm:10.0f} ({rlo:.0f} .. {rhi:.0f})")
                verdicts.append(f"(i) {what}: {'within' if nhi >= ylo and nlo <= yhi else 'OUTSIDE'} the spread")
                if what == "delivered":
                    verdicts.append(f"(ii) rows delivered {'faster than' if rlo > yhi else 'NOT faster than'} the yardstick's"
                                    f" traces delivered by more than the spread ({rm / ym:.2f}x)")
            off, on = leg("new", "rows_resident_events_per_s"), leg("new", "rows_baseline_resident_events_per_s")
            yard_rows = leg("yardstick", "rows_resident_events_per_s")
            if yard_rows:
                (ym, ylo, yhi), (nm, nlo, nhi) = _spread(yard_rows), _spread(off)
                print(f"  resident  rows yardstick {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   rows, baseline off {nm:10.0f} ({nlo:.0f} .. {nhi:.0f})")
                verdicts.append(f"(iii) rows resident, baseline off: {'within' if nhi >= ylo and nlo <= yhi else 'OUTSIDE'} the spread")
            if on:
                (fm, flo, fhi), (nm, _, _) = _spread(on), _spread(off)
                print(f"  resident  rows, baseline on {fm:10.0f} ({flo:.0f} .. {fhi:.0f}): {1e6 / fm - 1e6 / nm:+.2f} us per event")
            for key, plain in (("traces", "traces_resident_events_per_s"), ("rows", "rows_resident_events_per_s")):
                gained = leg("new", f"{key}_gain_resident_events_per_s")
                if gained:
                    (gm, glo, ghi), (nm, _, _) = _spread(gained), _spread(leg("new", plain))
                    print(f"  resident  {key}, gain on {gm:10.0f} ({glo:.0f} .. {ghi:.0f}): {1e6 / gm - 1e6 / nm:+.2f} us per event")
            print("  " + "; ".join(verdicts))


if __name__ == "__main__":
    main()
