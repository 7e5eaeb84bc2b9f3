"""Rate of the summary run (attpc_sim_run_summary) against the two ways to the same numbers that exist without it, with
a yardstick build of the library (the parent commit's, built from a ``git worktree`` of it with tools/build_variant.sh
and kept beside this build's): one GPU, o16aa and be10dp.

  leg 1  run(fetch=False), yardstick against this build: the mode costs nothing when unused (this build within the
         yardstick's spread);
  leg 2  run_summary of this build against the yardstick's run(fetch=True, pinned=True, reuse_buffers=True) -- the
         clouds delivered to page-locked host arrays, the host-side reduction not even counted: run_summary must be
         faster by more than the spread of the repeats;
  leg 3  run_summary as a fraction of leg 1 (reported).

Every (library, workload) measurement runs in a child process of its own (the library is chosen once per process,
ATTPC_HIP_LIBRARY); the children of the two libraries alternate, ``--reps`` times, so that drift of the machine hits
both alike.  Each child warms every leg up with one call (buffers settle) and times the next one, on other ids: a
leg's figure is the median of ``--reps`` single timed calls, its spread their minimum and maximum.  ``--out FILE``
appends the children's JSON lines.  ``--profile WORKLOAD`` is the program for a kernel trace of one summary call
(``rocprofv3 --kernel-trace --stats -- python tools/summary_rate.py --profile o16aa``, a run of its own).

    python tools/summary_rate.py [--yardstick attpc_engine_amd/_lib/libattpc_parent.so] [--events o16aa=1000000,be10dp=100000]
                                 [--deliver-events M] [--reps K] [--out FILE]
    python tools/summary_rate.py --child WORKLOAD --n N   (one measurement of the library ATTPC_HIP_LIBRARY names)
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

RECORD_BYTES = {"event": 32, "track": 80}


def _engine(name):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    ctx = _abi.Context(0)
    pipeline, config, indices = workloads.WORKLOADS[name]()
    return ctx, Engine(pipeline, config, indices, context=ctx)


def child(name: str, events: int, deliver_events: int) -> None:
    from attpc_engine_amd import _abi

    ctx, eng = _engine(name)
    has_summary = all(hasattr(ctx.lib, symbol) for symbol in _abi.SUMMARY_SYMBOLS)
    seed = 1

    def timed(call, n):
        """One warm-up call, one timed call on other ids -> (seconds, what the timed call returned)."""
        call(0, n)
        t0 = time.perf_counter()
        result = call(n, n)
        return time.perf_counter() - t0, result

    line = {"library": Path(os.environ["ATTPC_HIP_LIBRARY"]).name, "workload": name, "events": events,
            "delivered_events": deliver_events}
    t, res = timed(lambda first, n: eng.run(n, seed=seed, first_event=first), events)
    rows_per_event = res["stats"]["n_points"] / events
    line.update(resident_events_per_s=events / t, rows_per_event=rows_per_event, cloud_bytes_per_event=rows_per_event * 32)
    t, res = timed(lambda first, n: eng.run(n, seed=seed, first_event=first, fetch=True, pinned=True, reuse_buffers=True),
                   deliver_events)
    line.update(fetch_events_per_s=deliver_events / t, fetch_GB_per_s=int(res["offsets"][-1]) * 32 / t / 1e9)
    eng._out_cache = None
    del res
    if has_summary:
        eng.configure_summary()
        t, res = timed(lambda first, n: eng.run_summary(n, seed=seed, first_event=first), events)
        n_sim = res["tracks"].shape[1]
        line.update(summary_events_per_s=events / t, kept_per_event=float(res["events"]["n_kept"].mean()),
                    pads_per_event=float(res["events"]["n_pads"].mean()),
                    record_bytes_per_event=RECORD_BYTES["event"] + n_sim * RECORD_BYTES["track"],
                    samples_per_event=res["stats"]["n_track_samples"] / events)
    print(json.dumps(line), flush=True)
    ctx.close()


def profile(name: str, events: int) -> None:
    """One warm-up call and one summary call: the program of a kernel trace."""
    ctx, eng = _engine(name)
    eng.configure_summary()
    eng.run_summary(events, seed=1, first_event=0)
    t0 = time.perf_counter()
    eng.run_summary(events, seed=1, first_event=events)
    print(json.dumps({"workload": name, "events": events, "summary_events_per_s": events / (time.perf_counter() - t0)}))
    ctx.close()


def _spread(values):
    values = sorted(values)
    return values[len(values) // 2], values[0], values[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--profile", default=None)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--yardstick", default=str(ROOT / "attpc_engine_amd" / "_lib" / "libattpc_parent.so"))
    ap.add_argument("--events", default="o16aa=1000000,be10dp=100000", help="events per resident / summary call")
    ap.add_argument("--deliver-events", type=int, default=16384, help="events per delivered call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n, args.deliver_events)
        return
    if args.profile:
        profile(args.profile, args.n or 1000000)
        return

    new = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
    libraries = [Path(args.yardstick).resolve(), new]
    for lib in libraries:
        if not lib.exists():
            raise SystemExit(f"{lib} is missing (tools/build_variant.sh builds a yardstick from another checkout)")
    events = {name: int(n) for name, n in (item.split("=") for item in args.events.split(","))}
    lines = []
    for rep in range(args.reps):
        for lib in libraries:
            for name, n in events.items():
                env = dict(os.environ, ATTPC_HIP_LIBRARY=str(lib))
                proc = subprocess.run([sys.executable, __file__, "--child", name, "--n", str(n), "--deliver-events",
                                       str(min(args.deliver_events, n))], env=env, capture_output=True, text=True, timeout=300)
                if proc.returncode != 0:  # nothing more is started on the GPU after a failure
                    sys.stderr.write(proc.stdout + proc.stderr)
                    raise SystemExit(f"{lib.name} / {name} ended with status {proc.returncode}")
                for text in proc.stdout.splitlines():
                    if text.startswith("{"):
                        line = dict(json.loads(text), rep=rep)
                        lines.append(line)
                        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    yard = libraries[0].name
    print(f"\nmedian (min .. max) of {args.reps} alternating repeats, events/s; yardstick = {yard}")
    for name in events:
        def leg(lib, key):
            return [ln[key] for ln in lines if (ln["library"], ln["workload"]) == (lib, name)]

        some = next(ln for ln in lines if (ln["library"], ln["workload"]) == (new.name, name))
        print(f"{name}: {some['rows_per_event']:.0f} cloud rows = {some['cloud_bytes_per_event'] / 1e3:.1f} KB per event, "
              f"{some['kept_per_event']:.0f} kept on {some['pads_per_event']:.0f} pads; records {some['record_bytes_per_event']} B per event")
        (ym, ylo, yhi), (nm, nlo, nhi) = _spread(leg(yard, "resident_events_per_s")), _spread(leg(new.name, "resident_events_per_s"))
        (fm, flo, fhi), (sm, slo, shi) = _spread(leg(yard, "fetch_events_per_s")), _spread(leg(new.name, "summary_events_per_s"))
        print(f"  leg 1  run(fetch=False)   yardstick {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   this build {nm:10.0f} ({nlo:.0f} .. {nhi:.0f})"
              f"   -> {'within' if nhi >= ylo and nlo <= yhi else 'OUTSIDE'} the spread")
        print(f"  leg 2  yardstick run(fetch=True, pinned) {fm:10.0f} ({flo:.0f} .. {fhi:.0f})   run_summary {sm:10.0f} ({slo:.0f} .. {shi:.0f})"
              f"   -> {'faster' if slo > fhi else 'NOT faster'} by more than the spread ({sm / fm:.1f}x)")
        print(f"  leg 3  run_summary / run(fetch=False) of this build = {sm / nm:.3f}")


if __name__ == "__main__":
    main()
