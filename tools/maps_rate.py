"""Rate of the run maps (attpc_sim_run_maps) against run_summary of the same library and ids, against what a user must
do without them -- deliver every cloud and histogram it in numpy -- and, for the paths that the maps do not touch,
against a yardstick build of the library (the parent commit's, built from a ``git worktree`` of it with
tools/build_variant.sh and kept beside this build's): one GPU, o16aa and be10dp.

  leg 1  the existing legs, yardstick against this build: run(fetch=False) and run_summary -- the mode costs nothing when
         unused (the difference of the medians inside the yardstick's own min .. max);
  leg 2  run_maps of this build (full mask; and of the events a cut on n_pads at the pilot's median keeps) against
         run_summary of this build, same ids: the cost of the mode;
  leg 3  run(fetch=True) into page-locked arrays followed by the numpy reduction of the delivered clouds (bincount on
         pads and buckets, np.unique on (event, pad) and (event, t)): the route the maps replace.

Every (library, workload) measurement runs in a child process of its own (the library is chosen once per process,
ATTPC_HIP_LIBRARY); the children of the two libraries alternate, ``--reps`` times, so that drift of the machine hits
both alike.  Each child warms every leg up with one call (buffers settle) and times the next one, on other ids, wall
clock around a call that ends synchronised: a leg's figure is the median of ``--reps`` single timed calls, its spread
their minimum and maximum.  ``--profile WORKLOAD`` is the program for a kernel trace of one maps call (``rocprofv3
--kernel-trace --stats -- python tools/maps_rate.py --profile o16aa``, a run of its own).

    python tools/maps_rate.py [--yardstick attpc_engine_amd/_lib/libattpc_parent.so] [--events o16aa=1000000,be10dp=100000]
                              [--deliver-events M] [--reps K] [--out FILE]
    python tools/maps_rate.py --child WORKLOAD --n N   (one measurement of the library ATTPC_HIP_LIBRARY names)
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


def _engine(name):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    ctx = _abi.Context(0)
    pipeline, config, indices = workloads.WORKLOADS[name]()
    return ctx, Engine(pipeline, config, indices, context=ctx)


def _timed(call, n):
    """One warm-up call, one timed call on other ids -> (seconds, what the timed call returned)."""
    call(0, n)
    t0 = time.perf_counter()
    result = call(n, n)
    return time.perf_counter() - t0, result


def numpy_maps(offsets, points, min_electrons):
    """The five maps of a delivered cloud in numpy, as a user without the mode would make them (every label counts)."""
    import numpy as np

    from attpc_engine_amd import _abi

    event = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    kept = points[:, 2] >= min_electrons
    event, pad, t = event[kept], points[kept, 0].astype(np.int64), points[kept, 1].astype(np.int64)
    q = points[kept, 2].astype(np.int64)
    pad_charge = np.zeros(_abi.NUM_PADS, dtype=np.int64)
    tb_charge = np.zeros(_abi.NUM_TB, dtype=np.int64)
    np.add.at(pad_charge, pad, q)  # (bincount's weights are f64: not exact beyond 2^53)
    np.add.at(tb_charge, t, q)
    return {"pad_events": np.bincount(np.unique(event * _abi.NUM_PADS + pad) % _abi.NUM_PADS, minlength=_abi.NUM_PADS),
            "tb_events": np.bincount(np.unique(event * _abi.NUM_TB + t) % _abi.NUM_TB, minlength=_abi.NUM_TB),
            "tb_rows": np.bincount(t, minlength=_abi.NUM_TB), "pad_charge": pad_charge, "tb_charge": tb_charge}


def child(name: str, events: int, deliver_events: int) -> None:
    import numpy as np

    from attpc_engine_amd import _abi
    from attpc_engine_amd.detector.summary import electrons_above_threshold

    ctx, eng = _engine(name)
    has_maps = all(hasattr(ctx.lib, symbol) for symbol in _abi.MAPS_SYMBOLS)
    seed, m = 1, deliver_events
    line = {"library": Path(os.environ["ATTPC_HIP_LIBRARY"]).name, "workload": name, "events": events, "delivered_events": m}
    t, res = _timed(lambda first, n: eng.run(n, seed=seed, first_event=first), events)
    line.update(resident_events_per_s=events / t, rows_per_event=res["stats"]["n_points"] / events)
    eng.configure_summary()
    t, res = _timed(lambda first, n: eng.run_summary(n, seed=seed, first_event=first), events)
    line.update(summary_events_per_s=events / t)
    median_pads = int(np.median(res["events"]["n_pads"]))
    if has_maps:
        eng.configure_maps(other_labels=True)
        t, res = _timed(lambda first, n: eng.run_maps(n, seed=seed, first_event=first), events)
        line.update(maps_events_per_s=events / t, maps_n_hit=res["maps"].n_hit, maps_rows=int(res["maps"].tb_rows.sum()))
        eng.configure_selection(n_pads=(median_pads, None))
        eng.configure_maps(other_labels=True, selected=True)
        t, res = _timed(lambda first, n: eng.run_maps(n, seed=seed, first_event=first), events)
        line.update(maps_selected_events_per_s=events / t, maps_selected_accepted=res["maps"].n_events / events)
        # the numpy route on m events: delivery, then the reduction; the maps of the same ids for the comparison
        threshold = electrons_above_threshold(eng.config)
        fetch = lambda first, n: eng.run(n, seed=seed, first_event=first, fetch=True, pinned=True, reuse_buffers=True)  # noqa: E731
        fetch(0, m)
        t0 = time.perf_counter()
        cloud = fetch(m, m)
        t1 = time.perf_counter()
        host = numpy_maps(cloud["offsets"], cloud["points"], threshold)
        t2 = time.perf_counter()
        eng.configure_maps(other_labels=True)
        device = eng.run_maps(m, seed=seed, first_event=m)["maps"]
        same = all(np.array_equal(host[key], getattr(device, key)) for key in host)
        line.update(fetch_events_per_s=m / (t1 - t0), numpy_events_per_s=m / (t2 - t1), numpy_route_events_per_s=m / (t2 - t0),
                    numpy_equals_device=bool(same))
    print(json.dumps(line), flush=True)
    ctx.close()


def profile(name: str, events: int) -> None:
    """One warm-up call and one maps call (full mask): the program of a kernel trace."""
    ctx, eng = _engine(name)
    eng.configure_summary()
    eng.configure_maps(other_labels=True)
    t, res = _timed(lambda first, n: eng.run_maps(n, seed=1, first_event=first), events)
    print(json.dumps({"workload": name, "events": events, "maps_events_per_s": events / t, "n_hit": res["maps"].n_hit}))
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
    ap.add_argument("--events", default="o16aa=1000000,be10dp=100000", help="events per resident / summary / maps call")
    ap.add_argument("--deliver-events", type=int, default=16384, help="events of the delivered call of the numpy route")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n, args.deliver_events)
        return
    if args.profile:
        profile(args.profile, args.n or 200_000)
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
                                       str(min(args.deliver_events, n))], env=env, capture_output=True, text=True, timeout=600)
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
                                f.write(json.dumps(line) + "\n")
    yard = libraries[0].name
    print(f"\nmedian (min .. max) of {args.reps} alternating repeats, events/s; yardstick = {yard}")
    for name in events:
        def leg(lib, key):
            return _spread([ln[key] for ln in lines if (ln["library"], ln["workload"]) == (lib, name)])

        print(f"{name}:")
        for key, label in (("resident_events_per_s", "run(fetch=False)"), ("summary_events_per_s", "run_summary")):
            (ym, ylo, yhi), (nm, nlo, nhi) = leg(yard, key), leg(new.name, key)
            verdict = "inside" if abs(nm - ym) <= yhi - ylo else "OUTSIDE"
            print(f"  leg 1  {label:18s} yardstick {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   this build {nm:10.0f} ({nlo:.0f} .. {nhi:.0f})"
                  f"   difference {nm - ym:+.0f}, {verdict} the yardstick's spread of {yhi - ylo:.0f}")
        sm = leg(new.name, "summary_events_per_s")[0]
        for key, label in (("maps_events_per_s", "run_maps"), ("maps_selected_events_per_s", "run_maps, selected"),
                           ("fetch_events_per_s", "run(fetch=True)"), ("numpy_events_per_s", "numpy reduction alone"),
                           ("numpy_route_events_per_s", "delivery + numpy")):
            m, lo, hi = leg(new.name, key)
            print(f"  {'leg 2' if key.startswith('maps') else 'leg 3'}  {label:22s} {m:10.0f} ({lo:.0f} .. {hi:.0f})   {m / sm:.3f} of run_summary ({sm:.0f})")
        print(f"         accepted by the cut {leg(new.name, 'maps_selected_accepted')[0]:.3f}; numpy maps equal the device's: "
              f"{all(ln['numpy_equals_device'] for ln in lines if (ln['library'], ln['workload']) == (new.name, name))}")


if __name__ == "__main__":
    main()
