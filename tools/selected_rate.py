"""Rate of selected delivery (attpc_sim_run_selected) against what a user must do without it -- deliver every event and
discard on the host -- with a yardstick build of the library (the parent commit's, built from a ``git worktree`` of it
with tools/build_variant.sh and kept beside this build's): one GPU, o16aa and be10dp.

  leg 1  the existing legs, yardstick against this build: run(fetch=False), run(fetch=True) into page-locked arrays,
         run_spyral and run_summary -- the mode costs nothing when unused (this build within the yardstick's min .. max);
  leg 2  run_selected of this build, cloud rows and Spyral rows, with cuts that accept about 100 %, 50 %, 10 % and 0 %
         of the events (n_pads at a quantile of a pilot's records), against the yardstick's full delivery of the same
         events: the 10 % and 0 % legs must be faster by more than the combined spread of the two; the 100 % leg's cost
         over plain delivery (the summary kernels) is reported;
  leg 3  this build's run_summary rate beside each selected leg: the ceiling.

Every (library, workload) measurement runs in a child process of its own (the library is chosen once per process,
ATTPC_HIP_LIBRARY); the children of the two libraries alternate, ``--reps`` times, so that drift of the machine hits
both alike.  Each child warms every leg up with one call (buffers settle) and times the next one, on other ids, wall
clock around a call that ends synchronised: a leg's figure is the median of ``--reps`` single timed calls, its spread
their minimum and maximum.  ``--out FILE`` appends the children's JSON lines.  ``--profile WORKLOAD`` is the program
for a kernel trace of one selected call at 10 % (``rocprofv3 --kernel-trace --stats -- python tools/selected_rate.py
--profile o16aa``, a run of its own).

    python tools/selected_rate.py [--yardstick attpc_engine_amd/_lib/libattpc_parent.so] [--events o16aa=1000000,be10dp=100000]
                                  [--deliver-events M] [--reps K] [--out FILE]
    python tools/selected_rate.py --child WORKLOAD --n N   (one measurement of the library ATTPC_HIP_LIBRARY names)
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

FRACTIONS = (100, 50, 10, 0)


def _engine(name):
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.engine import Engine

    ctx = _abi.Context(0)
    pipeline, config, indices = workloads.WORKLOADS[name]()
    return ctx, Engine(pipeline, config, indices, context=ctx)


def _cut(n_pads, percent):
    """n_pads >= the quantile of the pilot's n_pads that about ``percent`` % of its events reach."""
    import numpy as np

    from attpc_engine_amd import _abi

    if percent >= 100:
        return {}
    if percent <= 0:
        return {"n_pads": (_abi.NUM_PADS + 1, None)}
    return {"n_pads": (int(np.quantile(n_pads, 1.0 - percent / 100.0, method="higher")), None)}


def _timed(call, n):
    """One warm-up call, one timed call on other ids -> (seconds, what the timed call returned)."""
    call(0, n)
    t0 = time.perf_counter()
    result = call(n, n)
    return time.perf_counter() - t0, result


def child(name: str, events: int, deliver_events: int) -> None:
    from attpc_engine_amd import _abi

    ctx, eng = _engine(name)
    has_summary = all(hasattr(ctx.lib, symbol) for symbol in _abi.SUMMARY_SYMBOLS)
    has_select = all(hasattr(ctx.lib, symbol) for symbol in _abi.SELECT_SYMBOLS)
    seed, m = 1, deliver_events
    line = {"library": Path(os.environ["ATTPC_HIP_LIBRARY"]).name, "workload": name, "events": events, "delivered_events": m}
    t, res = _timed(lambda first, n: eng.run(n, seed=seed, first_event=first), events)
    line.update(resident_events_per_s=events / t, rows_per_event=res["stats"]["n_points"] / events)
    t, res = _timed(lambda first, n: eng.run(n, seed=seed, first_event=first, fetch=True, pinned=True, reuse_buffers=True), m)
    line.update(fetch_events_per_s=m / t, fetch_rows=int(res["offsets"][-1]))
    eng._out_cache = None
    t, res = _timed(lambda first, n: eng.run_spyral(n, seed=seed, first_event=first, pinned=True, reuse_buffers=True), m)
    line.update(spyral_events_per_s=m / t, spyral_rows=int(res["offsets"][-1]))
    eng._out_cache = None
    del res
    if has_summary:
        eng.configure_summary()
        t, res = _timed(lambda first, n: eng.run_summary(n, seed=seed, first_event=first), events)
        line.update(summary_events_per_s=events / t)
    if has_select:
        pilot = eng.run_summary(m, seed=seed, first_event=0)["events"]["n_pads"]
        for kind in ("cloud", "spyral"):
            for percent in FRACTIONS:
                eng.configure_selection(**_cut(pilot, percent))
                t, res = _timed(lambda first, n: eng.run_selected(n, seed=seed, first_event=first, rows=kind, pinned=True,
                                                                  reuse_buffers=True), m)
                line.update({f"selected_{kind}_{percent}_events_per_s": m / t,
                             f"selected_{kind}_{percent}_accepted": res["n_passed"] / m,
                             f"selected_{kind}_{percent}_rows": res["n_rows"]})
                del res
            eng._out_cache = None  # (the four legs of a kind share their page-locked arrays)
    print(json.dumps(line), flush=True)
    ctx.close()


def profile(name: str, events: int) -> None:
    """One warm-up call and one selected call (cloud rows, about 10 % accepted): the program of a kernel trace."""
    ctx, eng = _engine(name)
    eng.configure_summary()
    pilot = eng.run_summary(events, seed=1, first_event=0)["events"]["n_pads"]
    eng.configure_selection(**_cut(pilot, 10))
    t, res = _timed(lambda first, n: eng.run_selected(n, seed=1, first_event=first, pinned=True, reuse_buffers=True), events)
    print(json.dumps({"workload": name, "events": events, "accepted": res["n_passed"] / events,
                      "selected_events_per_s": events / t}))
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
    ap.add_argument("--deliver-events", type=int, default=16384, help="events per delivered / selected call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.n, args.deliver_events)
        return
    if args.profile:
        profile(args.profile, args.n or 16384)
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
        for key, label in (("resident_events_per_s", "run(fetch=False)"), ("fetch_events_per_s", "run(fetch=True, pinned)"),
                           ("spyral_events_per_s", "run_spyral"), ("summary_events_per_s", "run_summary")):
            (ym, ylo, yhi), (nm, nlo, nhi) = leg(yard, key), leg(new.name, key)
            verdict = "within" if ylo <= nm <= yhi else ("ABOVE" if nm > yhi else "BELOW")
            print(f"  leg 1  {label:24s} yardstick {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   this build {nm:10.0f} ({nlo:.0f} .. {nhi:.0f})"
                  f"   -> {verdict} the yardstick's spread")
        ceiling = leg(new.name, "summary_events_per_s")[0]
        for kind, base in (("cloud", "fetch_events_per_s"), ("spyral", "spyral_events_per_s")):
            ym, ylo, yhi = leg(yard, base)
            for percent in FRACTIONS:
                sm, slo, shi = leg(new.name, f"selected_{kind}_{percent}_events_per_s")
                accepted = leg(new.name, f"selected_{kind}_{percent}_accepted")[0]
                gain, combined = sm - ym, (yhi - ylo) + (shi - slo)
                verdict = "faster" if gain > combined else ("slower" if -gain > combined else "within")
                print(f"  leg 2  selected {kind:6s} {percent:3d} % (accepted {100 * accepted:5.1f} %) {sm:10.0f} ({slo:.0f} .. {shi:.0f})"
                      f"   yardstick full delivery {ym:10.0f} ({ylo:.0f} .. {yhi:.0f})   -> {sm / ym:.2f}x, {verdict} "
                      f"(difference {gain:.0f}, combined spread {combined:.0f}); ceiling run_summary {ceiling:.0f}")


if __name__ == "__main__":
    main()
