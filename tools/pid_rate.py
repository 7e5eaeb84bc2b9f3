"""Cost and quality of the particle identification (attpc_trace_configure_pid): one GPU, o16aa and be10dp
in partial readout with sigma = 5, pedestals and threshold 20, the settings of tools/cluster_rate.py's r31 / r32 runs:
estimates with ``--min-points`` points, thinning at ``--thinning`` mm, geometric circle fit and helix slope on, clustering
at its defaults with the joining at ``--radius-ratio`` in every leg.

Gates: ``Gate.from_band`` (``--bins``, ``--coverage-lo``, ``--coverage-hi``) per position on the estimates of a run of
``--stats-events`` events with ``match="truth"`` and ANOTHER seed (3) than every measured run (1 and 2).
(a) Cost: ``run_estimates`` of ``--events`` events in ``match="rank"``, the identification off and on alternating, with
the track fit off and with it on; ``--reps`` timed calls each behind one warm-up call of each kind; a leg's figure is the
median of its timed calls, its spread their minimum and maximum.
(b) Identification, per position p, on ``--stats-events`` events in ``match="rank"`` (seed 2): of the ranked clusters
whose truth majority is p and that are complete and pure to 0.9, the share the identification assigns to p (and to
another position, and to none); of the slots assigned to p, the share whose majority is another position.
(c) Outcome: the fit's B rho and kinetic energy against the kinematics, median and half the 16 .. 84 % range, per
position, for ``match="truth"``, for ``match="rank"`` alone (slot k taken for position k) and for ``match="rank"`` with
the identification (``by_position``), on the same events.
Reported values for the settings used, no limits.

    python tools/pid_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
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
SETTINGS = ("events", "min_points", "thinning", "peak_threshold", "peak_prominence", "radius_ratio", "bins", "coverage_lo",
            "coverage_hi", "time_step", "max_steps", "max_evaluations")


def _engine(name: str, args):
    import numpy as np

    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.WORKLOADS[name]()
    eng = Engine(pipeline, config, indices, context=_abi.Context(0))
    eng.configure_traces(config, offset=int(np.argmax(get_response(config))), **PARTIAL)
    peaks = {k: v for k, v in (("threshold", args.peak_threshold), ("prominence", args.peak_prominence)) if v is not None}
    eng.configure_peaks(**peaks)
    eng.configure_estimates(min_points=args.min_points)
    eng.configure_thinning(z_step=args.thinning)
    eng.configure_circle_fit()
    eng.configure_helix_slope()
    eng.configure_cluster_join(radius_ratio=args.radius_ratio or None)
    return eng, pipeline, indices


def _fit(args):
    from attpc_engine_amd.detector.fit import TrackFitSettings

    return TrackFitSettings(time_step=args.time_step, max_steps=args.max_steps, max_evaluations=args.max_evaluations)


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def _spread(values):
    import numpy as np

    values = values[np.isfinite(values)]
    if len(values) == 0:
        return [0, None, None]
    lo, mid, hi = np.percentile(values, [16.0, 50.0, 84.0])
    return [int(len(values)), float(mid), float(0.5 * (hi - lo))]


def calibrate(eng, indices, args):
    """The gates of every position from a run with match="truth" and seed 3 (None where the band cannot be made)."""
    import numpy as np

    from attpc_engine_amd.detector.pid import Gate

    eng.configure_clustering(match="truth")
    eng.configure_track_fit()
    eng.configure_pid()
    est, done = [], 0
    while done < args.stats_events:
        est.append(eng.run_estimates(args.events, seed=3, first_event=done)["estimates"])
        done += args.events
    est = np.concatenate(est)
    gates, info = [], []
    for p in range(len(indices)):
        with np.errstate(invalid="ignore"):
            usable = int((np.isfinite(est["brho"][:, p]) & np.isfinite(est["dedx"][:, p]) & (est["brho"][:, p] > 0) & (est["dedx"][:, p] > 0)).sum())
        try:
            gates.append(Gate.from_band(est["brho"][:, p], est["dedx"][:, p], bins=args.bins, coverage=(args.coverage_lo, args.coverage_hi)))
        except ValueError:
            gates.append(None)
        g = gates[-1]
        info.append({"position": p, "records": usable, "vertices": None if g is None else len(g),
                     "brho_range": None if g is None else [float(g.vertices[:, 0].min()), float(g.vertices[:, 0].max())],
                     "dedx_range": None if g is None else [float(g.vertices[:, 1].min()), float(g.vertices[:, 1].max())],
                     "own_share": None if g is None else float(g.contains(est["brho"][:, p], est["dedx"][:, p]).sum() / max(usable, 1)),
                     "holds_share_of_position": [None if g is None else float(g.contains(est["brho"][:, q], est["dedx"][:, q]).sum() / max(
                         int(np.isfinite(est["brho"][:, q]).sum()), 1)) for q in range(len(indices))]})
    return gates, {"events": done, "gates": info}


def rates(eng, gates, args) -> dict:
    out = {}
    eng.configure_clustering(match="rank")
    for fit_on in (False, True):
        eng.configure_track_fit(_fit(args) if fit_on else None)
        legs = {"off": [], "on": []}
        fitted = {}

        def call(on: bool):
            eng.configure_pid(gates if on else None)
            t0 = time.perf_counter()
            res = eng.run_estimates(args.events, seed=1)
            rate = args.events / (time.perf_counter() - t0)
            if fit_on:
                fitted["on" if on else "off"] = int((res["fits"]["evaluations"] > 0).sum())
            return rate

        for on in (False, True):
            call(on)
        for _ in range(args.reps):
            for on in (False, True):
                legs["on" if on else "off"].append(call(on))
        leg = {k: [_median(v), min(v), max(v)] for k, v in legs.items()}
        leg["calls"] = legs
        leg["cost_share"] = 1.0 - leg["on"][0] / leg["off"][0]
        leg["seconds_per_event"] = 1.0 / leg["on"][0] - 1.0 / leg["off"][0]
        if fit_on:
            leg["tracks_fitted"] = fitted
        out["fit_on" if fit_on else "fit_off"] = leg
    eng.configure_pid()
    eng.configure_track_fit()
    return out


def quality(eng, pipeline, indices, gates, args) -> dict:
    import numpy as np

    from attpc_engine_amd import nuclear_map
    from attpc_engine_amd.detector import estimate
    from attpc_engine_amd.detector.pid import STATUS_BITS, by_position

    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    n_sim = len(indices)
    eng.configure_track_fit(_fit(args))
    legs = {"truth": ("truth", False), "rank": ("rank", False), "rank_pid": ("rank", True)}
    fits = {k: [] for k in legs}
    pids, events, records, brho_true, ke_true = [], [], [], [], []
    t0, done = time.perf_counter(), 0
    while done < args.stats_events:
        for leg, (match, pid_on) in legs.items():
            eng.configure_clustering(match=match)
            eng.configure_pid(gates if pid_on else None)
            res = eng.run_estimates(args.events, seed=2, first_event=done)
            fits[leg].append(res["fits"])
        pids.append(res["pid"])
        events.append(res["clusters"][0])
        records.append(res["clusters"][1][:, :n_sim])
        brho_true.append(estimate.truth_tracks(res["p4"], indices, z)["brho"])
        p4 = res["p4"][:, [int(i) for i in indices]]
        ke_true.append(p4[..., 3] - np.sqrt(np.maximum(p4[..., 3] ** 2 - (p4[..., :3] ** 2).sum(axis=-1), 0.0)))
        done += args.events
    eng.configure_pid()
    eng.configure_track_fit()
    eng.configure_clustering()
    fits = {k: np.concatenate(v) for k, v in fits.items()}
    pid, events, records = np.concatenate(pids), np.concatenate(events), np.concatenate(records)
    brho_true, ke_true = np.concatenate(brho_true), np.concatenate(ke_true)
    fits["rank_pid"], slot_of = by_position(fits["rank_pid"], pid)
    out = {"events": done, "seconds": time.perf_counter() - t0, "positions": []}
    out["status_share"] = {name: float((pid["status"] & bit != 0).mean()) for name, bit in STATUS_BITS.items()}
    out["status_share"]["assigned"] = float((pid["position"] >= 0).mean())
    # the ranked clusters: majority, purity and completeness from the cluster records (tests/cluster_reference.py's scores)
    majority = records["majority"]
    used = records["first_row"] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        purity = records["majority_rows"] / records["rows"]
        truth_rows = np.take_along_axis(events["truth_rows"].astype(np.int64), np.maximum(majority, 0), axis=1)
        completeness = records["majority_rows"] / truth_rows
    good = used & (majority >= 0) & (purity >= 0.9) & (completeness >= 0.9)
    for p in range(n_sim):
        mine = good & (majority == p)
        assigned = pid["position"] == p
        row = {"position": p, "row": int(indices[p]), "Z": int(z[int(indices[p])]), "A": int(a[int(indices[p])]),
               "mass": float(nuclear_map.get_data(int(z[int(indices[p])]), int(a[int(indices[p])])).mass),
               "good_clusters": int(mine.sum()),
               "good_assigned_to_it": float((mine & assigned).sum() / max(mine.sum(), 1)),
               "good_assigned_elsewhere": float((mine & (pid["position"] >= 0) & ~assigned).sum() / max(mine.sum(), 1)),
               "good_without_estimate": float((mine & (pid["status"] & STATUS_BITS["NO_ESTIMATE"] != 0)).sum() / max(mine.sum(), 1)),
               "good_held_by_its_gate": float((mine & ((pid["held"] >> p) & 1 == 1)).sum() / max(mine.sum(), 1)),
               "slots_assigned": int(assigned.sum()),
               "assigned_with_another_majority": float((assigned & used & (majority != p)).sum() / max(assigned.sum(), 1)),
               "assigned_from_slot": np.bincount(slot_of[:, p][slot_of[:, p] >= 0], minlength=n_sim).tolist(),
               "fit": {}}
        for leg, f in fits.items():
            f = f[:, p]
            ok = (f["evaluations"] > 0) & np.isfinite(brho_true[:, p]) & np.isfinite(f["brho"])
            row["fit"][leg] = {"brho": _spread(f["brho"][ok] / brho_true[ok, p] - 1.0), "ke": _spread(f["ke"][ok] / ke_true[ok, p] - 1.0)}
        out["positions"].append(row)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=114688)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--min-points", type=int, default=10)
    ap.add_argument("--thinning", type=float, default=5.0)
    ap.add_argument("--peak-threshold", type=float, default=None)
    ap.add_argument("--peak-prominence", type=float, default=None)
    ap.add_argument("--radius-ratio", type=float, default=1.5)
    ap.add_argument("--bins", type=int, default=12)
    ap.add_argument("--coverage-lo", type=float, default=0.02)
    ap.add_argument("--coverage-hi", type=float, default=0.98)
    ap.add_argument("--time-step", type=float, default=1.0e-10)
    ap.add_argument("--max-steps", type=int, default=10000)
    ap.add_argument("--max-evaluations", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    for name in args.workloads.split(","):
        eng, pipeline, indices = _engine(name, args)
        settings = {k: getattr(args, k) for k in SETTINGS}
        gates, info = calibrate(eng, indices, args)
        emit({"workload": name, "kind": "gates", **settings, **info})
        if args.reps > 0:
            emit({"workload": name, "kind": "rates_pid", **settings, **rates(eng, gates, args)})
        if args.stats_events > 0:
            emit({"workload": name, "kind": "pid_quality", **settings, **quality(eng, pipeline, indices, gates, args)})
        eng.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
