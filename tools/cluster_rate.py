"""Cost and quality of the clustering (attpc_trace_configure_clustering): one GPU, o16aa and be10dp in
partial readout with sigma = 5, pedestals and threshold 20; estimates with ``--min-points`` points, thinning at
``--thinning`` mm, geometric circle fit and helix slope on in every leg.  ``--peak-threshold`` / ``--peak-prominence``
replace the default peak parameters (at the default threshold of 40 counts a noise of 5 makes no row at all).

(a) Cost: per workload one engine in this process; ``run_estimates`` of ``--events`` events with the stage off and on,
alternating, ``--reps`` timed calls each behind one warm-up call of each kind.  A leg's figure is the median of its timed
calls, its spread their minimum and maximum.  ``--off-only`` times the stage-off leg alone, which a build without the
stage (the parent commit's, named by ATTPC_HIP_LIBRARY) can run too.
(b) Quality: ``--stats-events`` events through ``run_estimates`` in calls of ``--events``, every call once with the stage
off (the truth labels) and once with it on (``match="truth"``): per nucleus the tracks with rows, the share of them with a
cluster, the share with completeness >= 0.9 and purity >= 0.9, and the median and half the 16 .. 84 % range of
brho(estimate) / brho(truth) - 1, truth-labelled and clustered side by side, on the tracks both legs estimate and on all
that each leg estimates; per workload the share of events with n_split, n_fake, n_small > 0 and the rows rejected.
Reported values for the settings used, no limits.
``--join`` is the leg of the cluster joining (attpc_trace_configure_cluster_join): in (a) both legs cluster
and "on" also joins, so the cost is the joining's against the clustering alone; in (b) the clustered leg joins too, and
the line carries the join counts (events joined, clusters joined away, events capped).  ``--overlap-ratio``,
``--min-radius``, ``--radius-ratio`` (0 = no condition) and ``--max-clusters`` are its settings.

    python tools/cluster_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp]
                                 [--eps-xy MM] [--eps-z MM] [--min-samples N] [--min-cluster-size N] [--out FILE]
                                 [--join [--overlap-ratio R] [--min-radius MM] [--radius-ratio Q] [--max-clusters K]]
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
SETTINGS = ("events", "min_points", "thinning", "eps_xy", "eps_z", "min_samples", "min_cluster_size", "peak_threshold",
            "peak_prominence", "join", "overlap_ratio", "min_radius", "radius_ratio", "max_clusters")


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
    return eng, pipeline, indices


def _clustering(args):
    from attpc_engine_amd.detector.clustering import ClusterSettings

    return ClusterSettings(args.eps_xy, args.eps_z, args.min_samples, args.min_cluster_size)


def _join(args):
    from attpc_engine_amd.detector.joining import JoinSettings

    return JoinSettings(args.overlap_ratio, args.min_radius, args.radius_ratio or None, args.max_clusters) if args.join else None


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def rates(eng, args) -> dict:
    legs = {"off": [], "on": []}

    def call(on: bool):
        if args.join:  # both legs cluster; "on" joins
            eng.configure_clustering(_clustering(args))
            eng.configure_cluster_join(_join(args) if on else None)
        elif not args.off_only:
            eng.configure_clustering(_clustering(args) if on else None)
        t0 = time.perf_counter()
        eng.run_estimates(args.events, seed=1)
        return args.events / (time.perf_counter() - t0)

    kinds = (False,) if args.off_only else (False, True)
    for on in kinds:
        call(on)
    for _ in range(args.reps):
        for on in kinds:
            legs["on" if on else "off"].append(call(on))
    out = {k: [_median(v), min(v), max(v)] for k, v in legs.items() if v}
    out["calls"] = legs
    if args.off_only:
        return out
    eng.configure_clustering()
    if args.join:
        eng.configure_cluster_join()
    out["cost_share"] = 1.0 - out["on"][0] / out["off"][0]
    out["seconds_per_event"] = 1.0 / out["on"][0] - 1.0 / out["off"][0]
    return out


def _spread(values):
    import numpy as np

    values = values[np.isfinite(values)]
    if len(values) == 0:
        return [0, None, None]
    lo, mid, hi = np.percentile(values, [16.0, 50.0, 84.0])
    return [int(len(values)), float(mid), float(0.5 * (hi - lo))]


def quality(eng, pipeline, indices, args) -> dict:
    import numpy as np

    from attpc_engine_amd.detector import estimate
    from attpc_engine_amd.detector.clustering import cluster_scores

    z = pipeline.get_proton_numbers()
    est = {"truth": [], "clustered": []}
    events, records, truth, joins = [], [], [], []
    t0, done = time.perf_counter(), 0
    while done < args.stats_events:
        for leg in ("truth", "clustered"):
            eng.configure_clustering(_clustering(args) if leg == "clustered" else None)
            eng.configure_cluster_join(_join(args) if leg == "clustered" else None)
            res = eng.run_estimates(args.events, seed=2, first_event=done)
            est[leg].append(res["estimates"])
        if args.join:
            joins.append(res["joins"][0])
        events.append(res["clusters"][0])
        records.append(res["clusters"][1])
        truth.append(estimate.truth_tracks(res["p4"], indices, z)["brho"])
        done += args.events
    eng.configure_clustering()
    eng.configure_cluster_join()
    est = {k: np.concatenate(v) for k, v in est.items()}
    events, records, truth = np.concatenate(events), np.concatenate(records), np.concatenate(truth)
    completeness, purity = cluster_scores(events, records)
    out = {"events": done, "seconds": time.perf_counter() - t0, "positions": []}
    out["event_share"] = {name: float((events[name] > 0).mean()) for name in ("n_split", "n_fake", "n_small")}
    out["event_share"]["status"] = float((events["status"] != 0).mean())
    out["rows"] = {name: int(events[name].sum()) for name in ("n_rows", "n_range", "n_core", "n_border", "n_noise")}
    out["clusters_per_event"] = np.bincount(np.minimum(events["n_clusters"], 9), minlength=10).tolist()
    if joins:
        joins = np.concatenate(joins)
        out["joins"] = {"events_joined": float((joins["n_joined"] > 0).mean()), "n_joined": int(joins["n_joined"].sum()),
                        "n_pairs": int(joins["n_pairs"].sum()), "n_candidates": int(joins["n_candidates"].sum()),
                        "n_circles": int(joins["n_circles"].sum()), "n_taking_part": int(joins["n_taking_part"].sum()),
                        "events_capped": int((joins["status"] == 1).sum()), "events_not_clustered": int((joins["status"] == 2).sum())}
    for s in range(len(indices)):
        has_rows = events["truth_rows"][:, s] > 0
        found = has_rows & np.isfinite(completeness[:, s])
        good = found & (completeness[:, s] >= 0.9) & (purity[:, s] >= 0.9)
        a, b = est["truth"][:, s], est["clustered"][:, s]
        ok_a = np.isfinite(a["brho"]) & np.isfinite(truth[:, s])
        ok_b = np.isfinite(b["brho"]) & np.isfinite(truth[:, s])
        both = ok_a & ok_b
        row = {"position": s, "row": int(indices[s]), "Z": int(z[int(indices[s])]), "tracks_with_rows": int(has_rows.sum()),
               "share_with_a_cluster": float(found.sum() / max(has_rows.sum(), 1)),
               "share_complete_and_pure": float(good.sum() / max(has_rows.sum(), 1)),
               "completeness": _spread(completeness[found, s]), "purity": _spread(purity[found, s]),
               "brho_truth_labelled": _spread(a["brho"][ok_a] / truth[ok_a, s] - 1.0),
               "brho_clustered": _spread(b["brho"][ok_b] / truth[ok_b, s] - 1.0),
               "brho_truth_labelled_on_both": _spread(a["brho"][both] / truth[both, s] - 1.0),
               "brho_clustered_on_both": _spread(b["brho"][both] / truth[both, s] - 1.0)}
        out["positions"].append(row)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=100000)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--min-points", type=int, default=10)
    ap.add_argument("--thinning", type=float, default=5.0)
    ap.add_argument("--eps-xy", type=float, default=20.0)
    ap.add_argument("--eps-z", type=float, default=20.0)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--min-cluster-size", type=int, default=10)
    ap.add_argument("--peak-threshold", type=float, default=None)
    ap.add_argument("--peak-prominence", type=float, default=None)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--join", action="store_true")
    ap.add_argument("--overlap-ratio", type=float, default=0.5)
    ap.add_argument("--min-radius", type=float, default=10.0)
    ap.add_argument("--radius-ratio", type=float, default=0.0)
    ap.add_argument("--max-clusters", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.workloads.split(","):
        eng, pipeline, indices = _engine(name, args)
        settings = {k: getattr(args, k) for k in SETTINGS}
        if args.reps > 0:
            lines.append({"workload": name, "kind": "rates_off_only" if args.off_only else "rates_join" if args.join else "rates", **settings, **rates(eng, args)})
            print(json.dumps(lines[-1]), flush=True)
        if args.stats_events > 0 and not args.off_only:
            lines.append({"workload": name, "kind": "quality", **settings, **quality(eng, pipeline, indices, args)})
            print(json.dumps(lines[-1]), flush=True)
        eng.ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
