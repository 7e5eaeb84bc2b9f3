"""Cost and quality of the fit hypotheses (attpc_trace_configure_hypotheses): one GPU, o16aa and be10dp
with the set-up of tools/pid_rate.py (partial readout with sigma = 5, pedestals and threshold 20, estimates with
``--min-points`` points, thinning at ``--thinning`` mm, geometric circle fit and helix slope, clustering with the joining
at ``--radius-ratio``, the track fit at ``--time-step`` / ``--max-steps`` / ``--max-evaluations``), gates from
``Gate.from_band`` on a ``match="truth"`` run of seed 3.

(a) Cost: ``run_estimates`` of ``--events`` events in ``match="rank"`` with the fit on, four legs interleaved in one
process -- the plain fit, PID -> fit, hypotheses alone, PID -> hypotheses --, ``--reps`` timed calls each behind one
warm-up call of each; a leg's figure is the median of its timed calls, its spread their minimum and maximum; the
checksums of every leg beside them.  ``--off-only``: the plain leg alone (for a library named by ATTPC_HIP_LIBRARY that
lacks the stage).
(b) Quality on ``--stats-events`` events of seed 2, per position: of the ranked clusters whose truth majority is the
position and that are complete and pure to 0.9, the share assigned to a position of its species (and of another species,
and to none), by the gates and by the hypotheses; the fit's B rho and kinetic energy against the kinematics, median and
half the 16 .. 84 % range, for ``match="truth"``, rank + PID, rank + hypotheses and rank + PID + hypotheses
(``by_position``); the reaction reconstruction's Ex - truth Ex for the track of ``--track`` in the same legs; and the
distribution of f_next / f of the slots assigned to a position of their majority's species and to another.
Reported values for the settings used, no limits.

    python tools/hypothesis_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
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

LEGS = {"fit": (False, False), "pid_fit": (True, False), "hypotheses": (False, True), "pid_hypotheses": (True, True)}
RATIO_EDGES = [1.0, 1.1, 1.5, 2.0, 5.0, 10.0, 100.0, 1e3, 1e4]


def rates(eng, gates, args) -> dict:
    from pid_rate import _fit, _median

    eng.configure_clustering(match="rank")
    eng.configure_track_fit(_fit(args))
    names = ["fit"] if args.off_only else list(LEGS)
    legs, sums, fitted = {name: [] for name in names}, {}, {}

    def call(name: str):
        pid_on, hyp_on = LEGS[name]
        if not args.off_only:
            eng.configure_pid(gates if pid_on else None)
            eng.configure_fit_hypotheses(candidates=0xFF) if hyp_on else eng.configure_fit_hypotheses()
        t0 = time.perf_counter()
        res = eng.run_estimates(args.events, seed=1)
        rate = args.events / (time.perf_counter() - t0)
        sums[name] = [res["stats"]["key_checksum"], res["stats"]["charge_checksum"], res["trace_rows"]["row_checksum"]]
        fitted[name] = int((res["fits"]["evaluations"] > 0).sum())
        return rate

    for name in names:
        call(name)
    for _ in range(args.reps):
        for name in names:
            legs[name].append(call(name))
    out = {name: [_median(v), min(v), max(v)] for name, v in legs.items()}
    out["calls"], out["checksums"], out["tracks_fitted"] = legs, sums, fitted
    if not args.off_only:
        eng.configure_pid()
        eng.configure_fit_hypotheses()
    eng.configure_track_fit()
    return out


def quality(eng, name, pipeline, indices, gates, args) -> dict:
    import numpy as np

    from attpc_engine_amd.detector import estimate
    from attpc_engine_amd.detector.hypothesis import STATUS_BITS
    from attpc_engine_amd.detector.pid import by_position
    from pid_rate import _fit, _spread
    from reaction_rate import _settings

    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    n_sim = len(indices)
    species = [(int(z[int(i)]), int(a[int(i)])) for i in indices]
    same = np.array([[species[p] == species[q] for q in range(n_sim)] for p in range(n_sim)])
    eng.configure_track_fit(_fit(args))
    eng.configure_reaction(_settings(eng, name, args, args.track))
    legs = {"truth": ("truth", False, False), "rank_pid": ("rank", True, False), "rank_hyp": ("rank", False, True),
            "rank_pid_hyp": ("rank", True, True)}
    kept = {leg: {"fits": [], "assign": [], "reaction": [], "hyp": []} for leg in legs}
    events, records, brho_true, ke_true = [], [], [], []
    t0, done = time.perf_counter(), 0
    while done < args.stats_events:
        for leg, (match, pid_on, hyp_on) in legs.items():
            eng.configure_clustering(match=match)
            eng.configure_pid(gates if pid_on else None)
            eng.configure_fit_hypotheses(candidates=0xFF) if hyp_on else eng.configure_fit_hypotheses()
            res = eng.run_estimates(args.events, seed=2, first_event=done)
            kept[leg]["fits"].append(res["fits"])
            kept[leg]["reaction"].append(res["reaction"])
            if hyp_on:
                kept[leg]["hyp"].append(res["hypotheses"])
            kept[leg]["assign"].append(res["hypotheses"]["position"] if hyp_on else res["pid"]["position"] if pid_on
                                       else np.tile(np.arange(n_sim, dtype=np.int32), (args.events, 1)))
        events.append(res["clusters"][0])
        records.append(res["clusters"][1][:, :n_sim])
        brho_true.append(estimate.truth_tracks(res["p4"], indices, z)["brho"])
        p4 = res["p4"][:, [int(i) for i in indices]]
        ke_true.append(p4[..., 3] - np.sqrt(np.maximum(p4[..., 3] ** 2 - (p4[..., :3] ** 2).sum(axis=-1), 0.0)))
        done += args.events
    eng.configure_reaction()
    eng.configure_pid()
    eng.configure_fit_hypotheses()
    eng.configure_track_fit()
    eng.configure_clustering()
    events, records = np.concatenate(events), np.concatenate(records)
    brho_true, ke_true = np.concatenate(brho_true), np.concatenate(ke_true)
    majority, used = records["majority"], records["first_row"] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        purity = records["majority_rows"] / records["rows"]
        truth_rows = np.take_along_axis(events["truth_rows"].astype(np.int64), np.maximum(majority, 0), axis=1)
        completeness = records["majority_rows"] / truth_rows
    good = used & (majority >= 0) & (purity >= 0.9) & (completeness >= 0.9)
    out = {"events": done, "seconds": time.perf_counter() - t0, "track": args.track, "species": species, "legs": {}}
    for leg in legs:
        fits, position = np.concatenate(kept[leg]["fits"]), np.concatenate(kept[leg]["assign"])
        reaction = np.concatenate(kept[leg]["reaction"])
        ordered, _ = by_position(fits, np.rec.fromarrays([position], names="position")) if leg != "truth" else (fits, None)
        ok_rx = reaction["status"] == 0
        row = {"ex_minus_truth": _spread((reaction["ex"] - reaction["truth_ex"])[ok_rx]), "reaction_status_0": float(ok_rx.mean()),
               "positions": []}
        right = np.zeros(position.shape, dtype=bool)  # the slot's position is of its cluster's majority species
        right[position >= 0] = same[np.maximum(majority, 0), np.maximum(position, 0)][position >= 0] & (majority >= 0)[position >= 0]
        for p in range(n_sim):
            mine = good & (majority == p)
            assigned = position >= 0
            f = ordered[:, p]
            ok = (f["evaluations"] > 0) & np.isfinite(brho_true[:, p]) & np.isfinite(f["brho"])
            entry = {"position": p, "Z": species[p][0], "A": species[p][1], "good_clusters": int(mine.sum()),
                     "fit": {"brho": _spread(f["brho"][ok] / brho_true[ok, p] - 1.0), "ke": _spread(f["ke"][ok] / ke_true[ok, p] - 1.0)}}
            if leg != "truth":
                entry.update(good_to_its_species=float((mine & right).sum() / max(mine.sum(), 1)),
                             good_to_another_species=float((mine & assigned & ~right).sum() / max(mine.sum(), 1)),
                             good_to_none=float((mine & ~assigned).sum() / max(mine.sum(), 1)),
                             slots_assigned=int((position == p).sum()),
                             assigned_with_another_species=float(((position == p) & used & ~right).sum() / max((position == p).sum(), 1)))
            row["positions"].append(entry)
        if kept[leg]["hyp"]:
            hyp = np.concatenate(kept[leg]["hyp"])
            row["status_share"] = {bit: float((hyp["status"] & value != 0).mean()) for bit, value in STATUS_BITS.items()}
            row["status_share"]["assigned"] = float((hyp["position"] >= 0).mean())
            chosen = np.take_along_axis(hyp["f"], np.maximum(hyp["position"], 0)[..., None], axis=2)[..., 0]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = hyp["f_next"] / chosen
            has = (hyp["position"] >= 0) & np.isfinite(ratio) & good
            row["f_ratio"] = {"edges": RATIO_EDGES}
            for key, which in (("right", has & right), ("wrong", has & ~right)):
                counts = np.histogram(ratio[which], bins=[0.0] + RATIO_EDGES + [np.inf])[0]
                row["f_ratio"][key] = {"n": int(which.sum()), "counts": counts.tolist(),
                                       "median": float(np.median(ratio[which])) if which.any() else None}
            row["f_ratio"]["no_other_species_fitted"] = int(((hyp["position"] >= 0) & ~np.isfinite(hyp["f_next"]) & good).sum())
        out["legs"][leg] = row
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-events", type=int, default=114688)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--track", type=int, default=0)
    ap.add_argument("--ex-bins", type=int, default=64)
    ap.add_argument("--theta-bins", type=int, default=36)
    ap.add_argument("--off-only", action="store_true")
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
    from pid_rate import _engine, calibrate

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    for name in args.workloads.split(","):
        eng, pipeline, indices = _engine(name, args)
        head = {"workload": name, "events": args.events, "off_only": args.off_only}
        gates = None
        if not args.off_only:
            gates, info = calibrate(eng, indices, args)
            emit({**head, "kind": "gates", **info})
        if args.reps > 0:
            emit({**head, "kind": "rates_hypotheses", **rates(eng, gates, args)})
        if args.stats_events > 0 and not args.off_only:
            emit({**head, "kind": "hypothesis_quality", **quality(eng, name, pipeline, indices, gates, args)})
        eng.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
