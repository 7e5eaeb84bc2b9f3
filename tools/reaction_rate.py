"""Cost and quality of the reaction reconstruction (attpc_reaction_configure): one GPU, o16aa and be10dp
with the settings of tools/pid_rate.py's r33 runs (partial readout with sigma = 5, pedestals and threshold 20, estimates
with ``--min-points`` points, thinning at ``--thinning`` mm, geometric circle fit, helix slope, clustering at its defaults
with the joining at ``--radius-ratio``, the track fit at its defaults), whose engine, gates and fit settings it reuses.

(a) Cost: ``run_estimates`` of ``--events`` events in ``match="truth"`` with the track fit on, the reconstruction off
and on alternating, and ``run_spectra`` of the same events; ``--reps`` timed calls each behind one warm-up call of each
kind; a leg's figure is the median of its timed calls, its spread their minimum and maximum.  ``--off-only``: the off leg
alone, for a library without the stage (``ATTPC_HIP_LIBRARY``: the parent commit's); ``--spectra-first``: the three legs
in the opposite order within a round.
(b) Quality on ``--stats-events`` events (seed 2), the observed track at position ``--track`` (and, for be10dp, the 11Be
at position 1 as a leg of its own): for ``match="truth"`` and for ``match="rank"`` with the particle identification
(gates from ``Gate.from_band`` on a ``match="truth"`` run of seed 3): the share of every status, and over the records of
status 0 the median and half the 16 .. 84 % range of Ex - truth Ex and of theta_cm - truth theta_cm; the efficiency
truth_reconstructed / truth over all cells and per theta_cm bin, and the two (Ex, theta_cm) maps themselves.  The spectra are those of ``run_estimates`` added up
call by call (``ReactionSpectra.__add__``).
Reported values for the settings used, no limits.

    python tools/reaction_rate.py [--events N] [--reps K] [--stats-events M] [--workloads o16aa,be10dp] [--out FILE]
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

EX_RANGE = {"be10dp": (-8.0, 8.0), "o16aa": (0.0, 20.0)}  # around the sampled state (0.32 MeV, 9.585 MeV)


def _median(values):
    v = sorted(values)
    return v[len(v) // 2]


def _settings(eng, name, args, track, source="fit"):
    from attpc_engine_amd.detector.reaction import ReactionSettings

    return ReactionSettings.from_pipeline(eng.pipeline, track=track, source=source, ex_range=EX_RANGE.get(name, (-4.0, 12.0)),
                                          ex_bins=args.ex_bins, theta_bins=args.theta_bins, indices=eng.indices)


def rates(eng, name, args) -> dict:
    from pid_rate import _fit

    eng.configure_clustering(match="truth")
    eng.configure_pid()
    eng.configure_track_fit(_fit(args))
    settings = None if args.off_only else _settings(eng, name, args, args.track)
    legs = {"off": [], "on": [], "spectra": []}
    sums = {}

    def call(leg: str):
        if not args.off_only:
            eng.configure_reaction(None if leg == "off" else settings)
        t0 = time.perf_counter()
        res = eng.run_spectra(args.events, seed=1) if leg == "spectra" else eng.run_estimates(args.events, seed=1)
        rate = args.events / (time.perf_counter() - t0)
        sums[leg] = [res["stats"]["key_checksum"], res["stats"]["charge_checksum"]]
        if leg == "off":
            sums["rows"] = res["trace_rows"]
        return rate

    order = ("off",) if args.off_only else ("spectra", "on", "off") if args.spectra_first else ("off", "on", "spectra")
    for leg in order:
        call(leg)
    for _ in range(args.reps):
        for leg in order:
            legs[leg].append(call(leg))
    out = {leg: [_median(v), min(v), max(v)] for leg, v in legs.items() if v}
    out["calls"] = {leg: v for leg, v in legs.items() if v}
    out["checksums"] = sums
    out["order"] = list(order)
    if not args.off_only:
        out["cost_share"] = 1.0 - out["on"][0] / out["off"][0]
        out["seconds_per_event"] = 1.0 / out["on"][0] - 1.0 / out["off"][0]
        eng.configure_reaction()
    eng.configure_track_fit()
    return out


def quality(eng, name, gates, track, args) -> dict:
    import numpy as np

    from attpc_engine_amd.detector.reaction import STATUS_BITS
    from pid_rate import _fit, _spread

    eng.configure_track_fit(_fit(args))
    settings = _settings(eng, name, args, track)
    eng.configure_reaction(settings)
    legs = {"truth": ("truth", False), "rank_pid": ("rank", True)}
    out = {"track": track, "observed_row": settings.observed_row, "charge": settings.charge, "ex_range": [settings.ex_lo, settings.ex_hi],
           "legs": {}}
    t0 = time.perf_counter()
    for leg, (match, pid_on) in legs.items():
        eng.configure_clustering(match=match)
        eng.configure_pid(gates if pid_on else None)
        records, spectra, done = [], None, 0
        while done < args.stats_events:
            res = eng.run_estimates(args.events, seed=2, first_event=done)
            records.append(res["reaction"])
            spectra = res["spectra"] if spectra is None else spectra + res["spectra"]
            done += args.events
        rec = np.concatenate(records)
        good = rec["status"] == 0
        truth = spectra.truth.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            per_theta = (spectra.truth_reconstructed.sum(axis=0) / truth.sum(axis=0)).tolist()
        out["legs"][leg] = {
            "events": done, "status_0": float(good.mean()),
            "status_share": {bit: float((rec["status"] & value != 0).mean()) for bit, value in STATUS_BITS.items()},
            "ex_minus_truth": _spread((rec["ex"] - rec["truth_ex"])[good]),
            "theta_minus_truth": _spread((rec["theta_cm"] - rec["truth_theta_cm"])[good]),
            "beam_ke_minus_truth": _spread((rec["beam_ke"] - rec["truth_beam_ke"])[good]),
            "truth_ex": _spread(rec["truth_ex"][np.isfinite(rec["truth_ex"])]),
            "efficiency": float(spectra.truth_reconstructed.sum() / max(truth.sum(), 1.0)),
            "efficiency_per_theta_bin": [None if v != v else round(v, 4) for v in per_theta],
            # the (Ex, theta_cm) maps themselves, [ex_bins][theta_bins]: their ratio is the efficiency map
            "truth_map": spectra.truth.tolist(), "truth_reconstructed_map": spectra.truth_reconstructed.tolist(),
            "truth_in_bins": int(truth.sum()), "outside": spectra.outside.tolist(),
            "reconstructed_in_bins": int(spectra.reconstructed.sum()),
            "response_on_diagonal": float(np.trace(spectra.ex_response) / max(int(spectra.ex_response.sum()), 1))}
    out["seconds"] = time.perf_counter() - t0
    eng.configure_reaction()
    eng.configure_pid()
    eng.configure_track_fit()
    eng.configure_clustering()
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
    ap.add_argument("--spectra-first", action="store_true", help="the legs of (a) in the order run_spectra, on, off")
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
        if args.reps > 0:
            emit({**head, "kind": "rates_reaction", **rates(eng, name, args)})
        if args.stats_events > 0 and not args.off_only:
            gates, _ = calibrate(eng, indices, args)
            tracks = [args.track] + ([1] if name == "be10dp" and args.track != 1 else [])
            for track in tracks:
                emit({**head, "kind": "reaction_quality", **quality(eng, name, gates, track, args)})
        eng.ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
