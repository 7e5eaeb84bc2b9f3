"""Rate of the digitised pad traces (attpc_sim_run_traces) on one GPU, for the headline workload (o16aa) and be10dp:
device-resident events/s (the traces are written to HBM and stay there; only the checksums come back), and delivered
events/s and GB/s into page-locked host arrays (pads, 1 KiB of samples and the label of every kept pad row).  Prints
one JSON line per workload with kept trace rows and bytes per event.  ``--noise-sigma S`` adds S ADC counts of
Gaussian electronic noise, ``--pedestal P`` a pedestal of P counts on every pad (both off by default).
``--readout partial|full`` reads out the noise-only pads of every pad not in BEAM_PADS as well (default hit),
``--threshold T`` sets the ADC threshold (default the workload's).  ``--common-sigma C`` adds C counts of common-mode
noise (off by default) over ``--common-groups G`` groups of consecutive pads (default 40).
``--packed`` measures the packed entry points (attpc_sim_run_traces_packed) beside the plain ones, every variant once per
rep in turn: the device-resident rate with the pack passes, delivered events/s with the rows left packed and with
``unpack_traces`` on the host behind every call, and the packed bytes per event and per row.

    python tools/trace_rate.py [--events N] [--deliver-events M] [--reps K] [--workloads o16aa,be10dp]
                               [--noise-sigma S] [--pedestal P] [--readout hit|partial|full] [--threshold T]
                               [--common-sigma C] [--common-groups G] [--packed]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=262144, help="events per device-resident call")
    ap.add_argument("--deliver-events", type=int, default=16384, help="events per delivered call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="o16aa,be10dp")
    ap.add_argument("--noise-sigma", type=float, default=0.0, help="Gaussian electronic noise, ADC counts (0 = off)")
    ap.add_argument("--pedestal", type=int, default=None, help="pedestal of every pad, ADC counts (default none)")
    ap.add_argument("--readout", default="hit", choices=["hit", "partial", "full"], help="readout of noise-only pads")
    ap.add_argument("--threshold", type=float, default=None, help="ADC threshold (default the workload's)")
    ap.add_argument("--common-sigma", type=float, default=0.0, help="Gaussian common-mode noise, ADC counts (0 = off)")
    ap.add_argument("--common-groups", type=int, default=40, help="groups of consecutive pads that share it (1 .. 255)")
    ap.add_argument("--packed", action="store_true", help="measure the packed entry points beside the plain ones")
    args = ap.parse_args()
    if not 1 <= args.common_groups <= 255:
        ap.error("--common-groups must lie in 1 .. 255")

    import numpy as np

    import __graft_entry__ as entry

    entry.build()
    from attpc_engine_amd import _abi, workloads
    from attpc_engine_amd.outputs import TraceArrays
    from attpc_engine_amd.engine import Engine

    ctx = _abi.Context(0)
    for name in args.workloads.split(","):
        pipeline, config, indices = workloads.WORKLOADS[name]()
        eng = Engine(pipeline, config, indices, context=ctx)
        eng.configure_traces(config, threshold=args.threshold, noise_sigma=args.noise_sigma, pedestals=args.pedestal,
                             readout=args.readout)
        if args.common_sigma > 0.0:
            from attpc_engine_amd.detector.traces import CommonModeSettings

            groups = (np.arange(_abi.NUM_PADS) * args.common_groups // _abi.NUM_PADS).astype(np.uint8)
            eng.configure_common_mode(CommonModeSettings(sigma=args.common_sigma, groups=groups))
        lib, seed = ctx.lib, 1

        def resident(first):
            out, stats = _abi.TraceOut(), _abi.RunStats()
            ctx.check(lib.attpc_sim_run_traces(ctx.handle, seed, first, args.events, eng.layout, None, None, None, out,
                                               stats), "attpc_sim_run_traces")
            return out, stats

        resident(0)  # warm-up: buffers settle
        times, rows = [], 0
        for rep in range(args.reps):
            t0 = time.perf_counter()
            out, stats = resident((rep + 1) * args.events)
            times.append(time.perf_counter() - t0)
            rows += out.n_rows
        t_res = float(np.median(times))
        rows_per_event = rows / (args.reps * args.events)

        n = args.deliver_events
        cap = int(rows_per_event * n * (1.0 if args.readout == "full" else 1.3)) + 4096
        arrays = TraceArrays(n, cap, ctx.pinned_empty)
        stats = _abi.RunStats()

        def delivered(first):
            rc = lib.attpc_sim_run_traces(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats)
            ctx.check(rc, "attpc_sim_run_traces")
            return int(arrays.out.n_rows)

        delivered(0)
        d_times, d_rows = [], 0
        for rep in range(args.reps):
            t0 = time.perf_counter()
            d_rows += delivered((rep + 1) * n)
            d_times.append(time.perf_counter() - t0)
        t_del = float(np.median(d_times))
        row_bytes = 512 * 2 + 4 + 8
        d_bytes = d_rows / args.reps * row_bytes + 16 * n  # rows + offsets / event points
        extra = packed_rates(ctx, eng, args, seed, rows_per_event, resident, delivered) if args.packed else {}
        print(json.dumps({
            "workload": name, "noise_sigma": args.noise_sigma, "pedestal": args.pedestal, "readout": args.readout,
            "threshold": float(config.elec_params.adc_threshold if args.threshold is None else args.threshold),
            "common_sigma": args.common_sigma, "common_groups": args.common_groups if args.common_sigma > 0.0 else 0,
            "resident_events": args.events, "resident_events_per_s": args.events / t_res,
            "resident_s": times, "trace_rows_per_event": rows_per_event,
            "bytes_written_per_event": rows_per_event * row_bytes,
            "cloud_rows_per_event": stats.n_points / n,
            "delivered_events": n, "delivered_events_per_s": n / t_del, "delivered_GB_per_s": d_bytes / t_del / 1e9,
            "delivered_s": d_times, "device_bytes": int(stats.device_bytes), **extra}), flush=True)
    ctx.close()


def packed_rates(ctx, eng, args, seed, rows_per_event, resident, delivered) -> dict:
    """The packed variants beside the plain ones (``resident(first)`` / ``delivered(first)`` of main), each once per rep
    in turn so that whatever else the host is doing falls on all of them alike."""
    import numpy as np

    from attpc_engine_amd import _abi
    from attpc_engine_amd.detector.traces import unpack_traces
    from attpc_engine_amd.outputs import PackedTraceArrays

    lib, n = ctx.lib, args.deliver_events

    def resident_packed(first):
        out, stats = _abi.TracePackedOut(), _abi.RunStats()
        ctx.check(lib.attpc_sim_run_traces_packed(ctx.handle, seed, first, args.events, eng.layout, None, None, None, out,
                                                  stats), "attpc_sim_run_traces_packed")
        return out

    first_try = resident_packed(0)  # warm-up, and the bytes a row takes
    bytes_per_row = first_try.n_bytes / max(1, first_try.n_rows)
    cap = int(rows_per_event * n * (1.0 if args.readout == "full" else 1.3)) + 4096
    arrays = PackedTraceArrays(n, cap, ctx.pinned_empty, byte_capacity=int(cap * bytes_per_row * 1.1) + 4096)
    stats = _abi.RunStats()

    def delivered_packed(first, unpack=False):
        rc = lib.attpc_sim_run_traces_packed(ctx.handle, seed, first, n, eng.layout, None, None, None, arrays.out, stats)
        ctx.check(rc, "attpc_sim_run_traces_packed")
        if unpack:
            _, _, row_start, records, _ = arrays.result()
            return unpack_traces(row_start, records).shape[0]
        return int(arrays.out.n_rows)

    delivered_packed(0)
    delivered_packed(0, unpack=True)
    variants = {"resident_plain": lambda r: resident((r + 1) * args.events),
                "resident_packed": lambda r: resident_packed((r + 1) * args.events),
                "delivered_plain": lambda r: delivered((r + 1) * n), "delivered_packed": lambda r: delivered_packed((r + 1) * n),
                "delivered_packed_unpacked": lambda r: delivered_packed((r + 1) * n, unpack=True)}
    times = {name: [] for name in variants}
    for r in range(args.reps):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run(r)
            times[name].append(time.perf_counter() - t0)
    events = {name: args.events if name.startswith("resident") else n for name in variants}
    last_rows, last_bytes = int(arrays.out.n_rows), int(arrays.out.n_bytes)
    return {"packed": {
        "format": _abi.TRACE_PACK_FORMAT, "bytes_per_row": bytes_per_row, "ratio_to_1KiB": bytes_per_row / 1024.0,
        "sample_bytes_per_event_packed": bytes_per_row * rows_per_event, "sample_bytes_per_event_plain": 1024.0 * rows_per_event,
        "link_bytes_per_event_packed": (last_bytes + last_rows * (8 + 4 + 8)) / n + 16,
        "link_bytes_per_event_plain": last_rows * (1024 + 4 + 8) / n + 16,
        "events_per_s": {name: events[name] / float(np.median(t)) for name, t in times.items()},
        "seconds": times}}


if __name__ == "__main__":
    main()
