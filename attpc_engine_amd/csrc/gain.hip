// gain.hip -- micromegas gain of the traces: avalanche fluctuations and a per-pad gain map, run on the event-ordered
// cloud of a chunk in front of the trace count pass (opt-in; the contract is written out in include/attpc_engine.h,
// "micromegas gain of the traces"; tests/gain_reference.py restates it in numpy).
//
// One workgroup per event (the global event id is part of every row's Philox counter), the event's rows strided over
// its threads: a row reads its 24 B (pad, tau, electrons), makes one Philox4x32-10 call, looks its standardised
// fluctuation up in the 4097-knot inverse CDF (32 KiB, copied to LDS once per workgroup: a random gather), and writes
// the gained charge q'' as one f64.  Both trace passes read that array in place of the cloud's charge (pad_trace,
// traces.hip), so they agree by construction.
// Why a kernel of its own: the contract needs one correctly rounded f64 division and square root per row, and the
// hardware expands both into chains of fused multiply-adds, which the trace kernels must not contain
// (tests/test_traces_cpu.py).  Every other operation here is rounded once: contraction is off in gained_charge.
// Bound: by its traffic (24 B read, 8 B written per row) the memory roof; a kernel trace has it at half of that roof
// (3.5 .. 4.0 TB/s), no counters were taken (profiles/r14_trace_gain.md).
#include "tracks_args.hpp"

namespace attpc {

constexpr int GN_THREADS = 512;  // 32 KiB of LDS a workgroup: four of them, 8 waves per SIMD

// q'' of one row in range (include/attpc_engine.h): zq = the quantile table in LDS, read only with `draw`
// (rel_variance > 0).
__device__ __forceinline__ double gained_charge(const GainDev& g, bool draw, const double* zq, uint64_t seed,
                                                uint64_t event, uint32_t pad, uint32_t t, double q) {
#pragma clang fp contract(off)
  if (q == 0.0) return 0.0;
  double qg = q;
  if (draw) {  // uniform
    uint32_t u[4];
    philox4x32<10>((uint32_t)event, (uint32_t)(event >> 32), pad * (uint32_t)ATTPC_NUM_TB + t, g.domain, (uint32_t)seed,
                   (uint32_t)(seed >> 32), u);
    const uint32_t i = u[0] >> 20;
    const double w = (double)(u[0] & 0xFFFFFu) * (1.0 / 1048576.0);
    const double z0 = zq[i], z1 = zq[i + 1];
    const double z = z0 + (z1 - z0) * w;
    const double r = g.c / q;
    const double s = sqrt(r);
    const double y = (1.0 - r) + z * s;
    const double x = y > 0.0 ? y : 0.0;
    qg = ((q * x) * x) * x;
  }
  return g.pad_gain ? qg * g.pad_gain[pad] : qg;
}

__global__ __launch_bounds__(GN_THREADS) void gain_kernel(GainDev g, uint64_t seed, uint64_t first_event,
                                                          const int64_t* __restrict__ event_start,
                                                          const double* __restrict__ points,
                                                          double* __restrict__ gained) {
  __shared__ double zq[ATTPC_GAIN_KNOTS];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x;
  const int64_t lo = event_start[e], hi = event_start[e + 1];
  if (hi <= lo) return;  // uniform
  const bool draw = g.quantiles != nullptr;
  if (draw) {  // uniform
    for (int i = t; i < ATTPC_GAIN_KNOTS; i += GN_THREADS) zq[i] = g.quantiles[i];
    block_sync();
  }
  const uint64_t event = first_event + e;
  for (int64_t r = lo + t; r < hi; r += GN_THREADS) {
    const double padf = points[3 * r], tb = points[3 * r + 1], q = points[3 * r + 2];
    // a row the trace kernels never place (trace_row_ok) is never read back either: it gets 0
    gained[r] = trace_row_ok(padf, tb)
                    ? gained_charge(g, draw, zq, seed, event, (uint32_t)(int)padf, (uint32_t)(int)floor(tb), q)
                    : 0.0;
  }
}

void launch_gain(hipStream_t s, const GainDev& g, uint64_t seed, uint32_t n_events, uint64_t first_event,
                 const int64_t* event_start, const double* points, double* gained) {
  hipLaunchKernelGGL(gain_kernel, dim3(n_events), dim3(GN_THREADS), 0, s, g, seed, first_event, event_start, points, gained);
}

}  // namespace attpc
