// select.hip -- selected delivery: the predicate on a chunk's summary records (the contract is in
// include/attpc_engine.h); the gather that skips the events that failed it is in assemble.hip.
//
// Behind a chunk's scatter and its summary kernels (summary.hip) the records of its events lie in the batch's record
// buffers.  Between them and the assembly:
//   1. select_kernel           one lane per event: the contract's predicate (select_passes, tracks_args.hpp) on the
//                              event record and its n_sim track records -> passed[event], and
//                              sel_rows[event] = passed ? ev_rows[event] : 0,
//   2. the assembly (assemble.hip): exclusive_scan_kernel turns sel_rows into the set's CSR offsets, a rejected event
//      is an empty range, and gather_selected_kernel skips its segments: the rows of a rejected event are never read.
// Everything behind (pack, Spyral count / write, the copies) works on the offsets and sees empty events.  Nothing is
// accumulated: a chunk that is scattered again (its buffers were too small) overwrites passed and sel_rows.  A launch
// that ran out of room (CTRL_OVERFLOW) left records and segment slots unwritten: both kernels return at once then, the
// scan turns every offset into 0, and the host repeats scatter, summary and selection.
#include "tracks_args.hpp"

namespace attpc {

__global__ __launch_bounds__(256) void select_kernel(SelectArgs a) {
  if (launch_overflowed(a.ctrl)) return;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < a.n_events; e += gridDim.x * 256u) {
    const size_t ev = (size_t)a.event0 + e;
    const attpc_track_summary* tracks = a.tracks != nullptr ? a.tracks + ev * (size_t)a.n_sim : nullptr;
    const bool pass = select_passes(a.desc, a.events[ev], tracks, a.n_sim);
    a.passed[ev] = pass ? (uint8_t)1 : (uint8_t)0;
    if (a.sel_rows != nullptr) a.sel_rows[e] = pass ? a.ev_rows[e] : 0u;
  }
}

void launch_select(hipStream_t s, const SelectArgs& a) {
  const uint32_t wgs = a.n_events ? (a.n_events + 255u) / 256u : 1u;
  hipLaunchKernelGGL(select_kernel, dim3(wgs < 1024u ? wgs : 1024u), dim3(256), 0, s, a);
}

}  // namespace attpc
