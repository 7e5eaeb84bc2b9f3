// select.hip -- selected delivery: the predicate on a chunk's summary records, and the gather that skips the events
// that failed it (the contract is in include/attpc_engine.h).
//
// Behind a chunk's scatter and its summary kernels (summary.hip) the records of its events lie in the batch's record
// buffers.  Between them and the assembly:
//   1. select_kernel           one lane per event: the contract's predicate (select_passes, tracks_args.hpp) on the
//                              event record and its n_sim track records -> passed[event], and
//                              sel_rows[event] = passed ? ev_rows[event] : 0,
//   2. an exclusive scan of sel_rows into the assembly set's CSR offsets (the host queues exclusive_scan_kernel of
//      abi.hip): a rejected event is an empty range,
//   3. gather_selected_kernel  gather_segments_kernel of abi.hip with one more test per segment: the rows of a rejected
//                              event are never read.
// Everything behind (pack, Spyral count / write, the copies) works on the offsets and sees empty events.  Nothing is
// accumulated: a chunk that is scattered again (its buffers were too small) overwrites passed and sel_rows.  A launch
// that ran out of room (control word 6) left records and segment slots unwritten: both kernels return at once then, the
// scan turns every offset into 0, and the host repeats scatter, summary and selection.
#include "tracks_args.hpp"

namespace attpc {

__global__ __launch_bounds__(256) void select_kernel(SelectArgs a) {
  if (a.ctrl[6] != 0ull) return;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < a.n_events; e += gridDim.x * 256u) {
    const size_t ev = (size_t)a.event0 + e;
    const attpc_track_summary* tracks = a.tracks != nullptr ? a.tracks + ev * (size_t)a.n_sim : nullptr;
    const bool pass = select_passes(a.desc, a.events[ev], tracks, a.n_sim);
    a.passed[ev] = pass ? (uint8_t)1 : (uint8_t)0;
    if (a.sel_rows != nullptr) a.sel_rows[e] = pass ? a.ev_rows[e] : 0u;
  }
}

__global__ __launch_bounds__(256) void gather_selected_kernel(GatherSelectedArgs g) {
  if (g.ctrl[6] != 0ull) return;
  const unsigned long long n_all = g.ctrl[1];
  const uint32_t n_segs = (uint32_t)(n_all < (unsigned long long)g.seg_capacity ? n_all : (unsigned long long)g.seg_capacity);
  for (uint32_t s = blockIdx.x; s < n_segs; s += gridDim.x) {
    const Segment sg = g.segments[s];
    if (sg.count <= 0 || (uint32_t)sg.event >= g.n_events) continue;
    if (g.passed[(size_t)g.event0 + (uint32_t)sg.event] == 0) continue;
    if (sg.offset < 0 || sg.offset + (int64_t)sg.count > g.row_capacity) continue;
    const int64_t dst = g.ev_start[sg.event] + sg.ev_offset;
    if (sg.ev_offset < 0 || dst < 0 || dst + (int64_t)sg.count > g.out_capacity) continue;
    const double* __restrict__ src_p = g.points + sg.offset * 3;
    double* __restrict__ dst_p = g.out_points + dst * 3;
    for (int i = threadIdx.x; i < sg.count * 3; i += 256) dst_p[i] = src_p[i];
    const int64_t* __restrict__ src_l = g.labels + sg.offset;
    int64_t* __restrict__ dst_l = g.out_labels + dst;
    for (int i = threadIdx.x; i < sg.count; i += 256) dst_l[i] = src_l[i];
  }
}

void launch_select(hipStream_t s, const SelectArgs& a) {
  const uint32_t wgs = a.n_events ? (a.n_events + 255u) / 256u : 1u;
  hipLaunchKernelGGL(select_kernel, dim3(wgs < 1024u ? wgs : 1024u), dim3(256), 0, s, a);
}

void launch_gather_selected(hipStream_t s, const GatherSelectedArgs& a, uint32_t n_workgroups) {
  hipLaunchKernelGGL(gather_selected_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
}

}  // namespace attpc
