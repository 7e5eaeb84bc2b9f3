// assemble.hip -- a scattered chunk (ChunkView, common.hpp: rows with holes, found through the launch's segment list
// and control words) put in event order for delivery, and the small kernels of the host pipeline (abi.hip):
//   exclusive_scan_kernel    the rows per event (all of them, or those select.hip left) -> CSR offsets,
//   gather_segments_kernel / gather_selected_kernel    every segment to its place in the event-ordered arrays,
//   pack_rows_kernel         the event-ordered rows as 16- or 8-byte transfer records,
//   count_status_kernel      the events whose kinematics ended at the sample limit.
#include "tracks_args.hpp"

namespace attpc {

// out[i] = sum of in[0..i), i = 0..n (one workgroup; n is a chunk's event count).
// `ctrl` (may be null): control words of the scatter launch that produced the counts -- if that launch ran out of
// capacity (launch_overflowed) every offset becomes 0: the kernels behind this one then see empty events and touch nothing.
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(const uint32_t* __restrict__ in, uint32_t n, int64_t* __restrict__ out,
                                                              const unsigned long long* __restrict__ ctrl) {
  __shared__ long long wave_sum[16];
  __shared__ long long carry;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool dead = ctrl != nullptr && launch_overflowed(ctrl);
  if (t == 0) carry = 0;
  block_sync();
  for (uint32_t base = 0; base < n; base += 1024u) {
    const uint32_t i = base + (uint32_t)t;
    const long long v = (i < n && !dead) ? (long long)in[i] : 0ll;
    long long incl = v;
    for (int off = 1; off < 64; off <<= 1) {
      const long long up = __shfl_up(incl, off);
      incl += lane >= off ? up : 0ll;
    }
    if (lane == 63) wave_sum[wave] = incl;
    block_sync();
    long long before = carry;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (i < n) out[i] = before + incl - v;
    block_sync();
    if (t == 1023) carry = before + incl;
    block_sync();
  }
  if (t == 0) out[n] = carry;
}

// Device-side CSR assembly: segment s (one flushed window of one event) is copied to rows ev_start[event] + ev_offset of
// the event-ordered arrays.  The number of segments is read from the launch's control words (the host never sees the
// segment list).  SELECTED: the segments of the events that failed the selection are skipped, their rows never read.
template <bool SELECTED>
__device__ __forceinline__ void gather_segments(const GatherArgs& g) {
  if (launch_overflowed(g.chunk.ctrl)) return;  // unwritten segment slots, see exclusive_scan_kernel
  const uint32_t n_segs = launch_segments(g.chunk);
  for (uint32_t s = blockIdx.x; s < n_segs; s += gridDim.x) {
    const Segment sg = g.chunk.segments[s];
    if (sg.count <= 0 || (uint32_t)sg.event >= g.n_events) continue;
    if (SELECTED && g.passed[(size_t)g.event0 + (uint32_t)sg.event] == 0) continue;
    if (sg.offset < 0 || sg.offset + (int64_t)sg.count > g.chunk.row_capacity) continue;
    const int64_t dst = g.ev_start[sg.event] + sg.ev_offset;
    if (sg.ev_offset < 0 || dst < 0 || dst + (int64_t)sg.count > g.out_capacity) continue;
    const double* __restrict__ src_p = g.chunk.points + sg.offset * 3;
    double* __restrict__ dst_p = g.out_points + dst * 3;
    for (int i = threadIdx.x; i < sg.count * 3; i += 256) dst_p[i] = src_p[i];
    const int64_t* __restrict__ src_l = g.chunk.labels + sg.offset;
    int64_t* __restrict__ dst_l = g.out_labels + dst;
    for (int i = threadIdx.x; i < sg.count; i += 256) dst_l[i] = src_l[i];
  }
}
__global__ __launch_bounds__(256) void gather_segments_kernel(GatherArgs g) { gather_segments<false>(g); }
__global__ __launch_bounds__(256) void gather_selected_kernel(GatherArgs g) { gather_segments<true>(g); }

// ---- compact transfer of delivered clouds ----
// The delivered path is PCIe bound (234 KB per event in the reference's dtypes), so a chunk crosses the link as 16-byte
// records (PackedRow, unpack_host.hpp) that host threads expand into the caller's arrays (abi.hip).  A chunk with a row
// that does not fit (charge >= 2^45, label >= 32) goes the plain way.
// tight != 0: the 8-byte record (PackedRow8, unpack_host.hpp) -- the jitter is not sent at all: it is a pure function of
// (seed, event, time bucket, pad), and the host regenerates it with the same Philox2x32-7.  flag[0] != 0: a row does not fit
// the 16-byte record; flag[1] != 0: a row does not fit the 8-byte one (charge >= 2^36, or a jittered time bucket that
// is a whole number -- tb + U rounded up to tb + 1, about one row in 1e13 -- from which the bucket cannot be read back).
__global__ __launch_bounds__(256) void pack_rows_kernel(const int64_t* __restrict__ ev_start, uint32_t n_events,
                                                        const double* __restrict__ points, const int64_t* __restrict__ labels,
                                                        PackedRow* __restrict__ packed, int64_t* __restrict__ flag, int tight) {
  const int64_t total = ev_start[n_events];
  bool bad = false, bad8 = false;
  unsigned long long* __restrict__ packed8 = reinterpret_cast<unsigned long long*>(packed);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < total; r += (int64_t)gridDim.x * 256) {
    const double padf = points[3 * r], tbj = points[3 * r + 1], q = points[3 * r + 2];
    const long long label = labels[r];
    const unsigned long long charge = (unsigned long long)q, pad = (unsigned long long)padf;
    bad = bad || !(q >= 0.0) || charge >= (1ull << PACK_CHARGE_BITS) || pad >= (1ull << PACK_PAD_BITS) || label < 0 || label >= 32;
    if (tight) {
      const double tbf = floor(tbj);
      bad8 = bad8 || charge >= (1ull << PACK8_CHARGE_BITS) || !(tbf >= 0.0) || tbf >= (double)(1 << PACK8_TB_BITS) || tbf == tbj;
      packed8[r] = (charge & ((1ull << PACK8_CHARGE_BITS) - 1)) | ((unsigned long long)tbf << PACK8_CHARGE_BITS) |
                   (pad << (PACK8_CHARGE_BITS + PACK8_TB_BITS)) |
                   ((unsigned long long)label << (PACK8_CHARGE_BITS + PACK8_TB_BITS + PACK_PAD_BITS));
    } else {
      PackedRow row;
      row.tb = tbj;
      row.bits = (charge & ((1ull << PACK_CHARGE_BITS) - 1)) | (pad << PACK_CHARGE_BITS) |
                 ((unsigned long long)label << (PACK_CHARGE_BITS + PACK_PAD_BITS));
      packed[r] = row;
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(flag), 1ull);
  if (__any(bad8 || bad) && (threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(flag) + 1, 1ull);
}

__global__ __launch_bounds__(256) void count_status_kernel(const int32_t* __restrict__ status, uint32_t n,
                                                           uint32_t* __restrict__ counter) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool bad = i < n && status[i] != 0;
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (uint32_t)__popcll(m));
}

void launch_exclusive_scan(hipStream_t s, const uint32_t* in, uint32_t n, int64_t* out, const unsigned long long* ctrl) {
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, in, n, out, ctrl);
}
void launch_gather(hipStream_t s, const GatherArgs& a, bool selected, uint32_t n_workgroups) {
  hipLaunchKernelGGL(selected ? gather_selected_kernel : gather_segments_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
}
void launch_pack_rows_kernel(hipStream_t s, uint32_t n_workgroups, const int64_t* ev_start, uint32_t n_events,
                             const double* points, const int64_t* labels, PackedRow* packed, int64_t* flag, int tight) {
  hipLaunchKernelGGL(pack_rows_kernel, dim3(n_workgroups), dim3(256), 0, s, ev_start, n_events, points, labels, packed, flag, tight);
}
void launch_count_status(hipStream_t s, const int32_t* status, uint32_t n, uint32_t* counter) {
  hipLaunchKernelGGL(count_status_kernel, dim3((n + 255) / 256), dim3(256), 0, s, status, n, counter);
}

}  // namespace attpc
