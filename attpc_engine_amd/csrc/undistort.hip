// undistort.hip -- drift correction of trace rows on the device: every row of an event is taken back from its apparent
// (x, y, time) to where its electrons were made and the event's rows are sorted again by their corrected time (the
// contract is in include/attpc_engine.h, "drift correction"; the arithmetic of one row is undistort_host.hpp, shared
// with the host).
//
// One workgroup of four waves per event, empty events included.  The sort is peak_rows_kernel's (peaks.hip): a counting
// sort over 512 time buckets x 16 sixteenths in LDS, an exclusive scan over the bins, a scatter of (index, key) and a
// rank inside the bin on (t, input index).  A corrected time may leave 0 .. 511: its whole part is clamped at both ends,
// and since the rank inside a bin is exact, a crowded end bin costs time, never order.
//   Pass 1 corrects every row once (a lane per row) and keeps x, y, t in a.xyt; t = NaN marks a skipped row (a
//   corrected t is always finite).  The bins and the skipped rows are counted with LDS atomics; the call's counts with
//   one global atomic per wave, of the sum of the tiles' ballots.
//   Pass 2 scatters (index, key) to the bin's region of the event's part of sort_idx / sort_key; the skipped rows take
//   the region behind every bin.
//   Pass 3 ranks an entry inside its region and writes the row, its label and its input index at that place.  Columns
//   3 .. 7 (every column of a skipped row) are moved as 64-bit words, so a NaN keeps its payload.
// 32 KiB of LDS for the bins, as peak_rows_kernel, is what bounds the kernel: four workgroups a CU, so four waves a SIMD
// at 256 threads (50 VGPRs would admit more).  A larger workgroup would not raise that, a smaller one lowers it; four
// waves keep the scan at 32 bins a thread and the LDS atomics of a tile spread over the corrected times of 256 rows.
#include "tracks_args.hpp"

namespace attpc {

constexpr int UD_THREADS = 256;
constexpr int UD_SUB = 16;
constexpr int UD_BINS = ATTPC_NUM_TB * UD_SUB;
constexpr int UD_BINS_PER_THREAD = UD_BINS / UD_THREADS;

namespace {

// descending t, monotone in t; below 0 and from 512 on the end bins
__device__ __forceinline__ int undistort_bin(double t) {
  int whole = 0, sub = 0;
  if (t >= (double)ATTPC_NUM_TB) {
    whole = ATTPC_NUM_TB - 1;
    sub = UD_SUB - 1;
  } else if (t >= 0.0) {
    whole = (int)t;
    sub = (int)((t - (double)whole) * (double)UD_SUB);
    sub = sub > UD_SUB - 1 ? UD_SUB - 1 : sub;
  }
  return (ATTPC_NUM_TB - 1 - whole) * UD_SUB + (UD_SUB - 1 - sub);
}

}  // namespace

__global__ __launch_bounds__(UD_THREADS) void undistort_kernel(UndistortArgs a) {
  __shared__ uint32_t bin_cursor[UD_BINS];
  __shared__ uint32_t wave_total[UD_THREADS / 64];
  __shared__ uint32_t skip_count, skip_cursor;
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = a.ev_start[e];
  const uint32_t n = (uint32_t)(a.ev_start[e + 1] - lo);
  if (n == 0u) return;  // uniform
  for (int b = t; b < UD_BINS; b += UD_THREADS) bin_cursor[b] = 0u;
  if (t == 0) {
    skip_count = 0u;
    skip_cursor = 0u;
  }
  block_sync();
  // ---- pass 1: the corrected points, the bins' counts ----
  uint32_t n_skipped = 0u, n_unconverged = 0u;  // of this wave's tiles (uniform over the wave)
  for (uint32_t base = 0u; base < n; base += UD_THREADS) {
    const uint32_t i = base + (uint32_t)t;
    int status = 0;
    if (i < n) {
      double x = 0.0, y = 0.0, tc = 0.0;
      status = undistort_row(a.s, a.rows + 8 * (lo + i), x, y, tc);
      double* p = a.xyt + 3 * (lo + i);
      if (status == UNDISTORT_SKIPPED) {
        p[2] = __builtin_nan("");
        atomicAdd(&skip_count, 1u);
      } else {
        p[0] = x;
        p[1] = y;
        p[2] = tc;
        atomicAdd(&bin_cursor[undistort_bin(tc)], 1u);
      }
    }
    n_skipped += (uint32_t)__popcll(__ballot(status == UNDISTORT_SKIPPED));
    n_unconverged += (uint32_t)__popcll(__ballot(status == UNDISTORT_UNCONVERGED));
  }
  if (lane == 0) {
    if (n_skipped) atomicAdd(&a.counts[1], (unsigned long long)n_skipped);
    if (n_unconverged) atomicAdd(&a.counts[2], (unsigned long long)n_unconverged);
  }
  if (t == 0) atomicAdd(&a.counts[0], (unsigned long long)n);
  block_sync();
  {  // exclusive prefix over the bins
    uint32_t local = 0u;
    for (int k = 0; k < UD_BINS_PER_THREAD; ++k) local += bin_cursor[t * UD_BINS_PER_THREAD + k];
    uint32_t incl = local;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      incl += lane >= off ? up : 0u;
    }
    if (lane == 63) wave_total[wave] = incl;
    block_sync();
    uint32_t run = incl - local;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    for (int k = 0; k < UD_BINS_PER_THREAD; ++k) {
      const int b = t * UD_BINS_PER_THREAD + k;
      const uint32_t c = bin_cursor[b];
      bin_cursor[b] = run;
      run += c;
    }
  }
  block_sync();
  const uint32_t n_sorted = n - skip_count;  // the corrected rows; the skipped ones stand behind them
  // ---- pass 2: (index, key) to the bin's region ----
  for (uint32_t i = (uint32_t)t; i < n; i += UD_THREADS) {
    const double tc = a.xyt[3 * (lo + i) + 2];
    const uint32_t p = tc == tc ? atomicAdd(&bin_cursor[undistort_bin(tc)], 1u) : n_sorted + atomicAdd(&skip_cursor, 1u);
    a.sort_idx[lo + p] = i;
    a.sort_key[lo + p] = tc;
  }
  __threadfence_block();  // (the lists are written and read by this workgroup only)
  block_sync();
  // ---- pass 3: the rank inside the region, and the row ----
  uint32_t n_moved = 0u;
  for (uint32_t base = 0u; base < n; base += UD_THREADS) {
    const uint32_t p = base + (uint32_t)t;
    bool moved = false;
    if (p < n) {
      const uint32_t ri = a.sort_idx[lo + p];
      const double tc = a.sort_key[lo + p];
      const bool skipped = p >= n_sorted;
      uint32_t r_lo = n_sorted, r_hi = n;
      if (!skipped) {
        const int b = undistort_bin(tc);
        r_lo = b > 0 ? bin_cursor[b - 1] : 0u;
        r_hi = bin_cursor[b];
      }
      uint32_t rank = 0u;
      for (uint32_t q = r_lo; q < r_hi; ++q) {
        const double other = a.sort_key[lo + q];
        const bool earlier = a.sort_idx[lo + q] < ri;
        rank += (skipped ? earlier : (other > tc || (other == tc && earlier))) ? 1u : 0u;
      }
      const uint32_t place = r_lo + rank;
      moved = place != ri;
      const int64_t o = lo + place;
      const unsigned long long* in = reinterpret_cast<const unsigned long long*>(a.rows + 8 * (lo + ri));
      unsigned long long* out = reinterpret_cast<unsigned long long*>(a.out_rows + 8 * o);
      if (skipped) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = in[k];
      } else {
        const double* c = a.xyt + 3 * (lo + ri);
        double* row = a.out_rows + 8 * o;
        row[0] = c[0] * 1000.0;
        row[1] = c[1] * 1000.0;
        row[2] = undistort_z(a.s, tc);
      }
#pragma unroll
      for (int k = 3; k < 8; ++k) out[k] = in[k];
      if (a.out_labels) a.out_labels[o] = a.labels[lo + ri];
      if (a.order) a.order[o] = a.order_base + lo + ri;
    }
    n_moved += (uint32_t)__popcll(__ballot(moved));
  }
  if (lane == 0 && n_moved) atomicAdd(&a.counts[3], (unsigned long long)n_moved);
}

void launch_undistort(hipStream_t s, uint32_t n_events, const UndistortArgs& a) {
  hipLaunchKernelGGL(undistort_kernel, dim3(n_events), dim3(UD_THREADS), 0, s, a);
}

}  // namespace attpc
