// summary.hip -- event and track summaries of a scattered chunk (the contract is in include/attpc_engine.h).
//
// After a chunk's scatter its cloud lies in CloudBuffers::points / labels with holes, found only through the launch's
// segment list (one segment per flushed window of one event, plus lone buckets).  The rows are reduced where they lie:
//   1. summary_count_kernel   segments per event (one integer atomic per segment, which also gives the segment its
//                             place among its event's),
//   2. an exclusive scan of those counts (the host queues exclusive_scan_kernel of assemble.hip),
//   3. summary_fill_kernel    the segment numbers grouped by event,
//   4. summary_event_kernel   one workgroup per event: every thread folds the rows it reads into accumulators of its
//                             own in LDS (one set per position of layout->indices plus one for every other label), the
//                             kept pads go into one LDS bitmap per set; the sets are then reduced over the threads and
//                             the final records written with plain stores.
// Shape (b) of the two that fit: no record is ever accumulated into across workgroups, so a chunk that is scattered
// again (its buffers were too small) simply overwrites its records, nothing has to be zeroed but the per-event segment
// counts, and no result depends on the order of anything: counts, integer sums, minima and maxima only.
// A launch that ran out of room (CTRL_OVERFLOW) left segment slots unwritten: every kernel here returns at once then,
// as gather_segments_kernel does, and the host repeats scatter and summary.
#include "tracks_args.hpp"

namespace attpc {

constexpr int SM_THREADS = 128;                 // threads of summary_event_kernel
constexpr int SM_WORDS = ATTPC_NUM_PADS / 32;   // words of a pad bitmap
constexpr int SM_NO_SLOT = 15;

__global__ __launch_bounds__(256) void summary_count_kernel(SummaryArgs a) {
  if (launch_overflowed(a.chunk.ctrl)) return;
  const uint32_t n_segs = launch_segments(a.chunk);
  for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_segs; s += gridDim.x * 256u) {
    const Segment sg = a.chunk.segments[s];
    if (sg.count <= 0 || (uint32_t)sg.event >= a.n_events) continue;
    a.seg_rank[s] = atomicAdd(&a.seg_count[sg.event], 1u);
  }
}

__global__ __launch_bounds__(256) void summary_fill_kernel(SummaryArgs a) {
  if (launch_overflowed(a.chunk.ctrl)) return;
  const uint32_t n_segs = launch_segments(a.chunk);
  for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_segs; s += gridDim.x * 256u) {
    const Segment sg = a.chunk.segments[s];
    if (sg.count <= 0 || (uint32_t)sg.event >= a.n_events) continue;
    const int64_t at = a.seg_start[sg.event] + (int64_t)a.seg_rank[s];
    if (at >= 0 && at < (int64_t)n_segs) a.seg_list[at] = s;
  }
}

// x * x + y * y, each product rounded, then added (the contract's rho2)
__device__ __forceinline__ double rho2_of(double x, double y) {
#pragma clang fp contract(off)
  const double xx = x * x, yy = y * y;
  return xx + yy;
}

template <typename T>
__device__ __forceinline__ T wave_add(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}

// LDS of summary_event_kernel for n_slots = n_sim + 1 accumulator sets (the last one: labels outside layout->indices)
__host__ __device__ constexpr size_t summary_lds_bytes(int n_slots) {
  return (size_t)n_slots * SM_THREADS * (2 * 8 + 4 * 4)   // per thread and set: charge, rho2; rows, kept, tb_min, tb_max
         + (size_t)n_slots * SM_WORDS * 4                  // pad bitmaps
         + (size_t)n_slots * (3 * 8 + 5 * 4) + 8;          // the reduced sets, the tracks' electrons, the event's pads
}

__global__ __launch_bounds__(SM_THREADS) void summary_event_kernel(SummaryArgs a) {
  extern __shared__ unsigned long long sm_raw[];
  if (launch_overflowed(a.chunk.ctrl)) return;
  const int n_sim = a.n_sim, n_slots = n_sim + 1;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int cells = n_slots * SM_THREADS;
  unsigned long long* acc_charge = sm_raw;
  double* acc_rho2 = reinterpret_cast<double*>(acc_charge + cells);
  unsigned long long* res_charge = reinterpret_cast<unsigned long long*>(acc_rho2 + cells);
  double* res_rho2 = reinterpret_cast<double*>(res_charge + n_slots);
  unsigned long long* res_electrons = reinterpret_cast<unsigned long long*>(res_rho2 + n_slots);
  uint32_t* acc_rows = reinterpret_cast<uint32_t*>(res_electrons + n_slots);
  uint32_t* acc_kept = acc_rows + cells;
  int32_t* acc_tmin = reinterpret_cast<int32_t*>(acc_kept + cells);
  int32_t* acc_tmax = acc_tmin + cells;
  uint32_t* bitmap = reinterpret_cast<uint32_t*>(acc_tmax + cells);
  uint32_t* res_rows = bitmap + n_slots * SM_WORDS;
  uint32_t* res_kept = res_rows + n_slots;
  int32_t* res_tmin = reinterpret_cast<int32_t*>(res_kept + n_slots);
  int32_t* res_tmax = res_tmin + n_slots;
  uint32_t* res_pads = reinterpret_cast<uint32_t*>(res_tmax + n_slots);  // [n_slots + 1]: the last one is the event's

  const uint32_t n_segs = launch_segments(a.chunk);
  const uint64_t nib_lo = a.slot_nibbles[0], nib_hi = a.slot_nibbles[1];
  const double min_q = a.min_electrons;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  for (uint32_t ev = blockIdx.x; ev < a.n_events; ev += gridDim.x) {
    for (int s = 0; s < n_slots; ++s) {
      const int c = s * SM_THREADS + t;
      acc_charge[c] = 0ull;
      acc_rho2[c] = -1.0;
      acc_rows[c] = 0u;
      acc_kept[c] = 0u;
      acc_tmin[c] = 0x7fffffff;
      acc_tmax[c] = -1;
    }
    for (int i = t; i < n_slots * SM_WORDS; i += SM_THREADS) bitmap[i] = 0u;
    if (t < n_slots) res_electrons[t] = 0ull;
    block_sync();

    // ---- the event's cloud rows, in place ----
    int64_t k0 = a.seg_start[ev], k1 = a.seg_start[ev + 1];
    if (k0 < 0) k0 = 0;
    if (k1 > (int64_t)n_segs) k1 = (int64_t)n_segs;
    for (int64_t k = k0; k < k1; ++k) {
      const uint32_t s = a.seg_list[k];
      if (s >= n_segs) continue;
      const Segment sg = a.chunk.segments[s];
      if (sg.count <= 0 || sg.offset < 0 || sg.offset + (int64_t)sg.count > a.chunk.row_capacity) continue;
      const double* __restrict__ rows = a.chunk.points + sg.offset * 3;
      const int64_t* __restrict__ labs = a.chunk.labels + sg.offset;
      for (int i = t; i < sg.count; i += SM_THREADS) {
        const double padf = rows[(size_t)3 * i], tau = rows[(size_t)3 * i + 1], q = rows[(size_t)3 * i + 2];
        const long long lab = labs[i];
        int slot = SM_NO_SLOT;
        if (lab >= 0 && lab < 16) slot = (int)((nib_lo >> (4 * (int)lab)) & 15ull);
        else if (lab >= 16 && lab < ATTPC_MAX_ROWS) slot = (int)((nib_hi >> (4 * ((int)lab - 16))) & 15ull);
        if (slot >= n_sim) slot = n_sim;  // a label outside layout->indices: the event record only
        const int c = slot * SM_THREADS + t;
        acc_rows[c] += 1u;
        acc_charge[c] += (unsigned long long)(long long)q;
        if (q >= min_q) {
          acc_kept[c] += 1u;
          const int tb = (int)tau;  // tau >= 0: floor
          acc_tmin[c] = min(acc_tmin[c], tb);
          acc_tmax[c] = max(acc_tmax[c], tb);
          const uint32_t pad = (uint32_t)(int)padf;
          if (pad < (uint32_t)ATTPC_NUM_PADS) {
            atomicOr(&bitmap[slot * SM_WORDS + (int)(pad >> 5)], 1u << (pad & 31u));
            const double r2 = rho2_of(a.pad_centers[2 * pad], a.pad_centers[2 * pad + 1]);
            acc_rho2[c] = r2 > acc_rho2[c] ? r2 : acc_rho2[c];
          }
        }
      }
    }

    // ---- the tracks' electrons: thread t takes sample t of every 128-sample block ----
    if (a.trk.counts != nullptr) {
      for (int s = 0; s < n_sim; ++s) {
        const size_t track = ((size_t)a.event0 + ev) * (size_t)n_sim + (size_t)s;
        int cnt = a.trk.counts[track];
        cnt = cnt < 0 ? 0 : (cnt > MAX_BLOCKS_PER_TRACK * ARENA_BLK ? MAX_BLOCKS_PER_TRACK * ARENA_BLK : cnt);
        long long sum = 0ll;
        for (int b = 0; b * ARENA_BLK < cnt; ++b) {
          const int32_t blk = a.trk.block_table[track * MAX_BLOCKS_PER_TRACK + b];
          if (blk < 0 || (uint32_t)blk >= a.trk.arena_blocks) continue;
          if (b * ARENA_BLK + t < cnt) sum += (long long)a.trk.arena[((size_t)blk * ARENA_BLK + t) * 4 + 3];
        }
        sum = wave_add(sum);
        if (lane == 0 && sum != 0ll) atomicAdd(&res_electrons[s], (unsigned long long)sum);
      }
    }
    block_sync();

    // ---- the sets reduced over the threads, a wave per set; task n_slots: the event's pads (the union) ----
    for (int task = wave; task <= n_slots; task += SM_THREADS / 64) {
      if (task < n_slots) {
        const int c0 = task * SM_THREADS + lane, c1 = c0 + 64;
        const unsigned long long charge = wave_add(acc_charge[c0] + acc_charge[c1]);
        const double r2 = wave_max(acc_rho2[c0] > acc_rho2[c1] ? acc_rho2[c0] : acc_rho2[c1]);
        const uint32_t n_rows = wave_add(acc_rows[c0] + acc_rows[c1]);
        const uint32_t n_kept = wave_add(acc_kept[c0] + acc_kept[c1]);
        const int32_t tmin = wave_min(min(acc_tmin[c0], acc_tmin[c1]));
        const int32_t tmax = wave_max(max(acc_tmax[c0], acc_tmax[c1]));
        uint32_t pads = 0u;
        for (int w = lane; w < SM_WORDS; w += 64) pads += (uint32_t)__popc(bitmap[task * SM_WORDS + w]);
        pads = wave_add(pads);
        if (lane == 0) {
          res_charge[task] = charge;
          res_rho2[task] = r2;
          res_rows[task] = n_rows;
          res_kept[task] = n_kept;
          res_tmin[task] = tmin;
          res_tmax[task] = tmax;
          res_pads[task] = pads;
        }
      } else {
        uint32_t pads = 0u;
        for (int w = lane; w < SM_WORDS; w += 64) {
          uint32_t bits = 0u;
          for (int s = 0; s < n_slots; ++s) bits |= bitmap[s * SM_WORDS + w];
          pads += (uint32_t)__popc(bits);
        }
        pads = wave_add(pads);
        if (lane == 0) res_pads[n_slots] = pads;
      }
    }
    block_sync();

    // ---- the records: thread s < n_sim its track's, thread 64 the event's ----
    const size_t ev_batch = (size_t)a.event0 + ev;
    if (t < n_sim && a.tracks != nullptr) {
      attpc_track_summary r;
      r.n_points = res_rows[t];
      r.n_kept = res_kept[t];
      r.n_pads = res_pads[t];
      r.tb_min = r.n_kept ? res_tmin[t] : -1;
      r.tb_max = r.n_kept ? res_tmax[t] : -1;
      r.reserved = 0;
      r.charge = (int64_t)res_charge[t];
      r.rho2_max = r.n_kept ? res_rho2[t] : -1.0;
      r.n_steps = 0;
      r.n_samples = 0;
      r.electrons = (int64_t)res_electrons[t];
      r.end_x = r.end_y = r.end_tb = nan;
      if (a.trk.counts != nullptr) {
        const size_t track = ev_batch * (size_t)n_sim + (size_t)t;
        const int cnt = a.trk.counts[track];
        r.n_steps = a.trk.n_steps[track];
        r.n_samples = cnt;
        if (cnt > 0 && cnt <= MAX_BLOCKS_PER_TRACK * ARENA_BLK) {
          const int32_t blk = a.trk.block_table[track * MAX_BLOCKS_PER_TRACK + (cnt - 1) / ARENA_BLK];
          if (blk >= 0 && (uint32_t)blk < a.trk.arena_blocks) {
            const double* last = a.trk.arena + ((size_t)blk * ARENA_BLK + (size_t)((cnt - 1) % ARENA_BLK)) * 4;
            r.end_x = last[0];
            r.end_y = last[1];
            r.end_tb = last[2];
          }
        }
      }
      a.tracks[ev_batch * (size_t)n_sim + (size_t)t] = r;
    }
    if (t == 64 && a.events != nullptr) {
      attpc_event_summary r;
      uint32_t n_rows = 0u, n_kept = 0u;
      int32_t tmin = 0x7fffffff, tmax = -1;
      unsigned long long charge = 0ull;
      for (int s = 0; s < n_slots; ++s) {
        n_rows += res_rows[s];
        n_kept += res_kept[s];
        tmin = min(tmin, res_tmin[s]);
        tmax = max(tmax, res_tmax[s]);
        charge += res_charge[s];
      }
      r.n_points = n_rows;
      r.n_kept = n_kept;
      r.n_pads = res_pads[n_slots];
      r.tb_min = n_kept ? tmin : -1;
      r.tb_max = n_kept ? tmax : -1;
      r.reserved = 0;
      r.charge = (int64_t)charge;
      a.events[ev_batch] = r;
    }
    block_sync();  // the next event's initialisation overwrites what was just read
  }
}

void launch_summary_count(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups) {
  hipLaunchKernelGGL(summary_count_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
}

void launch_summary_fill(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups) {
  hipLaunchKernelGGL(summary_fill_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
}

void launch_summary_events(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups) {
  hipLaunchKernelGGL(summary_event_kernel, dim3(n_workgroups), dim3(SM_THREADS), summary_lds_bytes(a.n_sim + 1), s, a);
}

}  // namespace attpc
