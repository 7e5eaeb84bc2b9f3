// distort.hip -- drift distortion of the track records on the device: every kept record (x, y, time bucket, electrons)
// of a track batch is shifted in place by the configured map (the contract is in include/attpc_engine.h, "drift
// distortion"; its arithmetic is distort_host.hpp, shared with the host).
//
// A pass of its own right behind track_kernel (launch_tracks, abi.hip): it walks counts / block_table of the batch and
// rewrites the arena blocks the tracks own.  Persistent waves; a wave takes the next four tracks from a control word
// (TRK_NEXT_DISTORT, one atomic per visit) and walks their chains, one whole 4 KiB arena block per trip:
//   four 16-byte loads per lane, lane l element 64 k + l of the block's 256 double2 -- every wave instruction reads
//   1 KiB contiguously.  Lanes 2 m and 2 m + 1 then hold the (x, y) halves (lane 2 m) and the (tb, q) halves (lane
//   2 m + 1) of records 32 k + m; one exchange with the neighbour lane per pair of loads gives lane 2 m all of record
//   64 p + m and lane 2 m + 1 all of record 64 p + 32 + m (p = 0, 1), so that every record is shifted once, by one lane.
//   The exchange in reverse puts the halves back where they were loaded and the stores are the loads' mirror images.
// Only records below counts[t] are stored; what the loads bring of the rest of a block is computed on and dropped (the
// cell of a record is clamped, so the table reads stay in range for any bits).  The tables (at most 1.5 MiB) stay in the
// caches; the traffic is 32 B in and 32 B out per record.
// A batch whose arena ran out (TRK_OVERFLOW) has unset block-table entries: the kernel leaves it alone, the host runs
// the batch again and this pass with it.
#include "tracks_args.hpp"

namespace attpc {

constexpr int DISTORT_THREADS = 256;
// tracks a wave takes per visit to the control word: every visit is an atomic on one address, and with one track per
// visit those atomics, not the records, set the kernel's time (profiles/r28_drift_distortion.md)
constexpr uint32_t DISTORT_CLAIM = 4u;

namespace {

// the value of lane ^ 1: one DPP move per 32-bit half (quad_perm [1, 0, 3, 2]), every lane of the wave active
__device__ __forceinline__ double from_neighbour(double v) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)bits, 0xB1, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), 0xB1, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned int)lo);
}

}  // namespace

__global__ __launch_bounds__(DISTORT_THREADS) void distort_kernel(DistortArgs a) {
  if (a.buf.ctrl[TRK_OVERFLOW] != 0u) return;
  const int lane = (int)(threadIdx.x & 63u);
  const bool odd = (lane & 1) != 0;
  const int m = lane >> 1;
  for (;;) {
    uint32_t begin = 0u;
    if (lane == 0) begin = atomicAdd(&a.buf.ctrl[TRK_NEXT_DISTORT], DISTORT_CLAIM);
    begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)begin);
    if (begin >= a.n_tracks) break;
    const uint32_t end = a.n_tracks - begin < DISTORT_CLAIM ? a.n_tracks : begin + DISTORT_CLAIM;
    for (uint32_t t = begin; t < end; ++t) {
      int count = a.buf.counts[t];
      count = count < 0 ? 0 : (count > MAX_BLOCKS_PER_TRACK * ARENA_BLK ? MAX_BLOCKS_PER_TRACK * ARENA_BLK : count);
      const int n_blocks = (count + ARENA_BLK - 1) / ARENA_BLK;
      for (int b = 0; b < n_blocks; ++b) {
        const int32_t blk = a.buf.block_table[(size_t)t * MAX_BLOCKS_PER_TRACK + b];
        if (blk < 0 || (uint32_t)blk >= a.buf.arena_blocks) continue;  // (never after a launch that did not overflow)
        double2* p = reinterpret_cast<double2*>(a.buf.arena + (size_t)blk * ARENA_BLK * 4);
        const int left = count - b * ARENA_BLK;  // records of this block, >= 1
        double2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[64 * k + lane];
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
          const double2 first = v[2 * pair], second = v[2 * pair + 1];
          // even lane: `first` is the (x, y) of its record and the neighbour's `first` its (tb, q); odd lane: `second`
          // is the (tb, q) of its record and the neighbour's `second` its (x, y)
          const double got0 = from_neighbour(odd ? first.x : second.x), got1 = from_neighbour(odd ? first.y : second.y);
          double x = odd ? got0 : first.x, y = odd ? got1 : first.y;
          double tb = odd ? second.x : got0;
          const double q = odd ? second.y : got1;
          distort_record(a.map, x, y, tb);
          const double back0 = from_neighbour(odd ? x : tb), back1 = from_neighbour(odd ? y : q);
          v[2 * pair] = odd ? make_double2(back0, back1) : make_double2(x, y);
          v[2 * pair + 1] = odd ? make_double2(tb, q) : make_double2(back0, back1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (32 * k + m < left) p[64 * k + lane] = v[k];
      }
    }
  }
}

void launch_distort(uint32_t workgroups, hipStream_t s, const DistortArgs& a) {
  hipLaunchKernelGGL(distort_kernel, dim3(workgroups), dim3(DISTORT_THREADS), 0, s, a);
}

}  // namespace attpc
