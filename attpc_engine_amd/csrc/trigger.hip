// trigger.hip -- the GET multiplicity trigger on the device: kept trace rows -> one 32-byte record per event, run on a
// chunk's trace outputs in HBM behind the trace write pass (the contract is in include/attpc_engine.h, "multiplicity
// trigger").  Integer arithmetic throughout: every field is a count, a sum, a minimum or a maximum.
//
// One workgroup of four waves per event, empty events included.  The event's kept rows are read once, one wave per row
// in turn: a lane loads 8 consecutive samples (16 bytes, the 1 KiB row coalesced, as peaks.hip and baseline.hip do) and
// turns them into 8 hit bits; the bit before a lane's first sample comes from the neighbouring lane.  The
// multiplicity m_g[j] is never summed row by row: a row changes it only at the EDGES of its hit runs, +1 where a run
// starts and -1 one past where it ends, so a row costs two non-returning LDS adds per run instead of one per hit
// sample.  (A run that lasts to sample 511 would end at 512; no sum reads that entry, so it is not kept: 512 counters
// per group, 32 KiB for the 16 groups.)
// After the rows, per group by one wave, a lane on 8 consecutive samples: a prefix over j gives m_g, a second one
// P_g[j] = sum of m_g[0..j], written back in place.  Then a thread takes samples t and t + 256 over all groups:
//   s_g[j] = P_g[j] - P_g[j - W]   (the second term 0 for j < W)
// and from it A[j], the sum over the groups and their maximum; wave shuffles and four LDS slots reduce them to the
// record, which every thread then holds (so the gate needs no further barrier) and thread 0 writes.
// Only the groups the map uses (tg.n_groups = 1 + its highest group) are cleared, scanned and summed.
#include "tracks_args.hpp"

namespace attpc {

constexpr int TG_THREADS = 256;
constexpr int TG_WAVES = TG_THREADS / 64;

// exclusive prefix of v over the wave
__device__ __forceinline__ int tg_wave_exclusive(int v, int lane) {
  int incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off);
    incl += lane >= off ? up : 0;
  }
  return incl - v;
}

__global__ __launch_bounds__(TG_THREADS) void trigger_kernel(TriggerArgs a) {
  __shared__ int cnt[ATTPC_MAX_TRIGGER_GROUPS * ATTPC_NUM_TB];
  __shared__ int hit_pads;
  __shared__ uint32_t red[TG_WAVES][4];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = a.kept_start[e], hi = a.kept_start[e + 1];
  if (hi == lo) {  // uniform: zeros and -1s
    if (t == 0) {
      int4* rec = reinterpret_cast<int4*>(a.records + e);
      rec[0] = make_int4(0, -1, 0, 0);
      rec[1] = make_int4(0, 0, 0, -1);
    }
    return;
  }
  const TriggerDev& tg = a.tg;
  const int n_groups = tg.n_groups;
  for (int i = t; i < n_groups * ATTPC_NUM_TB; i += TG_THREADS) cnt[i] = 0;
  if (t == 0) hit_pads = 0;
  block_sync();
  int rows_hit = 0;  // (the same in every lane of the wave)
  for (int64_t row = lo + wave; row < hi; row += TG_WAVES) {
    const int pad = a.pads[row];
    const int g = tg.groups ? (int)tg.groups[pad] : 0;
    if (g >= n_groups) continue;  // 255: the pad takes no part (uniform: one row per wave)
    const int level = tg.threshold + (a.pedestals ? (int)a.pedestals[pad] : 0);  // y > threshold iff trace > level
    const uint4 v = reinterpret_cast<const uint4*>(a.samples + row * ATTPC_NUM_TB)[lane];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t h = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h |= ((int)(short)(w[i] & 0xffffu) > level ? 1u : 0u) << (2 * i);
      h |= ((int)(short)(w[i] >> 16) > level ? 1u : 0u) << (2 * i + 1);
    }
    const uint32_t left = __shfl_up(h, 1);
    const uint32_t before = ((h << 1) | (lane ? left >> 7 : 0u)) & 0xffu;  // bit s: the sample before 8 lane + s hits
    int* c = cnt + g * ATTPC_NUM_TB + lane * 8;
    for (uint32_t rise = h & ~before; rise; rise &= rise - 1u) atomicAdd(&c[__ffs((int)rise) - 1], 1);
    for (uint32_t fall = ~h & before; fall; fall &= fall - 1u) atomicAdd(&c[__ffs((int)fall) - 1], -1);
    rows_hit += __ballot(h != 0u) != 0ull ? 1 : 0;
  }
  if (lane == 0 && rows_hit) atomicAdd(&hit_pads, rows_hit);
  block_sync();
  for (int g = wave; g < n_groups; g += TG_WAVES) {  // d -> m -> P, in place
    int* c = cnt + g * ATTPC_NUM_TB + lane * 8;
    int p[8];
    int run = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) p[s] = run += c[s];
    int base = tg_wave_exclusive(run, lane);
    run = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) p[s] = run += p[s] + base;
    base = tg_wave_exclusive(run, lane);
#pragma unroll
    for (int s = 0; s < 8; ++s) c[s] = p[s] + base;
  }
  block_sync();
  int first = ATTPC_NUM_TB;     // first sample with A[j] >= min_groups
  uint32_t asserted = 0u;       // groups that assert at any sample
  uint32_t group_peak = 0u;     // max over g, j of s_g[j]
  uint32_t peak_key = 0u;       // (sum over g of s_g[j]) << 9 | 511 - j: the maximum is the first j of the highest sum
#pragma unroll
  for (int k = 0; k < ATTPC_NUM_TB / TG_THREADS; ++k) {
    const int j = t + k * TG_THREADS;
    int n_assert = 0;
    uint32_t sum = 0u;
    for (int g = 0; g < n_groups; ++g) {
      const int* P = cnt + g * ATTPC_NUM_TB;
      const int s = P[j] - (j >= tg.window ? P[j - tg.window] : 0);
      if (s >= tg.group_multiplicity) {
        ++n_assert;
        asserted |= 1u << g;
      }
      sum += (uint32_t)s;
      group_peak = (uint32_t)s > group_peak ? (uint32_t)s : group_peak;
    }
    if (n_assert >= tg.min_groups && j < first) first = j;
    const uint32_t key = (sum << 9) | (uint32_t)(ATTPC_NUM_TB - 1 - j);  // sum <= 10240 * 512 < 2^23
    peak_key = key > peak_key ? key : peak_key;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int f = __shfl_xor(first, off);
    first = f < first ? f : first;
    asserted |= __shfl_xor(asserted, off);
    const uint32_t gp = __shfl_xor(group_peak, off), pk = __shfl_xor(peak_key, off);
    group_peak = gp > group_peak ? gp : group_peak;
    peak_key = pk > peak_key ? pk : peak_key;
  }
  if (lane == 0) {
    red[wave][0] = (uint32_t)first;
    red[wave][1] = asserted;
    red[wave][2] = group_peak;
    red[wave][3] = peak_key;
  }
  block_sync();
#pragma unroll
  for (int w = 0; w < TG_WAVES; ++w) {
    first = (int)red[w][0] < first ? (int)red[w][0] : first;
    asserted |= red[w][1];
    group_peak = red[w][2] > group_peak ? red[w][2] : group_peak;
    peak_key = red[w][3] > peak_key ? red[w][3] : peak_key;
  }
  const int fired = first < ATTPC_NUM_TB ? 1 : 0;
  if (t == 0) {
    const int peak_sum = (int)(peak_key >> 9);
    int4* rec = reinterpret_cast<int4*>(a.records + e);
    rec[0] = make_int4(fired, fired ? first : -1, (int)asserted, (int)(hi - lo));
    rec[1] = make_int4(hit_pads, (int)group_peak, peak_sum,
                       peak_sum ? ATTPC_NUM_TB - 1 - (int)(peak_key & (uint32_t)(ATTPC_NUM_TB - 1)) : -1);
  }
  if (a.row_pass)
    for (int64_t row = lo + t; row < hi; row += TG_THREADS) a.row_pass[row] = (uint8_t)fired;
}

void launch_trigger(hipStream_t s, uint32_t n_events, const TriggerArgs& a) {
  hipLaunchKernelGGL(trigger_kernel, dim3(n_events), dim3(TG_THREADS), 0, s, a);
}

}  // namespace attpc
