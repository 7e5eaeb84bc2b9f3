// peaks.hip -- the first phase of Spyral on the device: kept trace rows -> peaks -> Spyral rows, run on a chunk's trace
// outputs in HBM behind the trace write pass (the contract is in include/attpc_engine.h, "trace rows").
//
// One wave per kept trace row (a workgroup IS one wave, so block_sync() costs nothing and every loop is uniform):
// a lane loads 8 consecutive samples (16 bytes, the 1 KiB row coalesced), y = trace - pedestal goes to 1 KiB of LDS,
// and the flat tops are walked there; prominence, width and integral of a survivor are searches by the whole wave
// over the samples in its registers (peak_passes): one lane walking through LDS would be a chain of up to 512
// dependent reads for a row's highest peak.
//   peak_count_kernel   candidates, separation, prominence / width / threshold -> a 512-bit map of the row's points
//                       (one byte per lane) and their number
//   peak_scan_*         the exclusive scan of those numbers over the chunk's trace rows
//   peak_write_kernel   the points of the map again (prominence and width for the interpolated positions, integral)
//                       -> 16-byte records (trace row, sample, amplitude, integral) at the row's scanned offset
//   peak_rows_kernel    one workgroup per event: centroid = sample + jitter, the per-event order (descending centroid,
//                       ascending pad on a tie; the counting sort of spyral.hip) and the rows of eight doubles
//
// The separation rule is sequential as written (highest priority first).  Here it runs in rounds on a priority table
// in LDS: an undecided candidate with a kept candidate within the distance is dropped; otherwise, if no undecided
// candidate of higher priority lies within the distance, it is kept.  By induction over the priority order this is the
// greedy result; every round decides at least the highest undecided candidate.
//
// Every f64 product is rounded before it is added (contract off for the whole file), and the two quotients of the
// contract -- both by an integer -- are long divisions on the mantissa (div_by_int_rn, div_rn.hpp): correctly rounded like the
// hardware's, without the fused multiply-adds of its expansion, so the generated code of these kernels has no
// v_fma_f64 at all and tests/test_peaks_cpu.py can say so.
// (before the includes: the helpers of common.hpp this file inlines -- u53 of the jitter -- follow the same rule)
#pragma clang fp contract(off)

#include "tracks_args.hpp"
#include "div_rn.hpp"

namespace attpc {

constexpr int PK_KEPT = 1 << 24;       // priority table: the candidate is kept (priorities are below 2^23)
constexpr int PK_ROWS_THREADS = 256;

// y = trace - pedestal of one row into the wave's LDS: lane l holds samples 8 l .. 8 l + 7
__device__ __forceinline__ void load_row(short* y, const int16_t* __restrict__ samples, int64_t row, int ped, int lane) {
  const uint4 v = reinterpret_cast<const uint4*>(samples + row * ATTPC_NUM_TB)[lane];
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    y[lane * 8 + 2 * i] = (short)((int)(short)(w[i] & 0xffffu) - ped);
    y[lane * 8 + 2 * i + 1] = (short)((int)(short)(w[i] >> 16) - ped);
  }
}

// wave-wide minimum / sum (every lane gets the result)
__device__ __forceinline__ int wave_min(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// the highest / lowest sample of a per-lane 8-bit map over the wave (the map is not empty), -1 / 512 for an empty one
__device__ __forceinline__ int wave_highest(uint32_t map, int none) {
  const unsigned long long lanes = __ballot(map != 0u);
  if (!lanes) return none;
  const int l = 63 - __clzll((long long)lanes);
  return l * 8 + 31 - __clz((int)__shfl(map, l));
}
__device__ __forceinline__ int wave_lowest(uint32_t map, int none) {
  const unsigned long long lanes = __ballot(map != 0u);
  if (!lanes) return none;
  const int l = __ffsll((unsigned long long)lanes) - 1;
  return l * 8 + __ffs((int)__shfl(map, l)) - 1;
}

// Steps 4 to 6 of the contract for the candidate at sample k (the same k in every lane), by the whole wave: lane l
// holds samples 8 l .. 8 l + 7 in v, y is the row in LDS.  The walks of the contract become searches: the walk of the
// prominence ends at the nearest higher sample, its minimum is the minimum in between with the position nearest the
// peak (a key of value and distance, minimised over the wave); the walk of the width ends at the nearest sample not
// above h, or at the base.  left_ip / right_ip: the interpolated positions of the width.
__device__ __forceinline__ bool peak_passes(const short* y, const int (&v)[8], int lane, int k, const PeakDev& pk,
                                            double& left_ip, double& right_ip) {
  const int top = y[k];
  uint32_t higher_l = 0u, higher_r = 0u;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int p = lane * 8 + s;
    if (v[s] > top) {
      higher_l |= p < k ? 1u << s : 0u;
      higher_r |= p > k ? 1u << s : 0u;
    }
  }
  const int stop_l = wave_highest(higher_l, -1), stop_r = wave_lowest(higher_r, ATTPC_NUM_TB);
  int key_l = 0x7fffffff, key_r = 0x7fffffff;  // (value + 4096) << 9 | distance order: of equal minima the nearest
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int p = lane * 8 + s, val = (v[s] + 4096) << 9;
    if (p > stop_l && p <= k) key_l = min(key_l, val | (ATTPC_NUM_TB - 1 - p));
    if (p >= k && p < stop_r) key_r = min(key_r, val | p);
  }
  key_l = wave_min(key_l);
  key_r = wave_min(key_r);
  const int left_min = (key_l >> 9) - 4096, left_base = ATTPC_NUM_TB - 1 - (key_l & (ATTPC_NUM_TB - 1));
  const int right_min = (key_r >> 9) - 4096, right_base = key_r & (ATTPC_NUM_TB - 1);
  const int prominence = top - (left_min > right_min ? left_min : right_min);
  if (!((double)prominence >= pk.prominence)) return false;
  const double scaled = (double)prominence * pk.rel_height;
  const double h = (double)top - scaled;
  uint32_t end_l = 0u, end_r = 0u;  // where the walks of the width can end: the base, or a sample not above h
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int p = lane * 8 + s;
    const bool below = !(h < (double)v[s]);
    end_l |= (p >= left_base && p <= k && (p == left_base || below)) ? 1u << s : 0u;
    end_r |= (p >= k && p <= right_base && (p == right_base || below)) ? 1u << s : 0u;
  }
  int i = wave_highest(end_l, left_base);
  left_ip = (double)i;
  if ((double)y[i] < h) left_ip += div_by_int_rn(h - (double)y[i], (int)y[i + 1] - (int)y[i]);
  i = wave_lowest(end_r, right_base);
  right_ip = (double)i;
  if ((double)y[i] < h) right_ip -= div_by_int_rn(h - (double)y[i], (int)y[i - 1] - (int)y[i]);
  const double width = right_ip - left_ip;
  if (!(width >= pk.min_width && width <= pk.max_width)) return false;
  return (double)top > pk.threshold;
}

__global__ __launch_bounds__(64) void peak_count_kernel(PeakDev pk, const int16_t* __restrict__ pedestals,
                                                         const int32_t* __restrict__ pads,
                                                         const int16_t* __restrict__ samples, uint8_t* __restrict__ maps,
                                                         uint32_t* __restrict__ counts,
                                                         const uint8_t* __restrict__ row_pass) {
  __shared__ short y[ATTPC_NUM_TB];
  __shared__ int prio[ATTPC_NUM_TB];  // candidate at sample j: (height + 4096) << 9 | j (| PK_KEPT), else 0
  __shared__ int block_max[64];       // the largest entry of every lane's eight
  const int64_t row = blockIdx.x;
  const int lane = (int)threadIdx.x;
  if (row_pass && !row_pass[row]) {  // uniform: the row's event did not fire (the trigger's gate), no points
    maps[row * 64 + lane] = 0;
    if (lane == 0) counts[row] = 0u;
    return;
  }
  const int ped = pedestals ? (int)pedestals[pads[row]] : 0;
  load_row(y, samples, row, ped, lane);
#pragma unroll
  for (int s = 0; s < 8; ++s) prio[lane * 8 + s] = 0;
  block_sync();
  int v[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s] = y[lane * 8 + s];
  // step 2: a rise starts a plateau; it is a peak, at its middle, when a fall ends it before the last sample
  for (int s = 0; s < 8; ++s) {
    const int j = lane * 8 + s;
    if (j < 1 || j > ATTPC_NUM_TB - 2 || !(y[j - 1] < v[s])) continue;
    int last = j;
    while (last + 1 < ATTPC_NUM_TB && y[last + 1] == v[s]) ++last;
    if (last + 1 < ATTPC_NUM_TB && y[last + 1] < v[s]) {
      const int pos = (j + last) >> 1;
      prio[pos] = ((v[s] + 4096) << 9) | pos;
    }
  }
  block_sync();
  // step 3: rounds over the candidates of this lane's samples; a lane owns its eight entries of the table
  int own[8];
  uint32_t undecided = 0u, kept = 0u;
  int mine = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    own[s] = prio[lane * 8 + s];
    undecided |= own[s] ? 1u << s : 0u;
    mine = own[s] > mine ? own[s] : mine;
  }
  block_max[lane] = mine;
  block_sync();
  const int reach = pk.distance - 1;
  while (__ballot(undecided != 0u) != 0ull) {
    uint32_t drop = 0u, keep = 0u;
    for (uint32_t rest = undecided; rest; rest &= rest - 1u) {
      const int s = __ffs((int)rest) - 1, pos = lane * 8 + s;
      const int lo = pos - reach < 0 ? 0 : pos - reach, hi = pos + reach > ATTPC_NUM_TB - 1 ? ATTPC_NUM_TB - 1 : pos + reach;
      const int lo_block = lo >> 3, hi_block = hi >> 3;
      int best = 0;  // a kept entry has the top bit: the maximum says both "a kept one is near" and "the highest is"
      if (lo_block == hi_block) {
        for (int q = lo; q <= hi; ++q) best = max(best, prio[q]);
      } else {
        for (int q = lo; q < (lo_block + 1) * 8; ++q) best = max(best, prio[q]);
        for (int b = lo_block + 1; b < hi_block; ++b) best = max(best, block_max[b]);
        for (int q = hi_block * 8; q <= hi; ++q) best = max(best, prio[q]);
      }
      if (best & PK_KEPT) drop |= 1u << s;
      else if (best == own[s]) keep |= 1u << s;
    }
    block_sync();
    mine = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (drop >> s & 1u) own[s] = 0;
      if (keep >> s & 1u) own[s] |= PK_KEPT;
      if ((drop | keep) >> s & 1u) prio[lane * 8 + s] = own[s];
      mine = own[s] > mine ? own[s] : mine;
    }
    block_max[lane] = mine;
    undecided &= ~(drop | keep);
    kept |= keep;
    block_sync();
  }
  // steps 4 to 6, survivor by survivor, the whole wave on each
  uint32_t points = 0u;
  for (unsigned long long lanes = __ballot(kept != 0u); lanes; lanes &= lanes - 1ull) {
    const int l = __ffsll(lanes) - 1;
    for (uint32_t rest = __shfl(kept, l); rest; rest &= rest - 1u) {
      const int s = __ffs((int)rest) - 1;
      double left_ip, right_ip;
      const bool pass = peak_passes(y, v, lane, l * 8 + s, pk, left_ip, right_ip);
      if (pass && lane == l) points |= 1u << s;
    }
  }
  maps[row * 64 + lane] = (uint8_t)points;
  const int n = wave_sum(__popc(points));
  if (lane == 0) counts[row] = (uint32_t)n;
}

__global__ __launch_bounds__(64) void peak_write_kernel(PeakDev pk, const int16_t* __restrict__ pedestals,
                                                         const int32_t* __restrict__ pads,
                                                         const int16_t* __restrict__ samples,
                                                         const uint8_t* __restrict__ maps,
                                                         const int64_t* __restrict__ row_start, uint4* __restrict__ records,
                                                         const uint8_t* __restrict__ row_pass) {
  __shared__ short y[ATTPC_NUM_TB];
  const int64_t row = blockIdx.x;
  const int lane = (int)threadIdx.x;
  if (row_pass && !row_pass[row]) return;  // uniform (such a row has no points either: the count pass left none)
  int64_t o = row_start[row];
  if (row_start[row + 1] == o) return;  // uniform
  const int ped = pedestals ? (int)pedestals[pads[row]] : 0;
  load_row(y, samples, row, ped, lane);
  block_sync();
  int v[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s] = y[lane * 8 + s];
  const uint32_t points = maps[row * 64 + lane];
  for (unsigned long long lanes = __ballot(points != 0u); lanes; lanes &= lanes - 1ull) {
    const int l = __ffsll(lanes) - 1;
    for (uint32_t rest = __shfl(points, l); rest; rest &= rest - 1u) {
      const int k = l * 8 + __ffs((int)rest) - 1;
      double left_ip = 0.0, right_ip = 0.0;
      (void)peak_passes(y, v, lane, k, pk, left_ip, right_ip);
      const int from = (int)floor(left_ip), to = (int)ceil(right_ip);
      int part = 0;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int p = lane * 8 + s;
        part += (p >= from && p < to) ? (v[s] < 0 ? -v[s] : v[s]) : 0;
      }
      const int integral = wave_sum(part);
      if (lane == 0) records[o] = make_uint4((uint32_t)row, (uint32_t)k, (uint32_t)(int)y[k], (uint32_t)integral);
      ++o;
    }
  }
}

// The exclusive scan of the points per trace row (millions of rows a chunk) in three steps: every workgroup scans
// PK_SCAN_ITEMS counts and leaves its total, one workgroup scans the totals, every workgroup adds its start.
constexpr int PK_SCAN_THREADS = 256;
constexpr int PK_SCAN_ITEMS = PK_SCAN_THREADS * 8;

__device__ __forceinline__ long long block_exclusive(long long v, long long* wave_sums, int n_waves, long long& total) {
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  long long incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const long long up = __shfl_up(incl, off);
    incl += lane >= off ? up : 0ll;
  }
  if (lane == 63) wave_sums[wave] = incl;
  block_sync();
  long long before = 0;
  total = 0;
  for (int w = 0; w < n_waves; ++w) {
    before += w < wave ? wave_sums[w] : 0ll;
    total += wave_sums[w];
  }
  block_sync();
  return before + incl - v;
}

__global__ __launch_bounds__(PK_SCAN_THREADS) void peak_scan_blocks_kernel(const uint32_t* __restrict__ counts, uint32_t n,
                                                                            int64_t* __restrict__ out,
                                                                            uint32_t* __restrict__ block_sums) {
  __shared__ long long wave_sums[PK_SCAN_THREADS / 64];
  const uint32_t first = blockIdx.x * (uint32_t)PK_SCAN_ITEMS + threadIdx.x * 8u;
  uint32_t c[8];
  long long local = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c[i] = first + i < n ? counts[first + i] : 0u;
    local += c[i];
  }
  long long total;
  long long run = block_exclusive(local, wave_sums, PK_SCAN_THREADS / 64, total);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (first + i < n) out[first + i] = run;
    run += c[i];
  }
  if (threadIdx.x == 0) block_sums[blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(1024) void peak_scan_sums_kernel(const uint32_t* __restrict__ block_sums, uint32_t n_blocks,
                                                               int64_t* __restrict__ block_start) {
  __shared__ long long wave_sums[16];
  const uint32_t per = (n_blocks + 1023u) / 1024u, first = threadIdx.x * per;
  long long local = 0;
  for (uint32_t i = first; i < first + per && i < n_blocks; ++i) local += block_sums[i];
  long long total;
  long long run = block_exclusive(local, wave_sums, 16, total);
  for (uint32_t i = first; i < first + per && i < n_blocks; ++i) {
    block_start[i] = run;
    run += block_sums[i];
  }
  if (threadIdx.x == 0) block_start[n_blocks] = total;
}

__global__ __launch_bounds__(PK_SCAN_THREADS) void peak_scan_add_kernel(uint32_t n, uint32_t n_blocks,
                                                                         const int64_t* __restrict__ block_start,
                                                                         int64_t* __restrict__ out) {
  const int64_t start = block_start[blockIdx.x];
  const uint32_t first = blockIdx.x * (uint32_t)PK_SCAN_ITEMS + threadIdx.x * 8u;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (first + i < n) out[first + i] += start;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = block_start[n_blocks];
}

// ev_start[e] = row_start[kept_start[e]]: the CSR offsets of the events' points from those of the trace rows
__global__ __launch_bounds__(256) void peak_event_start_kernel(uint32_t n_events, const int64_t* __restrict__ kept_start,
                                                                const int64_t* __restrict__ row_start,
                                                                int64_t* __restrict__ ev_start) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e <= n_events) ev_start[e] = row_start[kept_start[e]];
}

// The points of one event as rows of eight doubles, in descending centroid (ascending z), equal centroids in ascending
// pad.  The sort is spyral_write_kernel's: counting sort over 512 samples x 16 sixteenths of the jitter, then a rank
// inside the bin on the centroid itself; records of an event come in ascending pad, so the earlier record wins a tie.
constexpr int PK_SORT_SUB = 16;
constexpr int PK_SORT_BINS = ATTPC_NUM_TB * PK_SORT_SUB;
constexpr int PK_BINS_PER_THREAD = PK_SORT_BINS / PK_ROWS_THREADS;

__global__ __launch_bounds__(PK_ROWS_THREADS) void peak_rows_kernel(SpyralDev sp, uint32_t key_word, uint64_t first_event,
                                                                     const int64_t* __restrict__ ev_start,
                                                                     const uint4* __restrict__ records,
                                                                     const int32_t* __restrict__ pads,
                                                                     const int64_t* __restrict__ labels,
                                                                     double* __restrict__ centroid,
                                                                     uint32_t* __restrict__ sort_idx,
                                                                     double* __restrict__ sort_key,
                                                                     double* __restrict__ rows,
                                                                     int64_t* __restrict__ out_labels,
                                                                     unsigned long long* __restrict__ sums) {
  __shared__ uint32_t bin_cursor[PK_SORT_BINS];
  __shared__ uint32_t wave_total[PK_ROWS_THREADS / 64];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = ev_start[e];
  const uint32_t n = (uint32_t)(ev_start[e + 1] - lo);
  if (n == 0u) return;  // uniform
  const uint64_t event = first_event + e;
  const uint32_t ev_lo = (uint32_t)event, ev_hi = (uint32_t)(event >> 32);
  for (int b = t; b < PK_SORT_BINS; b += PK_ROWS_THREADS) bin_cursor[b] = 0u;
  block_sync();
  auto bin_of = [](double c) -> int {  // descending centroid; monotone in c (c = 512.0 can come of rounding 511 + u)
    int whole = (int)c;
    whole = whole > ATTPC_NUM_TB - 1 ? ATTPC_NUM_TB - 1 : whole;
    int sub = (int)((c - (double)whole) * (double)PK_SORT_SUB);
    sub = sub > PK_SORT_SUB - 1 ? PK_SORT_SUB - 1 : sub;
    return (ATTPC_NUM_TB - 1 - whole) * PK_SORT_SUB + (PK_SORT_SUB - 1 - sub);
  };
  unsigned long long key_sum = 0ull;
  for (uint32_t i = (uint32_t)t; i < n; i += PK_ROWS_THREADS) {
    const uint4 rec = records[lo + i];
    const uint32_t pad = (uint32_t)pads[rec.x];
    const double c = (double)rec.y + jitter_uniform_k(key_word, ev_lo, ev_hi, (rec.y << 14) | pad);
    centroid[lo + i] = c;
    atomicAdd(&bin_cursor[bin_of(c)], 1u);
    key_sum += (event << 23) + ((unsigned long long)pad << 9) + rec.y;
  }
  for (int off = 32; off > 0; off >>= 1) key_sum += __shfl_down(key_sum, off);
  if (lane == 0 && key_sum) atomicAdd(&sums[0], key_sum);
  block_sync();
  {  // exclusive prefix over the bins
    uint32_t local = 0u;
    for (int k = 0; k < PK_BINS_PER_THREAD; ++k) local += bin_cursor[t * PK_BINS_PER_THREAD + k];
    uint32_t incl = local;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off);
      incl += lane >= off ? up : 0u;
    }
    if (lane == 63) wave_total[wave] = incl;
    block_sync();
    uint32_t run = incl - local;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    for (int k = 0; k < PK_BINS_PER_THREAD; ++k) {
      const int b = t * PK_BINS_PER_THREAD + k;
      const uint32_t c = bin_cursor[b];
      bin_cursor[b] = run;
      run += c;
    }
  }
  block_sync();
  for (uint32_t i = (uint32_t)t; i < n; i += PK_ROWS_THREADS) {
    const double c = centroid[lo + i];
    const uint32_t p = atomicAdd(&bin_cursor[bin_of(c)], 1u);
    sort_idx[lo + p] = i;
    sort_key[lo + p] = c;
  }
  __threadfence_block();  // (the lists are written and read by this workgroup only)
  block_sync();
  const int32_t span = (int32_t)(sp.window_edge - sp.mm_edge);
  for (uint32_t p = (uint32_t)t; p < n; p += PK_ROWS_THREADS) {
    const uint32_t ri = sort_idx[lo + p];
    const double c = sort_key[lo + p];
    const int b = bin_of(c);
    const uint32_t b_lo = b > 0 ? bin_cursor[b - 1] : 0u, b_hi = bin_cursor[b];
    uint32_t rank = 0u;
    for (uint32_t q = b_lo; q < b_hi; ++q) {
      const double other = sort_key[lo + q];
      rank += (other > c || (other == c && sort_idx[lo + q] < ri)) ? 1u : 0u;
    }
    const uint4 rec = records[lo + ri];
    const int32_t pad = pads[rec.x];
    const int64_t o = lo + b_lo + rank;
    double* row = rows + 8 * o;
    row[0] = sp.pad_centers[2 * pad];
    row[1] = sp.pad_centers[2 * pad + 1];
    row[2] = div_by_int_rn(sp.window_edge - c, span) * sp.length * 1000.0;  // writer.py:103-105
    row[3] = (double)(int32_t)rec.z;
    row[4] = (double)(int32_t)rec.w;
    row[5] = (double)pad;
    row[6] = c;
    row[7] = sp.pad_sizes[pad];
    out_labels[o] = labels[rec.x];
  }
}

void launch_peak_count(hipStream_t s, const PeakDev& pk, const int16_t* pedestals, uint32_t n_rows, const int32_t* pads,
                       const int16_t* samples, uint8_t* maps, uint32_t* counts, const uint8_t* row_pass) {
  hipLaunchKernelGGL(peak_count_kernel, dim3(n_rows), dim3(64), 0, s, pk, pedestals, pads, samples, maps, counts, row_pass);
}
uint32_t peak_scan_blocks(uint32_t n_rows) { return (n_rows + (uint32_t)PK_SCAN_ITEMS - 1u) / (uint32_t)PK_SCAN_ITEMS; }
void launch_peak_scan(hipStream_t s, const uint32_t* counts, uint32_t n_rows, int64_t* row_start, uint32_t* block_sums,
                      int64_t* block_start) {
  const uint32_t blocks = peak_scan_blocks(n_rows);  // >= 1: n_rows > 0
  hipLaunchKernelGGL(peak_scan_blocks_kernel, dim3(blocks), dim3(PK_SCAN_THREADS), 0, s, counts, n_rows, row_start, block_sums);
  hipLaunchKernelGGL(peak_scan_sums_kernel, dim3(1), dim3(1024), 0, s, block_sums, blocks, block_start);
  hipLaunchKernelGGL(peak_scan_add_kernel, dim3(blocks), dim3(PK_SCAN_THREADS), 0, s, n_rows, blocks, block_start, row_start);
}
void launch_peak_event_start(hipStream_t s, uint32_t n_events, const int64_t* kept_start, const int64_t* row_start,
                             int64_t* ev_start) {
  hipLaunchKernelGGL(peak_event_start_kernel, dim3(n_events / 256u + 1u), dim3(256), 0, s, n_events, kept_start, row_start,
                     ev_start);
}
void launch_peak_write(hipStream_t s, const PeakDev& pk, const int16_t* pedestals, uint32_t n_rows, const int32_t* pads,
                       const int16_t* samples, const uint8_t* maps, const int64_t* row_start, uint4* records,
                       const uint8_t* row_pass) {
  hipLaunchKernelGGL(peak_write_kernel, dim3(n_rows), dim3(64), 0, s, pk, pedestals, pads, samples, maps, row_start, records,
                     row_pass);
}
void launch_peak_rows(hipStream_t s, const SpyralDev& sp, uint64_t seed, uint32_t n_events, uint64_t first_event,
                      const int64_t* ev_start, const uint4* records, const int32_t* pads, const int64_t* labels,
                      double* centroid, uint32_t* sort_idx, double* sort_key, double* rows, int64_t* out_labels,
                      unsigned long long* sums) {
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  const uint32_t key_word = seed_lo ^ ((seed_hi << 13) | (seed_hi >> 19)) ^ DOMAIN_PEAK_JITTER;
  hipLaunchKernelGGL(peak_rows_kernel, dim3(n_events), dim3(PK_ROWS_THREADS), 0, s, sp, key_word, first_event, ev_start,
                     records, pads, labels, centroid, sort_idx, sort_key, rows, out_labels, sums);
}

}  // namespace attpc
