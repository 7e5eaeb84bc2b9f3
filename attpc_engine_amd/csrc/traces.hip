// traces.hip -- digitised GET pad traces on the device, run on the event-ordered cloud of a chunk before D2H
// (EXTENSION: the reference stops at point clouds; the contract is written out in include/attpc_engine.h).
//
// One workgroup per event, two passes with a device scan in between (as spyral.hip):
//   count: LDS counting sort of the event's rows by pad (10 240 pads x 4 B), the pad-grouped row list and the list of
//          hit pads (ascending) into a global scratch range of the event's own cloud rows; then one wave per hit pad
//          works out the pad's trace and keeps the verdict max > threshold; a block scan turns the verdicts into each
//          kept pad's rank inside the event.
//   write: one wave per kept pad works the trace out again and writes pad, label and 512 samples (1 KiB, coalesced) at
//          kept_start[event] + rank; checksums are summed per workgroup, one global atomic per event.
// A pad's trace: its rows are scattered into a 512-entry LDS table q[t] (0 where no row exists; with the micromegas
// gain on, gain.hip, the row's gained charge from TraceDev::gained in place of the cloud's), the non-zero entries
// are walked in ascending t, 64 at a time by ballot, and every lane keeps the samples j = lane + 64 s (s = 0..7) as 8 f64
// accumulators, reading R from LDS.  The dense walk gives the same bits as the sparse ordered sum of the contract: the
// terms it skips would add +0.0 to an accumulator that starts at +0.0 and never becomes -0.0.
// Bound: the latency of the per-row LDS reads (the row's charge, then 8 ds_read_b64 of R per lane) at 16 waves per CU --
// not LDS bandwidth, FP64 issue or HBM (profiles/r04_trace_rate.md).
// Electronic noise and pedestals (attpc_trace_configure_noise): both kernels are templated on NOISE; the NOISE = false
// instantiations are the noiseless code.  With NOISE, a pad's samples get its pedestal and one table-driven noise draw
// each (add_noise), both passes draw the same numbers, and the count pass's verdict is taken above the pedestal.  The
// noise table (2 KiB of cdf, 0.5 KiB of guide) sits in LDS: the count pass stays at two workgroups per CU.
// Readout of noise-only pads (attpc_trace_configure_readout, PARTIAL / FULL): the count pass is templated on RO as well
// (the RO = false instantiations are the hit-mode code); with RO it drops the rows of pads outside the readout set S and
// in FULL keeps every hit pad of S.  Two kernels of their own follow it:
//   scan:  one workgroup per event, empty events included; one wave per candidate pad (in S, no rows) takes the
//          contract's two Philox calls per lane, compares the 8 words with the cutoff u32 of the decision rule and
//          ballots; the kept bitmap (hit and noise-only) gets a popcount prefix per word, which gives every kept pad its
//          rank in the event and overwrites the hit pads' ranks of the count pass.  No LDS tables: full occupancy.
//   noise write: one wave per kept noise-only pad writes pad, label -1 and the clamped pedestal plus noise.
// The scan is skipped when the decision rule keeps no noise-only pad (PARTIAL, thr >= 0 and a cutoff above the table):
// the count pass's ranks are then already those of the union.
// Common-mode noise (attpc_trace_configure_common_mode): common_mode_kernel, in front of the count pass, draws the 512
// values of every (event, group) of the chunk with noise_values -- the stage's own table and domain, the group in the
// pad's place -- and stores them as int16 in the lanes' own order (lane l: samples l + 64 s, 16 contiguous bytes).  Every
// kernel that makes samples is templated on CM (the CM = false instantiations are the code without the stage): a wave
// working on a pad of group g != 255 fetches its group's values with one 16-byte load per lane and adds them to the pad
// noise before the clamp; the scan's verdict for such a pad makes the pad's own draw and compares the sums.  With CM the
// NOISE kernels run whether a pad table is configured or not (n_p = 0, ped_p = 0 without one).
#include "tracks_args.hpp"

namespace attpc {

constexpr int TR_THREADS = 512;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_PADS_PER_THREAD = ATTPC_NUM_PADS / TR_THREADS;  // 20
static_assert(ATTPC_NUM_PADS % TR_THREADS == 0, "the pad table is split evenly over the threads");
static_assert(ATTPC_NUM_TB == 512, "a lane keeps 8 samples");

// Product rounded, then added: no contraction into a fused multiply-add (tests/test_traces_cpu.py checks the code).
__device__ __forceinline__ double mul_then_add(double acc, double q, double r) {
#pragma clang fp contract(off)
  const double prod = q * r;
  return acc + prod;
}

struct PadTrace {
  int v[8];       // trace samples j = lane + 64 s
  int max;        // over the pad's 512 samples (wave-uniform)
  long long label;
};

// The trace of the k-th hit pad of the event, worked out by one whole wave.  `qt`: the wave's 512-entry LDS table.
__device__ __forceinline__ PadTrace pad_trace(const TraceDev& tr, const double* resp, double* qt, int lane,
                                              const double* __restrict__ points, const int64_t* __restrict__ labels,
                                              const uint32_t* __restrict__ row, int64_t lo, uint32_t start, uint32_t end) {
  for (int s = 0; s < 8; ++s) qt[lane + 64 * s] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double best_q = -1.0;
  int best_t = ATTPC_NUM_TB;
  long long best_label = 0;
  for (uint32_t i = start + (uint32_t)lane; i < end; i += 64u) {
    const int64_t r = lo + row[lo + i];
    const int t = (int)floor(points[3 * r + 1]);  // in 0..511: rows outside were never placed
    const double q = points[3 * r + 2];  // the label rule stays on the cloud's own charge
    qt[t] = tr.gained ? tr.gained[r] : q;
    if (q > best_q || (q == best_q && t < best_t)) {
      best_q = q;
      best_t = t;
      best_label = labels[r];
    }
  }
  for (int off = 32; off > 0; off >>= 1) {  // the largest q, the smallest t on a tie
    const double oq = __shfl_xor(best_q, off);
    const int ot = __shfl_xor(best_t, off);
    const long long ol = __shfl_xor(best_label, off);
    if (oq > best_q || (oq == best_q && ot < best_t)) {
      best_q = oq;
      best_t = ot;
      best_label = ol;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double acc[8];
  for (int s = 0; s < 8; ++s) acc[s] = 0.0;
  for (int c = 0; c < 8; ++c) {
    const double qc = qt[64 * c + lane];
    unsigned long long mask = __ballot(qc != 0.0);
    while (mask) {
      const int b = __builtin_ctzll(mask);
      mask &= mask - 1ull;
      const double q = __shfl(qc, b);
      const int k0 = lane + tr.offset - (64 * c + b);  // response index of sample j = lane: k = j + offset - t
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int k = k0 + 64 * s;
        if ((unsigned)k < (unsigned)ATTPC_NUM_TB) acc[s] = mul_then_add(acc[s], q, resp[k]);
      }
    }
  }
  PadTrace out;
  int m = 0;
  for (int s = 0; s < 8; ++s) {
    const double a = acc[s] < 4095.0 ? acc[s] : 4095.0;
    out.v[s] = (int)rint(a);  // half to even
    m = out.v[s] > m ? out.v[s] : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  out.max = m;
  out.label = best_label;
  return out;
}

// The noise and the pedestal of one pad (include/attpc_engine.h): sample j = lane + 64 s takes word s % 4 of Philox
// call h = s / 4, counter (event, pad * 128 + 2 * lane + h, domain), so a lane makes two calls per pad.  The level
// index #{k : cdf[k] <= u} starts at the guide entry of u's top byte and walks the few cdf entries inside that byte.
// Afterwards pt.max = max_j (trace_p[j] - ped_p), the quantity the threshold is taken on.
__device__ __forceinline__ void noise_values(int n[8], const TraceNoiseDev& nz, const uint32_t* cdf,
                                             const uint16_t* guide, uint64_t seed, uint64_t event, uint32_t pad,
                                             int lane) {
  for (int s = 0; s < 8; ++s) n[s] = 0;
  if (nz.n_levels > 0) {  // uniform
    const int n_cdf = nz.n_levels - 1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t u[4];
      philox4x32<10>((uint32_t)event, (uint32_t)(event >> 32), pad * 128u + 2u * (uint32_t)lane + (uint32_t)h, nz.domain,
                     (uint32_t)seed, (uint32_t)(seed >> 32), u);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        int i = guide[u[w] >> 24];
        while (i < n_cdf && cdf[i] <= u[w]) ++i;
        n[4 * h + w] = nz.min_level + i;
      }
    }
  }
}

// The group of a pad in the common-mode map (wave-uniform; 255 = the pad has no common-mode term).
__device__ __forceinline__ uint32_t common_group(const CommonDev& cm, uint32_t pad) {
  return cm.groups ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cm.groups[pad]) : 0u;
}

// n[s] += c_g[lane + 64 s] for group g (!= 255) of event e of the launch: the lane's 8 values are 16 contiguous bytes
// of the buffer common_mode_kernel wrote, 1 KiB coalesced over the wave.
struct alignas(16) CommonLane {
  int16_t v[8];
};
__device__ __forceinline__ void add_common(int n[8], const CommonDev& cm, uint32_t e, uint32_t g, int lane) {
  const CommonLane c =
      *reinterpret_cast<const CommonLane*>(cm.values + ((size_t)e * (size_t)cm.n_groups + g) * ATTPC_NUM_TB + 8 * lane);
  for (int s = 0; s < 8; ++s) n[s] += (int)c.v[s];
}

// (`e`: the event within the launch, which places its common-mode values; `event` its global id)
template <bool CM>
__device__ __forceinline__ void add_noise(PadTrace& pt, const TraceNoiseDev& nz, const uint32_t* cdf,
                                          const uint16_t* guide, uint64_t seed, uint64_t event, uint32_t pad, int lane,
                                          const CommonDev& cm, uint32_t e) {
  const int ped = nz.pedestals ? (int)nz.pedestals[pad] : 0;
  int n[8];
  noise_values(n, nz, cdf, guide, seed, event, pad, lane);
  if constexpr (CM) {
    const uint32_t g = common_group(cm, pad);
    if (g != 255u) add_common(n, cm, e, g, lane);  // uniform
  }
  int m = -4096;  // below any trace_p[j] - ped_p (>= -4095)
  for (int s = 0; s < 8; ++s) {
    int v = pt.v[s] + ped + n[s];
    v = v < 0 ? 0 : (v > 4095 ? 4095 : v);
    pt.v[s] = v;
    m = v - ped > m ? v - ped : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  pt.max = m;
}

// A row of the count pass with readout RO: in range and on a pad of the readout set (rows elsewhere are dropped).
template <bool RO>
__device__ __forceinline__ bool trace_row_read(double padf, double tb, const TraceReadoutDev& ro) {
  if constexpr (RO) return trace_row_ok(padf, tb) && ((ro.channels[(int)padf >> 5] >> ((int)padf & 31)) & 1u);
  return trace_row_ok(padf, tb);
}

template <bool NOISE, bool RO, bool CM>
__global__ __launch_bounds__(TR_THREADS) void trace_count_kernel(TraceDev tr, TraceNoiseDev nz, uint64_t seed,
                                                                 uint64_t first_event,
                                                                 const int64_t* __restrict__ event_start,
                                                                 const double* __restrict__ points,
                                                                 const int64_t* __restrict__ labels, TraceScratch sc,
                                                                 uint32_t* __restrict__ kept, TraceReadoutDev ro,
                                                                 CommonDev cm) {
  static_assert(NOISE || !CM, "the common-mode term is added where the pad noise is");
  __shared__ uint32_t cursor[ATTPC_NUM_PADS];  // counts, then the next free place of every pad's group
  __shared__ double resp[ATTPC_NUM_TB];
  __shared__ uint32_t noise_cdf[ATTPC_MAX_NOISE_LEVELS];  // (NOISE only: the noiseless kernel never names them)
  __shared__ uint16_t noise_guide[256];
  __shared__ double qtab[TR_WAVES][ATTPC_NUM_TB];
  __shared__ uint32_t wave_rows[TR_WAVES], wave_hits[TR_WAVES];
  __shared__ uint32_t n_hits, n_placed, kept_run;
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = event_start[e], hi = event_start[e + 1];
  if (hi <= lo) {  // uniform
    if (t == 0) {
      kept[e] = 0u;
      sc.info[2 * e] = 0u;
      sc.info[2 * e + 1] = 0u;
    }
    return;
  }
  for (int p = t; p < ATTPC_NUM_PADS; p += TR_THREADS) cursor[p] = 0u;
  for (int j = t; j < ATTPC_NUM_TB; j += TR_THREADS) resp[j] = tr.response[j];
  if constexpr (NOISE) {
    if (!CM || nz.n_levels > 0) {  // uniform (with CM the pad table may be off: no table on the device then)
      for (int i = t; i < ATTPC_MAX_NOISE_LEVELS; i += TR_THREADS) noise_cdf[i] = nz.cdf[i];
      if (t < 256) noise_guide[t] = nz.guide[t];
    }
  }
  if (t == 0) kept_run = 0u;
  block_sync();
  for (int64_t r = lo + t; r < hi; r += TR_THREADS) {
    const double padf = points[3 * r], tb = points[3 * r + 1];
    if (trace_row_read<RO>(padf, tb, ro)) atomicAdd(&cursor[(int)padf], 1u);
  }
  block_sync();
  {  // exclusive prefix over the pads (rows and hit pads): 20 consecutive pads per thread, wave scan, wave offsets
    uint32_t rows = 0u, hits = 0u;
    for (int k = 0; k < TR_PADS_PER_THREAD; ++k) {
      const uint32_t c = cursor[t * TR_PADS_PER_THREAD + k];
      rows += c;
      hits += c ? 1u : 0u;
    }
    uint32_t rows_incl = rows, hits_incl = hits;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t ur = __shfl_up(rows_incl, off), uh = __shfl_up(hits_incl, off);
      rows_incl += lane >= off ? ur : 0u;
      hits_incl += lane >= off ? uh : 0u;
    }
    if (lane == 63) {
      wave_rows[wave] = rows_incl;
      wave_hits[wave] = hits_incl;
    }
    block_sync();
    uint32_t run = rows_incl - rows, hrun = hits_incl - hits;
    for (int w = 0; w < wave; ++w) {
      run += wave_rows[w];
      hrun += wave_hits[w];
    }
    for (int k = 0; k < TR_PADS_PER_THREAD; ++k) {
      const int p = t * TR_PADS_PER_THREAD + k;
      const uint32_t c = cursor[p];
      if (c) {
        sc.hit[lo + hrun] = (uint32_t)p;
        sc.hit_start[lo + hrun] = run;
        ++hrun;
      }
      cursor[p] = run;
      run += c;
    }
    if (t == TR_THREADS - 1) {
      n_hits = hrun;
      n_placed = run;
    }
  }
  block_sync();
  for (int64_t r = lo + t; r < hi; r += TR_THREADS) {
    const double padf = points[3 * r], tb = points[3 * r + 1];
    if (trace_row_read<RO>(padf, tb, ro)) sc.row[lo + atomicAdd(&cursor[(int)padf], 1u)] = (uint32_t)(r - lo);
  }
  // workgroup scope is enough: the lists are written and read by this workgroup only (as spyral_write_kernel)
  __threadfence_block();
  block_sync();
  const uint32_t H = n_hits, V = n_placed;
  for (uint32_t k = (uint32_t)wave; k < H; k += TR_WAVES) {
    if constexpr (RO) {
      if (ro.full) {  // uniform: every pad of S is read out
        if (lane == 0) sc.rank[lo + k] = 1;
        continue;
      }
    }
    const uint32_t start = sc.hit_start[lo + k], end = k + 1 < H ? sc.hit_start[lo + k + 1] : V;
    PadTrace pt = pad_trace(tr, resp, qtab[wave], lane, points, labels, sc.row, lo, start, end);
    if constexpr (NOISE) add_noise<CM>(pt, nz, noise_cdf, noise_guide, seed, first_event + e, sc.hit[lo + k], lane, cm, e);
    if (lane == 0) sc.rank[lo + k] = (double)pt.max > tr.threshold ? 1 : 0;
  }
  __threadfence_block();
  block_sync();
  // verdicts -> ranks among the kept pads (ascending pad), TR_THREADS hit pads at a time
  for (uint32_t base = 0; base < H; base += TR_THREADS) {
    const uint32_t k = base + (uint32_t)t;
    const bool keep = k < H && sc.rank[lo + k] != 0;
    const unsigned long long m = __ballot(keep);
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(m);
    block_sync();
    uint32_t before = kept_run;
    for (int w = 0; w < wave; ++w) before += wave_hits[w];
    if (k < H) sc.rank[lo + k] = keep ? (int32_t)(before + below) : -1;
    block_sync();
    if (t == 0) {
      uint32_t all = 0u;
      for (int w = 0; w < TR_WAVES; ++w) all += wave_hits[w];
      kept_run += all;
    }
    block_sync();
  }
  if (t == 0) {
    kept[e] = kept_run;
    sc.info[2 * e] = H;
    sc.info[2 * e + 1] = V;
  }
}

template <bool NOISE, bool CM>
__global__ __launch_bounds__(TR_THREADS) void trace_write_kernel(TraceDev tr, TraceNoiseDev nz, uint64_t seed,
                                                                 uint64_t first_event,
                                                                 const int64_t* __restrict__ event_start,
                                                                 const double* __restrict__ points,
                                                                 const int64_t* __restrict__ labels, TraceScratch sc,
                                                                 const int64_t* __restrict__ kept_start,
                                                                 int32_t* __restrict__ pads, int16_t* __restrict__ samples,
                                                                 int64_t* __restrict__ out_labels,
                                                                 unsigned long long* __restrict__ sums, CommonDev cm) {
  static_assert(NOISE || !CM, "the common-mode term is added where the pad noise is");
  __shared__ double resp[ATTPC_NUM_TB];
  __shared__ double qtab[TR_WAVES][ATTPC_NUM_TB];
  __shared__ unsigned long long wave_sum[TR_WAVES][2];
  __shared__ uint32_t noise_cdf[ATTPC_MAX_NOISE_LEVELS];  // (NOISE only)
  __shared__ uint16_t noise_guide[256];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t out0 = kept_start[e];
  if (kept_start[e + 1] == out0) return;  // uniform
  const int64_t lo = event_start[e];
  const uint32_t H = sc.info[2 * e], V = sc.info[2 * e + 1];
  for (int j = t; j < ATTPC_NUM_TB; j += TR_THREADS) resp[j] = tr.response[j];
  if constexpr (NOISE) {
    if (!CM || nz.n_levels > 0) {  // uniform
      for (int i = t; i < ATTPC_MAX_NOISE_LEVELS; i += TR_THREADS) noise_cdf[i] = nz.cdf[i];
      if (t < 256) noise_guide[t] = nz.guide[t];
    }
  }
  block_sync();
  const unsigned long long event = first_event + e;
  unsigned long long sample_sum = 0ull, pad_sum = 0ull;  // lane parts
  for (uint32_t k = (uint32_t)wave; k < H; k += TR_WAVES) {
    const int32_t rank = sc.rank[lo + k];
    if (rank < 0) continue;  // uniform
    const uint32_t start = sc.hit_start[lo + k], end = k + 1 < H ? sc.hit_start[lo + k + 1] : V;
    PadTrace pt = pad_trace(tr, resp, qtab[wave], lane, points, labels, sc.row, lo, start, end);
    const int64_t o = out0 + rank;
    const uint32_t pad = sc.hit[lo + k];
    if constexpr (NOISE) add_noise<CM>(pt, nz, noise_cdf, noise_guide, seed, event, pad, lane, cm, e);
    int16_t* dst = samples + o * ATTPC_NUM_TB;
    for (int s = 0; s < 8; ++s) {
      const int j = lane + 64 * s;
      dst[j] = (int16_t)pt.v[s];
      sample_sum += (unsigned long long)(long long)pt.v[s] * (unsigned long long)(j + 1);
    }
    if (lane == 0) {
      pads[o] = (int32_t)pad;
      out_labels[o] = pt.label;
      pad_sum += (event << 14) + (unsigned long long)pad;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sample_sum += __shfl_xor(sample_sum, off);
    pad_sum += __shfl_xor(pad_sum, off);
  }
  if (lane == 0) {
    wave_sum[wave][0] = sample_sum;
    wave_sum[wave][1] = pad_sum;
  }
  block_sync();
  if (t < 2) {
    unsigned long long v = 0ull;
    for (int w = 0; w < TR_WAVES; ++w) v += wave_sum[w][t];
    atomicAdd(sums + t, v);
  }
}

template <bool NOISE, bool RO, bool CM>
void launch_count(hipStream_t s, const TraceDev& tr, const TraceNoiseDev& nz, uint64_t seed, uint32_t n_events,
                  uint64_t first_event, const int64_t* event_start, const double* points, const int64_t* labels,
                  TraceScratch sc, uint32_t* kept, const TraceReadoutDev& ro, const CommonDev& cm) {
  hipLaunchKernelGGL((trace_count_kernel<NOISE, RO, CM>), dim3(n_events), dim3(TR_THREADS), 0, s, tr, nz, seed,
                     first_event, event_start, points, labels, sc, kept, ro, cm);
}

void launch_trace_count(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                        uint64_t first_event, const int64_t* event_start, const double* points, const int64_t* labels,
                        TraceScratch sc, uint32_t* kept, const TraceReadoutDev* ro, const CommonDev* common) {
  const TraceNoiseDev nz = noise ? *noise : TraceNoiseDev{};
  const TraceReadoutDev rd = ro ? *ro : TraceReadoutDev{};
  const CommonDev cm = common ? *common : CommonDev{};
  if (common && ro) launch_count<true, true, true>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
  else if (common) launch_count<true, false, true>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
  else if (noise && ro) launch_count<true, true, false>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
  else if (noise) launch_count<true, false, false>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
  else if (ro) launch_count<false, true, false>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
  else launch_count<false, false, false>(s, tr, nz, seed, n_events, first_event, event_start, points, labels, sc, kept, rd, cm);
}
void launch_trace_write(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                        uint64_t first_event, const int64_t* event_start, const double* points, const int64_t* labels,
                        TraceScratch sc, const int64_t* kept_start, int32_t* pads, int16_t* samples, int64_t* out_labels,
                        unsigned long long* sums, const CommonDev* common) {
  const TraceNoiseDev nz = noise ? *noise : TraceNoiseDev{};
  if (common)
    hipLaunchKernelGGL((trace_write_kernel<true, true>), dim3(n_events), dim3(TR_THREADS), 0, s, tr, nz, seed, first_event,
                       event_start, points, labels, sc, kept_start, pads, samples, out_labels, sums, *common);
  else if (noise)
    hipLaunchKernelGGL((trace_write_kernel<true, false>), dim3(n_events), dim3(TR_THREADS), 0, s, tr, nz, seed, first_event,
                       event_start, points, labels, sc, kept_start, pads, samples, out_labels, sums, CommonDev{});
  else
    hipLaunchKernelGGL((trace_write_kernel<false, false>), dim3(n_events), dim3(TR_THREADS), 0, s, tr, nz, seed,
                       first_event, event_start, points, labels, sc, kept_start, pads, samples, out_labels, sums, CommonDev{});
}


// ---- readout of noise-only pads (the scan and the noise-only write) ----
constexpr int RO_THREADS = 512;
constexpr int RO_WAVES = RO_THREADS / 64;
static_assert(TR_MAP_WORDS <= RO_THREADS, "a thread holds at most one word of the kept bitmap in the prefix");

// The verdict of noise-only pad `pad` of S in PARTIAL readout (wave-uniform), the decision rule of include/attpc_engine.h:
// kept iff 4095 - ped > thr and (-ped > thr or max_j n_j > thr), and max_j n_j > thr iff some u_j >= cdf[c - 1].
// With CM a pad of group g != 255 has the sums n_j + c_g[j] in place of n_j: the pedestal terms stay, the one-compare
// cutoff does not hold (it is the pad table's alone), so the pad's own draw is made and every sum compared -- unless no
// sum of two levels reaches above thr (cm.top <= thr: never).  `cdf` / `guide`: the pad table in LDS (CM only).
template <bool CM>
__device__ __forceinline__ bool noise_only_kept(const TraceDev& tr, const TraceNoiseDev& nz, const TraceReadoutDev& ro,
                                                uint64_t seed, uint64_t event, uint32_t pad, int lane, const uint32_t* cdf,
                                                const uint16_t* guide, const CommonDev& cm, uint32_t e) {
  const int ped = nz.pedestals ? (int)nz.pedestals[pad] : 0;
  if (!((double)(4095 - ped) > tr.threshold)) return false;
  if constexpr (CM) {
    const uint32_t g = common_group(cm, pad);
    if (g != 255u) {  // uniform
      if ((double)(-ped) > tr.threshold) return true;
      if (!((double)cm.top > tr.threshold)) return false;
      int n[8];
      noise_values(n, nz, cdf, guide, seed, event, pad, lane);
      add_common(n, cm, e, g, lane);
      bool over = false;
      for (int s = 0; s < 8; ++s) over |= (double)n[s] > tr.threshold;
      return __ballot(over) != 0ull;
    }
  }
  if ((double)(-ped) > tr.threshold || ro.cut_kind == TRACE_CUT_ALWAYS) return true;
  if (ro.cut_kind == TRACE_CUT_NEVER) return false;
  bool over = false;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t u[4];
    philox4x32<10>((uint32_t)event, (uint32_t)(event >> 32), pad * 128u + 2u * (uint32_t)lane + (uint32_t)h, nz.domain,
                   (uint32_t)seed, (uint32_t)(seed >> 32), u);
#pragma unroll
    for (int w = 0; w < 4; ++w) over |= u[w] >= ro.cut;
  }
  return __ballot(over) != 0ull;
}

template <bool CM>
__global__ __launch_bounds__(RO_THREADS) void trace_scan_kernel(TraceDev tr, TraceNoiseDev nz, TraceReadoutDev ro,
                                                                uint64_t seed, uint64_t first_event,
                                                                const int64_t* __restrict__ event_start, TraceScratch sc,
                                                                uint32_t* __restrict__ kept, TraceMaps maps, CommonDev cm) {
  __shared__ uint32_t hit_w[TR_MAP_WORDS], kept_w[TR_MAP_WORDS], before_w[TR_MAP_WORDS];
  __shared__ uint32_t wave_total[RO_WAVES];
  __shared__ uint32_t noise_cdf[ATTPC_MAX_NOISE_LEVELS];  // (CM only: 2.5 KiB, the occupancy stays full)
  __shared__ uint16_t noise_guide[256];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  if constexpr (CM) {
    if (nz.n_levels > 0 && !ro.full) {  // uniform
      for (int i = t; i < ATTPC_MAX_NOISE_LEVELS; i += RO_THREADS) noise_cdf[i] = nz.cdf[i];
      if (t < 256) noise_guide[t] = nz.guide[t];
    }
  }
  for (int w = t; w < TR_MAP_WORDS; w += RO_THREADS) {
    hit_w[w] = 0u;
    kept_w[w] = 0u;
  }
  block_sync();
  const int64_t lo = event_start[e];
  const uint32_t H = sc.info[2 * e];  // hit pads of S (0 for an event without rows)
  for (uint32_t k = (uint32_t)t; k < H; k += RO_THREADS) {
    const uint32_t p = sc.hit[lo + k], bit = 1u << (p & 31u);
    atomicOr(&hit_w[p >> 5], bit);
    if (sc.rank[lo + k] >= 0) atomicOr(&kept_w[p >> 5], bit);
  }
  block_sync();
  const uint64_t event = first_event + e;
  uint32_t* noise_w = maps.noise + (size_t)e * TR_MAP_WORDS;
  for (int w = wave; w < TR_MAP_WORDS; w += RO_WAVES) {
    uint32_t cand = ro.channels[w] & ~hit_w[w];  // the noise-only pads of S in this word
    uint32_t nw = 0u;
    if (ro.full) {
      nw = cand;
    } else {
      while (cand) {  // uniform
        const int b = __builtin_ctz(cand);
        cand &= cand - 1u;
        if (noise_only_kept<CM>(tr, nz, ro, seed, event, 32u * (uint32_t)w + (uint32_t)b, lane, noise_cdf, noise_guide, cm, e))
          nw |= 1u << b;
      }
    }
    if (lane == 0) {
      noise_w[w] = nw;
      kept_w[w] |= nw;
    }
  }
  block_sync();
  // exclusive prefix of the words' popcounts: the kept pads of the event below word w
  const uint32_t c = t < TR_MAP_WORDS ? (uint32_t)__popc(kept_w[t]) : 0u;
  uint32_t incl = c;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off);
    incl += lane >= off ? up : 0u;
  }
  if (lane == 63) wave_total[wave] = incl;
  block_sync();
  uint32_t before = incl - c;
  for (int w = 0; w < wave; ++w) before += wave_total[w];
  if (t < TR_MAP_WORDS) {
    before_w[t] = before;
    maps.kept[(size_t)e * TR_MAP_WORDS + t] = kept_w[t];
    maps.before[(size_t)e * TR_MAP_WORDS + t] = before;
  }
  if (t == RO_THREADS - 1) kept[e] = before + c;
  block_sync();
  // the hit pads' ranks among all kept pads of the event (ascending pad, hit and noise-only interleaved)
  for (uint32_t k = (uint32_t)t; k < H; k += RO_THREADS) {
    if (sc.rank[lo + k] < 0) continue;
    const uint32_t p = sc.hit[lo + k];
    sc.rank[lo + k] = (int32_t)(before_w[p >> 5] + (uint32_t)__popc(kept_w[p >> 5] & ((1u << (p & 31u)) - 1u)));
  }
}

template <bool CM>
__global__ __launch_bounds__(RO_THREADS) void trace_noise_write_kernel(TraceNoiseDev nz, uint64_t seed,
                                                                       uint64_t first_event, TraceMaps maps,
                                                                       const int64_t* __restrict__ kept_start,
                                                                       int32_t* __restrict__ pads,
                                                                       int16_t* __restrict__ samples,
                                                                       int64_t* __restrict__ out_labels,
                                                                       unsigned long long* __restrict__ sums,
                                                                       CommonDev cm) {
  __shared__ uint32_t noise_cdf[ATTPC_MAX_NOISE_LEVELS];
  __shared__ uint16_t noise_guide[256];
  __shared__ unsigned long long wave_sum[RO_WAVES][2];
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t out0 = kept_start[e];
  if (kept_start[e + 1] == out0) return;  // uniform
  if (nz.n_levels > 0) {                  // uniform
    for (int i = t; i < ATTPC_MAX_NOISE_LEVELS; i += RO_THREADS) noise_cdf[i] = nz.cdf[i];
    if (t < 256) noise_guide[t] = nz.guide[t];
  }
  block_sync();
  const unsigned long long event = first_event + e;
  const size_t m0 = (size_t)e * TR_MAP_WORDS;
  unsigned long long sample_sum = 0ull, pad_sum = 0ull;  // lane parts
  for (int w = wave; w < TR_MAP_WORDS; w += RO_WAVES) {
    uint32_t bits = maps.noise[m0 + w];
    if (!bits) continue;  // uniform
    const uint32_t kw = maps.kept[m0 + w], base = maps.before[m0 + w];
    while (bits) {  // uniform
      const int b = __builtin_ctz(bits);
      bits &= bits - 1u;
      const uint32_t pad = 32u * (uint32_t)w + (uint32_t)b;
      const int64_t o = out0 + base + __popc(kw & ((1u << b) - 1u));
      const int ped = nz.pedestals ? (int)nz.pedestals[pad] : 0;
      int n[8];
      noise_values(n, nz, noise_cdf, noise_guide, seed, event, pad, lane);
      if constexpr (CM) {
        const uint32_t g = common_group(cm, pad);
        if (g != 255u) add_common(n, cm, e, g, lane);  // uniform
      }
      int16_t* dst = samples + o * ATTPC_NUM_TB;
      for (int s = 0; s < 8; ++s) {
        const int j = lane + 64 * s;
        int v = ped + n[s];  // s_p[j] = 0
        v = v < 0 ? 0 : (v > 4095 ? 4095 : v);
        dst[j] = (int16_t)v;
        sample_sum += (unsigned long long)(long long)v * (unsigned long long)(j + 1);
      }
      if (lane == 0) {
        pads[o] = (int32_t)pad;
        out_labels[o] = -1;
        pad_sum += (event << 14) + (unsigned long long)pad;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sample_sum += __shfl_xor(sample_sum, off);
    pad_sum += __shfl_xor(pad_sum, off);
  }
  if (lane == 0) {
    wave_sum[wave][0] = sample_sum;
    wave_sum[wave][1] = pad_sum;
  }
  block_sync();
  if (t < 2) {
    unsigned long long v = 0ull;
    for (int w = 0; w < RO_WAVES; ++w) v += wave_sum[w][t];
    atomicAdd(sums + t, v);
  }
}

void launch_trace_scan(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, const TraceReadoutDev& ro,
                       uint64_t seed, uint32_t n_events, uint64_t first_event, const int64_t* event_start, TraceScratch sc,
                       uint32_t* kept, TraceMaps maps, const CommonDev* common) {
  const TraceNoiseDev nz = noise ? *noise : TraceNoiseDev{};
  if (common)
    hipLaunchKernelGGL(trace_scan_kernel<true>, dim3(n_events), dim3(RO_THREADS), 0, s, tr, nz, ro, seed, first_event,
                       event_start, sc, kept, maps, *common);
  else
    hipLaunchKernelGGL(trace_scan_kernel<false>, dim3(n_events), dim3(RO_THREADS), 0, s, tr, nz, ro, seed, first_event,
                       event_start, sc, kept, maps, CommonDev{});
}
void launch_trace_noise_write(hipStream_t s, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                              uint64_t first_event, TraceMaps maps, const int64_t* kept_start, int32_t* pads,
                              int16_t* samples, int64_t* out_labels, unsigned long long* sums, const CommonDev* common) {
  const TraceNoiseDev nz = noise ? *noise : TraceNoiseDev{};
  if (common)
    hipLaunchKernelGGL(trace_noise_write_kernel<true>, dim3(n_events), dim3(RO_THREADS), 0, s, nz, seed, first_event, maps,
                       kept_start, pads, samples, out_labels, sums, *common);
  else
    hipLaunchKernelGGL(trace_noise_write_kernel<false>, dim3(n_events), dim3(RO_THREADS), 0, s, nz, seed, first_event, maps,
                       kept_start, pads, samples, out_labels, sums, CommonDev{});
}

// ---- common-mode noise: the values of every (event, group) of a launch ----
constexpr int CMN_THREADS = 512;
constexpr int CMN_WAVES = CMN_THREADS / 64;

// One wave per (event, group): item i = e * n_groups + g, its 512 values drawn as a pad's noise is (noise_values with
// the stage's table and domain, the group in the pad's place) and stored where the lanes of the trace kernels read them
// (add_common): 1 KiB per item, one 16-byte store per lane.  The table sits in LDS as in the trace kernels.
__global__ __launch_bounds__(CMN_THREADS) void common_mode_kernel(TraceNoiseDev table, uint64_t seed, uint64_t first_event,
                                                                  uint32_t n_groups, uint64_t n_items,
                                                                  int16_t* __restrict__ values) {
  __shared__ uint32_t cdf[ATTPC_MAX_NOISE_LEVELS];
  __shared__ uint16_t guide[256];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int i = t; i < ATTPC_MAX_NOISE_LEVELS; i += CMN_THREADS) cdf[i] = table.cdf[i];
  if (t < 256) guide[t] = table.guide[t];
  block_sync();
  const uint64_t item = (uint64_t)blockIdx.x * CMN_WAVES + (uint64_t)wave;
  if (item >= n_items) return;  // uniform per wave
  const uint64_t e = item / n_groups;
  const uint32_t g = (uint32_t)(item - e * n_groups);
  int n[8];
  noise_values(n, table, cdf, guide, seed, first_event + e, g, lane);
  CommonLane c;
  for (int s = 0; s < 8; ++s) c.v[s] = (int16_t)n[s];  // levels lie in -4095 .. 4606
  *reinterpret_cast<CommonLane*>(values + item * ATTPC_NUM_TB + 8 * lane) = c;
}

void launch_common_mode(hipStream_t s, const TraceNoiseDev& table, uint64_t seed, uint32_t n_events, uint64_t first_event,
                        uint32_t n_groups, int16_t* values) {
  const uint64_t n_items = (uint64_t)n_events * n_groups;
  hipLaunchKernelGGL(common_mode_kernel, dim3((uint32_t)((n_items + CMN_WAVES - 1) / CMN_WAVES)), dim3(CMN_THREADS), 0, s,
                     table, seed, first_event, n_groups, n_items, values);
}

}  // namespace attpc
