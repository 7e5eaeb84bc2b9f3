// cluster.hip -- clustering of trace rows on the device without the truth labels: DBSCAN with every tie made definite,
// in integers, one cluster label per row (the contract is in include/attpc_engine.h, "clustering"; the metric, the
// neighbour predicate, the vote and the ranking key are cluster_host.hpp, shared with the host).  This is not Spyral's
// HDBSCAN + cluster joining + outlier-factor cleanup, and nothing here has been compared against Spyral.
//
// One workgroup of four waves per event, empty events included.  The per-row state lives in the chunk's scratch
// (ClusterArgs::scratch, CLUSTER_SCRATCH_WORDS words per row: an event of max_rows rows does not fit LDS), which only
// this workgroup touches and which stays in the caches; LDS holds the event's counters and the eight ranking keys.
//   Pass 0 sets every label to -1 and counts the truth rows of every position.
//   Pass 1 quantises the rows and compacts the in-range ones, in order (ballot, wave totals in LDS): everything behind
//   it works on the compact index, which is monotone in the row index, so "lowest row index" is "lowest compact index".
//   Pass 2, a lane per row: the row's candidates are one contiguous window of the Z-sorted rows, found by two binary
//   searches; the neighbours in it are counted, which decides CORE.
//   Pass 3: a core row unites itself with every core neighbour in front of it -- every edge once -- by a lock-free union
//   that always hooks the larger root under the smaller (atomicMin on the parent word), so the root of a component is
//   its lowest core index whatever the interleaving.  A row that is not core picks its nearest core neighbour.
//   Pass 4 flattens: every row walks to its root and adds itself to the root's counts, votes and extent (integer
//   atomics: order does not matter).
//   Pass 5, a lane per root: the size cut, the majority, and with MATCH_TRUTH the best key of every position (atomicMax).
//   Pass 6 finds the eight best keys, one per round, each the largest key below the one before.
//   Pass 7 gives the clusters their labels, pass 8 the rows, pass 9 writes the records.
// Every loop has a bound that follows from the rows n: a search is at most 32 halvings, a window at most n rows, a walk
// to the root at most n links (a parent is smaller than its child), a union at most n + 1 trips (the larger of the two
// roots falls with every trip).  A bound that is met sets INTERNAL and the event is labelled -1; nothing waits for
// another wave except at the workgroup's barriers.
// Occupancy: neither the registers (28 VGPRs) nor LDS (208 bytes) bound it but the wave slots: eight workgroups of four
// waves a CU.
// Memory model: the hooks are agent-scope atomicMin, done in L2, while cluster_find reads the parent words with relaxed
// workgroup-scope loads.  That is enough because a workgroup's waves share one CU and its vector L1 (the kernel is not
// built for tgsplit), and because a stale word only shows a larger, older ancestor of the same tree: the walk goes on
// from there, and a hook that meets a word no longer a root is retried by cluster_union.  The passes are separated by
// __threadfence_block and the workgroup's barrier.
#include "tracks_args.hpp"

#include "cluster_host.hpp"

namespace attpc {

constexpr int CL_THREADS = 256;
constexpr int CL_WAVES = CL_THREADS / 64;

namespace {

enum { CL_SMALL = 0, CL_KEPT, CL_SPLIT, CL_FAKE, CL_CORE, CL_BORDER, CL_BAD, CL_COUNTS };

// the root of x: at most m links, since a parent is smaller than its child (false in *bad otherwise)
__device__ __forceinline__ uint32_t cluster_find(const uint32_t* parent, uint32_t x, uint32_t m, bool* bad) {
  for (uint32_t step = 0u; step < m; ++step) {
    const uint32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
  *bad = true;
  return x;
}

// a and b in one tree, the larger root hooked under the smaller.  If the word of the larger root had been lowered
// meanwhile (it was no root any more), what it pointed to still has to meet b: the larger of the pair falls every trip.
__device__ __forceinline__ void cluster_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t m, bool* bad) {
  for (uint32_t trip = 0u; trip <= m; ++trip) {
    a = cluster_find(parent, a, m, bad);
    b = cluster_find(parent, b, m, bad);
    if (*bad || a == b) return;
    if (a < b) {
      const uint32_t c = a;
      a = b;
      b = c;
    }
    const uint32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
  *bad = true;
}

}  // namespace

__global__ __launch_bounds__(CL_THREADS) void cluster_kernel(ClusterArgs a) {
  __shared__ uint32_t wave_count[CL_WAVES];
  __shared__ uint32_t truth[ATTPC_MAX_SIM];
  __shared__ uint32_t counts[CL_COUNTS];
  __shared__ unsigned long long best_key[ATTPC_MAX_SIM];  // MATCH_TRUTH: the best-ranked cluster of every majority
  __shared__ unsigned long long top_key[ATTPC_MAX_SIM];   // the clusters of rank 0 .. 7
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = a.ev_start[e];
  const uint32_t n = (uint32_t)(a.ev_start[e + 1] - lo);
  const ClusterSettings& s = a.s;
  if (t < ATTPC_MAX_SIM) {
    truth[t] = 0u;
    best_key[t] = 0ull;
    top_key[t] = 0ull;
  }
  if (t < CL_COUNTS) counts[t] = 0u;
  block_sync();
  // ---- pass 0: no row has a cluster; the truth rows of every position ----
  for (uint32_t i = (uint32_t)t; i < n; i += CL_THREADS) {
    a.out_labels[lo + i] = -1;
    const int32_t p = a.labels ? cluster_vote(s, a.labels[lo + i]) : -1;
    if (p >= 0) atomicAdd(&truth[p], 1u);
  }
  block_sync();
  // the record of an event that is not clustered, and its unused cluster records (status is uniform)
  auto unclustered = [&](int32_t status) {
    if (t == 0 && a.events) {
      attpc_cluster_event ev;
      cluster_event_unclustered((int32_t)n, status, &ev);
      for (int p = 0; p < ATTPC_MAX_SIM; ++p) ev.truth_rows[p] = (uint16_t)(truth[p] < 65535u ? truth[p] : 65535u);
      a.events[e] = ev;
    }
    if (t < ATTPC_MAX_SIM && a.records) a.records[(size_t)e * ATTPC_MAX_SIM + t] = cluster_record_unused();
  };
  if (n == 0u || n > (uint32_t)s.max_rows) {  // uniform
    unclustered(n == 0u ? 0 : ATTPC_CLUSTER_CAPPED);
    return;
  }
  // the event's scratch: CLUSTER_SCRATCH_WORDS arrays of n words each
  int32_t* region = a.scratch + lo * (int64_t)CLUSTER_SCRATCH_WORDS;
  int32_t* cx = region;
  int32_t* cy = region + (size_t)n;
  int32_t* cz = region + 2 * (size_t)n;
  uint32_t* orig = reinterpret_cast<uint32_t*>(region + 3 * (size_t)n);     // the row of a compact index
  uint32_t* w_lo = reinterpret_cast<uint32_t*>(region + 4 * (size_t)n);     // the window, both ends included
  uint32_t* w_hi = reinterpret_cast<uint32_t*>(region + 5 * (size_t)n);
  uint32_t* core = reinterpret_cast<uint32_t*>(region + 6 * (size_t)n);
  uint32_t* parent = reinterpret_cast<uint32_t*>(region + 7 * (size_t)n);
  uint32_t* nearest = reinterpret_cast<uint32_t*>(region + 8 * (size_t)n);  // the border candidate, or CLUSTER_NONE
  uint32_t* comp = reinterpret_cast<uint32_t*>(region + 9 * (size_t)n);     // the root of the row's cluster, or CLUSTER_NONE
  uint32_t* c_rows = reinterpret_cast<uint32_t*>(region + 10 * (size_t)n);  // of a root: rows, core rows,
  uint32_t* c_core = reinterpret_cast<uint32_t*>(region + 11 * (size_t)n);
  int32_t* c_zmin = region + 12 * (size_t)n;                                // extent,
  int32_t* c_zmax = region + 13 * (size_t)n;
  int32_t* c_major = region + 14 * (size_t)n;                               // majority and its votes,
  uint32_t* c_major_rows = reinterpret_cast<uint32_t*>(region + 15 * (size_t)n);
  int32_t* c_label = region + 16 * (size_t)n;                               // the label given,
  uint32_t* c_votes = reinterpret_cast<uint32_t*>(region + 17 * (size_t)n); // and [n][8] votes
  // ---- pass 1: quantise, compact the in-range rows in order ----
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t m = 0u;  // the in-range rows so far (uniform)
  for (uint32_t base = 0u; base < n; base += CL_THREADS) {
    const uint32_t i = base + (uint32_t)t;
    bool ok = false;
    int32_t X = 0, Y = 0, Z = 0;
    if (i < n) {
      const double* p = a.rows + 8 * (lo + i);
      int64_t I;
      ok = estimate_quantise(p[0], p[1], p[2], p[4], &X, &Y, &Z, &I);
    }
    const uint64_t ballot = __ballot(ok);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
    block_sync();
    uint32_t at = m + (uint32_t)__popcll(ballot & below), total = 0u;
    for (int w = 0; w < CL_WAVES; ++w) {
      const uint32_t c = wave_count[w];
      at += w < wave ? c : 0u;
      total += c;
    }
    if (ok) {
      cx[at] = X;
      cy[at] = Y;
      cz[at] = Z;
      orig[at] = i;
    }
    m += total;
    block_sync();  // (before the totals are written again)
  }
  __threadfence_block();  // (the scratch is written and read by this workgroup only)
  block_sync();
  // ---- pass 2: the window, the neighbours, core ----
  for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
    const int32_t X = cx[k], Y = cy[k], Z = cz[k];
    uint32_t first = 0u, last = k;  // the first j in 0 .. k with cz[j] >= Z - Ez (k is one)
    for (int it = 0; it < 32 && first < last; ++it) {
      const uint32_t mid = first + (last - first) / 2u;
      if (cz[mid] >= Z - s.ez)
        last = mid;
      else
        first = mid + 1u;
    }
    uint32_t from = k, to = m - 1u;  // the last j in k .. m-1 with cz[j] <= Z + Ez (k is one)
    for (int it = 0; it < 32 && from < to; ++it) {
      const uint32_t mid = from + (to - from + 1u) / 2u;
      if (cz[mid] <= Z + s.ez)
        from = mid;
      else
        to = mid - 1u;
    }
    uint32_t count = 0u;
    for (uint32_t j = first; j <= from; ++j) count += cluster_neighbour(s, cx[j] - X, cy[j] - Y, cz[j] - Z) ? 1u : 0u;
    w_lo[k] = first;
    w_hi[k] = from;
    core[k] = count >= (uint32_t)s.min_samples ? 1u : 0u;
    parent[k] = k;
    nearest[k] = CLUSTER_NONE;
    c_rows[k] = 0u;
    c_core[k] = 0u;
    c_zmin[k] = INT32_MAX;
    c_zmax[k] = INT32_MIN;
#pragma unroll
    for (int p = 0; p < ATTPC_MAX_SIM; ++p) c_votes[(size_t)k * ATTPC_MAX_SIM + p] = 0u;
  }
  __threadfence_block();
  block_sync();
  // ---- pass 3: the components of the core rows; the nearest core neighbour of the others ----
  bool bad = false;
  for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
    const int32_t X = cx[k], Y = cy[k], Z = cz[k];
    const uint32_t first = w_lo[k], last = w_hi[k];
    if (core[k]) {
      for (uint32_t j = first; j < k; ++j)
        if (core[j] && cluster_neighbour(s, cx[j] - X, cy[j] - Y, cz[j] - Z)) cluster_union(parent, k, j, m, &bad);
    } else {
      uint32_t best = CLUSTER_NONE;
      int64_t best_d = 0;
      for (uint32_t j = first; j <= last; ++j) {
        if (!core[j]) continue;
        const int32_t dx = cx[j] - X, dy = cy[j] - Y, dz = cz[j] - Z;
        if (!cluster_neighbour(s, dx, dy, dz)) continue;
        const int64_t d = cluster_metric(s, dx, dy, dz);
        if (best == CLUSTER_NONE || d < best_d) {  // (ascending j: a tie stays with the lower row)
          best = j;
          best_d = d;
        }
      }
      nearest[k] = best;
    }
  }
  __threadfence_block();
  block_sync();
  // ---- pass 4: every row to its root ----
  for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
    const bool is_core = core[k] != 0u;
    const uint32_t via = is_core ? k : nearest[k];
    const uint32_t c = via == CLUSTER_NONE ? CLUSTER_NONE : cluster_find(parent, via, m, &bad);
    comp[k] = c;
    if (c == CLUSTER_NONE) continue;
    atomicAdd(&c_rows[c], 1u);
    if (is_core) atomicAdd(&c_core[c], 1u);
    atomicMin(&c_zmin[c], cz[k]);
    atomicMax(&c_zmax[c], cz[k]);
    const int32_t p = a.labels ? cluster_vote(s, a.labels[lo + orig[k]]) : -1;
    if (p >= 0) atomicAdd(&c_votes[(size_t)c * ATTPC_MAX_SIM + p], 1u);
  }
  if (bad) atomicOr(&counts[CL_BAD], 1u);
  __threadfence_block();
  block_sync();
  if (counts[CL_BAD]) {  // uniform
    unclustered(ATTPC_CLUSTER_INTERNAL);
    return;
  }
  // ---- pass 5: the roots: size cut, majority, the best cluster of every majority ----
  for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
    if (!core[k] || comp[k] != k) continue;
    const uint32_t rows = c_rows[k];
    if (rows < (uint32_t)s.min_cluster_size) {
      atomicAdd(&counts[CL_SMALL], 1u);
      continue;
    }
    atomicAdd(&counts[CL_KEPT], 1u);
    uint32_t major_rows = 0u;
    const int32_t major = cluster_majority(c_votes + (size_t)k * ATTPC_MAX_SIM, &major_rows);
    c_major[k] = major;
    c_major_rows[k] = major_rows;
    c_label[k] = -1;
    if (s.match == ATTPC_CLUSTER_MATCH_TRUTH && major >= 0) atomicMax(&best_key[major], cluster_key(rows, k));
  }
  __threadfence_block();
  block_sync();
  // ---- pass 6: the ranks 0 .. 7: each the largest key below the one before (keys differ: they hold the id) ----
  const uint32_t n_kept = counts[CL_KEPT];
  unsigned long long before = ~0ull;
  for (uint32_t r = 0u; r < (uint32_t)ATTPC_MAX_SIM && r < n_kept; ++r) {  // uniform
    unsigned long long mine = 0ull;
    for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
      if (!core[k] || comp[k] != k) continue;
      const uint32_t rows = c_rows[k];
      if (rows < (uint32_t)s.min_cluster_size) continue;
      const unsigned long long key = cluster_key(rows, k);
      mine = key < before && key > mine ? key : mine;
    }
    if (mine) atomicMax(&top_key[r], mine);
    block_sync();
    before = top_key[r];
  }
  // ---- pass 7: the labels of the clusters ----
  if (s.match == ATTPC_CLUSTER_MATCH_TRUTH) {
    for (uint32_t k = (uint32_t)t; k < m; k += CL_THREADS) {
      if (!core[k] || comp[k] != k) continue;
      const uint32_t rows = c_rows[k];
      if (rows < (uint32_t)s.min_cluster_size) continue;
      const int32_t major = c_major[k];
      if (major >= 0 && best_key[major] == cluster_key(rows, k))
        c_label[k] = s.give[major];
      else
        atomicAdd(&counts[major >= 0 ? CL_SPLIT : CL_FAKE], 1u);
    }
  } else if (t < ATTPC_MAX_SIM && t < s.n_sim && top_key[t]) {
    c_label[cluster_key_id(top_key[t])] = s.give[t];
  }
  __threadfence_block();
  block_sync();
  // ---- pass 8: the labels of the rows ----
  for (uint32_t base = 0u; base < m; base += CL_THREADS) {
    const uint32_t k = base + (uint32_t)t;
    bool in_core = false, in_border = false;
    if (k < m) {
      const uint32_t c = comp[k];
      if (c != CLUSTER_NONE && c_rows[c] >= (uint32_t)s.min_cluster_size) {
        a.out_labels[lo + orig[k]] = (int64_t)c_label[c];
        in_core = core[k] != 0u;
        in_border = !in_core;
      }
    }
    const uint32_t n_core = (uint32_t)__popcll(__ballot(in_core)), n_border = (uint32_t)__popcll(__ballot(in_border));
    if (lane == 0) {
      if (n_core) atomicAdd(&counts[CL_CORE], n_core);
      if (n_border) atomicAdd(&counts[CL_BORDER], n_border);
    }
  }
  block_sync();
  // ---- pass 9: the records ----
  if (t == 0 && a.events) {
    attpc_cluster_event ev;
    ev.n_rows = (int32_t)n;
    ev.n_range = (int32_t)(n - m);
    ev.n_core = (int32_t)counts[CL_CORE];
    ev.n_border = (int32_t)counts[CL_BORDER];
    ev.n_noise = (int32_t)(n - counts[CL_CORE] - counts[CL_BORDER]);
    ev.n_clusters = (int32_t)n_kept;
    ev.n_small = (int32_t)counts[CL_SMALL];
    ev.n_split = (int32_t)counts[CL_SPLIT];
    ev.n_fake = (int32_t)counts[CL_FAKE];
    ev.status = 0;
    ev.reserved[0] = ev.reserved[1] = 0;
    for (int p = 0; p < ATTPC_MAX_SIM; ++p) ev.truth_rows[p] = (uint16_t)(truth[p] < 65535u ? truth[p] : 65535u);
    a.events[e] = ev;
  }
  if (t < ATTPC_MAX_SIM && a.records) {
    attpc_cluster_record rec = cluster_record_unused();
    if (top_key[t]) {
      const uint32_t k = cluster_key_id(top_key[t]);
      rec = attpc_cluster_record{(int32_t)c_rows[k], (int32_t)c_core[k], (int32_t)orig[k], c_major[k], (int32_t)c_major_rows[k],
                                 c_label[k],         c_zmin[k],          c_zmax[k]};
    }
    a.records[(size_t)e * ATTPC_MAX_SIM + t] = rec;
  }
}

void launch_cluster(hipStream_t s, uint32_t n_events, const ClusterArgs& a) {
  hipLaunchKernelGGL(cluster_kernel, dim3(n_events), dim3(CL_THREADS), 0, s, a);
}

}  // namespace attpc
