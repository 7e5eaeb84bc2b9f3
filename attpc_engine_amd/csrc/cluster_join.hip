// cluster_join.hip -- cluster joining on the device: the clusters of cluster_kernel whose circles in the pad plane
// overlap become one (the contract is in include/attpc_engine.h, "cluster joining"; the terms of the sums, the circle,
// the overlap predicate and the merge are join_host.hpp, shared with the host).  The contract is Spyral's cluster
// joining in structure, with every tie made definite: it is not Spyral's code, Spyral iterates the joining and this
// does not, and nothing here has been compared against Spyral.
//
// cluster_join_kernel is launched right behind cluster_kernel on the same stream, one workgroup of four waves per
// event, and reads what that kernel left in the chunk's scratch (tracks_args.hpp, CLUSTER_SCRATCH_WORDS): cx, cy, cz,
// orig, core, comp and of every root its rows, core rows, votes and z extent.  It writes one scratch array, w_lo, which
// cluster_kernel no longer needs: the candidate slot of a root.  At most ATTPC_JOIN_MAX_CLUSTERS = 64 candidates take
// part, and everything about them lives in LDS (about 9 KiB).
//   6a: the surviving roots are compacted in ascending id (ballot, wave totals in LDS) into slots 0 .. K-1.  An event
//       that was not clustered, or has more than max_clusters candidates, gets its join event and is left as it is.
//   6b: a lane per row adds the row's seven terms to its candidate's sums in LDS (64-bit integer atomics: order does
//       not matter); a lane per candidate then makes the circle.
//   6c: a wave per candidate i, a lane per candidate j: one pair a lane, and the ballot is row i of the adjacency.
//   6d: the components by doubling: six rounds of reach[i] |= reach[j] for every j in reach[i] cover every path among
//       64 nodes; the lowest bit of reach[i] is the component's lowest slot, which has its lowest id.  A lane per
//       component then sums its members' counts (join_merge).
//   7 to 9 on the components, a lane each: the rank is the number of components with a larger key, the majority and
//       the labels as in cluster_kernel; the rows get their component's label; the event's n_clusters, n_split and
//       n_fake and its cluster records are overwritten, the join event and the join records written.
// Every loop has a bound that follows from K <= 64 (64 lanes, 64 bits of a mask, 6 rounds, 8 ranks) or from the rows
// (the strided passes); none can be met early or late, so this kernel adds no INTERNAL of its own, and nothing waits for
// another wave except at the workgroup's barriers.
#include "tracks_args.hpp"

#include "join_host.hpp"

namespace attpc {

constexpr int CJ_THREADS = 256;
constexpr int CJ_WAVES = CJ_THREADS / 64;
constexpr int CJ_MAX = ATTPC_JOIN_MAX_CLUSTERS;
static_assert(CJ_MAX == 64, "a candidate per lane of a wave, a bit per candidate in a 64-bit mask");

namespace {

enum { CJ_CIRCLES = 0, CJ_PART, CJ_PAIRS, CJ_COMPONENTS, CJ_SPLIT, CJ_FAKE, CJ_COUNTS };
enum { CJ_HAS = 1u, CJ_TAKES_PART = 2u };

}  // namespace

__global__ __launch_bounds__(CJ_THREADS) void cluster_join_kernel(ClusterJoinArgs a) {
  __shared__ uint32_t wave_count[CJ_WAVES];
  __shared__ uint32_t counts[CJ_COUNTS];
  __shared__ uint32_t cand[CJ_MAX];                           // the root (compact index) of a slot
  __shared__ unsigned long long sums[CJ_MAX][JOIN_SUMS];      // step 6b, two's complement
  __shared__ double circle_a[CJ_MAX], circle_b[CJ_MAX], circle_r[CJ_MAX];
  __shared__ uint32_t flags[CJ_MAX];                          // CJ_HAS, CJ_TAKES_PART
  __shared__ unsigned long long reach[2][CJ_MAX];             // the slots a slot is joined with, itself included
  __shared__ uint32_t root_of[CJ_MAX];                        // the lowest slot of a slot's component
  __shared__ uint32_t m_rows[CJ_MAX], m_core[CJ_MAX], m_major_rows[CJ_MAX], m_parts[CJ_MAX];  // of a component's root slot
  __shared__ int32_t m_zmin[CJ_MAX], m_zmax[CJ_MAX], m_major[CJ_MAX], m_label[CJ_MAX], m_circle[CJ_MAX];
  __shared__ unsigned long long best_key[ATTPC_MAX_SIM];      // MATCH_TRUTH: the best-ranked component of every majority
  __shared__ uint32_t top_slot[ATTPC_MAX_SIM];                // the root slot of rank 0 .. 7, CLUSTER_NONE: none
  const uint32_t e = blockIdx.x;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = a.c.ev_start[e];
  const uint32_t n = (uint32_t)(a.c.ev_start[e + 1] - lo);
  const ClusterSettings& s = a.c.s;
  const JoinSettings& js = a.j;
  const int32_t cluster_status = a.c.events[e].status;
  const uint32_t n_range = (uint32_t)a.c.events[e].n_range;
  // the join event of an event that is not joined, and its unused join records (uniform)
  auto not_joined = [&](int32_t n_candidates, int32_t status) {
    if (t == 0 && a.join_events) a.join_events[e] = join_event_not_joined(n_candidates, status);
    if (t < ATTPC_MAX_SIM && a.join_records) a.join_records[(size_t)e * ATTPC_MAX_SIM + t] = join_record_unused();
  };
  if (n == 0u || cluster_status != 0 || n_range > n) {  // uniform
    not_joined(0, ATTPC_JOIN_NOT_CLUSTERED);
    return;
  }
  const uint32_t m = n - n_range;  // the in-range rows, as cluster_kernel compacted them
  // the event's scratch as cluster.hip lays it out: CLUSTER_SCRATCH_WORDS arrays of n words each
  int32_t* region = a.c.scratch + lo * (int64_t)CLUSTER_SCRATCH_WORDS;
  const int32_t* cx = region;
  const int32_t* cy = region + (size_t)n;
  const uint32_t* orig = reinterpret_cast<const uint32_t*>(region + 3 * (size_t)n);
  uint32_t* slot_of = reinterpret_cast<uint32_t*>(region + 4 * (size_t)n);  // (w_lo of cluster_kernel, free behind its pass 3)
  const uint32_t* core = reinterpret_cast<const uint32_t*>(region + 6 * (size_t)n);
  const uint32_t* comp = reinterpret_cast<const uint32_t*>(region + 9 * (size_t)n);
  const uint32_t* c_rows = reinterpret_cast<const uint32_t*>(region + 10 * (size_t)n);
  const uint32_t* c_core = reinterpret_cast<const uint32_t*>(region + 11 * (size_t)n);
  const int32_t* c_zmin = region + 12 * (size_t)n;
  const int32_t* c_zmax = region + 13 * (size_t)n;
  const uint32_t* c_votes = reinterpret_cast<const uint32_t*>(region + 17 * (size_t)n);
  if (t < CJ_MAX) {
    cand[t] = 0u;
#pragma unroll
    for (int q = 0; q < JOIN_SUMS; ++q) sums[t][q] = 0ull;
    flags[t] = 0u;
    reach[0][t] = reach[1][t] = 0ull;
    root_of[t] = (uint32_t)t;
  }
  if (t < ATTPC_MAX_SIM) {
    best_key[t] = 0ull;
    top_slot[t] = CLUSTER_NONE;
  }
  if (t < CJ_COUNTS) counts[t] = 0u;
  block_sync();
  // ---- 6a: the surviving roots in ascending id -> slots ----
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t K = 0u;  // the candidates so far (uniform)
  for (uint32_t base = 0u; base < m; base += CJ_THREADS) {
    const uint32_t k = base + (uint32_t)t;
    const bool is_cand = k < m && core[k] != 0u && comp[k] == k && c_rows[k] >= (uint32_t)s.min_cluster_size;
    const uint64_t ballot = __ballot(is_cand);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
    block_sync();
    uint32_t at = K + (uint32_t)__popcll(ballot & below), total = 0u;
    for (int w = 0; w < CJ_WAVES; ++w) {
      const uint32_t c = wave_count[w];
      at += w < wave ? c : 0u;
      total += c;
    }
    if (is_cand && at < (uint32_t)CJ_MAX) {
      cand[at] = k;
      slot_of[k] = at;
    }
    K += total;
    block_sync();  // (before the totals are written again)
  }
  if (K > (uint32_t)js.max_clusters) {  // uniform: labels, cluster event and cluster records stay those of cluster_kernel
    not_joined((int32_t)K, ATTPC_JOIN_CAPPED);
    return;
  }
  __threadfence_block();  // (slot_of is written and read by this workgroup only)
  block_sync();
  // ---- 6b: the sums of every candidate over its rows, core and border; its circle ----
  for (uint32_t k = (uint32_t)t; k < m; k += CJ_THREADS) {
    const uint32_t c = comp[k];
    if (c == CLUSTER_NONE || c >= m || c_rows[c] < (uint32_t)s.min_cluster_size) continue;
    const uint32_t slot = slot_of[c];
    if (slot >= K) continue;  // (cannot be: every surviving root has a slot)
    int64_t term[JOIN_SUMS];
    join_terms(cx[k] - cx[c], cy[k] - cy[c], term);
#pragma unroll
    for (int q = 0; q < JOIN_SUMS; ++q) atomicAdd(&sums[slot][q], (unsigned long long)term[q]);
  }
  block_sync();
  if ((uint32_t)t < K) {
    const uint32_t id = cand[t];
    int64_t sum[JOIN_SUMS];
#pragma unroll
    for (int q = 0; q < JOIN_SUMS; ++q) sum[q] = (int64_t)sums[t][q];
    const JoinCircle c = join_circle(c_rows[id], cx[id], cy[id], sum);
    const bool part = join_takes_part(js, c);
    circle_a[t] = c.a;
    circle_b[t] = c.b;
    circle_r[t] = c.R;
    flags[t] = (c.has ? CJ_HAS : 0u) | (part ? CJ_TAKES_PART : 0u);
    if (c.has) atomicAdd(&counts[CJ_CIRCLES], 1u);
    if (part) atomicAdd(&counts[CJ_PART], 1u);
  }
  block_sync();
  // ---- 6c: one pair a lane; the ballot of wave i's lanes is row i of "is joined with" ----
  for (uint32_t i = (uint32_t)wave; i < K; i += CJ_WAVES) {  // uniform in a wave
    const uint32_t j = (uint32_t)lane;
    bool joined = false;
    if (j < K && j != i && (flags[i] & CJ_TAKES_PART) && (flags[j] & CJ_TAKES_PART)) {
      const uint32_t low = i < j ? i : j, high = i < j ? j : i;
      joined = join_pair(js, JoinCircle{circle_a[low], circle_b[low], circle_r[low], true},
                         JoinCircle{circle_a[high], circle_b[high], circle_r[high], true});
    }
    const uint64_t row = __ballot(joined);
    if (lane == 0) {
      reach[0][i] = row | (1ull << i);
      const uint32_t above = (uint32_t)__popcll(row & ~((2ull << i) - 1ull));  // (every pair once: j > i)
      if (above) atomicAdd(&counts[CJ_PAIRS], above);
    }
  }
  block_sync();
  // ---- 6d: the components, by doubling (a path among K <= 64 slots has at most 63 steps: six rounds) ----
  for (int round = 0; round < 6; ++round) {  // uniform
    const int from = round & 1, to = from ^ 1;
    if ((uint32_t)t < K) {
      const unsigned long long mine = reach[from][t];
      unsigned long long all = mine, rest = mine;
      for (int trip = 0; trip < CJ_MAX && rest; ++trip) {
        const int j = __ffsll((long long)rest) - 1;
        rest &= rest - 1ull;
        all |= reach[from][j];
      }
      reach[to][t] = all;
    }
    block_sync();
  }
  // (six rounds end in reach[0]) a lane per slot: its root; a lane per component: the members' sums, the majority
  if ((uint32_t)t < K) {
    const unsigned long long members = reach[0][t];
    const uint32_t root = (uint32_t)(__ffsll((long long)members) - 1);
    root_of[t] = root;
    if (root == (uint32_t)t) {
      JoinCounts sum{0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, INT32_MAX, INT32_MIN};
      int32_t with_circle = -1;
      unsigned long long rest = members;
      for (int trip = 0; trip < CJ_MAX && rest; ++trip) {  // (ascending slot, which is ascending id)
        const int j = __ffsll((long long)rest) - 1;
        rest &= rest - 1ull;
        const uint32_t id = cand[j];
        JoinCounts member{c_rows[id], c_core[id], {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, c_zmin[id], c_zmax[id]};
#pragma unroll
        for (int p = 0; p < ATTPC_MAX_SIM; ++p) member.votes[p] = c_votes[(size_t)id * ATTPC_MAX_SIM + p];
        join_merge(&sum, member);
        if (with_circle < 0 && (flags[j] & CJ_HAS)) with_circle = j;
      }
      uint32_t major_rows = 0u;
      const int32_t major = cluster_majority(sum.votes, &major_rows);
      m_rows[t] = sum.rows;
      m_core[t] = sum.core_rows;
      m_zmin[t] = sum.z_min;
      m_zmax[t] = sum.z_max;
      m_major[t] = major;
      m_major_rows[t] = major_rows;
      m_parts[t] = (uint32_t)__popcll(members);
      m_circle[t] = with_circle;
      m_label[t] = -1;
      atomicAdd(&counts[CJ_COMPONENTS], 1u);
      if (s.match == ATTPC_CLUSTER_MATCH_TRUTH && major >= 0) atomicMax(&best_key[major], cluster_key(sum.rows, cand[t]));
    }
  }
  block_sync();
  // ---- 7 and 8 on the components: the rank is the number of components with a larger key (keys differ) ----
  if ((uint32_t)t < K && root_of[t] == (uint32_t)t) {
    const unsigned long long key = cluster_key(m_rows[t], cand[t]);
    uint32_t rank = 0u;
    for (uint32_t j = 0u; j < K; ++j) rank += root_of[j] == j && cluster_key(m_rows[j], cand[j]) > key ? 1u : 0u;
    if (rank < (uint32_t)ATTPC_MAX_SIM) top_slot[rank] = (uint32_t)t;
    const int32_t major = m_major[t];
    if (s.match == ATTPC_CLUSTER_MATCH_TRUTH) {
      if (major >= 0 && best_key[major] == key)
        m_label[t] = s.give[major];
      else
        atomicAdd(&counts[major >= 0 ? CJ_SPLIT : CJ_FAKE], 1u);
    } else if (rank < (uint32_t)ATTPC_MAX_SIM && rank < (uint32_t)s.n_sim) {
      m_label[t] = s.give[rank];
    }
  }
  block_sync();
  // ---- the labels of the rows ----
  for (uint32_t k = (uint32_t)t; k < m; k += CJ_THREADS) {
    const uint32_t c = comp[k];
    if (c == CLUSTER_NONE || c >= m || c_rows[c] < (uint32_t)s.min_cluster_size) continue;
    const uint32_t slot = slot_of[c];
    if (slot >= K) continue;
    a.c.out_labels[lo + orig[k]] = (int64_t)m_label[root_of[slot]];
  }
  // ---- 9: the records ----
  if (t == 0) {
    attpc_cluster_event ev = a.c.events[e];  // (n_rows, n_range, n_core, n_border, n_noise, n_small, truth_rows stay)
    ev.n_clusters = (int32_t)counts[CJ_COMPONENTS];
    ev.n_split = (int32_t)counts[CJ_SPLIT];
    ev.n_fake = (int32_t)counts[CJ_FAKE];
    a.c.events[e] = ev;
    if (a.join_events)
      a.join_events[e] = attpc_join_event{(int32_t)K, (int32_t)counts[CJ_CIRCLES], (int32_t)counts[CJ_PART], (int32_t)counts[CJ_PAIRS],
                                          (int32_t)(K - counts[CJ_COMPONENTS]), 0, {0, 0}};
  }
  if (t < ATTPC_MAX_SIM) {
    attpc_cluster_record rec = cluster_record_unused();
    attpc_join_record jrec = join_record_unused();
    const uint32_t slot = top_slot[t];
    if (slot < K) {
      const uint32_t id = cand[slot];
      rec = attpc_cluster_record{(int32_t)m_rows[slot], (int32_t)m_core[slot], (int32_t)orig[id], m_major[slot],
                                 (int32_t)m_major_rows[slot], m_label[slot], m_zmin[slot], m_zmax[slot]};
      const double nan = __builtin_nan("");
      const int32_t w = m_circle[slot];
      jrec = attpc_join_record{(int32_t)m_parts[slot], (int32_t)orig[id], w >= 0 ? circle_a[w] : nan, w >= 0 ? circle_b[w] : nan,
                               w >= 0 ? circle_r[w] : nan};
    }
    if (a.c.records) a.c.records[(size_t)e * ATTPC_MAX_SIM + t] = rec;
    if (a.join_records) a.join_records[(size_t)e * ATTPC_MAX_SIM + t] = jrec;
  }
}

void launch_cluster_join(hipStream_t s, uint32_t n_events, const ClusterJoinArgs& a) {
  hipLaunchKernelGGL(cluster_join_kernel, dim3(n_events), dim3(CJ_THREADS), 0, s, a);
}

}  // namespace attpc
