// join_host.hpp -- the parts of the cluster joining (include/attpc_engine.h, "cluster joining") that are one piece of
// code for the device and the host: the checks of an attpc_join_desc, the terms a row adds to its cluster's seven
// integer sums, the circle from the sums, the overlap predicate, the merge of two clusters' counts -- and a plain
// sequential form of steps 6a to 9 on top of cluster_event_host.  cluster_join.hip uses the shared parts on the device,
// abi.hip the checks on the host, and tests/native/join_check.cpp compiles this file alone (tests/test_join_cpu.py
// holds the sequential form to tests/join_reference.py exactly).
//
// The contract is Spyral's cluster joining in structure, with every tie made definite.  It is not Spyral's code,
// Spyral iterates the joining and this does not, and nothing here has been compared against Spyral.
//
// Bounds of the sums (step 6b): X and Y are in -5120 .. 5120 (estimate_quantise), so |u|, |v| <= 10 240 and
// u^2 + v^2 <= 2 * 10 240^2 < 2^28; a term |u (u^2 + v^2)| <= 10 240 * 2 * 10 240^2 < 2^42.  A cluster has at most
// 65 535 rows (max_rows), so every sum is below 65 535 * 10 240 * 2 * 10 240^2 < 2^57: nothing overflows 64 bits, and
// integer additions give one result in any order.
#pragma once
#include <stdint.h>

#include <vector>

#include "cluster_host.hpp"
#include "helix_host.hpp"

namespace attpc {

constexpr double JOIN_PI = 3.141592653589793;  // the constant of helix_atan2w

// nullptr, or what is wrong with the settings (a NaN fails the comparisons)
inline const char* join_desc_error(const attpc_join_desc& d) {
  if (!(d.overlap_ratio > 0.0 && d.overlap_ratio <= 1.0)) return "overlap_ratio: in (0, 1]";
  if (!(d.min_radius >= 1.0 / 16.0 && d.min_radius <= 5000.0)) return "min_radius: 1/16 .. 5000 mm";
  if (!(d.radius_ratio == 0.0 || (d.radius_ratio >= 1.0 && d.radius_ratio - d.radius_ratio == 0.0))) return "radius_ratio: 0 or finite and >= 1";
  if (d.max_clusters < 2 || d.max_clusters > ATTPC_JOIN_MAX_CLUSTERS) return "max_clusters: 2 .. 64";
  if (d.reserved[0] != 0 || d.reserved[1] != 0 || d.reserved[2] != 0) return "reserved: 0";
  return nullptr;
}

struct JoinSettings {  // what the kernel reads of a checked desc
  double overlap_ratio, min_radius, radius_ratio;
  int32_t max_clusters;
};

inline JoinSettings join_settings(const attpc_join_desc& d) {
  return JoinSettings{d.overlap_ratio, d.min_radius, d.radius_ratio, d.max_clusters};
}

enum { JOIN_SU = 0, JOIN_SV, JOIN_SUU, JOIN_SVV, JOIN_SUV, JOIN_SUQ, JOIN_SVQ, JOIN_SUMS };

// step 6b: what a row at (u, v) from its cluster's id row adds to the seven sums
ATTPC_EST_HD void join_terms(int32_t u, int32_t v, int64_t* term) {
  const int64_t U = u, V = v, q = U * U + V * V;
  term[JOIN_SU] = U;
  term[JOIN_SV] = V;
  term[JOIN_SUU] = U * U;
  term[JOIN_SVV] = V * V;
  term[JOIN_SUV] = U * V;
  term[JOIN_SUQ] = U * q;
  term[JOIN_SVQ] = V * q;
}

struct JoinCircle {
  double a, b, R;  // mm, absolute
  bool has;        // step 6b: the candidate has a circle
};

// step 6b: the circle of a candidate of `rows` rows with the id row (x_id, y_id) in units and the seven sums
ATTPC_EST_HD JoinCircle join_circle(uint32_t rows, int32_t x_id, int32_t y_id, const int64_t* sum) {
#pragma clang fp contract(off)
  JoinCircle c{0.0, 0.0, 0.0, false};
  if (rows < 3u) return c;
  EstimateSums k{};
  k.m = (int64_t)rows;
  k.x0 = x_id;
  k.y0 = y_id;
  k.su = sum[JOIN_SU];
  k.sv = sum[JOIN_SV];
  k.suu = sum[JOIN_SUU];
  k.svv = sum[JOIN_SVV];
  k.suv = sum[JOIN_SUV];
  k.suuu = sum[JOIN_SUQ];  // (u^3 + u v^2 as one sum: estimate_kasa adds the other, 0, to it, which is exact)
  k.svvv = sum[JOIN_SVQ];
  double uc = 0.0, vc = 0.0, r2 = 0.0;
  if (!estimate_kasa(k, &uc, &vc, &r2)) return c;
  c.a = ((double)x_id + uc) / 16.0;
  c.b = ((double)y_id + vc) / 16.0;
  c.R = sqrt(r2) / 16.0;
  // (x - x is 0 for a finite x and NaN otherwise)
  c.has = c.a - c.a == 0.0 && c.b - c.b == 0.0 && c.R - c.R == 0.0;
  return c;
}

// step 6b: the candidate takes part in step 6c
ATTPC_EST_HD bool join_takes_part(const JoinSettings& s, const JoinCircle& c) { return c.has && !(c.R < s.min_radius); }

// step 6c: acos(c) of a c in -1 .. 1 by the written arctangent
ATTPC_EST_HD double join_acos(double c) {
#pragma clang fp contract(off)
  const double q = 1.0 - c * c;
  return helix_atan2w(sqrt(q > 0.0 ? q : 0.0), c);
}

// step 6c: the area two circles of radii Rs <= Rl share, their centres d apart
ATTPC_EST_HD double join_overlap_area(double Rs, double Rl, double d) {
#pragma clang fp contract(off)
  if (d >= Rs + Rl) return 0.0;
  if (d <= Rl - Rs) return JOIN_PI * (Rs * Rs);
  const double cs = (d * d + Rs * Rs - Rl * Rl) / (2.0 * d * Rs);
  const double cl = (d * d + Rl * Rl - Rs * Rs) / (2.0 * d * Rl);
  const double k = (-d + Rs + Rl) * (d + Rs - Rl) * (d - Rs + Rl) * (d + Rs + Rl);
  return Rs * Rs * join_acos(cs) + Rl * Rl * join_acos(cl) - 0.5 * sqrt(k > 0.0 ? k : 0.0);
}

// step 6c: two candidates that take part are joined; `lower` is the one of the lower id
ATTPC_EST_HD bool join_pair(const JoinSettings& s, const JoinCircle& lower, const JoinCircle& higher) {
#pragma clang fp contract(off)
  const bool swap = higher.R < lower.R;  // (on a tie the lower id is "s")
  const double Rs = swap ? higher.R : lower.R, Rl = swap ? lower.R : higher.R;
  const double da = higher.a - lower.a, db = higher.b - lower.b;
  const double d = sqrt(da * da + db * db);
  const double A = join_overlap_area(Rs, Rl, d);
  return A >= s.overlap_ratio * (JOIN_PI * (Rs * Rs)) && (s.radius_ratio == 0.0 || Rl <= s.radius_ratio * Rs);
}

struct JoinCounts {  // what step 6d sums over the members of a component
  uint32_t rows, core_rows, votes[ATTPC_MAX_SIM];
  int32_t z_min, z_max;
};

// step 6d: a member's counts added to its component's
ATTPC_EST_HD void join_merge(JoinCounts* into, const JoinCounts& member) {
  into->rows += member.rows;
  into->core_rows += member.core_rows;
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) into->votes[p] += member.votes[p];
  into->z_min = member.z_min < into->z_min ? member.z_min : into->z_min;
  into->z_max = member.z_max > into->z_max ? member.z_max : into->z_max;
}

ATTPC_EST_HD attpc_join_record join_record_unused() { return attpc_join_record{0, -1, 0.0, 0.0, 0.0}; }

// the join event of an event that is not joined: zeros, `n_candidates` and the status
ATTPC_EST_HD attpc_join_event join_event_not_joined(int32_t n_candidates, int32_t status) {
  return attpc_join_event{n_candidates, 0, 0, 0, 0, status, {0, 0}};
}

// Steps 6a to 6d of one event, one candidate after the other, as the hook of cluster_event_host; *ev and
// rec_by_id are filled here, join_event_host puts the records in rank order.
struct JoinHostHook : ClusterHostHook {
  JoinSettings s;
  attpc_join_event ev;
  bool ran = false;
  struct Part { uint32_t id; int32_t parts; JoinCircle circle; };
  std::vector<Part> components;

  explicit JoinHostHook(const JoinSettings& settings) : s(settings), ev(join_event_not_joined(0, 0)) {}

  void between_6_and_7(std::vector<HostCluster>& kept, int64_t n, const int32_t* X, const int32_t* Y,
                       std::vector<uint32_t>& cluster_of_row) override {
    ran = true;
    for (size_t a = 1; a < kept.size(); ++a)  // 6a: ascending id
      for (size_t b = a; b > 0 && kept[b].id < kept[b - 1].id; --b) std::swap(kept[b], kept[b - 1]);
    const size_t K = kept.size();
    ev = join_event_not_joined((int32_t)K, 0);
    if (K > (size_t)s.max_clusters) {
      ev.status = ATTPC_JOIN_CAPPED;
      return;
    }
    std::vector<JoinCircle> circle(K);
    std::vector<bool> part(K);
    for (size_t c = 0; c < K; ++c) {  // 6b
      int64_t sum[JOIN_SUMS] = {0, 0, 0, 0, 0, 0, 0}, term[JOIN_SUMS];
      const uint32_t id = kept[c].id;
      for (int64_t i = 0; i < n; ++i) {
        if (cluster_of_row[i] != id) continue;
        join_terms(X[i] - X[id], Y[i] - Y[id], term);
        for (int q = 0; q < JOIN_SUMS; ++q) sum[q] += term[q];
      }
      circle[c] = join_circle(kept[c].rows, X[id], Y[id], sum);
      part[c] = join_takes_part(s, circle[c]);
      ev.n_circles += circle[c].has;
      ev.n_taking_part += part[c];
    }
    std::vector<size_t> root(K);  // 6c and 6d: the lowest member of every candidate's component
    for (size_t c = 0; c < K; ++c) root[c] = c;
    for (size_t i = 0; i < K; ++i)
      for (size_t j = i + 1; j < K; ++j) {
        if (!part[i] || !part[j] || !join_pair(s, circle[i], circle[j])) continue;
        ev.n_pairs += 1;
        const size_t ri = root[i], rj = root[j], low = ri < rj ? ri : rj, high = ri < rj ? rj : ri;
        for (size_t c = 0; c < K; ++c) root[c] = root[c] == high ? low : root[c];
      }
    std::vector<HostCluster> joined;
    components.clear();
    for (size_t c = 0; c < K; ++c) {
      if (root[c] != c) continue;
      JoinCounts sum{0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, INT32_MAX, INT32_MIN};
      Part p{kept[c].id, 0, JoinCircle{0.0, 0.0, 0.0, false}};
      for (size_t j = c; j < K; ++j) {
        if (root[j] != c) continue;
        JoinCounts member{kept[j].rows, kept[j].core_rows, {}, kept[j].z_min, kept[j].z_max};
        for (int q = 0; q < ATTPC_MAX_SIM; ++q) member.votes[q] = kept[j].votes[q];
        join_merge(&sum, member);
        p.parts += 1;
        if (!p.circle.has && circle[j].has) p.circle = circle[j];
      }
      HostCluster k = kept[c];
      k.rows = sum.rows;
      k.core_rows = sum.core_rows;
      for (int q = 0; q < ATTPC_MAX_SIM; ++q) k.votes[q] = sum.votes[q];
      k.z_min = sum.z_min;
      k.z_max = sum.z_max;
      joined.push_back(k);
      components.push_back(p);
    }
    ev.n_joined = (int32_t)(K - joined.size());
    for (int64_t i = 0; i < n; ++i)
      for (size_t c = 0; c < K; ++c)
        if (cluster_of_row[i] == kept[c].id) {
          cluster_of_row[i] = kept[root[c]].id;
          break;
        }
    kept.swap(joined);
  }
};

// Steps 1 to 9 of one event with the joining between 6 and 7: as cluster_event_host, and *jev and jrec[ATTPC_MAX_SIM].
inline void join_event_host(const ClusterSettings& s, const JoinSettings& js, int64_t n, const double* rows,
                            const int64_t* labels, int64_t* out_labels, attpc_cluster_event* ev, attpc_cluster_record* rec,
                            attpc_join_event* jev, attpc_join_record* jrec) {
  JoinHostHook hook(js);
  cluster_event_host(s, n, rows, labels, out_labels, ev, rec, &hook);
  for (int k = 0; k < ATTPC_MAX_SIM; ++k) jrec[k] = join_record_unused();
  if (!hook.ran || n == 0) {  // (CAPPED; the sequential form has no INTERNAL)
    *jev = join_event_not_joined(0, ATTPC_JOIN_NOT_CLUSTERED);
    return;
  }
  *jev = hook.ev;
  if (jev->status) return;
  const double nan = __builtin_nan("");
  for (int k = 0; k < ATTPC_MAX_SIM; ++k) {
    if (rec[k].first_row < 0) continue;
    for (const JoinHostHook::Part& p : hook.components)
      if (p.id == (uint32_t)rec[k].first_row)
        jrec[k] = attpc_join_record{p.parts, rec[k].first_row, p.circle.has ? p.circle.a : nan, p.circle.has ? p.circle.b : nan,
                                    p.circle.has ? p.circle.R : nan};
  }
}

}  // namespace attpc
