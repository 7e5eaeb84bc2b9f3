// cluster_host.hpp -- the parts of the clustering (include/attpc_engine.h, "clustering") that are one piece of code for
// the device and the host: the checks of an attpc_cluster_desc, the settings a row reads, the metric, the neighbour
// predicate, the vote of a truth label and the key that ranks a cluster -- and a plain sequential form of steps 1 to 9
// for the host.  Integer arithmetic only.  cluster.hip uses the shared parts on the device, abi.hip the checks on the
// host, and tests/native/cluster_check.cpp compiles this file alone (tests/test_cluster_cpu.py holds the sequential
// form to tests/cluster_reference.py exactly).
//
// This is DBSCAN with every tie made definite, not Spyral's HDBSCAN + cluster joining + outlier-factor cleanup; nothing
// here has been compared against Spyral.
//
// Bounds of the metric (step 2): X and Y are in -5120 .. 5120 (estimate_quantise), so |dX|, |dY| <= 10 240 and
// dX^2 + dY^2 <= 209 715 200 < 2^28; Ez <= 1024 gives Ez^2 <= 2^20 and (dX^2 + dY^2) Ez^2 < 2^48.  The metric is
// formed only where |dZ| <= Ez, so dZ^2 Exy^2 <= 2^20 * 2^20 = 2^40.  d < 2^48 + 2^40 < 2^49, the threshold
// Exy^2 Ez^2 <= 2^40: nothing overflows 64 bits.  The sequential form takes dZ from any pair: |dZ| <= 262 144 = 2^18
// and Exy^2 <= 2^20 give dZ^2 Exy^2 <= 2^56, still inside 64 bits.
#pragma once
#include <stdint.h>

#include <vector>

#include "estimate_host.hpp"

namespace attpc {

constexpr int32_t CLUSTER_MAX_UNITS = 1024;     // Exy, Ez: 1 .. 1024 (1/16 .. 64 mm)
constexpr int32_t CLUSTER_MAX_ROWS_LIMIT = 65535;
constexpr uint32_t CLUSTER_NONE = 0xffffffffu;  // no cluster, no candidate

// Exy or Ez of a linking length in mm; 0: out of range (a NaN fails the comparisons)
inline int32_t cluster_units(double eps) {
  if (!(eps >= 1.0 / 16.0 && eps <= 64.0)) return 0;
  return (int32_t)rint(16.0 * eps);
}

// nullptr, or what is wrong with the settings
inline const char* cluster_desc_error(const attpc_cluster_desc& d) {
  if (cluster_units(d.eps_xy) < 1) return "eps_xy: 1/16 .. 64 mm";
  if (cluster_units(d.eps_z) < 1) return "eps_z: 1/16 .. 64 mm";
  if (d.min_samples < 1) return "min_samples: >= 1";
  if (d.min_cluster_size < 1) return "min_cluster_size: >= 1";
  if (d.max_rows < 1 || d.max_rows > CLUSTER_MAX_ROWS_LIMIT) return "max_rows: 1 .. 65535";
  if (d.match != ATTPC_CLUSTER_MATCH_TRUTH && d.match != ATTPC_CLUSTER_MATCH_RANK) return "match: ATTPC_CLUSTER_MATCH_TRUTH or _RANK";
  if (d.reserved[0] != 0 || d.reserved[1] != 0) return "reserved: 0";
  return nullptr;
}

// nullptr, or what is wrong with the layout as the clustering reads it
inline const char* cluster_layout_error(const attpc_event_layout& lay) {
  if (lay.n_sim < 0 || lay.n_sim > ATTPC_MAX_SIM) return "n_sim outside 0 .. 8";
  return nullptr;
}

struct ClusterSettings {  // what the kernel reads of a checked desc and a layout
  int64_t exy2, ez2, limit;            // Exy^2, Ez^2 and the threshold Exy^2 Ez^2
  int32_t ez;
  int32_t min_samples, min_cluster_size, max_rows, match, n_sim;
  int64_t vote_label[ATTPC_MAX_SIM];   // the truth label that votes for position s; -1: nobody does
  int32_t give[ATTPC_MAX_SIM];         // the label a cluster matched to position s gets: indices[s], -1 from n_sim on
};

inline ClusterSettings cluster_settings(const attpc_cluster_desc& d, const attpc_event_layout& lay) {
  ClusterSettings s{};
  const int64_t exy = cluster_units(d.eps_xy), ez = cluster_units(d.eps_z);
  s.exy2 = exy * exy;
  s.ez2 = ez * ez;
  s.limit = s.exy2 * s.ez2;
  s.ez = (int32_t)ez;
  s.min_samples = d.min_samples;
  s.min_cluster_size = d.min_cluster_size;
  s.max_rows = d.max_rows;
  s.match = d.match;
  s.n_sim = lay.n_sim;
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) {
    s.give[p] = p < lay.n_sim ? lay.indices[p] : -1;
    s.vote_label[p] = p < lay.n_sim && lay.indices[p] >= 0 ? (int64_t)lay.indices[p] : -1;
    for (int q = 0; q < p && q < lay.n_sim; ++q)
      if (lay.indices[q] == lay.indices[p]) s.vote_label[p] = -1;  // (a label given twice votes for the lower position)
  }
  return s;
}

// step 2: d(i, j) of the differences in units
ATTPC_EST_HD int64_t cluster_metric(const ClusterSettings& s, int32_t dx, int32_t dy, int32_t dz) {
  return ((int64_t)dx * dx + (int64_t)dy * dy) * s.ez2 + (int64_t)dz * dz * s.exy2;
}

// step 2: j is a neighbour of i
ATTPC_EST_HD bool cluster_neighbour(const ClusterSettings& s, int32_t dx, int32_t dy, int32_t dz) {
  const int32_t az = dz < 0 ? -dz : dz;
  return az <= s.ez && cluster_metric(s, dx, dy, dz) <= s.limit;
}

// step 8: the position a truth label votes for, -1: none
ATTPC_EST_HD int32_t cluster_vote(const ClusterSettings& s, int64_t label) {
  int32_t p = -1;
  if (label >= 0)
    for (int q = ATTPC_MAX_SIM - 1; q >= 0; --q) p = s.vote_label[q] == label ? q : p;
  return p;
}

// step 7 as one number: a cluster ranks before another iff its key is larger (rows descending, id ascending); 0 is
// the key of no cluster, since a cluster has a row
ATTPC_EST_HD unsigned long long cluster_key(uint32_t rows, uint32_t id) {
  return ((unsigned long long)rows << 32) | (unsigned long long)(0xffffffffu - id);
}
ATTPC_EST_HD uint32_t cluster_key_id(unsigned long long key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffull); }

// step 8: the majority of a cluster's eight vote counts -> position (-1: none) and its votes
ATTPC_EST_HD int32_t cluster_majority(const uint32_t* votes, uint32_t* majority_rows) {
  int32_t p = -1;
  uint32_t best = 0u;
  for (int q = 0; q < ATTPC_MAX_SIM; ++q)
    if (votes[q] > best) {
      best = votes[q];
      p = q;
    }
  *majority_rows = best;
  return p;
}

// the record of an event that is not clustered (step 9, or a bound that was met): truth_rows stay as they are
ATTPC_EST_HD void cluster_event_unclustered(int32_t n_rows, int32_t status, attpc_cluster_event* ev) {
  ev->n_rows = n_rows;
  ev->n_range = ev->n_core = ev->n_border = 0;
  ev->n_noise = n_rows;
  ev->n_clusters = ev->n_small = ev->n_split = ev->n_fake = 0;
  ev->status = status;
  ev->reserved[0] = ev->reserved[1] = 0;
}

ATTPC_EST_HD attpc_cluster_record cluster_record_unused() { return attpc_cluster_record{0, 0, -1, 0, 0, 0, 0, 0}; }

// the in-range rows of an event stand in nondecreasing Z (step 1; the stage-alone entry point checks it)
inline bool cluster_rows_sorted(int64_t n, const double* rows) {
  bool first = true;
  int32_t last = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double* p = rows + 8 * i;
    int32_t X, Y, Z;
    int64_t I;
    if (!estimate_quantise(p[0], p[1], p[2], p[4], &X, &Y, &Z, &I)) continue;
    if (!first && Z < last) return false;
    first = false;
    last = Z;
  }
  return true;
}

// a cluster of the sequential form: the id is a row index
struct HostCluster { uint32_t id, rows, core_rows, votes[ATTPC_MAX_SIM], majority_rows; int32_t majority, label, z_min, z_max; };

// What may stand between step 6 and step 7 of the sequential form (join_host.hpp, "cluster joining"): it sees the
// surviving clusters, the rows in units and the cluster id of every row (CLUSTER_NONE: none), and may replace the
// clusters and move rows from one id to another.
struct ClusterHostHook {
  virtual void between_6_and_7(std::vector<HostCluster>& kept, int64_t n, const int32_t* X, const int32_t* Y,
                               std::vector<uint32_t>& cluster_of_row) = 0;
  virtual ~ClusterHostHook() {}
};

// Steps 1 to 9 of one event, one row after the other: rows [n][8], labels [n] or nullptr -> out_labels [n], *ev and
// rec[ATTPC_MAX_SIM].  n < 2^31.  `hook`: see ClusterHostHook; nullptr is the clustering alone.
inline void cluster_event_host(const ClusterSettings& s, int64_t n, const double* rows, const int64_t* labels,
                               int64_t* out_labels, attpc_cluster_event* ev, attpc_cluster_record* rec,
                               ClusterHostHook* hook = nullptr) {
  *ev = attpc_cluster_event{};
  for (int k = 0; k < ATTPC_MAX_SIM; ++k) rec[k] = cluster_record_unused();
  for (int64_t i = 0; i < n; ++i) {
    out_labels[i] = -1;
    const int32_t p = labels ? cluster_vote(s, labels[i]) : -1;
    if (p >= 0 && ev->truth_rows[p] < 65535) ev->truth_rows[p] = (uint16_t)(ev->truth_rows[p] + 1);
  }
  if (n > s.max_rows) {
    cluster_event_unclustered((int32_t)n, ATTPC_CLUSTER_CAPPED, ev);
    return;
  }
  struct Row { int32_t X, Y, Z; bool ok, core; uint32_t cluster; };
  std::vector<Row> r((size_t)n);
  int32_t n_range = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double* p = rows + 8 * i;
    int64_t I;
    r[i].ok = estimate_quantise(p[0], p[1], p[2], p[4], &r[i].X, &r[i].Y, &r[i].Z, &I);
    r[i].core = false;
    r[i].cluster = CLUSTER_NONE;
    n_range += !r[i].ok;
  }
  auto near = [&](int64_t i, int64_t j) {
    return r[i].ok && r[j].ok && cluster_neighbour(s, r[j].X - r[i].X, r[j].Y - r[i].Y, r[j].Z - r[i].Z);
  };
  for (int64_t i = 0; i < n; ++i) {  // step 3
    int64_t count = 0;
    for (int64_t j = 0; j < n; ++j) count += near(i, j);
    r[i].core = r[i].ok && count >= s.min_samples;
  }
  // step 4: in ascending row order a core row without a cluster starts one under its own index and floods it
  std::vector<int64_t> todo;
  for (int64_t i = 0; i < n; ++i) {
    if (!r[i].core || r[i].cluster != CLUSTER_NONE) continue;
    r[i].cluster = (uint32_t)i;
    todo.assign(1, i);
    while (!todo.empty()) {
      const int64_t a = todo.back();
      todo.pop_back();
      for (int64_t j = 0; j < n; ++j)
        if (r[j].core && r[j].cluster == CLUSTER_NONE && near(a, j)) {
          r[j].cluster = (uint32_t)i;
          todo.push_back(j);
        }
    }
  }
  for (int64_t i = 0; i < n; ++i) {  // step 5
    if (!r[i].ok || r[i].core) continue;
    int64_t best = -1, best_d = 0;
    for (int64_t j = 0; j < n; ++j) {
      if (!r[j].core || !near(i, j)) continue;
      const int64_t d = cluster_metric(s, r[j].X - r[i].X, r[j].Y - r[i].Y, r[j].Z - r[i].Z);
      if (best < 0 || d < best_d) {
        best = j;
        best_d = d;
      }
    }
    if (best >= 0) r[i].cluster = r[best].cluster;
  }
  // steps 6 and 7: the clusters by id, their sizes, votes and extent
  typedef HostCluster Cluster;
  std::vector<Cluster> clusters;
  std::vector<int64_t> slot((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    if (r[i].cluster == CLUSTER_NONE) continue;
    int64_t& c = slot[r[i].cluster];
    if (c < 0) {
      c = (int64_t)clusters.size();
      clusters.push_back(Cluster{r[i].cluster, 0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, 0u, -1, -1, r[i].Z, r[i].Z});
    }
    Cluster& k = clusters[(size_t)c];
    k.rows += 1u;
    k.core_rows += r[i].core ? 1u : 0u;
    k.z_min = r[i].Z < k.z_min ? r[i].Z : k.z_min;
    k.z_max = r[i].Z > k.z_max ? r[i].Z : k.z_max;
    const int32_t p = labels ? cluster_vote(s, labels[i]) : -1;
    if (p >= 0) k.votes[p] += 1u;
  }
  std::vector<Cluster> kept;
  int32_t n_small = 0;
  for (const Cluster& k : clusters) {
    if (k.rows < (uint32_t)s.min_cluster_size)
      n_small += 1;
    else
      kept.push_back(k);
  }
  if (hook) {
    std::vector<int32_t> X((size_t)n), Y((size_t)n);
    std::vector<uint32_t> of((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      X[i] = r[i].X;
      Y[i] = r[i].Y;
      of[i] = r[i].cluster;
    }
    hook->between_6_and_7(kept, n, X.data(), Y.data(), of);
    for (int64_t i = 0; i < n; ++i) r[i].cluster = of[i];
  }
  for (size_t a = 1; a < kept.size(); ++a)  // (insertion sort by the key, descending)
    for (size_t b = a; b > 0 && cluster_key(kept[b].rows, kept[b].id) > cluster_key(kept[b - 1].rows, kept[b - 1].id); --b)
      std::swap(kept[b], kept[b - 1]);
  // step 8
  int32_t n_split = 0, n_fake = 0;
  bool taken[ATTPC_MAX_SIM] = {false, false, false, false, false, false, false, false};
  for (size_t k = 0; k < kept.size(); ++k) {
    Cluster& c = kept[k];
    c.majority = cluster_majority(c.votes, &c.majority_rows);
    if (s.match == ATTPC_CLUSTER_MATCH_RANK) {
      c.label = k < (size_t)s.n_sim ? s.give[k] : -1;
    } else if (c.majority >= 0 && !taken[c.majority]) {
      taken[c.majority] = true;
      c.label = s.give[c.majority];
    } else {
      c.label = -1;
      n_split += c.majority >= 0;
      n_fake += c.majority < 0;
    }
  }
  int32_t n_core = 0, n_border = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (r[i].cluster == CLUSTER_NONE) continue;
    for (const Cluster& c : kept)
      if (c.id == r[i].cluster) {
        out_labels[i] = c.label;
        n_core += r[i].core;
        n_border += !r[i].core;
      }
  }
  ev->n_rows = (int32_t)n;
  ev->n_range = n_range;
  ev->n_core = n_core;
  ev->n_border = n_border;
  ev->n_noise = (int32_t)n - n_core - n_border;
  ev->n_clusters = (int32_t)kept.size();
  ev->n_small = n_small;
  ev->n_split = n_split;
  ev->n_fake = n_fake;
  ev->status = 0;
  for (size_t k = 0; k < kept.size() && k < (size_t)ATTPC_MAX_SIM; ++k) {
    const Cluster& c = kept[k];
    rec[k] = attpc_cluster_record{(int32_t)c.rows, (int32_t)c.core_rows, (int32_t)c.id, c.majority, (int32_t)c.majority_rows,
                                  c.label, c.z_min, c.z_max};
  }
}

}  // namespace attpc
