// join_check.cpp -- csrc/join_host.hpp compiled alone for the host (tests/test_join_cpu.py).  The input file is doubles:
// eps_xy, eps_z, min_samples, min_cluster_size, max_rows, match, the two reserved words, n_sim and the eight indices
// (as cluster_check.cpp), then overlap_ratio, min_radius, radius_ratio, max_clusters and the three reserved words of the
// join desc; and then, for `rows`, n_events, the n_events + 1 offsets, and per row its 8 doubles and its label.
//   join_check rows in.bin out.bin  -> per row its cluster label; then per event the 10 counts of its cluster event and
//                                      its 8 truth_rows; then per event its 8 cluster records of 8 numbers each; then
//                                      per event the 6 numbers of its join event; then per event its 8 join records of
//                                      5 numbers each (parts, first_row, a, b, radius)
//   join_check desc in.bin out.bin  -> 1 double: 1 = the join desc is refused
#include <cstdio>
#include <cstring>
#include <vector>

#include "join_host.hpp"

static std::vector<double> read_all(const char* path) {
  std::vector<double> data;
  FILE* f = std::fopen(path, "rb");
  if (!f) return data;
  double buf[1024];
  size_t n;
  while ((n = std::fread(buf, sizeof(double), 1024, f)) > 0) data.insert(data.end(), buf, buf + n);
  std::fclose(f);
  return data;
}

static int32_t as_int(double v) { return v >= -2147483648.0 && v <= 2147483647.0 ? (int32_t)v : -1; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<double> in = read_all(argv[2]);
  if (in.size() < 24) return 3;
  attpc_cluster_desc d{};
  d.eps_xy = in[0];
  d.eps_z = in[1];
  d.min_samples = as_int(in[2]);
  d.min_cluster_size = as_int(in[3]);
  d.max_rows = as_int(in[4]);
  d.match = as_int(in[5]);
  d.reserved[0] = as_int(in[6]);
  d.reserved[1] = as_int(in[7]);
  attpc_event_layout lay{};
  lay.n_sim = as_int(in[8]);
  for (int s = 0; s < ATTPC_MAX_SIM; ++s) lay.indices[s] = as_int(in[9 + s]);
  attpc_join_desc j{};
  j.overlap_ratio = in[17];
  j.min_radius = in[18];
  j.radius_ratio = in[19];
  j.max_clusters = as_int(in[20]);
  for (int k = 0; k < 3; ++k) j.reserved[k] = as_int(in[21 + k]);
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    out.push_back(attpc::join_desc_error(j) != nullptr ? 1.0 : 0.0);
  } else if (!std::strcmp(argv[1], "rows")) {
    size_t at = 24;
    if (attpc::cluster_desc_error(d) || attpc::cluster_layout_error(lay) || attpc::join_desc_error(j) || at >= in.size()) return 3;
    const size_t n_events = (size_t)in[at++];
    if (at + n_events + 1 > in.size()) return 3;
    const double* offsets = in.data() + at;
    at += n_events + 1;
    const size_t n_rows = (size_t)offsets[n_events];
    if (offsets[0] != 0.0 || in.size() - at != n_rows * 9) return 3;
    std::vector<double> rows(n_rows * 8 + 1);
    std::vector<int64_t> labels(n_rows + 1), got(n_rows + 1);
    for (size_t r = 0; r < n_rows; ++r) {
      std::memcpy(rows.data() + 8 * r, in.data() + at + 9 * r, 8 * sizeof(double));
      labels[r] = (int64_t)in[at + 9 * r + 8];
    }
    const attpc::ClusterSettings s = attpc::cluster_settings(d, lay);
    const attpc::JoinSettings js = attpc::join_settings(j);
    std::vector<attpc_cluster_event> events(n_events + 1);
    std::vector<attpc_cluster_record> records((n_events + 1) * ATTPC_MAX_SIM);
    std::vector<attpc_join_event> join_events(n_events + 1);
    std::vector<attpc_join_record> join_records((n_events + 1) * ATTPC_MAX_SIM);
    for (size_t e = 0; e < n_events; ++e) {
      const size_t lo = (size_t)offsets[e];
      attpc::join_event_host(s, js, (int64_t)(offsets[e + 1] - offsets[e]), rows.data() + 8 * lo, labels.data() + lo, got.data() + lo,
                             &events[e], &records[e * ATTPC_MAX_SIM], &join_events[e], &join_records[e * ATTPC_MAX_SIM]);
    }
    for (size_t r = 0; r < n_rows; ++r) out.push_back((double)got[r]);
    for (size_t e = 0; e < n_events; ++e) {
      const attpc_cluster_event& v = events[e];
      const int32_t counts[10] = {v.n_rows, v.n_range, v.n_core, v.n_border, v.n_noise, v.n_clusters, v.n_small, v.n_split, v.n_fake, v.status};
      for (int32_t c : counts) out.push_back((double)c);
      for (int s2 = 0; s2 < ATTPC_MAX_SIM; ++s2) out.push_back((double)v.truth_rows[s2]);
    }
    for (size_t k = 0; k < n_events * ATTPC_MAX_SIM; ++k) {
      const attpc_cluster_record& c = records[k];
      const int32_t fields[8] = {c.rows, c.core_rows, c.first_row, c.majority, c.majority_rows, c.label, c.z_min, c.z_max};
      for (int32_t f : fields) out.push_back((double)f);
    }
    for (size_t e = 0; e < n_events; ++e) {
      const attpc_join_event& v = join_events[e];
      const int32_t counts[6] = {v.n_candidates, v.n_circles, v.n_taking_part, v.n_pairs, v.n_joined, v.status};
      for (int32_t c : counts) out.push_back((double)c);
    }
    for (size_t k = 0; k < n_events * ATTPC_MAX_SIM; ++k) {
      const attpc_join_record& c = join_records[k];
      out.push_back((double)c.parts);
      out.push_back((double)c.first_row);
      out.push_back(c.a);
      out.push_back(c.b);
      out.push_back(c.radius);
    }
  } else {
    return 2;
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
