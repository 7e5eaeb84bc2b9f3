// undistort_check.cpp -- csrc/undistort_host.hpp compiled alone for the host (tests/test_undistort_cpu.py).  The input
// file is doubles: windows_edge, micromegas_edge, length, iterations, tolerance_xy, tolerance_tb; a map as
// distort_check.cpp takes it -- rho_step, tau_step, tb_origin, n_rho, n_tau, three flags, the tables that follow --; and
// then, for `rows`, n_events, the n_events + 1 offsets, and per row its 8 doubles and its label.
//   undistort_check rows in.bin out.bin  -> per output row its 8 doubles, its label and its input row; then the four
//                                            counts (n_rows, n_skipped, n_unconverged, n_moved)
//   undistort_check desc in.bin out.bin  -> 1 double: 1 = the desc is refused
// The order of an event's rows is the contract's step 6, by a stable sort of the host.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "undistort_host.hpp"

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

static int32_t as_int(double v) { return v >= -1.0e9 && v <= 1.0e9 ? (int32_t)v : -1; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<double> in = read_all(argv[2]);
  if (in.size() < 14) return 3;
  attpc_undistort_desc u{};
  u.windows_edge = as_int(in[0]);
  u.micromegas_edge = as_int(in[1]);
  u.length = in[2];
  u.iterations = as_int(in[3]);
  u.tolerance_xy = in[4];
  u.tolerance_tb = in[5];
  attpc_distort_desc& d = u.map;
  d.rho_step = in[6];
  d.tau_step = in[7];
  d.tb_origin = in[8];
  d.n_rho = as_int(in[9]);
  d.n_tau = as_int(in[10]);
  const bool sized = d.n_rho >= 1 && d.n_rho <= 4096 && d.n_tau >= 1 && d.n_tau <= 4096;
  const size_t nodes = sized ? (size_t)d.n_rho * (size_t)d.n_tau : 0;
  size_t at = 14;
  const double** tables[3] = {&d.radial, &d.azimuthal, &d.time};
  for (int k = 0; k < 3; ++k) {
    if (in[11 + k] == 0.0 || !sized) continue;
    if (at + nodes > in.size()) return 3;
    *tables[k] = in.data() + at;
    at += nodes;
  }
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    out.push_back(attpc::undistort_desc_error(u) != nullptr ? 1.0 : 0.0);
  } else if (!std::strcmp(argv[1], "rows")) {
    if (attpc::undistort_desc_error(u) || at >= in.size()) return 3;
    const size_t n_events = (size_t)in[at++];
    if (at + n_events + 1 > in.size()) return 3;
    const double* offsets = in.data() + at;
    at += n_events + 1;
    const size_t n_rows = (size_t)offsets[n_events];
    if (offsets[0] != 0.0 || in.size() - at != n_rows * 9) return 3;
    const double* rows = in.data() + at;  // 9 doubles a row: the row and its label
    const attpc::DistortMap m{d.rho_step, d.tau_step, d.tb_origin, d.n_rho, d.n_tau, d.radial, d.azimuthal, d.time};
    const attpc::UndistortSettings s = attpc::undistort_settings(u, m);
    double counts[4] = {0.0, 0.0, 0.0, 0.0};
    out.resize(n_rows * 10);
    struct Point { double x, y, t; int status; };
    for (size_t e = 0; e < n_events; ++e) {
      const size_t lo = (size_t)offsets[e], n = (size_t)offsets[e + 1] - lo;
      std::vector<Point> points(n);
      std::vector<size_t> sorted, skipped;
      for (size_t i = 0; i < n; ++i) {
        Point& p = points[i];
        p.status = attpc::undistort_row(s, rows + 9 * (lo + i), p.x, p.y, p.t);
        (p.status == attpc::UNDISTORT_SKIPPED ? skipped : sorted).push_back(i);
        counts[1] += p.status == attpc::UNDISTORT_SKIPPED;
        counts[2] += p.status == attpc::UNDISTORT_UNCONVERGED;
      }
      counts[0] += (double)n;
      std::stable_sort(sorted.begin(), sorted.end(), [&](size_t a, size_t b) { return points[a].t > points[b].t; });
      sorted.insert(sorted.end(), skipped.begin(), skipped.end());
      for (size_t k = 0; k < n; ++k) {
        const size_t i = sorted[k];
        const double* src = rows + 9 * (lo + i);
        double* dst = out.data() + 10 * (lo + k);
        std::memcpy(dst, src, 9 * sizeof(double));
        if (points[i].status != attpc::UNDISTORT_SKIPPED) {
          dst[0] = points[i].x * 1000.0;
          dst[1] = points[i].y * 1000.0;
          dst[2] = attpc::undistort_z(s, points[i].t);
        }
        dst[9] = (double)(lo + i);
        counts[3] += i != k;
      }
    }
    out.insert(out.end(), counts, counts + 4);
  } else {
    return 2;
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
