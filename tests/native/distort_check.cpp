// distort_check.cpp -- csrc/distort_host.hpp compiled alone for the host (tests/test_distortion_cpu.py).  The input file
// is doubles: a map -- rho_step, tau_step, tb_origin, n_rho, n_tau, three flags (1 = the radial / azimuthal / time table
// follows), then the tables that follow, n_rho * n_tau values each -- and then, for `shift`, records of 4 doubles.
//   distort_check shift in.bin out.bin   -> the shifted records
//   distort_check desc in.bin out.bin    -> 2 doubles: 1 = the desc is refused, 1 = it is the stage off
#include <cstdio>
#include <cstring>
#include <vector>

#include "distort_host.hpp"

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

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::vector<double> in = read_all(argv[2]);
  if (in.size() < 8) return 3;
  attpc_distort_desc d{};
  d.rho_step = in[0];
  d.tau_step = in[1];
  d.tb_origin = in[2];
  // (the counts come as doubles: out-of-range ones are part of the desc checks, and must not be used as sizes before)
  d.n_rho = in[3] >= -1.0e9 && in[3] <= 1.0e9 ? (int32_t)in[3] : -1;
  d.n_tau = in[4] >= -1.0e9 && in[4] <= 1.0e9 ? (int32_t)in[4] : -1;
  const bool sized = d.n_rho >= 1 && d.n_rho <= 4096 && d.n_tau >= 1 && d.n_tau <= 4096;
  const size_t nodes = sized ? (size_t)d.n_rho * (size_t)d.n_tau : 0;
  size_t at = 8;
  const double** tables[3] = {&d.radial, &d.azimuthal, &d.time};
  for (int k = 0; k < 3; ++k) {
    if (in[5 + k] == 0.0 || !sized) continue;
    if (at + nodes > in.size()) return 3;
    *tables[k] = in.data() + at;
    at += nodes;
  }
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    const bool refused = attpc::distort_desc_error(d) != nullptr;
    out.push_back(refused ? 1.0 : 0.0);
    out.push_back(!refused && attpc::distort_desc_is_off(d) ? 1.0 : 0.0);
  } else if (!std::strcmp(argv[1], "shift")) {
    if (attpc::distort_desc_error(d) || (in.size() - at) % 4) return 3;
    const attpc::DistortMap m{d.rho_step, d.tau_step, d.tb_origin, d.n_rho, d.n_tau, d.radial, d.azimuthal, d.time};
    out.assign(in.begin() + (long)at, in.end());
    for (size_t i = 0; i < out.size(); i += 4) attpc::distort_record(m, out[i], out[i + 1], out[i + 2]);
  } else {
    return 2;
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
