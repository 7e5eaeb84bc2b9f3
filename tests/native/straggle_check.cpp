// straggle_check.cpp -- csrc/straggle_host.hpp compiled alone for the host (tests/test_straggling_cpu.py):
//   straggle_check kick in.bin out.bin   records of 13 doubles (g[3], mass, z, ds, n1, n2, n3, angular_scale,
//                                         energy_scale, radiation_length, electron_density) -> 4 doubles (g'[3], clamped)
//   straggle_check step in.bin out.bin   records of 2 doubles (gv2, h_sample) -> 1 double (ds)
//   straggle_check desc in.bin out.bin   records of 5 doubles (the four of the desc, stream) -> 1 double (1 = refused)
#include <cstdio>
#include <cstring>
#include <vector>

#include "straggle_host.hpp"

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
  std::vector<double> out;
  if (!std::strcmp(argv[1], "kick")) {
    if (in.size() % 13) return 3;
    for (size_t i = 0; i < in.size(); i += 13) {
      const double* r = in.data() + i;
      double g[3] = {r[0], r[1], r[2]};
      const attpc::StraggleParams p{r[9], r[10], r[11], r[12]};
      const bool clamped = attpc::straggle_kick(g, r[3], r[4], r[5], r[6], r[7], r[8], p);
      out.insert(out.end(), {g[0], g[1], g[2], clamped ? 1.0 : 0.0});
    }
  } else if (!std::strcmp(argv[1], "step")) {
    if (in.size() % 2) return 3;
    for (size_t i = 0; i < in.size(); i += 2) out.push_back(attpc::straggle_step_length(in[i], in[i + 1]));
  } else if (!std::strcmp(argv[1], "desc")) {
    if (in.size() % 5) return 3;
    for (size_t i = 0; i < in.size(); i += 5) {
      attpc_straggle_desc d{in[i], in[i + 1], in[i + 2], in[i + 3], (uint32_t)in[i + 4]};
      out.push_back(attpc::straggle_desc_error(d) ? 1.0 : 0.0);
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
