// pid_check.cpp -- csrc/pid_host.hpp compiled alone for the host (tests/test_pid_cpu.py).  The input file is doubles:
// mode, reserved, the eight n_vertices, the 8 x 32 x 2 vertices of the desc, the eight species of the positions; and
// then, for `records`, n_sim, n_events and per (event, slot) brho and dedx.
//   pid_check records in.bin out.bin -> per (event, slot) position, species, held, status
//   pid_check desc in.bin out.bin    -> 1 double: 1 = the desc is refused
#include <cstdio>
#include <cstring>
#include <vector>

#include "pid_host.hpp"

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
  constexpr size_t GATES = (size_t)ATTPC_MAX_SIM * ATTPC_PID_MAX_VERTICES * 2, HEAD = 2 + ATTPC_MAX_SIM + GATES + ATTPC_MAX_SIM;
  if (in.size() < HEAD) return 3;
  attpc_pid_desc d{};
  d.mode = as_int(in[0]);
  d.reserved = as_int(in[1]);
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) d.n_vertices[p] = as_int(in[2 + p]);
  std::memcpy(d.vertices, in.data() + 2 + ATTPC_MAX_SIM, GATES * sizeof(double));
  int32_t species[ATTPC_MAX_SIM];
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) species[p] = as_int(in[2 + ATTPC_MAX_SIM + GATES + p]);
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    out.push_back(attpc::pid_desc_error(d) != nullptr ? 1.0 : 0.0);
  } else if (!std::strcmp(argv[1], "records")) {
    if (attpc::pid_desc_error(d) || in.size() < HEAD + 2) return 3;
    const int32_t n_sim = as_int(in[HEAD]);
    const size_t n_events = (size_t)in[HEAD + 1];
    if (n_sim < 0 || n_sim > ATTPC_MAX_SIM || in.size() - (HEAD + 2) != n_events * (size_t)n_sim * 2) return 3;
    std::vector<attpc_track_estimate> est((size_t)n_sim + 1);
    std::vector<attpc_pid_record> rec((size_t)n_sim + 1);
    for (size_t e = 0; e < n_events; ++e) {
      for (int32_t k = 0; k < n_sim; ++k) {
        est[k] = attpc_track_estimate{};
        est[k].brho = in[HEAD + 2 + (e * n_sim + k) * 2];
        est[k].dedx = in[HEAD + 2 + (e * n_sim + k) * 2 + 1];
      }
      attpc::pid_event_host(d, est.data(), n_sim, species, rec.data());
      for (int32_t k = 0; k < n_sim; ++k) {
        out.push_back((double)rec[k].position);
        out.push_back((double)rec[k].species);
        out.push_back((double)rec[k].held);
        out.push_back((double)rec[k].status);
      }
    }
  } else {
    return 2;
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = out.empty() ? 0 : std::fwrite(out.data(), sizeof(double), out.size(), f);  // (no events: an empty file)
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
