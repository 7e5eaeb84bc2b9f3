// hypothesis_check.cpp -- csrc/hypothesis_host.hpp compiled alone for the host (tests/test_hypothesis_cpu.py).  The
// input file is doubles: candidates, reserved, has_pid, n_sim, n_events, the eight species of the positions; then per
// (event, slot) held and n_used; then per (event, slot, hypothesis) status, f and ke of the fit record (H is what the
// layout gives; ke is a tag that says which record was copied).
//   hypothesis_check records in.bin out.bin -> per (event, slot) position, species, tried, fitted, status, reserved,
//                                              f[8], f_next, and status, n_points, f, ke of the chosen fit record
//   hypothesis_check desc in.bin out.bin    -> 1 double: 1 = the desc is refused
//   hypothesis_check layout in.bin out.bin  -> H, candidates, first[8], positions[8], of_position[8]
#include <cstdio>
#include <cstring>
#include <vector>

#include "hypothesis_host.hpp"

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
  constexpr size_t HEAD = 5 + ATTPC_MAX_SIM;
  if (in.size() < HEAD) return 3;
  attpc_hypothesis_desc d{as_int(in[0]), as_int(in[1])};
  const bool has_pid = in[2] != 0.0;
  const int32_t n_sim = as_int(in[3]);
  const size_t n_events = (size_t)in[4];
  int32_t species[ATTPC_MAX_SIM];
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) species[p] = as_int(in[5 + p]);
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    out.push_back(attpc::hypothesis_desc_error(d) != nullptr ? 1.0 : 0.0);
  } else {
    if (attpc::hypothesis_desc_error(d) || n_sim < 0 || n_sim > ATTPC_MAX_SIM) return 3;
    const attpc::HypLayout l = attpc::hypothesis_layout(species, n_sim, d.candidates);
    if (!std::strcmp(argv[1], "layout")) {
      out.push_back((double)l.n);
      out.push_back((double)l.candidates);
      for (int p = 0; p < ATTPC_MAX_SIM; ++p) out.push_back((double)l.first[p]);
      for (int p = 0; p < ATTPC_MAX_SIM; ++p) out.push_back((double)l.positions[p]);
      for (int p = 0; p < ATTPC_MAX_SIM; ++p) out.push_back((double)l.of_position[p]);
    } else if (!std::strcmp(argv[1], "records")) {
      const size_t slots = n_events * (size_t)n_sim, pairs = slots * (size_t)l.n;
      if (in.size() != HEAD + 2 * slots + 3 * pairs) return 3;
      std::vector<attpc_pid_record> pid(slots + 1);
      std::vector<attpc_track_estimate> est(slots + 1);
      std::vector<attpc_track_fit> all(pairs + 1), fits(slots + 1);
      std::vector<attpc_fit_hypothesis> records(slots + 1);
      for (size_t i = 0; i < slots; ++i) {
        pid[i] = attpc_pid_record{-1, -1, as_int(in[HEAD + 2 * i]), 0};
        est[i] = attpc_track_estimate{};
        est[i].n_used = as_int(in[HEAD + 2 * i + 1]);
      }
      for (size_t i = 0; i < pairs; ++i) {
        const double* v = in.data() + HEAD + 2 * slots + 3 * i;
        attpc::fit_no_fit(as_int(v[0]), 7, &all[i]);
        all[i].f = v[1];
        all[i].ke = v[2];
      }
      attpc::hypothesis_records_host(l, (int64_t)n_events, n_sim, all.data(), has_pid ? pid.data() : nullptr, est.data(),
                                     records.data(), fits.data());
      for (size_t i = 0; i < slots; ++i) {
        const attpc_fit_hypothesis& r = records[i];
        for (int32_t v : {r.position, r.species, r.tried, r.fitted, r.status, r.reserved}) out.push_back((double)v);
        for (int p = 0; p < ATTPC_MAX_SIM; ++p) out.push_back(r.f[p]);
        out.push_back(r.f_next);
        out.push_back((double)fits[i].status);
        out.push_back((double)fits[i].n_points);
        out.push_back(fits[i].f);
        out.push_back(fits[i].ke);
      }
    } else {
      return 2;
    }
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = out.empty() ? 0 : std::fwrite(out.data(), sizeof(double), out.size(), f);  // (no events: an empty file)
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
