// reaction_check.cpp -- csrc/reaction_host.hpp compiled alone for the host (tests/test_reaction_cpu.py).  The input file
// is doubles: the 20 scalar fields of the desc in the order of the struct (masses[4], beam_energy, z_min, z_max, ex_lo,
// ex_hi, ex_inv_width, theta_inv_width, eloss_len, has_target, charge, track, observed_row, source, n_ex, n_theta,
// reserved), the table, and then
//   reaction_check desc in.bin out.bin    -> 1 double: 1 = the desc is refused
//   reaction_check bins in.bin out.bin    n, lo, hi, inv_width, count, the values -> the bin of every value
//   reaction_check records in.bin out.bin n_sim, n_rows, n_events, with_pid; per event: per slot (status, a, b, c, d) --
//       a fit record's g[0 .. 2] and vertex z in mm, or an estimate record's brho, slope, vz and one unused --, per slot
//       the pid position if with_pid, the p4 rows, the vertex, the kinematics status
//       -> per event status, slot and the six values, then the cells
#include <cstdio>
#include <cstring>
#include <vector>

#include "reaction_host.hpp"

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
  constexpr size_t HEAD = 20;
  if (in.size() < HEAD) return 3;
  attpc_reaction_desc d{};
  for (int i = 0; i < 4; ++i) d.masses[i] = in[i];
  d.beam_energy = in[4];
  d.z_min = in[5];
  d.z_max = in[6];
  d.ex_lo = in[7];
  d.ex_hi = in[8];
  d.ex_inv_width = in[9];
  d.theta_inv_width = in[10];
  d.eloss_len = as_int(in[11]);
  d.has_target = as_int(in[12]);
  d.charge = as_int(in[13]);
  d.track = as_int(in[14]);
  d.observed_row = as_int(in[15]);
  d.source = as_int(in[16]);
  d.n_ex = as_int(in[17]);
  d.n_theta = as_int(in[18]);
  d.reserved = as_int(in[19]);
  const size_t table = d.eloss_len > 0 && d.eloss_len <= ATTPC_REACTION_MAX_ELOSS ? (size_t)d.eloss_len : 0;
  if (in.size() < HEAD + table) return 3;
  const std::vector<double> eloss(in.begin() + HEAD, in.begin() + HEAD + table);  // (a copy: its end is the table's end)
  d.eloss = table ? eloss.data() : nullptr;
  const double* rest = in.data() + HEAD + table;
  const size_t n_rest = in.size() - HEAD - table;
  std::vector<double> out;
  if (!std::strcmp(argv[1], "desc")) {
    out.push_back(attpc::reaction_desc_error(d) != nullptr ? 1.0 : 0.0);
  } else if (!std::strcmp(argv[1], "bins")) {
    if (n_rest < 5 || n_rest != 5 + (size_t)rest[4]) return 3;
    for (size_t i = 0; i < (size_t)rest[4]; ++i)
      out.push_back((double)attpc::reaction_bin(rest[5 + i], rest[1], rest[2], rest[3], as_int(rest[0])));
  } else if (!std::strcmp(argv[1], "records")) {
    if (attpc::reaction_desc_error(d) || n_rest < 4) return 3;
    const int32_t n_sim = as_int(rest[0]), n_rows = as_int(rest[1]);
    const size_t n_events = (size_t)rest[2];
    const bool with_pid = rest[3] != 0.0;
    if (n_sim < 1 || n_sim > ATTPC_MAX_SIM || n_rows < 4 || n_rows > ATTPC_MAX_ROWS) return 3;
    const size_t per = (size_t)n_sim * (with_pid ? 6 : 5) + (size_t)n_rows * 4 + 4;
    if (n_rest - 4 != n_events * per) return 3;
    std::vector<attpc_track_fit> fits(n_events * n_sim);
    std::vector<attpc_track_estimate> est(n_events * n_sim);
    std::vector<attpc_pid_record> pid(n_events * n_sim);
    std::vector<double> p4(n_events * n_rows * 4), vertex(n_events * 3);
    std::vector<int32_t> kin(n_events);
    for (size_t e = 0; e < n_events; ++e) {
      const double* w = rest + 4 + e * per;
      for (int32_t k = 0; k < n_sim; ++k, w += 5) {
        attpc_track_fit& f = fits[e * n_sim + k];
        attpc_track_estimate& t = est[e * n_sim + k];
        f = attpc_track_fit{};
        t = attpc_track_estimate{};
        f.status = t.status = as_int(w[0]);
        f.g[0] = w[1];
        f.g[1] = w[2];
        f.g[2] = w[3];
        f.vertex[2] = w[4];
        t.brho = w[1];
        t.slope = w[2];
        t.vz = w[3];
      }
      for (int32_t k = 0; k < n_sim && with_pid; ++k, ++w) pid[e * n_sim + k] = attpc_pid_record{as_int(*w), -1, 0, 0};
      std::memcpy(&p4[e * n_rows * 4], w, (size_t)n_rows * 4 * sizeof(double));
      w += (size_t)n_rows * 4;
      std::memcpy(&vertex[e * 3], w, 3 * sizeof(double));
      kin[e] = as_int(w[3]);
    }
    std::vector<attpc_reaction_record> rec(n_events + 1);
    std::vector<uint64_t> cells((size_t)attpc::reaction_cells(d.n_ex, d.n_theta), 0);
    const bool from_fit = d.source == ATTPC_REACTION_FROM_FIT;
    attpc::reaction_records_host(d, (int64_t)n_events, n_sim, n_rows, from_fit ? fits.data() : nullptr,
                                 from_fit ? nullptr : est.data(), with_pid ? pid.data() : nullptr, p4.data(), vertex.data(),
                                 kin.data(), rec.data(), cells.data());
    for (size_t e = 0; e < n_events; ++e) {
      const attpc_reaction_record& r = rec[e];
      const double row[8] = {(double)r.status, (double)r.slot, r.beam_ke, r.ex, r.theta_cm, r.truth_beam_ke, r.truth_ex,
                             r.truth_theta_cm};
      out.insert(out.end(), row, row + 8);
      if (r.reserved != 0.0) return 5;
    }
    for (uint64_t c : cells) out.push_back((double)c);
  } else {
    return 2;
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 4;
  const size_t written = out.empty() ? 0 : std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return written == out.size() ? 0 : 4;
}
