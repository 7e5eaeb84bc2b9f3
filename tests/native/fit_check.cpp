// The host-side parts of the track fit (attpc_engine_amd/csrc/fit_host.hpp) alone, for tests/test_fit_cpu.py to compare
// with tests/fit_reference.py:
//   fit_check desc IN OUT    IN: attpc_fit_desc records                                   OUT: one byte each, 1 = refused
//   fit_check dedx IN OUT    IN: a table of ATTPC_DEDX_NODES f64, then energies (f64)     OUT: the table read there, f64
//   fit_check fit IN OUT     IN: cases {FitCase, the table, n x {x, y, z} f64 in metres}  OUT: attpc_track_fit per case
// A case's sums have the lanes' order of summation (fit_evaluate_lanes).  Compile with -ffp-contract=off (the header's
// pragma is clang's).  The program is also what runs under the address and undefined-behaviour sanitizers: everything
// it touches is host code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fit_host.hpp"

namespace {
struct FitCase {
  double mass, bfield, efield, density, length;
  attpc_fit_desc desc;
  attpc_track_estimate estimate;
  double start[6];
  int32_t Z;           // 0: the position has no species
  int32_t use_start;
  int32_t n;           // points that follow
  int32_t capped;
};
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(attpc_fit_desc) == 32 && sizeof(attpc_track_fit) == 128 && sizeof(FitCase) == 264, "layout");
  if (argc != 4) return 2;
  std::FILE* in = std::fopen(argv[2], "rb");
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  if (!std::strcmp(argv[1], "desc")) {
    attpc_fit_desc d;
    while (std::fread(&d, sizeof d, 1, in) == 1) {
      const uint8_t bad = attpc::fit_desc_error(d) != nullptr;
      if (std::fwrite(&bad, 1, 1, out) != 1) return 2;
    }
  } else if (!std::strcmp(argv[1], "dedx")) {
    std::vector<double> table(ATTPC_DEDX_NODES);
    if (std::fread(table.data(), sizeof(double), table.size(), in) != table.size()) return 2;
    double ke;
    while (std::fread(&ke, sizeof ke, 1, in) == 1) {
      const double v = attpc::fit_dedx(table.data(), ke);
      if (std::fwrite(&v, sizeof v, 1, out) != 1) return 2;
    }
  } else if (!std::strcmp(argv[1], "fit")) {
    FitCase c;
    std::vector<double> table(ATTPC_DEDX_NODES), pts, res;
    while (std::fread(&c, sizeof c, 1, in) == 1) {
      if (c.n < 0 || c.n > ATTPC_FIT_MAX_POINTS || attpc::fit_desc_error(c.desc)) return 2;
      if (std::fread(table.data(), sizeof(double), table.size(), in) != table.size()) return 2;
      pts.assign((size_t)c.n * 3, 0.0);
      res.assign((size_t)c.n * 3 * 7, 0.0);
      if (c.n && std::fread(pts.data(), sizeof(double), pts.size(), in) != pts.size()) return 2;
      const attpc::FitSpecies sp = attpc::fit_species(c.mass, c.Z, c.bfield, c.efield, c.density);
      attpc_track_fit rec;
      double q[6];
      const int32_t no_fit = attpc::fit_begin(c.estimate, c.Z > 0, sp, c.use_start ? c.start : nullptr, q);
      if (no_fit) {
        attpc::fit_no_fit(no_fit, c.estimate.n_used < ATTPC_FIT_MAX_POINTS ? c.estimate.n_used : ATTPC_FIT_MAX_POINTS, &rec);
      } else {
        attpc::fit_iterate(q, sp, c.desc, c.n, c.capped ? ATTPC_FIT_CAPPED : 0,
                           [&](const double* at, const double* delta) {
                             return attpc::fit_evaluate_lanes(at, delta, sp, table.data(), pts.data(), c.n, c.desc, c.length,
                                                              res.data());
                           },
                           &rec);
      }
      if (std::fwrite(&rec, sizeof rec, 1, out) != 1) return 2;
    }
  } else {
    return 2;
  }
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}
