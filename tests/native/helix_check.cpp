// The host-side parts of the helix slope (attpc_engine_amd/csrc/helix_host.hpp) alone, for tests/test_helix_cpu.py to
// compare with tests/helix_reference.py:
//   helix_check desc IN OUT     IN: attpc_helix_desc records                        OUT: one byte each, 1 = refused
//   helix_check atan2 IN OUT    IN: {y, x} f64 pairs                                OUT: atan2w(y, x), f64
//   helix_check phi IN OUT      IN: cases {PhiCase, m x {u, v, w} i32}              OUT: m x {phi_q, PHI} i32 per case
//   helix_check record IN OUT   IN: cases {RecordCase, m x {u, v, w} i32}           OUT: RecordOut: the four sums, the
//                                                                                   NO_HELIX flag of steps 1 to 3, the record
// Compile with -ffp-contract=off (the header's pragma is clang's).  The program is also what runs under the address and
// undefined-behaviour sanitizers: everything it touches is host code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "helix_host.hpp"

namespace {
struct Pair {
  double y, x;
};
struct PhiCase {
  double a, b;
  int32_t m, pad;
};
struct RecordCase {
  attpc::EstimateSums sums;  // sums.m points follow
  double field, tolerance;
  int32_t max_evaluations;   // 0: the Kasa circle, else the geometric circle fit with these settings
  int32_t regressor;
};
struct RecordOut {
  int64_t sp, spp, spw, sww;
  int32_t no_helix, pad;
  attpc_track_estimate record;
};

// the m points behind a case's head into u, v and w; false if they are not there
bool read_points(std::FILE* in, int64_t m, std::vector<int32_t>* u, std::vector<int32_t>* v, std::vector<int32_t>* w) {
  if (m < 0 || m > ATTPC_EST_MAX_FIT) return false;
  u->assign((size_t)m, 0);
  v->assign((size_t)m, 0);
  w->assign((size_t)m, 0);
  for (int64_t i = 0; i < m; ++i) {
    int32_t uvw[3];
    if (std::fread(uvw, sizeof uvw, 1, in) != 1) return false;
    (*u)[(size_t)i] = uvw[0];
    (*v)[(size_t)i] = uvw[1];
    (*w)[(size_t)i] = uvw[2];
  }
  return true;
}

template <typename In, typename F>
int convert(const char* in_path, const char* out_path, F f) {
  std::FILE* in = std::fopen(in_path, "rb");
  std::FILE* out = std::fopen(out_path, "wb");
  if (!in || !out) return 2;
  In rec;
  while (std::fread(&rec, sizeof rec, 1, in) == 1)
    if (!f(in, rec, out)) return 2;
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(attpc_helix_desc) == 8 && sizeof(Pair) == 16 && sizeof(PhiCase) == 24 && sizeof(RecordCase) == 176 &&
                    sizeof(RecordOut) == 168 && sizeof(attpc_track_estimate) == 128, "layout");
  if (argc != 4) return 2;
  const char* mode = argv[1];
  std::vector<int32_t> u, v, w;
  if (!std::strcmp(mode, "desc"))
    return convert<attpc_helix_desc>(argv[2], argv[3], [](std::FILE*, const attpc_helix_desc& d, std::FILE* out) {
      const uint8_t bad = attpc::helix_desc_error(d) != nullptr;
      return std::fwrite(&bad, 1, 1, out) == 1;
    });
  if (!std::strcmp(mode, "atan2"))
    return convert<Pair>(argv[2], argv[3], [](std::FILE*, const Pair& p, std::FILE* out) {
      const double at = attpc::helix_atan2w(p.y, p.x);
      return std::fwrite(&at, sizeof at, 1, out) == 1;
    });
  if (!std::strcmp(mode, "phi"))
    return convert<PhiCase>(argv[2], argv[3], [&](std::FILE* in, const PhiCase& c, std::FILE* out) {
      if (!read_points(in, c.m, &u, &v, &w)) return false;
      std::vector<int32_t> phi((size_t)c.m), unwrapped((size_t)c.m);
      attpc::helix_sums_host(u.data(), v.data(), w.data(), c.m, c.a, c.b, phi.data(), unwrapped.data());
      for (int32_t i = 0; i < c.m; ++i) {
        const int32_t both[2] = {phi[(size_t)i], unwrapped[(size_t)i]};
        if (std::fwrite(both, sizeof both, 1, out) != 1) return false;
      }
      return true;
    });
  if (!std::strcmp(mode, "record"))
    return convert<RecordCase>(argv[2], argv[3], [&](std::FILE* in, const RecordCase& c, std::FILE* out) {
      if (!read_points(in, c.sums.m, &u, &v, &w)) return false;
      const int32_t m = (int32_t)c.sums.m;
      RecordOut o;
      std::memset(&o, 0, sizeof o);
      o.record.n_fit = m;
      double a = 0.0, b = 0.0, R = 0.0;
      const bool circle = attpc::helix_step6(c.sums, c.field, c.max_evaluations != 0, c.tolerance, c.max_evaluations,
                                             [&](double ta, double tb, double tr) {
                                               return attpc::circle_evaluate_lanes(u.data(), v.data(), m, ta, tb, tr);
                                             },
                                             &o.record, &a, &b, &R);
      if (!circle) {
        o.record.status |= ATTPC_EST_NO_HELIX;
      } else {
        const attpc::HelixSums h = attpc::helix_sums_host(u.data(), v.data(), w.data(), m, a, b);
        o.sp = h.sp;
        o.spp = h.spp;
        o.spw = h.spw;
        o.sww = h.sww;
        o.no_helix = h.no_helix ? 1 : 0;
        attpc::helix_closed_form(c.sums, h, c.regressor, c.field, a, b, R, &o.record);
      }
      return std::fwrite(&o, sizeof o, 1, out) == 1;
    });
  return 2;
}
