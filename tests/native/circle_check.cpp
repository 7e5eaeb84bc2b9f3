// The host-side parts of the geometric circle fit (attpc_engine_amd/csrc/circle_host.hpp) alone, for
// tests/test_circle_cpu.py to compare with tests/circle_reference.py:
//   circle_check desc IN OUT     IN: attpc_circle_desc records                      OUT: one byte each, 1 = refused
//   circle_check eval IN OUT     IN: cases {Case, m x {u, v} i32}                   OUT: the nine sums at (a, b, R), f64
//   circle_check fit IN OUT      IN: the same cases, (a, b, R) the start            OUT: FitOut
//   circle_check record IN OUT   IN: cases {RecordCase, m x {u, v} i32}             OUT: attpc_track_estimate records
//   circle_check halves IN OUT   IN: RecordCase records (no points)                 OUT: two records each: step 6 in one
//                                                                                   piece, and as Kasa + from-circle
// Compile with -ffp-contract=off (the header's pragma is clang's).  The program is also what runs under the address and
// undefined-behaviour sanitizers: everything it touches is host code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "circle_host.hpp"

namespace {
struct Case {
  double a, b, R, tolerance;
  int32_t max_evaluations, m;
};
struct FitOut {
  double a, b, R;
  int32_t evaluations, converged;
};
struct RecordCase {
  attpc::EstimateSums sums;  // sums.m points follow
  double field, tolerance;
  int32_t max_evaluations, pad;
};

// the m points behind a case's head into u and v; false if they are not there
bool read_points(std::FILE* in, int64_t m, std::vector<int32_t>* u, std::vector<int32_t>* v) {
  if (m < 0 || m > ATTPC_EST_MAX_FIT) return false;
  u->assign((size_t)m, 0);
  v->assign((size_t)m, 0);
  for (int64_t i = 0; i < m; ++i) {
    int32_t uv[2];
    if (std::fread(uv, sizeof uv, 1, in) != 1) return false;
    (*u)[(size_t)i] = uv[0];
    (*v)[(size_t)i] = uv[1];
  }
  return true;
}

template <typename In, typename Out, typename F>
int convert(const char* in_path, const char* out_path, F f) {
  std::FILE* in = std::fopen(in_path, "rb");
  std::FILE* out = std::fopen(out_path, "wb");
  if (!in || !out) return 2;
  In rec;
  while (std::fread(&rec, sizeof rec, 1, in) == 1) {
    Out res;
    std::memset(&res, 0, sizeof res);
    if (!f(in, rec, &res)) return 2;
    if (std::fwrite(&res, sizeof res, 1, out) != 1) return 2;
  }
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(attpc_circle_desc) == 16 && sizeof(Case) == 40 && sizeof(FitOut) == 32 && sizeof(RecordCase) == 176 &&
                    sizeof(attpc::CircleSums) == 72 && sizeof(attpc_track_estimate) == 128, "layout");
  if (argc != 4) return 2;
  const char* mode = argv[1];
  std::vector<int32_t> u, v;
  if (!std::strcmp(mode, "desc"))
    return convert<attpc_circle_desc, uint8_t>(argv[2], argv[3], [](std::FILE*, const attpc_circle_desc& d, uint8_t* bad) {
      *bad = attpc::circle_desc_error(d) != nullptr;
      return true;
    });
  if (!std::strcmp(mode, "eval"))
    return convert<Case, attpc::CircleSums>(argv[2], argv[3], [&](std::FILE* in, const Case& c, attpc::CircleSums* k) {
      if (!read_points(in, c.m, &u, &v)) return false;
      *k = attpc::circle_evaluate_lanes(u.data(), v.data(), c.m, c.a, c.b, c.R);
      return true;
    });
  if (!std::strcmp(mode, "fit"))
    return convert<Case, FitOut>(argv[2], argv[3], [&](std::FILE* in, const Case& c, FitOut* o) {
      if (!read_points(in, c.m, &u, &v)) return false;
      const attpc::CircleFit fit = attpc::circle_refine(c.m, c.a, c.b, c.R, c.tolerance, c.max_evaluations, [&](double a, double b, double R) {
        return attpc::circle_evaluate_lanes(u.data(), v.data(), c.m, a, b, R);
      });
      *o = FitOut{fit.a, fit.b, fit.R, fit.evaluations, fit.converged ? 1 : 0};
      return true;
    });
  if (!std::strcmp(mode, "record"))
    return convert<RecordCase, attpc_track_estimate>(argv[2], argv[3], [&](std::FILE* in, const RecordCase& c, attpc_track_estimate* r) {
      if (!read_points(in, c.sums.m, &u, &v)) return false;
      const int32_t m = (int32_t)c.sums.m;
      r->n_fit = m;
      attpc::estimate_closed_form_circle(c.sums, c.field, c.tolerance, c.max_evaluations, [&](double a, double b, double R) {
        return attpc::circle_evaluate_lanes(u.data(), v.data(), m, a, b, R);
      }, r);
      return true;
    });
  if (!std::strcmp(mode, "halves")) {
    struct Two {
      attpc_track_estimate whole, halves;
    };
    return convert<RecordCase, Two>(argv[2], argv[3], [](std::FILE*, const RecordCase& c, Two* r) {
      attpc::estimate_closed_form(c.sums, c.field, &r->whole);
      double a = 0.0, b = 0.0, r2 = 0.0;
      const bool circle = attpc::estimate_kasa(c.sums, &a, &b, &r2);
      attpc::estimate_from_circle(c.sums, c.field, circle, a, b, circle ? sqrt(r2) : 0.0, &r->halves);
      return true;
    });
  }
  return 2;
}
