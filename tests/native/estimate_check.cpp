// The host-side parts of the track estimates (attpc_engine_amd/csrc/estimate_host.hpp) alone, for
// tests/test_estimate_cpu.py to compare with tests/estimate_reference.py:
//   estimate_check desc IN OUT     IN: attpc_estimate_desc records            OUT: one byte each, 1 = refused
//   estimate_check closed IN OUT   IN: {EstimateSums (19 x i64), f64 field}   OUT: attpc_track_estimate records
//   estimate_check rows IN OUT     IN: {x, y, z, integral} f64                OUT: {ok, X, Y, Z (i32), I (i64)}
//   estimate_check steps IN OUT    IN: {dx, dy} i32                           OUT: d (i32)
// Compile with -ffp-contract=off (the header's pragma is clang's).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "estimate_host.hpp"

namespace {
struct ClosedIn {
  attpc::EstimateSums sums;
  double field;
};
struct RowOut {
  int32_t ok, X, Y, Z;
  int64_t I;
};

template <typename In, typename Out, typename F>
int convert(const char* in_path, const char* out_path, F f) {
  std::FILE* in = std::fopen(in_path, "rb");
  std::FILE* out = std::fopen(out_path, "wb");
  if (!in || !out) return 2;
  In rec;
  while (std::fread(&rec, sizeof rec, 1, in) == 1) {
    Out res;
    std::memset(&res, 0, sizeof res);
    f(rec, &res);
    if (std::fwrite(&res, sizeof res, 1, out) != 1) return 2;
  }
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(attpc_track_estimate) == 128 && sizeof(attpc_estimate_desc) == 24 && sizeof(ClosedIn) == 160, "layout");
  if (argc != 4) return 2;
  const char* mode = argv[1];
  if (!std::strcmp(mode, "desc"))
    return convert<attpc_estimate_desc, uint8_t>(argv[2], argv[3], [](const attpc_estimate_desc& d, uint8_t* bad) {
      *bad = attpc::estimate_desc_error(d) != nullptr;
    });
  if (!std::strcmp(mode, "closed"))
    return convert<ClosedIn, attpc_track_estimate>(argv[2], argv[3], [](const ClosedIn& c, attpc_track_estimate* r) {
      r->n_fit = (int32_t)c.sums.m;
      attpc::estimate_closed_form(c.sums, c.field, r);
    });
  if (!std::strcmp(mode, "rows"))
    return convert<double[4], RowOut>(argv[2], argv[3], [](const double (&p)[4], RowOut* r) {
      r->ok = attpc::estimate_quantise(p[0], p[1], p[2], p[3], &r->X, &r->Y, &r->Z, &r->I);
    });
  if (!std::strcmp(mode, "steps"))
    return convert<int32_t[2], int32_t>(argv[2], argv[3], [](const int32_t (&s)[2], int32_t* d) {
      *d = attpc::estimate_step(s[0], s[1]);
    });
  return 2;
}
