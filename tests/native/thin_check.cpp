// The host-side parts of the thinned track points (attpc_engine_amd/csrc/thin_host.hpp) alone, for
// tests/test_thin_cpu.py to compare with tests/thin_reference.py:
//   thin_check desc IN OUT       IN: attpc_thin_desc records   OUT: {refused (i32), H (i32; 0 if refused)}
//   thin_check bins IN OUT       IN: {Z, H} i32                OUT: bin (i32)
//   thin_check centroid IN OUT   IN: {S, W} i64                OUT: C(S) (i64)
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "thin_host.hpp"

namespace {
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
  static_assert(sizeof(attpc_thin_desc) == 16 && sizeof(attpc_thin_info) == 16, "layout");
  if (argc != 4) return 2;
  const char* mode = argv[1];
  if (!std::strcmp(mode, "desc"))
    return convert<attpc_thin_desc, int32_t[2]>(argv[2], argv[3], [](const attpc_thin_desc& d, int32_t (*r)[2]) {
      (*r)[0] = attpc::thin_desc_error(d) != nullptr;
      (*r)[1] = (*r)[0] ? 0 : attpc::thin_step_units(d.z_step);
    });
  if (!std::strcmp(mode, "bins"))
    return convert<int32_t[2], int32_t>(argv[2], argv[3], [](const int32_t (&p)[2], int32_t* bin) {
      *bin = attpc::thin_bin(p[0], p[1]);
    });
  if (!std::strcmp(mode, "centroid"))
    return convert<int64_t[2], int64_t>(argv[2], argv[3], [](const int64_t (&p)[2], int64_t* c) {
      *c = attpc::thin_centroid(p[0], p[1]);
    });
  return 2;
}
