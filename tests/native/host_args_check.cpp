// The checks and the chunk walk of the operators on host arrays (attpc_engine_amd/csrc/host_args.hpp) alone, for
// tests/test_host_args_cpu.py.  IN is a sequence of cases in binary, OUT what the header made of each:
//   host_args_check walk ROWS EVENTS IN OUT   IN: {n i64, offsets i64[n + 1]}
//                                             OUT (i64): {chunks, then per chunk e0, e1, start[e1 - e0 + 1]}
//   host_args_check offsets IN OUT            IN: {order i64, n i64, given i64, offsets i64[max(n, 0) + 1] if given}
//   host_args_check samples IN OUT            IN: {r0 i64, r1 i64, rows i64, samples i16[rows][512]}
//                                             OUT of both: a line per case: "ok", "bare" or the text of the refusal
//   host_args_check noise IN OUT              IN: {n_levels i64, cdf u32[max(n_levels - 1, 0)]}
//                                             OUT: {cdf u32[ATTPC_MAX_NOISE_LEVELS], guide u16[256]}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_args.hpp"

namespace {
template <typename T>
bool get(std::FILE* in, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, in) == n;
}

bool get(std::FILE* in, int64_t* v) { return std::fread(v, sizeof *v, 1, in) == 1; }

template <typename T>
void put(std::FILE* out, const std::vector<T>& v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), out) != v.size()) std::exit(2);
}

void put_line(std::FILE* out, const attpc::ArgError& e) {
  std::fprintf(out, "%s\n", !e ? "ok" : e.text.empty() ? "bare" : e.text.c_str());
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const char* mode = argv[1];
  std::FILE* in = std::fopen(argv[argc - 2], "rb");
  std::FILE* out = std::fopen(argv[argc - 1], "wb");
  if (!in || !out) return 2;
  int64_t n = 0;
  std::vector<int64_t> offsets;
  if (!std::strcmp(mode, "walk") && argc == 6) {
    const int64_t max_rows = std::atoll(argv[2]), max_events = std::atoll(argv[3]);
    std::vector<int64_t> start;
    while (get(in, &n)) {
      if (!get(in, &offsets, (size_t)n + 1)) return 2;
      std::vector<int64_t> res{0};
      for (int64_t e0 = 0; e0 < n;) {
        const int64_t e1 = attpc::chunk_end(offsets.data(), n, e0, max_rows, max_events);
        attpc::chunk_starts(offsets.data(), e0, e1, &start);
        ++res[0];
        res.push_back(e0);
        res.push_back(e1);
        res.insert(res.end(), start.begin(), start.end());
        if (e1 <= e0) return 3;  // (no progress: the test would never end)
        e0 = e1;
      }
      put(out, res);
    }
  } else if (!std::strcmp(mode, "offsets") && argc == 4) {
    int64_t order = 0, given = 0;
    while (get(in, &order)) {
      if (!get(in, &n) || !get(in, &given) || !get(in, &offsets, given ? (size_t)(n > 0 ? n : 0) + 1 : 0)) return 2;
      put_line(out, attpc::csr_error("attpc_check", n, given ? offsets.data() : nullptr, order ? attpc::CSR_CLOUD : attpc::CSR_OPERATOR));
    }
  } else if (!std::strcmp(mode, "samples") && argc == 4) {
    int64_t r0 = 0, r1 = 0, rows = 0;
    std::vector<int16_t> samples;
    while (get(in, &r0)) {
      if (!get(in, &r1) || !get(in, &rows) || !get(in, &samples, (size_t)rows * ATTPC_NUM_TB)) return 2;
      put_line(out, attpc::sample_error(samples.data(), r0, r1));
    }
  } else if (!std::strcmp(mode, "noise") && argc == 4) {
    std::vector<uint32_t> cdf;
    while (get(in, &n)) {
      if (!get(in, &cdf, n > 1 ? (size_t)n - 1 : 0)) return 2;
      const attpc::NoiseTable t = attpc::noise_table((int32_t)n, cdf.empty() ? nullptr : cdf.data());
      if (t.cdf.size() != ATTPC_MAX_NOISE_LEVELS || t.guide.size() != 256) return 3;
      put(out, t.cdf);
      put(out, t.guide);
    }
  } else {
    return 2;
  }
  std::fclose(in);
  return std::fclose(out) ? 2 : 0;
}
