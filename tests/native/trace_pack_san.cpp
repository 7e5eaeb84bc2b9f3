// Driver for the sanitizer builds of the host-only packed-trace code (attpc_engine_amd/csrc/trace_pack_host.cpp):
// encodes synthetic rows into exactly-sized heap arrays, decodes them with 1 ... 16 threads into exactly-sized heap
// arrays (so that AddressSanitizer sees any access past a record, a span or a slice) and checks every sample; then
// hands the decoder every kind of malformed record, which it must refuse without touching anything outside what it
// was given.  Built and run by tests/test_trace_pack_sanitizers.py under -fsanitize=address,undefined and
// -fsanitize=thread; CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trace_pack_host.hpp"

using namespace attpc;

static unsigned long long lcg(unsigned long long& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 11;
}

static long long mismatches = 0, not_refused = 0;

// decode exactly-sized copies of (bytes, row_start) and expect `want` (0 ok, 1 refused)
static void expect(const std::vector<uint8_t>& bytes, long long n_bytes, const std::vector<int64_t>& row_start, int threads,
                   int want, const char* what) {
  const long long n_rows = (long long)row_start.size() - 1;
  const size_t keep = (size_t)n_bytes < bytes.size() ? (size_t)n_bytes : bytes.size();
  uint8_t* b = (uint8_t*)malloc(keep ? keep : 1);  // exactly n_bytes: a read past them is caught
  memcpy(b, bytes.data(), keep);
  int16_t* out = (int16_t*)malloc((size_t)n_rows * TP_SAMPLES * sizeof(int16_t) + 1);
  const int32_t rc = trace_unpack_host(b, n_bytes, row_start.data(), n_rows, out, threads);
  if (rc != want) {
    ++not_refused;
    printf("%s: status %d, expected %d\n", what, (int)rc, want);
  }
  free(out);
  free(b);
}

int main(int argc, char** argv) {
  const long long n = argc > 1 ? atoll(argv[1]) : 40000;  // > 4 x 4096: the thread pool really starts
  unsigned long long seed = 2024;
  std::vector<int16_t> rows((size_t)n * TP_SAMPLES);
  for (long long r = 0; r < n; ++r) {
    const int kind = (int)(lcg(seed) % 8);
    const int pedestal = kind == 0 ? 0 : kind == 1 ? 4095 : (int)(lcg(seed) % 600);
    for (int j = 0; j < TP_SAMPLES; ++j) {
      int v = pedestal + (kind > 2 ? (int)(lcg(seed) % 11) - 5 : 0);
      if (kind == 7 && j % 2) v = 4095;  // full-width blocks
      rows[(size_t)r * TP_SAMPLES + j] = (int16_t)(v < 0 ? 0 : v > 4095 ? 4095 : v);
    }
    if (kind >= 4) {  // a pulse, some of them saturating
      const int t0 = (int)(lcg(seed) % TP_SAMPLES), amp = (int)(lcg(seed) % 6000);
      for (int j = t0; j < TP_SAMPLES && j < t0 + 40; ++j) {
        const int v = rows[(size_t)r * TP_SAMPLES + j] + amp * (40 - (j - t0)) / 40;
        rows[(size_t)r * TP_SAMPLES + j] = (int16_t)(v > 4095 ? 4095 : v);
      }
    }
  }
  // sizes first, then the records into exactly that many bytes
  std::vector<int64_t> row_start((size_t)n + 1);
  int64_t n_bytes = 0;
  if (trace_pack_host(n, rows.data(), row_start.data(), nullptr, 0, &n_bytes) != 0) return 2;
  uint8_t* bytes = (uint8_t*)malloc((size_t)n_bytes + 1);
  int64_t again = 0;
  if (trace_pack_host(n, rows.data(), row_start.data(), bytes, n_bytes, &again) != 0 || again != n_bytes) return 3;
  if (n > 1 && trace_pack_host(n, rows.data(), row_start.data(), bytes, n_bytes - 8, &again) != 4) return 4;  // capacity
  for (int threads : {1, 2, 3, 7, 16}) {
    int16_t* out = (int16_t*)malloc((size_t)n * TP_SAMPLES * sizeof(int16_t));
    memset(out, 0xff, (size_t)n * TP_SAMPLES * sizeof(int16_t));
    if (trace_unpack_host(bytes, n_bytes, row_start.data(), n, out, threads) != 0) ++mismatches;
    for (size_t i = 0; i < (size_t)n * TP_SAMPLES; ++i) mismatches += out[i] != rows[i];
    free(out);
  }
  // a run of rows in the middle decodes alone
  if (n > 100) {
    int16_t* out = (int16_t*)malloc((size_t)50 * TP_SAMPLES * sizeof(int16_t));
    if (trace_unpack_host(bytes, n_bytes, row_start.data() + 30, 50, out, 2) != 0) ++mismatches;
    for (size_t i = 0; i < (size_t)50 * TP_SAMPLES; ++i) mismatches += out[i] != rows[(size_t)30 * TP_SAMPLES + i];
    free(out);
  }

  // malformed records: six rows, one defect each
  const long long m = n < 6 ? n : 6;
  std::vector<uint8_t> good(bytes, bytes + row_start[m]);
  std::vector<int64_t> start(row_start.begin(), row_start.begin() + m + 1);
  for (int threads : {1, 4}) {
    expect(good, (long long)good.size(), start, threads, 0, "well-formed");
    if (m < 6) break;
    std::vector<int64_t> s = start;
    s[3] += 8;
    expect(good, (long long)good.size(), s, threads, 1, "span larger than the headers imply");
    s = start;
    s[3] -= 8;
    expect(good, (long long)good.size(), s, threads, 1, "span smaller than the headers imply");
    std::vector<uint8_t> b = good;
    b[(size_t)start[2] + 1] = (uint8_t)((13 << 4) | (b[(size_t)start[2] + 1] & 0x0f));
    expect(b, (long long)b.size(), start, threads, 1, "width 13");
    b = good;
    b[(size_t)start[4] + 3] = (uint8_t)(15 << 4);  // width 15 claims 120 bytes of planes more than the span has
    expect(b, (long long)b.size(), start, threads, 1, "width 15");
    s = start;
    std::swap(s[2], s[3]);
    expect(good, (long long)good.size(), s, threads, 1, "offsets decrease");
    s = start;
    for (int64_t& v : s) v += 4;
    b.assign(good.size() + 4, 0);
    memcpy(b.data() + 4, good.data(), good.size());
    expect(b, (long long)b.size(), s, threads, 1, "offsets no multiples of 8");
    s = start;
    s[0] = -8;
    expect(good, (long long)good.size(), s, threads, 1, "negative offset");
    expect(good, (long long)good.size() - 8, start, threads, 1, "span past n_bytes");
    s = start;
    s[m] += 784;
    expect(good, (long long)good.size(), s, threads, 1, "last offset past n_bytes");
    s = {0, 8};
    expect(std::vector<uint8_t>(8, 0), 8, s, threads, 1, "span shorter than the headers");
    // base + 2^w - 1 > 4095 with a span that matches: 16 + 8 * 3 bytes, block 0 = 4090 | 3 << 12
    b.assign(40, 0);
    b[0] = (uint8_t)(4090 & 0xff);
    b[1] = (uint8_t)((4090 >> 8) | (3 << 4));
    s = {0, 40};
    expect(b, 40, s, threads, 1, "base + 2^w - 1 above 4095");
  }
  free(bytes);
  printf("rows %lld bytes %lld mismatches %lld unexpected %lld\n", n, (long long)n_bytes, mismatches, not_refused);
  return mismatches || not_refused ? 1 : 0;
}
