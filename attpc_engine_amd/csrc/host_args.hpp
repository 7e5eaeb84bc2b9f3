// host_args.hpp -- what the operators on host arrays (abi.hip: attpc_trigger_rows, attpc_rows_estimate, attpc_gain_rows,
// attpc_cloud_summary, ...) share and that needs no device: the checks of CSR offsets, 12-bit samples and host-cloud
// rows, the walk over chunks of whole events, the layout of a noise table and the range check of the *_last readers.
// Plain C++, no HIP header, no attpc_ctx: a check returns an ArgError the caller hands to fail(), and
// tests/native/host_args_check.cpp compiles the header alone (tests/test_host_args_cpu.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "attpc_engine.h"

namespace attpc {

// What a check found: nothing; an argument refused without a text (a missing array, a negative count: the bare
// ATTPC_E_INVALID, which leaves the context's last error as it was); or the text of the refusal.
struct ArgError {
  bool refused = false;
  std::string text;
  explicit operator bool() const { return refused; }
  __attribute__((format(printf, 1, 2))) static ArgError because(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return ArgError{true, buf};
  }
};

// The event count of entry point `what` and the presence of its offsets [n_events + 1].
inline ArgError csr_count_error(const char* what, int64_t n_events, const int64_t* offsets) {
  if (n_events < 0 || (n_events > 0 && !offsets)) return ArgError{true, {}};
  if (n_events > (int64_t)INT32_MAX) return ArgError::because("%s takes at most 2^31 - 1 events per call", what);
  return {};
}

// The two ways the entry points have always looked at their offsets, kept apart because an input can tell them apart
// (offsets -1, -2: the first reports the negative offsets[0], the second the decrease at event 0):
//   CSR_OPERATOR  offsets[0] >= 0, then event by event: no decrease, fewer than 2^31 rows
//   CSR_CLOUD     no decrease at any event, then offsets[0] >= 0; no limit per event (check_host_cloud bounds the call's
//                 rows by 2^32 instead: one event may hold 2^31 rows or more)
enum CsrOrder { CSR_OPERATOR, CSR_CLOUD };

// csr_count_error, then the offsets themselves: the first failure in the order of `order`, with its event.
inline ArgError csr_error(const char* what, int64_t n_events, const int64_t* offsets, CsrOrder order = CSR_OPERATOR) {
  if (ArgError bad = csr_count_error(what, n_events, offsets)) return bad;
  if (order == CSR_OPERATOR && n_events > 0 && offsets[0] < 0) return ArgError::because("offsets[0] < 0");
  for (int64_t e = 0; e < n_events; ++e) {
    if (offsets[e + 1] < offsets[e]) return ArgError::because("offsets decrease at event %lld", (long long)e);
    if (order == CSR_OPERATOR && offsets[e + 1] - offsets[e] > (int64_t)INT32_MAX)
      return ArgError::because("event %lld has 2^31 rows or more", (long long)e);
  }
  if (order == CSR_CLOUD && n_events > 0 && offsets[0] < 0) return ArgError::because("offsets[0] < 0");
  return {};
}

// The 12-bit samples of rows r0 .. r1 - 1 of samples [..][512] (rows numbered as the caller numbers them).
inline ArgError sample_error(const int16_t* samples, int64_t r0, int64_t r1) {
  for (int64_t i = r0 * ATTPC_NUM_TB; i < r1 * ATTPC_NUM_TB; ++i)
    if (samples[i] < 0 || samples[i] > 4095)
      return ArgError::because("sample %lld of row %lld is %d: 0 .. 4095", (long long)(i % ATTPC_NUM_TB),
                               (long long)(i / ATTPC_NUM_TB), (int)samples[i]);
  return {};
}

// The rows of a host cloud in checked CSR form, points [..][3] = (pad, time bucket, electrons): integer pad in range,
// 0 <= time bucket < 512, finite electrons >= 0; with `unique_cells` also a (pad, time bucket) of its own within the
// event (looked at once the event's rows have passed).
inline ArgError cloud_rows_error(int64_t n_events, const int64_t* offsets, const double* points, bool unique_cells) {
  std::vector<uint32_t> keys;
  for (int64_t e = 0; e < n_events; ++e) {
    keys.clear();
    for (int64_t r = offsets[e]; r < offsets[e + 1]; ++r) {
      const double padf = points[3 * r], tb = points[3 * r + 1], q = points[3 * r + 2];
      if (!(padf >= 0.0 && padf < (double)ATTPC_NUM_PADS) || padf != std::floor(padf))
        return ArgError::because("row %lld: pad %g is not an integer in [0, %d)", (long long)r, padf, ATTPC_NUM_PADS);
      if (!(tb >= 0.0 && tb < (double)ATTPC_NUM_TB))
        return ArgError::because("row %lld: time bucket %g outside [0, 512)", (long long)r, tb);
      if (!(q >= 0.0) || std::isinf(q)) return ArgError::because("row %lld: electrons %g", (long long)r, q);
      if (unique_cells) keys.push_back((uint32_t)padf * ATTPC_NUM_TB + (uint32_t)std::floor(tb));
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
      return ArgError::because("event %lld has two rows on one pad and time bucket", (long long)e);
  }
  return {};
}

// Chunks of whole events: the end e1 of the chunk that starts at event e0 < n_events.  Events are added while the chunk
// has fewer than max_events of them and the next one still fits max_rows rows; an event larger than that is a chunk alone.
inline int64_t chunk_end(const int64_t* offsets, int64_t n_events, int64_t e0, int64_t max_rows, int64_t max_events) {
  int64_t e1 = e0 + 1;
  while (e1 < n_events && e1 - e0 < max_events && offsets[e1 + 1] - offsets[e0] <= max_rows) ++e1;
  return e1;
}

// ... and the CSR offsets of its events e0 .. e1 - 1 counted from its first row: start [e1 - e0 + 1], start[0] = 0.
inline void chunk_starts(const int64_t* offsets, int64_t e0, int64_t e1, std::vector<int64_t>* start) {
  start->resize((size_t)(e1 - e0) + 1);
  for (int64_t e = e0; e <= e1; ++e) (*start)[(size_t)(e - e0)] = offsets[e] - offsets[e0];
}

// A noise table of n_levels levels (0 .. ATTPC_MAX_NOISE_LEVELS), cdf [n_levels - 1], as the kernels read it: the cdf
// padded to the full table with 0xFFFFFFFF (they copy all of it to LDS), and the guide: the search for u starts at
// guide[u >> 24] = #{k : cdf[k] <= (u >> 24) << 24}.
struct NoiseTable {
  std::vector<uint32_t> cdf;    // [ATTPC_MAX_NOISE_LEVELS]
  std::vector<uint16_t> guide;  // [256]
};
inline NoiseTable noise_table(int32_t n_levels, const uint32_t* cdf) {
  const int n_cdf = std::max(n_levels - 1, 0);
  NoiseTable t{std::vector<uint32_t>(ATTPC_MAX_NOISE_LEVELS, 0xFFFFFFFFu), std::vector<uint16_t>(256)};
  for (int k = 0; k < n_cdf; ++k) t.cdf[(size_t)k] = cdf[k];
  for (int b = 0, k = 0; b < 256; ++b) {
    while (k < n_cdf && t.cdf[(size_t)k] <= (uint32_t)b << 24) ++k;
    t.guide[(size_t)b] = (uint16_t)k;
  }
  return t;
}

// Records first .. first + count - 1 of the last call, one of call_events events (attpc_trigger_last, attpc_estimates_last).
inline ArgError records_range_error(const char* what, int64_t first, int64_t count, int64_t call_events) {
  if (first < 0 || count < 0 || first > call_events || count > call_events - first)
    return ArgError::because("%s: records %lld .. + %lld of a call of %lld events", what, (long long)first, (long long)count,
                             (long long)call_events);
  return {};
}

}  // namespace attpc
