// spyral_integral.hpp -- the clipped integral of a Spyral row in closed form: the tables attpc_spyral_configure builds
// from the response, and their evaluation per cloud row.  Plain C++: abi.hip builds the tables on the host, spyral.hip
// evaluates them on the device, and tests/native/spyral_integral_check.cpp compares both with a long double sum of the
// 512 clipped products (tests/test_spyral_cpu.py).
//
// reference response.py:35-57: integral = sum_i min(r_i q, 4095).  With the samples sorted descending and
// k = #{i : r_i q > 4095}:  integral = 4095 k + q tail[k],  tail[k] = the sum of all but the k largest samples.
// tail[] is accumulated from the smallest sample upwards (compensated), so every entry is the rounded sum of its own
// terms and nothing is obtained as a difference of two large sums: the error is a few ulp of the larger of 4095 k and
// q tail[k] at any charge (of the result, then, unless negative samples make the two cancel).
// (total - prefix[k] instead loses eps * total -- times q -- once the large samples are clipped.)
#pragma once

#if defined(__HIPCC__)
#define ATTPC_SI_HD __host__ __device__ __forceinline__
#else
#define ATTPC_SI_HD inline
#endif

#include <algorithm>
#include <cmath>
#include <functional>

namespace attpc {

constexpr int SPYRAL_SAMPLES = 512;        // ATTPC_NUM_TB
constexpr double SPYRAL_ADC_MAX = 4095.0;  // response.py:56

// sorted_desc [512]: the response, largest first.  tail [513]: tail[k] = sorted_desc[k] + ... + sorted_desc[511],
// tail[512] = 0.  Host side.
inline void spyral_integral_tables(const double* response, double* sorted_desc, double* tail) {
  std::copy(response, response + SPYRAL_SAMPLES, sorted_desc);
  std::sort(sorted_desc, sorted_desc + SPYRAL_SAMPLES, std::greater<double>());
  // Neumaier's sum from the small end: `lost` collects what every addition rounds away (a response with negative
  // lobes cancels on the way up)
  double sum = 0.0, lost = 0.0;
  tail[SPYRAL_SAMPLES] = 0.0;
  for (int k = SPYRAL_SAMPLES - 1; k >= 0; --k) {
    const double x = sorted_desc[k], t = sum + x;
    lost += std::fabs(sum) >= std::fabs(x) ? (sum - t) + x : (x - t) + sum;
    sum = t;
    tail[k] = sum + lost;
  }
}

// k = number of samples with r q > 4095: a binary search (the products fall with the index for q >= 0)
ATTPC_SI_HD int spyral_clipped_count(const double* sorted_desc, double q) {
  int lo = 0, hi = SPYRAL_SAMPLES;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted_desc[mid] * q > SPYRAL_ADC_MAX) lo = mid + 1; else hi = mid;
  }
  return lo;
}

ATTPC_SI_HD double spyral_clipped_integral(const double* sorted_desc, const double* tail, double q) {
  const int k = spyral_clipped_count(sorted_desc, q);
  return SPYRAL_ADC_MAX * (double)k + q * tail[k];
}

}  // namespace attpc
