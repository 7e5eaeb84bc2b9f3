// div_rn.hpp -- a double divided by a 32-bit integer, correctly rounded, without the hardware division (whose expansion
// on gfx950 is a chain of fused multiply-adds).  Plain C++: peaks.hip uses it on the device, and
// tests/native/div_rn_check.cpp compares it with the host's division (tests/test_peaks_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings ldexp for both sides)
#define ATTPC_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_HD inline
#endif

namespace attpc {

// a / d rounded to nearest even, for an integer 0 < |d| < 2^31 and a zero, normal (with a normal quotient), infinite
// or NaN `a`: long division on the mantissa.  A subnormal `a` counts as zero (peaks.hip divides differences of
// numbers that are whole multiples of 2^-41 and lengths of at most 512).
ATTPC_HD double div_by_int_rn(double a, int32_t d) {
  union { double f; uint64_t u; } in;
  in.f = a;
  const bool negative = ((in.u >> 63) != 0) != (d < 0);
  const int ex = (int)((in.u >> 52) & 0x7ff);
  if (ex == 0) return negative ? -0.0 : 0.0;
  if (ex == 0x7ff) return d < 0 ? -a : a;  // infinity keeps its magnitude, NaN stays NaN
  const uint64_t m = (in.u & ((1ull << 52) - 1)) | (1ull << 52);  // |a| = m 2^(ex - 1075)
  const uint64_t ud = (uint64_t)(d < 0 ? -(int64_t)d : (int64_t)d);
  const uint64_t hi = m / ud, r = m % ud;
  const uint64_t lo = (r << 32) / ud, r2 = (r << 32) % ud;  // floor(m 2^32 / d) = hi 2^32 + lo, exact iff r2 == 0
  const uint64_t top = hi >> 32, bot = (hi << 32) | lo;
#ifdef __HIP_DEVICE_COMPILE__
  const int nb = top ? 128 - __clzll((long long)top) : 64 - __clzll((long long)bot);
#else
  const int nb = top ? 128 - __builtin_clzll(top) : 64 - __builtin_clzll(bot);
#endif
  const int shift = nb - 53;  // 1 .. 32: the quotient has 54 .. 85 bits
  uint64_t mant = (bot >> shift) | (top << (64 - shift));
  const uint64_t rem = bot & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (r2 != 0 || (mant & 1ull)))) mant += 1;
  const double q = ldexp((double)mant, shift + ex - 1075 - 32);
  return negative ? -q : q;
}

}  // namespace attpc
