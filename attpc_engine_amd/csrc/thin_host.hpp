// thin_host.hpp -- the parts of the thinned track points (include/attpc_engine.h, "thinned track points") that are the
// same code on the device and on the host: the checks of an attpc_thin_desc, H, the floor bin and the rounded centroid
// C(S).  Plain C++: thin.hip uses it on the device, abi.hip on the host, and tests/native/thin_check.cpp compiles it
// alone (tests/test_thin_cpu.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings rint for both sides)
#define ATTPC_THIN_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_THIN_HD inline
#endif

namespace attpc {

// nullptr, or what is wrong with the settings
inline const char* thin_desc_error(const attpc_thin_desc& d) {
  // (a NaN fails both comparisons)
  if (!(d.z_step >= 1.0 / 16.0 && d.z_step <= 512.0)) return "z_step: finite, 1/16 .. 512 mm";
  if (d.reserved != 0) return "reserved: 0";
  if (d.pad != 0) return "pad: 0";
  return nullptr;
}

// H: the z step in units, 1 .. 8192 for a checked desc
inline int32_t thin_step_units(double z_step) { return (int32_t)rint(16.0 * z_step); }

// floor(a / b) for b > 0, also for a < 0
ATTPC_THIN_HD int64_t thin_floor_div(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return q * b > a ? q - 1 : q;  // (C truncates towards zero: one too high for a negative a that b does not divide)
}

// step 2: the bin of Z for the step H
ATTPC_THIN_HD int32_t thin_bin(int32_t Z, int32_t H) {
  const int32_t q = Z / H;
  return q * H > Z ? q - 1 : q;
}

// step 6: C(S) = floor((2 S + W) / (2 W)) for W > 0 -- S / W rounded to the nearest integer, a tie upwards
ATTPC_THIN_HD int64_t thin_centroid(int64_t S, int64_t W) { return thin_floor_div(2 * S + W, 2 * W); }

}  // namespace attpc
