// undistort_host.hpp -- the drift correction of one trace row (include/attpc_engine.h, "drift correction") as one piece
// of code for the device and the host: the checks of an attpc_undistort_desc, the fixed-point iteration on the forward
// map of distort_host.hpp and the z of a corrected time.  Plain C++, + - * / and sqrt only, every operation rounded
// once: undistort.hip uses it on the device, abi.hip its checks on the host, and tests/native/undistort_check.cpp
// compiles it alone (tests/test_undistort_cpu.py pins it bit for bit to tests/undistort_reference.py).
#pragma once
#include <stdint.h>

#include "distort_host.hpp"
#include "div_rn.hpp"

namespace attpc {

constexpr int32_t UNDISTORT_MAX_ITERATIONS = 64;

// finite and >= 0 (a NaN fails the comparison)
inline bool undistort_tolerance(double v) { return v >= 0.0 && !__builtin_isinf(v); }

// nullptr, or what is wrong with the settings
inline const char* undistort_desc_error(const attpc_undistort_desc& d) {
  if (const char* wrong = distort_desc_error(d.map)) return wrong;
  if (!(d.windows_edge > d.micromegas_edge)) return "windows_edge > micromegas_edge";
  if ((int64_t)d.windows_edge - (int64_t)d.micromegas_edge > (int64_t)INT32_MAX) return "windows_edge - micromegas_edge < 2^31";
  if (!distort_positive(d.length)) return "length: finite and > 0";
  if (d.iterations < 1 || d.iterations > UNDISTORT_MAX_ITERATIONS) return "iterations: 1 .. 64";
  if (!undistort_tolerance(d.tolerance_xy)) return "tolerance_xy: finite and >= 0";
  if (!undistort_tolerance(d.tolerance_tb)) return "tolerance_tb: finite and >= 0";
  return nullptr;
}

struct UndistortSettings {  // what a row reads of an attpc_undistort_desc (on the device: device pointers in the map)
  DistortMap map;
  double window_edge;  // windows_edge as a double (exact)
  int32_t span;        // windows_edge - micromegas_edge, > 0
  int32_t iterations;
  double length;
  double tolerance_xy, tolerance_tb;
};

inline UndistortSettings undistort_settings(const attpc_undistort_desc& d, const DistortMap& map) {
  return UndistortSettings{map, (double)d.windows_edge, (int32_t)(d.windows_edge - d.micromegas_edge), d.iterations,
                           d.length, d.tolerance_xy, d.tolerance_tb};
}

constexpr int UNDISTORT_SKIPPED = 1, UNDISTORT_UNCONVERGED = 2;

// Steps 1 to 4 of one row: the corrected (x m, y m, t time buckets) -> 0, UNDISTORT_UNCONVERGED, or UNDISTORT_SKIPPED
// (then x, y, t are not set: the row keeps its bits).
ATTPC_DISTORT_HD int undistort_row(const UndistortSettings& s, const double* row, double& x, double& y, double& t) {
#pragma clang fp contract(off)
  const double r0 = row[0], r1 = row[1], st = row[6];
  if (!(r0 - r0 == 0.0) || !(r1 - r1 == 0.0) || !(st - st == 0.0)) return UNDISTORT_SKIPPED;
  const double sx = r0 / 1000.0, sy = r1 / 1000.0;
  x = sx;
  y = sy;
  t = st;
  double dx = 0.0, dy = 0.0, dt = 0.0;
  for (int32_t k = 0; k < s.iterations; ++k) {
    double fx = x, fy = y, ft = t;
    distort_record(s.map, fx, fy, ft);
    dx = fx - sx;
    dy = fy - sy;
    dt = ft - st;
    x = x - dx;
    y = y - dy;
    t = t - dt;
  }
  const double ax = dx < 0.0 ? -dx : dx, ay = dy < 0.0 ? -dy : dy, at = dt < 0.0 ? -dt : dt;
  return (ax > s.tolerance_xy || ay > s.tolerance_xy || at > s.tolerance_tb) ? UNDISTORT_UNCONVERGED : 0;
}

// Step 5: the z (mm) of a corrected time -- the expression of the trace rows' own z (peaks.hip)
ATTPC_DISTORT_HD double undistort_z(const UndistortSettings& s, double t) {
#pragma clang fp contract(off)
  return div_by_int_rn(s.window_edge - t, s.span) * s.length * 1000.0;
}

}  // namespace attpc
