// distort_host.hpp -- the drift distortion of one track record (include/attpc_engine.h, "drift distortion") as one piece
// of code for the device and the host: the checks of an attpc_distort_desc and the shift of one record (x, y, time
// bucket).  Plain C++, + - * / and sqrt only, every operation rounded once: distort.hip uses it on the device, abi.hip
// on the host, and tests/native/distort_check.cpp compiles it alone (tests/test_distortion_cpu.py pins it bit for bit
// to tests/distortion_reference.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings sqrt for both sides)
#define ATTPC_DISTORT_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_DISTORT_HD inline
#endif

namespace attpc {

constexpr int32_t DISTORT_MAX_NODES = 256;      // per axis
constexpr double DISTORT_MAX_SHIFT = 1.0;       // m, |radial| and |azimuthal|
constexpr double DISTORT_MAX_TIME = 1024.0;     // time buckets, |time|

// finite and > 0 (a NaN fails every comparison)
inline bool distort_positive(double v) { return v > 0.0 && !__builtin_isinf(v); }
inline bool distort_finite(double v) { return v - v == 0.0; }

// nullptr, or what is wrong with the map
inline const char* distort_desc_error(const attpc_distort_desc& d) {
  if (!distort_positive(d.rho_step)) return "rho_step: finite and > 0";
  if (!distort_positive(d.tau_step)) return "tau_step: finite and > 0";
  if (!distort_finite(d.tb_origin)) return "tb_origin: finite";
  if (d.n_rho < 2 || d.n_rho > DISTORT_MAX_NODES) return "n_rho: 2 .. 256";
  if (d.n_tau < 2 || d.n_tau > DISTORT_MAX_NODES) return "n_tau: 2 .. 256";
  const int64_t nodes = (int64_t)d.n_rho * d.n_tau;
  const double* tables[3] = {d.radial, d.azimuthal, d.time};
  for (int k = 0; k < 3; ++k) {
    const double cap = k < 2 ? DISTORT_MAX_SHIFT : DISTORT_MAX_TIME;
    for (int64_t i = 0; tables[k] && i < nodes; ++i) {
      const double v = tables[k][i];
      if (!(v >= -cap && v <= cap))  // (a NaN fails both)
        return k == 0 ? "radial: every value finite, |value| <= 1 m"
                      : k == 1 ? "azimuthal: every value finite, |value| <= 1 m"
                               : "time: every value finite, |value| <= 1024 time buckets";
    }
  }
  return nullptr;
}

// a valid map that shifts nothing: every table NULL or all zeros (the stage off)
inline bool distort_desc_is_off(const attpc_distort_desc& d) {
  const int64_t nodes = (int64_t)d.n_rho * d.n_tau;
  const double* tables[3] = {d.radial, d.azimuthal, d.time};
  for (int k = 0; k < 3; ++k)
    for (int64_t i = 0; tables[k] && i < nodes; ++i)
      if (tables[k][i] != 0.0) return false;
  return true;
}

struct DistortMap {  // what the shift reads of an attpc_distort_desc (on the device: device pointers)
  double rho_step, tau_step, tb_origin;
  int32_t n_rho, n_tau;
  const double* radial;     // [n_rho][n_tau] or nullptr = zeros
  const double* azimuthal;
  const double* time;
};

// a / step clamped to [0, n - 1] -> the cell (at most n - 2) and the weight in it (1 on and beyond the last node)
ATTPC_DISTORT_HD void distort_cell(double v, double step, int32_t n, int32_t& cell, double& weight) {
#pragma clang fp contract(off)
  const double last = (double)(n - 1);
  double a = v / step;
  a = a > last ? last : a;
  a = a >= 0.0 ? a : 0.0;  // (a NaN, which a finite record does not give, lands on node 0)
  const int32_t whole = (int32_t)a;  // a >= 0: the floor
  cell = whole < n - 2 ? whole : n - 2;
  weight = a - (double)cell;
}

// the bilinear value of table T (nullptr: 0) in cell (i, j) at weights (fr, fs)
ATTPC_DISTORT_HD double distort_value(const double* T, int32_t n_tau, int32_t i, int32_t j, double fr, double fs) {
#pragma clang fp contract(off)
  if (!T) return 0.0;
  const double* row = T + (int64_t)i * n_tau + j;
  const double t00 = row[0], t01 = row[1], t10 = row[n_tau], t11 = row[n_tau + 1];
  const double lo = t00 + fs * (t01 - t00);
  const double hi = t10 + fs * (t11 - t10);
  return lo + fr * (hi - lo);
}

// The shift of one record, in place.  A record with a non-finite x, y or time bucket keeps its bits.
ATTPC_DISTORT_HD void distort_record(const DistortMap& m, double& x, double& y, double& tb) {
#pragma clang fp contract(off)
  if (!(x - x == 0.0) || !(y - y == 0.0) || !(tb - tb == 0.0)) return;
  const double xx = x * x, yy = y * y;
  const double rho = sqrt(xx + yy);
  const double tau = tb - m.tb_origin;
  int32_t i, j;
  double fr, fs;
  distort_cell(rho, m.rho_step, m.n_rho, i, fr);
  distort_cell(tau, m.tau_step, m.n_tau, j, fs);
  const double dr = distort_value(m.radial, m.n_tau, i, j, fr, fs);
  const double da = distort_value(m.azimuthal, m.n_tau, i, j, fr, fs);
  const double dt = distort_value(m.time, m.n_tau, i, j, fr, fs);
  double ux = 0.0, uy = 0.0;  // rho == 0: no direction, no shift in the plane
  if (rho != 0.0) {
    ux = x / rho;
    uy = y / rho;
  }
  const double rx = dr * ux, ry = dr * uy, ax = da * uy, ay = da * ux;
  x = (x + rx) - ax;
  y = (y + ry) + ay;
  tb = tb + dt;
}

}  // namespace attpc
