// estimate_host.hpp -- the parts of the track estimates (include/attpc_engine.h, "track estimates of the trace rows")
// that are the same code on the device and on the host: the checks of an attpc_estimate_desc, the quantisation of a
// row and the closed form on the moment sums.  Plain C++: estimate.hip uses it on the device, abi.hip on the host, and
// tests/native/estimate_check.cpp compiles it alone (tests/test_estimate_cpu.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings rint and sqrt for both sides)
#define ATTPC_EST_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_EST_HD inline
#endif

namespace attpc {

// nullptr, or what is wrong with the settings
inline const char* estimate_desc_error(const attpc_estimate_desc& d) {
  if (!(d.beam_region_radius >= 0.0) || __builtin_isinf(d.beam_region_radius)) return "beam_region_radius: finite and >= 0";
  if (d.min_points < 3) return "min_points: >= 3";
  if (d.magnetic_field != d.magnetic_field) return "magnetic_field: not NaN";
  if (d.reserved != 0) return "reserved: 0";
  return nullptr;
}

// Rb of step 1, clamped
inline int64_t estimate_beam_units(double beam_region_radius) {
  const double rb = rint(16.0 * beam_region_radius);
  return rb >= 2147483647.0 ? 2147483647ll : (int64_t)rb;
}

// step 1 of the contract: false = the row is out of range
ATTPC_EST_HD bool estimate_quantise(double x, double y, double z, double integral, int32_t* X, int32_t* Y, int32_t* Z,
                                    int64_t* I) {
  // (a NaN fails every comparison)
  const bool ok = fabs(x) <= 320.0 && fabs(y) <= 320.0 && fabs(z) <= 8192.0 && fabs(integral) < 2147483648.0;
  *X = ok ? (int32_t)rint(16.0 * x) : 0;
  *Y = ok ? (int32_t)rint(16.0 * y) : 0;
  *Z = ok ? (int32_t)rint(16.0 * z) : 0;
  *I = ok ? (int64_t)rint(integral) : 0;
  return ok;
}

// d_i of step 5 for a step (dx, dy) in units
ATTPC_EST_HD int32_t estimate_step(int32_t dx, int32_t dy) {
  const int64_t q = (int64_t)dx * dx + (int64_t)dy * dy;
  return (int32_t)rint(sqrt((double)q));
}

struct EstimateSums {  // step 5
  int64_t m, x0, y0, z0;
  int64_t su, sv, suu, suv, svv, suuu, suvv, svvv, svuu, ss, sw, sss, ssw, si;
  int64_t arc;
};

// estimate_kasa and estimate_from_circle are step 6 in two halves, for the geometric circle fit between them
// (circle_host.hpp).  estimate_closed_form below stays the one piece it was: the kernels of the stage off are then
// instruction for instruction what they were; tests/test_circle_cpu.py holds the halves to it bit for bit.
// step 6, the Kasa circle of the sums: (uc, vc, r2) in units relative to (X0, Y0); false = there is none (NO_CIRCLE)
ATTPC_EST_HD bool estimate_kasa(const EstimateSums& k, double* uc_out, double* vc_out, double* r2_out) {
#pragma clang fp contract(off)
  const double m = (double)k.m;
  const double Su = (double)k.su, Sv = (double)k.sv, Suu = (double)k.suu, Suv = (double)k.suv, Svv = (double)k.svv;
  const double Suuu = (double)k.suuu, Suvv = (double)k.suvv, Svvv = (double)k.svvv, Svuu = (double)k.svuu;
  const double A = m * Suu - Su * Su;
  const double B = m * Suv - Su * Sv;
  const double C = m * Svv - Sv * Sv;
  const double D = (m * (Suvv + Suuu) - Su * (Suu + Svv)) / 2.0;
  const double E = (m * (Svuu + Svvv) - Sv * (Suu + Svv)) / 2.0;
  const double den = A * C - B * B;
  if (den == 0.0) return false;
  const double uc = (D * C - B * E) / den;
  const double vc = (A * E - B * D) / den;
  const double r2 = (Suu + Svv - 2.0 * uc * Su - 2.0 * vc * Sv) / m + uc * uc + vc * vc;
  *uc_out = uc;
  *vc_out = vc;
  *r2_out = r2;
  return r2 > 0.0;
}

// step 6 behind the circle (a, b, R) in units relative to (X0, Y0) -- `circle`: there is one --: the f64 fields, charge
// and arc of *r, and the status bits it adds
ATTPC_EST_HD void estimate_from_circle(const EstimateSums& k, double magnetic_field, bool circle, double a, double b_units,
                                       double R, attpc_track_estimate* r) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  const double m = (double)k.m, X0 = (double)k.x0, Y0 = (double)k.y0, Z0 = (double)k.z0;
  const double Su = (double)k.su, Sv = (double)k.sv;
  const double SS = (double)k.ss, Sw = (double)k.sw, SSS = (double)k.sss, SSw = (double)k.ssw;
  int32_t status = 0;
  double cx = nan, cy = nan, radius = nan, vx = nan, vy = nan;
  if (circle) {
    cx = (X0 + a) / 16.0;
    cy = (Y0 + b_units) / 16.0;
    radius = R / 16.0;
  }
  bool vertex = circle;
  if (!circle) status |= ATTPC_EST_NO_CIRCLE;
  if (circle) {
    const double c = sqrt(cx * cx + cy * cy);
    if (c == 0.0) {
      status |= ATTPC_EST_ON_AXIS;
      vertex = false;
    } else {
      vx = cx * (1.0 - radius / c);
      vy = cy * (1.0 - radius / c);
    }
  }
  const double sden = m * SSS - SS * SS;
  double b = nan, vz = nan, brho = nan;
  if (sden == 0.0) {
    status |= ATTPC_EST_NO_SLOPE;
  } else {
    b = (m * SSw - SS * Sw) / sden;
    if (vertex) {
      const double a0 = (Sw - b * SS) / m;
      const double gx = X0 - 16.0 * vx, gy = Y0 - 16.0 * vy;
      const double chord0 = sqrt(gx * gx + gy * gy);
      vz = (Z0 + a0 - b * chord0) / 16.0;
    }
    if (circle) brho = magnetic_field * radius * 1.0e-3 * sqrt(1.0 + b * b);
  }
  r->status |= status;
  r->charge = k.si;
  r->arc = k.arc;
  r->cx = cx;
  r->cy = cy;
  r->radius = radius;
  r->vx = vx;
  r->vy = vy;
  r->vz = vz;
  r->slope = b;
  r->x_mean = (X0 + Su / m) / 16.0;
  r->y_mean = (Y0 + Sv / m) / 16.0;
  r->dedx = k.arc == 0 ? nan : (double)k.si / ((double)k.arc / 16.0);
  r->brho = brho;
}

// step 6: the f64 fields, charge and arc of *r, and the status bits it adds
ATTPC_EST_HD void estimate_closed_form(const EstimateSums& k, double magnetic_field, attpc_track_estimate* r) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  const double m = (double)k.m, X0 = (double)k.x0, Y0 = (double)k.y0, Z0 = (double)k.z0;
  const double Su = (double)k.su, Sv = (double)k.sv, Suu = (double)k.suu, Suv = (double)k.suv, Svv = (double)k.svv;
  const double Suuu = (double)k.suuu, Suvv = (double)k.suvv, Svvv = (double)k.svvv, Svuu = (double)k.svuu;
  const double SS = (double)k.ss, Sw = (double)k.sw, SSS = (double)k.sss, SSw = (double)k.ssw;
  int32_t status = 0;
  const double A = m * Suu - Su * Su;
  const double B = m * Suv - Su * Sv;
  const double C = m * Svv - Sv * Sv;
  const double D = (m * (Suvv + Suuu) - Su * (Suu + Svv)) / 2.0;
  const double E = (m * (Svuu + Svvv) - Sv * (Suu + Svv)) / 2.0;
  const double den = A * C - B * B;
  double cx = nan, cy = nan, radius = nan, vx = nan, vy = nan;
  bool circle = den != 0.0;
  if (circle) {
    const double uc = (D * C - B * E) / den;
    const double vc = (A * E - B * D) / den;
    const double r2 = (Suu + Svv - 2.0 * uc * Su - 2.0 * vc * Sv) / m + uc * uc + vc * vc;
    circle = r2 > 0.0;
    if (circle) {
      cx = (X0 + uc) / 16.0;
      cy = (Y0 + vc) / 16.0;
      radius = sqrt(r2) / 16.0;
    }
  }
  bool vertex = circle;
  if (!circle) status |= ATTPC_EST_NO_CIRCLE;
  if (circle) {
    const double c = sqrt(cx * cx + cy * cy);
    if (c == 0.0) {
      status |= ATTPC_EST_ON_AXIS;
      vertex = false;
    } else {
      vx = cx * (1.0 - radius / c);
      vy = cy * (1.0 - radius / c);
    }
  }
  const double sden = m * SSS - SS * SS;
  double b = nan, vz = nan, brho = nan;
  if (sden == 0.0) {
    status |= ATTPC_EST_NO_SLOPE;
  } else {
    b = (m * SSw - SS * Sw) / sden;
    if (vertex) {
      const double a0 = (Sw - b * SS) / m;
      const double gx = X0 - 16.0 * vx, gy = Y0 - 16.0 * vy;
      const double chord0 = sqrt(gx * gx + gy * gy);
      vz = (Z0 + a0 - b * chord0) / 16.0;
    }
    if (circle) brho = magnetic_field * radius * 1.0e-3 * sqrt(1.0 + b * b);
  }
  r->status |= status;
  r->charge = k.si;
  r->arc = k.arc;
  r->cx = cx;
  r->cy = cy;
  r->radius = radius;
  r->vx = vx;
  r->vy = vy;
  r->vz = vz;
  r->slope = b;
  r->x_mean = (X0 + Su / m) / 16.0;
  r->y_mean = (Y0 + Sv / m) / 16.0;
  r->dedx = k.arc == 0 ? nan : (double)k.si / ((double)k.arc / 16.0);
  r->brho = brho;
}

// the record of step 2 (n_used < min_points), and of a later position of a label given twice (n_rows = 0)
ATTPC_EST_HD void estimate_no_fit(int32_t n_rows, int32_t n_used, bool range, attpc_track_estimate* r) {
  const double nan = __builtin_nan("");
  r->n_rows = n_rows;
  r->n_used = n_used;
  r->n_fit = 0;
  r->status = (n_rows == 0 ? ATTPC_EST_EMPTY : ATTPC_EST_FEW) | (range ? ATTPC_EST_RANGE : 0);
  r->direction = 0;
  r->reserved = 0;
  r->charge = r->arc = 0;
  r->cx = r->cy = r->radius = r->vx = r->vy = r->vz = r->slope = r->x_mean = r->y_mean = r->dedx = r->brho = nan;
}

}  // namespace attpc
