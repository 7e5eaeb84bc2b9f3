// helix_host.hpp -- the parts of the helix slope (include/attpc_engine.h, "helix slope") that are the same code on the
// device and on the host: the checks of an attpc_helix_desc, the written arctangent, the quantised turning angle of a
// point, the unwrap step, the closed form on the four integer sums, and step 6 with the circle handed on to it.  Plain
// C++: estimate.hip uses it on the device (its sums come from a wave), abi.hip on the host, and
// tests/native/helix_check.cpp compiles it alone with helix_sums_host, the same sums in a plain loop
// (tests/test_helix_cpu.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"
#include "circle_host.hpp"
#include "estimate_host.hpp"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings fabs, rint and sqrt for both sides)
#define ATTPC_HELIX_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_HELIX_HD inline
#endif

namespace attpc {

constexpr int32_t HELIX_HALF_TURN = 205887;  // rint(pi * 65536)
constexpr int32_t HELIX_TURN = 411775;       // rint(2 pi * 65536)
constexpr int32_t HELIX_CAP = 1 << 24;       // |unwrapped angle| below this (about 40 turns)

// nullptr, or what is wrong with the settings
inline const char* helix_desc_error(const attpc_helix_desc& d) {
  if (d.regressor < ATTPC_HELIX_AUTO || d.regressor > ATTPC_HELIX_PATH_ON_Z) return "regressor: 0 .. 2";
  if (d.reserved != 0) return "reserved: 0";
  return nullptr;
}

// atan2(y, x) in written arithmetic: + - * / only, one rounding each, no branch (selects).  hi == 0 needs no case of
// its own: t = 0 / 1 then, and every later step keeps +0.
ATTPC_HELIX_HD double helix_atan2w(double y, double x) {
#pragma clang fp contract(off)
  const double ax = fabs(x), ay = fabs(y);
  const bool steep = ay > ax;
  const double hi = steep ? ay : ax, lo = steep ? ax : ay;
  const double t = lo / (hi == 0.0 ? 1.0 : hi);
  const bool upper = t > 0.41421356237309503;
  const double r = (upper ? t - 1.0 : t) / (upper ? t + 1.0 : 1.0);
  const double z = r * r;
  double p = -0.02564102564102564;  // c_19; c_k = (-1)^k / (2 k + 1)
  p = p * z + 0.02702702702702703;
  p = p * z + -0.02857142857142857;
  p = p * z + 0.030303030303030304;
  p = p * z + -0.03225806451612903;
  p = p * z + 0.034482758620689655;
  p = p * z + -0.037037037037037035;
  p = p * z + 0.04;
  p = p * z + -0.043478260869565216;
  p = p * z + 0.047619047619047616;
  p = p * z + -0.05263157894736842;
  p = p * z + 0.058823529411764705;
  p = p * z + -0.06666666666666667;
  p = p * z + 0.07692307692307693;
  p = p * z + -0.09090909090909091;
  p = p * z + 0.1111111111111111;
  p = p * z + -0.14285714285714285;
  p = p * z + 0.2;
  p = p * z + -0.3333333333333333;
  p = p * z + 1.0;
  double at = (upper ? 0.7853981633974483 : 0.0) + r * p;
  at = steep ? 1.5707963267948966 - at : at;
  at = x < 0.0 ? 3.141592653589793 - at : at;
  at = y < 0.0 ? -at : at;
  return at;
}

// phi_q of the point p = (px, py) about the centre, measured from p0; *bad: the angle is not a number (a circle so
// large that the products overflow), phi_q is 0 then and the record gets NO_HELIX
ATTPC_HELIX_HD int32_t helix_phi(double p0x, double p0y, double px, double py, bool* bad) {
#pragma clang fp contract(off)
  const double cr = p0x * py - p0y * px, dt = p0x * px + p0y * py;
  const double at = helix_atan2w(cr, dt);
  *bad = at != at;
  return *bad ? 0 : (int32_t)rint(65536.0 * at);
}

// j of the unwrap for the step from phi_q `before` to `phi`
ATTPC_HELIX_HD int32_t helix_wrap(int32_t before, int32_t phi) {
  const int32_t delta = phi - before;
  return delta > HELIX_HALF_TURN ? -1 : (delta < -HELIX_HALF_TURN ? 1 : 0);
}

struct HelixSums {   // step 3
  int64_t sp, spp, spw, sww;
  bool no_helix;     // an angle past the cap, or one that is not a number
};

// The closed form of step 4 on a record that step 6 has filled and that has a circle (a, b, R) in units relative to
// (X0, Y0): slope, vz, brho and the status.
ATTPC_HELIX_HD void helix_closed_form(const EstimateSums& k, const HelixSums& h, int32_t regressor, double magnetic_field,
                                      double a, double b_centre, double R, attpc_track_estimate* r) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  const double M = (double)k.m, X0 = (double)k.x0, Y0 = (double)k.y0, Z0 = (double)k.z0;
  const double SP = (double)h.sp, SPP = (double)h.spp, SPw = (double)h.spw, Sww = (double)h.sww, Sw = (double)k.sw;
  const double vp = M * SPP - SP * SP;
  const double vw = M * Sww - Sw * Sw;
  const double cv = M * SPw - SP * Sw;
  const bool use_b = regressor == ATTPC_HELIX_PATH_ON_Z ||
                     (regressor == ATTPC_HELIX_AUTO && vw * 4294967296.0 >= vp * R * R && cv != 0.0);
  const double q = use_b ? vw / (cv == 0.0 ? 1.0 : cv) : cv / (vp == 0.0 ? 1.0 : vp);
  // (a q that is not finite: q - q is NaN)
  if (h.no_helix || vp == 0.0 || (use_b && cv == 0.0) || q - q != 0.0) {
    r->status |= ATTPC_EST_NO_HELIX;
    return;
  }
  const double sg = h.sp >= 0 ? 1.0 : -1.0;
  const double b = (sg * 65536.0 * q) / R;
  const double a0 = (Sw - q * SP) / M;
  const double p0x = -a, p0y = -b_centre;
  const double pvx = -(X0 + a), pvy = -(Y0 + b_centre);
  const double Pv = rint(65536.0 * helix_atan2w(p0x * pvy - p0y * pvx, p0x * pvx + p0y * pvy));
  r->status &= ~ATTPC_EST_NO_SLOPE;
  r->slope = b;
  r->vz = (r->status & ATTPC_EST_ON_AXIS) ? nan : (Z0 + a0 + q * Pv) / 16.0;
  r->brho = magnetic_field * r->radius * 1.0e-3 * sqrt(1.0 + b * b);
}

// Step 6 of a record with the stage on, up to the circle: the Kasa circle, `refine`: its geometric fit (as
// estimate_closed_form_circle), and everything behind the circle.  true = the record has a circle, (a, b, R) in units
// relative to (X0, Y0); false = NO_CIRCLE.
template <typename Evaluate>
ATTPC_HELIX_HD bool helix_step6(const EstimateSums& k, double magnetic_field, bool refine, double tolerance,
                                int32_t max_evaluations, Evaluate&& evaluate, attpc_track_estimate* r, double* a_out,
                                double* b_out, double* R_out) {
#pragma clang fp contract(off)
  double a = 0.0, b = 0.0, r2 = 0.0, R = 0.0;
  const bool circle = estimate_kasa(k, &a, &b, &r2);
  if (circle) {
    R = sqrt(r2);
    if (refine) {
      const CircleFit fit = circle_refine((int32_t)k.m, a, b, R, tolerance, max_evaluations, evaluate);
      a = fit.a;
      b = fit.b;
      R = fit.R;
      r->reserved = fit.evaluations;
      r->status |= fit.converged ? 0 : ATTPC_EST_NOT_CONVERGED;
    }
  }
  estimate_from_circle(k, magnetic_field, circle, a, b, R, r);
  *a_out = a;
  *b_out = b;
  *R_out = R;
  return circle;
}

// Steps 1 to 3 on the host: the segment's integers (u, v, w) of step 5 in rank order -> the four sums; phi_q and the
// unwrapped angle of every rank go to phi_out and unwrapped_out if they are given.
inline HelixSums helix_sums_host(const int32_t* u, const int32_t* v, const int32_t* w, int32_t m, double a, double b,
                                 int32_t* phi_out = nullptr, int32_t* unwrapped_out = nullptr) {
#pragma clang fp contract(off)
  HelixSums h{0, 0, 0, 0, false};
  const double p0x = -a, p0y = -b;
  int32_t before = 0, turns = 0;
  for (int32_t i = 0; i < m; ++i) {
    bool bad;
    const int32_t phi = helix_phi(p0x, p0y, (double)u[i] - a, (double)v[i] - b, &bad);
    turns += i ? helix_wrap(before, phi) : 0;
    before = phi;
    const int32_t unwrapped = phi + HELIX_TURN * turns;  // (|turns| <= 2047: below 2^30)
    const bool over = bad || unwrapped >= HELIX_CAP || unwrapped <= -HELIX_CAP;
    h.no_helix = h.no_helix || over;
    const int64_t P = over ? 0 : unwrapped;  // (an angle past the cap adds nothing: the bounds hold in every record)
    h.sp += P;
    h.spp += P * P;
    h.spw += P * (int64_t)w[i];
    h.sww += (int64_t)w[i] * w[i];
    if (phi_out) phi_out[i] = phi;
    if (unwrapped_out) unwrapped_out[i] = unwrapped;
  }
  return h;
}

}  // namespace attpc
