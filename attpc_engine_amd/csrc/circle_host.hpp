// circle_host.hpp -- the parts of the geometric circle fit (include/attpc_engine.h, "geometric circle fit") that are the
// same code on the device and on the host: the checks of an attpc_circle_desc, the terms of one point, the 3x3 step, the
// accept / stop rule, the iteration around an evaluation that the caller supplies, and step 6 with the refined circle.
// Plain C++: estimate.hip uses it on the device (its evaluation walks the wave's points in LDS), abi.hip on the host,
// and tests/native/circle_check.cpp compiles it alone with circle_evaluate_lanes, the same order of summation on 64
// accumulators (tests/test_circle_cpu.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"
#include "estimate_host.hpp"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings fabs and sqrt for both sides)
#define ATTPC_CIRCLE_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_CIRCLE_HD inline
#endif

namespace attpc {

constexpr double CIRCLE_LAMBDA0 = 0.0009765625;  // 2^-10
constexpr double CIRCLE_LAMBDA_ACCEPT = 0.04, CIRCLE_LAMBDA_REJECT = 10.0;

// nullptr, or what is wrong with the settings
inline const char* circle_desc_error(const attpc_circle_desc& d) {
  if (!(d.tolerance > 0.0) || __builtin_isinf(d.tolerance)) return "tolerance: finite and > 0";
  if (d.max_evaluations < ATTPC_CIRCLE_MIN_EVALUATIONS || d.max_evaluations > ATTPC_CIRCLE_MAX_EVALUATIONS)
    return "max_evaluations: 2 .. 64";
  if (d.reserved != 0) return "reserved: 0";
  return nullptr;
}

struct CircleSums {  // the nine sums of one evaluation
  double f, uu, uv, vv, u, v, gu, gv, g;
};

ATTPC_CIRCLE_HD CircleSums circle_zero() { return CircleSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

ATTPC_CIRCLE_HD CircleSums circle_add(const CircleSums& x, const CircleSums& y) {
#pragma clang fp contract(off)
  return CircleSums{x.f + y.f, x.uu + y.uu, x.uv + y.uv, x.vv + y.vv, x.u + y.u, x.v + y.v, x.gu + y.gu, x.gv + y.gv, x.g + y.g};
}

// *s += the terms of the point (u, v) at p = (a, b, R)
ATTPC_CIRCLE_HD void circle_point(int32_t u, int32_t v, double a, double b, double R, CircleSums* s) {
#pragma clang fp contract(off)
  const double dx = (double)u - a, dy = (double)v - b;
  const double r = sqrt(dx * dx + dy * dy);
  const double U = r == 0.0 ? 0.0 : dx / r, V = r == 0.0 ? 0.0 : dy / r;
  const double g = r - R;
  s->f = s->f + g * g;
  s->uu = s->uu + U * U;
  s->uv = s->uv + U * V;
  s->vv = s->vv + V * V;
  s->u = s->u + U;
  s->v = s->v + V;
  s->gu = s->gu + g * U;
  s->gv = s->gv + g * V;
  s->g = s->g + g;
}

// the step d of (N + lambda diag N) d = rhs, by the header's elimination
ATTPC_CIRCLE_HD void circle_step(const CircleSums& k, double M, double lambda, double d[3]) {
#pragma clang fp contract(off)
  const double m00 = k.uu + lambda * k.uu, m11 = k.vv + lambda * k.vv, m22 = M + lambda * M;
  const double l10 = k.uv / m00, l20 = k.u / m00;
  const double a11 = m11 - l10 * k.uv, a12 = k.v - l10 * k.u, b1 = k.gv - l10 * k.gu;
  const double a22 = m22 - l20 * k.u, b2 = k.g - l20 * k.gu;
  const double l21 = a12 / a11;
  const double c22 = a22 - l21 * a12, c2 = b2 - l21 * b1;
  d[2] = c2 / c22;
  d[1] = (b1 - a12 * d[2]) / a11;
  d[0] = (k.gu - k.uv * d[1] - k.u * d[2]) / m00;
}

// is the trial with the objective f_trial and the radius R_trial taken?  (a NaN fails a comparison)
ATTPC_CIRCLE_HD bool circle_accept(double f, double f_trial, double R_trial) { return f_trial <= f && R_trial > 0.0; }

// does the accepted step d end the iteration?
ATTPC_CIRCLE_HD bool circle_converged(const double d[3], double tolerance) {
  const double d01 = fabs(d[0]) > fabs(d[1]) ? fabs(d[0]) : fabs(d[1]);
  return (d01 > fabs(d[2]) ? d01 : fabs(d[2])) <= tolerance;
}

struct CircleFit {
  double a, b, R;       // the last accepted p (the start if none was)
  int32_t evaluations;  // >= 1
  bool converged;
};

// The iteration from the start (a, b, R) on m points; evaluate(a, b, R) gives the nine sums there in the contract's
// order of summation.  On the device every lane runs this with the same values.
template <typename Evaluate>
ATTPC_CIRCLE_HD CircleFit circle_refine(int32_t m, double a, double b, double R, double tolerance, int32_t max_evaluations,
                                        Evaluate&& evaluate) {
#pragma clang fp contract(off)
  CircleFit fit{a, b, R, 1, false};
  CircleSums k = evaluate(a, b, R);
  double lambda = CIRCLE_LAMBDA0;
  const double M = (double)m;
  while (fit.evaluations < max_evaluations) {
    double d[3];
    circle_step(k, M, lambda, d);
    const double ta = fit.a + d[0], tb = fit.b + d[1], tR = fit.R + d[2];
    const CircleSums kt = evaluate(ta, tb, tR);
    ++fit.evaluations;
    if (circle_accept(k.f, kt.f, tR)) {
      fit.a = ta;
      fit.b = tb;
      fit.R = tR;
      k = kt;
      lambda = CIRCLE_LAMBDA_ACCEPT * lambda;
      if (circle_converged(d, tolerance)) {
        fit.converged = true;
        break;
      }
    } else {
      lambda = CIRCLE_LAMBDA_REJECT * lambda;
    }
  }
  return fit;
}

// step 6 with the stage on: the Kasa circle, its refinement if there is one, and everything behind the circle; the
// evaluations go to r->reserved, NOT_CONVERGED to the status
template <typename Evaluate>
ATTPC_CIRCLE_HD void estimate_closed_form_circle(const EstimateSums& k, double magnetic_field, double tolerance,
                                                 int32_t max_evaluations, Evaluate&& evaluate, attpc_track_estimate* r) {
#pragma clang fp contract(off)
  double a = 0.0, b = 0.0, r2 = 0.0, R = 0.0;
  const bool circle = estimate_kasa(k, &a, &b, &r2);
  if (circle) {
    const CircleFit fit = circle_refine((int32_t)k.m, a, b, sqrt(r2), tolerance, max_evaluations, evaluate);
    a = fit.a;
    b = fit.b;
    R = fit.R;
    r->reserved = fit.evaluations;
    r->status |= fit.converged ? 0 : ATTPC_EST_NOT_CONVERGED;
  }
  estimate_from_circle(k, magnetic_field, circle, a, b, R, r);
}

// One evaluation on the host in the contract's order of summation: 64 lane accumulators, rank i to lane i mod 64 in
// ascending i, then the xor tree over all lanes at once.
inline CircleSums circle_evaluate_lanes(const int32_t* u, const int32_t* v, int32_t m, double a, double b, double R) {
  CircleSums lane[64], next[64];
  for (int l = 0; l < 64; ++l) {
    lane[l] = circle_zero();
    for (int32_t i = l; i < m; i += 64) circle_point(u[i], v[i], a, b, R, &lane[l]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (int l = 0; l < 64; ++l) next[l] = circle_add(lane[l], lane[l ^ off]);
    for (int l = 0; l < 64; ++l) lane[l] = next[l];
  }
  return lane[0];
}

}  // namespace attpc
