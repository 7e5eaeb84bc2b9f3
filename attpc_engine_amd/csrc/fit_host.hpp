// fit_host.hpp -- the parts of the track fit (include/attpc_engine.h, "track fit") that are the same code on the device
// and on the host: the checks of an attpc_fit_desc, the stopping-power look-up, the equation of motion and its RK4 step,
// the end of a trial, the walk of a trial past the data points, the terms of one point, the 6x6 step, the iteration
// around an evaluation that the caller supplies, the start from an estimate record and the record itself.  Plain C++,
// only + - * / and sqrt: fit.hip uses it on the device (a lane per trial, the sums over eight lanes),
// tests/native/fit_check.cpp compiles it alone with fit_evaluate_lanes, the same trials one after the other and the
// same order of summation on eight accumulators (tests/test_fit_cpu.py).
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings sqrt for both sides)
#define ATTPC_FIT_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_FIT_HD inline
#endif

namespace attpc {

constexpr double FIT_LAMBDA0 = 0.0009765625;  // 2^-10, as the circle fit
constexpr double FIT_LAMBDA_ACCEPT = 0.04, FIT_LAMBDA_REJECT = 10.0;
constexpr double FIT_DELTA_MOMENTUM = 1.52587890625e-05;  // 2^-16 of |g_start|
constexpr double FIT_DELTA_POSITION = 1.52587890625e-05;  // 2^-16 m
constexpr double FIT_KE_LIMIT = 1e-6;                      // MeV
constexpr double FIT_RHO_MAX2 = 0.292 * 0.292;             // m^2
constexpr double FIT_P_PER_BRHO = 299.792458;              // MeV/c per (T m) and unit charge
constexpr int FIT_LANES = 8;                               // lanes of a track: trials 0 .. 6 and one more in the sums
constexpr int FIT_SUMS = 28;                               // f, J^T r (6), the upper triangle of J^T J (21)

// nullptr, or what is wrong with the settings
inline const char* fit_desc_error(const attpc_fit_desc& d) {
  if (!(d.time_step > 0.0) || __builtin_isinf(d.time_step)) return "time_step: finite and > 0";
  if (!(d.tolerance_momentum > 0.0) || __builtin_isinf(d.tolerance_momentum)) return "tolerance_momentum: finite and > 0";
  if (!(d.tolerance_position > 0.0) || __builtin_isinf(d.tolerance_position)) return "tolerance_position: finite and > 0";
  if (d.max_steps < 1 || d.max_steps > ATTPC_FIT_MAX_STEPS) return "max_steps: 1 .. 10000";
  if (d.max_evaluations < ATTPC_FIT_MIN_EVALUATIONS || d.max_evaluations > ATTPC_FIT_MAX_EVALUATIONS)
    return "max_evaluations: 2 .. 32";
  return nullptr;
}

struct FitSpecies {  // the constants of a position's nucleus (as tracks.hip makes them)
  double mass;       // MeV
  double charge;     // Z
  double qm_b;       // q/m * (-B) / c
  double qm_e;       // q/m * (-E) / c
  double drag;       // MEV_2_JOULE * density * 100 / mass_kg / c
};

ATTPC_FIT_HD FitSpecies fit_species(double mass, int32_t Z, double bfield, double efield, double density) {
#pragma clang fp contract(off)
  const double mass_kg = mass * 1.7826619216278976e-30;
  const double q_m = (double)Z * 1.602176634e-19 / mass_kg;
  FitSpecies s;
  s.mass = mass;
  s.charge = (double)Z;
  s.qm_b = q_m * (-bfield) / 299792458.0;
  s.qm_e = q_m * (-efield) / 299792458.0;
  s.drag = 1.6021766339999998e-13 * density * 100.0 / mass_kg / 299792458.0;
  return s;
}

ATTPC_FIT_HD bool fit_finite(double v) { return v - v == 0.0; }

// the stopping-power table on the binade grid, as dedx_lookup of common.hpp: the same bit arithmetic, no contraction
ATTPC_FIT_HD double fit_dedx(const double* tab, double ke) {
#pragma clang fp contract(off)
  if (!(ke >= 9.313225746154785e-10)) return tab[0];
  if (ke >= 16384.0) return tab[ATTPC_DEDX_NODES - 1];
  uint64_t bits;
  __builtin_memcpy(&bits, &ke, sizeof bits);
  const int e = (int)((bits >> 52) & 0x7ff) - 1023;
  const int j = (int)((bits >> 47) & 31);
  const double t = (double)(bits & ((1ull << 47) - 1)) * (1.0 / 140737488355328.0);
  const int i = (e - ATTPC_DEDX_EMIN) * ATTPC_DEDX_SUB + j;
  const double lo = tab[i], hi = tab[i + 1];
  return lo + t * (hi - lo);
}

// the kinetic energy of the state's gamma beta, MeV
ATTPC_FIT_HD double fit_ke(double gx, double gy, double gz, double mass) {
#pragma clang fp contract(off)
  const double gv2 = gx * gx + gy * gy + gz * gz;
  return mass * (sqrt(1.0 + gv2) - 1.0);
}

// the right-hand side of tracks.hip with sqrt and / in the place of rsqrt; s = (x, y, z, gx, gy, gz)
ATTPC_FIT_HD void fit_rhs(const double s[6], const FitSpecies& sp, const double* tab, double r[6]) {
#pragma clang fp contract(off)
  const double gv2 = s[3] * s[3] + s[4] * s[4] + s[5] * s[5];
  const double gv = sqrt(gv2);
  const double gamma = sqrt(1.0 + gv2);
  const double ke = sp.mass * (gamma - 1.0);
  const double vscale = 299792458.0 / gamma;
  const double vx = s[3] * vscale, vy = s[4] * vscale, vz = s[5] * vscale;
  const double dec = fit_dedx(tab, ke) * sp.drag / gv;
  r[0] = vx;
  r[1] = vy;
  r[2] = vz;
  r[3] = sp.qm_b * vy - dec * s[3];
  r[4] = -sp.qm_b * vx - dec * s[4];
  r[5] = sp.qm_e - dec * s[5];
}

// one classical RK4 step of length h
ATTPC_FIT_HD void fit_rk4(double s[6], const FitSpecies& sp, const double* tab, double h) {
#pragma clang fp contract(off)
  const double hh = 0.5 * h, h6 = h / 6.0;
  double k1[6], k2[6], k3[6], k4[6], y[6];
  fit_rhs(s, sp, tab, k1);
  for (int i = 0; i < 6; ++i) y[i] = s[i] + hh * k1[i];
  fit_rhs(y, sp, tab, k2);
  for (int i = 0; i < 6; ++i) y[i] = s[i] + hh * k2[i];
  fit_rhs(y, sp, tab, k3);
  for (int i = 0; i < 6; ++i) y[i] = s[i] + h * k3[i];
  fit_rhs(y, sp, tab, k4);
  for (int i = 0; i < 6; ++i) s[i] = s[i] + h6 * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
}

// how the trial ends at sample number `sample` in the state s: 0 = it goes on
ATTPC_FIT_HD int32_t fit_end(const double s[6], const FitSpecies& sp, double length, int32_t sample, int32_t max_steps) {
#pragma clang fp contract(off)
  const bool finite = fit_finite(s[0]) && fit_finite(s[1]) && fit_finite(s[2]) && fit_finite(s[3]) && fit_finite(s[4]) &&
                      fit_finite(s[5]);
  if (!finite) return ATTPC_FIT_END_NOT_FINITE;
  if (fit_ke(s[3], s[4], s[5], sp.mass) <= FIT_KE_LIMIT) return ATTPC_FIT_END_STOPPED;
  if (s[2] < 0.0 || s[2] > length || s[0] * s[0] + s[1] * s[1] >= FIT_RHO_MAX2) return ATTPC_FIT_END_LEFT;
  if (sample >= max_steps) return ATTPC_FIT_END_STEP_CAP;
  return 0;
}

struct FitTrial {
  int32_t steps, end, n_inside;
  double path;
};

// The trial of q = (gx, gy, gz, x0, y0, z0) past the n points pts[i] = (x, y, z) in metres: the residual of every point
// goes to res[3 i ..].  One cursor: point c is data point c for gz >= 0 and n - 1 - c otherwise.
ATTPC_FIT_HD FitTrial fit_trial(const double q[6], const FitSpecies& sp, const double* tab, const double* pts, int32_t n,
                                double h, int32_t max_steps, double length, double* res) {
#pragma clang fp contract(off)
  double s[6] = {q[3], q[4], q[5], q[0], q[1], q[2]};
  const bool up = q[2] >= 0.0;
  const double sg = up ? 1.0 : -1.0;
  FitTrial t{0, 0, 0, 0.0};
  int32_t c = 0;
  for (; c < n; ++c) {  // the near side of the vertex
    const int32_t i = up ? c : n - 1 - c;
    if (!(sg * pts[3 * i + 2] < sg * s[2])) break;
    res[3 * i] = s[0] - pts[3 * i];
    res[3 * i + 1] = s[1] - pts[3 * i + 1];
    res[3 * i + 2] = s[2] - pts[3 * i + 2];
  }
  t.end = fit_end(s, sp, length, 0, max_steps);
  while (t.end == 0) {
    const double px = s[0], py = s[1], pz = s[2];
    fit_rk4(s, sp, tab, h);
    ++t.steps;
    const double dx = s[0] - px, dy = s[1] - py, dz = s[2] - pz;
    t.path = t.path + sqrt((dx * dx + dy * dy) + dz * dz);
    const double zs = sg * s[2];
    for (; c < n; ++c) {  // the points of the bracket (a tie in z goes to the first bracket that reaches it)
      const int32_t i = up ? c : n - 1 - c;
      const double zc = pts[3 * i + 2];
      if (!(sg * zc <= zs)) break;
      const double w = dz == 0.0 ? 0.0 : (zc - pz) / dz;
      res[3 * i] = (px + w * dx) - pts[3 * i];
      res[3 * i + 1] = (py + w * dy) - pts[3 * i + 1];
      res[3 * i + 2] = 0.0;
      ++t.n_inside;
    }
    t.end = fit_end(s, sp, length, t.steps, max_steps);
  }
  for (; c < n; ++c) {  // beyond the last sample
    const int32_t i = up ? c : n - 1 - c;
    res[3 * i] = s[0] - pts[3 * i];
    res[3 * i + 1] = s[1] - pts[3 * i + 1];
    res[3 * i + 2] = s[2] - pts[3 * i + 2];
  }
  return t;
}

ATTPC_FIT_HD double fit_dot(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// acc[0 .. 27] += the terms of point i; res: the seven trials' residuals, trial k at res + k * stride
ATTPC_FIT_HD void fit_point(const double* res, int64_t stride, int32_t i, const double delta[6], double acc[FIT_SUMS]) {
#pragma clang fp contract(off)
  double r0[3], J[6][3];
  for (int c = 0; c < 3; ++c) r0[c] = res[3 * i + c];
  for (int k = 0; k < 6; ++k)
    for (int c = 0; c < 3; ++c) J[k][c] = (res[(int64_t)(k + 1) * stride + 3 * i + c] - r0[c]) / delta[k];
  acc[0] = acc[0] + fit_dot(r0, r0);
  for (int k = 0; k < 6; ++k) acc[1 + k] = acc[1 + k] + fit_dot(J[k], r0);
  int at = 7;
  for (int k = 0; k < 6; ++k)
    for (int l = k; l < 6; ++l, ++at) acc[at] = acc[at] + fit_dot(J[k], J[l]);
}

struct FitEval {
  double s[FIT_SUMS];
  FitTrial trial;  // trial 0
};

// the step d of (N + lambda diag N) d = -J^T r by elimination without pivoting; false: a pivot is not > 0
ATTPC_FIT_HD bool fit_step(const double s[FIT_SUMS], double lambda, double d[6]) {
#pragma clang fp contract(off)
  double A[6][6], b[6];
  int at = 7;
  for (int k = 0; k < 6; ++k)
    for (int l = k; l < 6; ++l, ++at) {
      A[k][l] = s[at];
      A[l][k] = s[at];
    }
  for (int k = 0; k < 6; ++k) {
    A[k][k] = A[k][k] + lambda * A[k][k];
    b[k] = -s[1 + k];
  }
  bool ok = true;
  for (int p = 0; p < 6; ++p) {
    const double piv = A[p][p];
    ok = ok && piv > 0.0;
    for (int r = p + 1; r < 6; ++r) {
      const double l = A[r][p] / piv;
      for (int c = p; c < 6; ++c) A[r][c] = A[r][c] - l * A[p][c];
      b[r] = b[r] - l * b[p];
    }
  }
  for (int p = 5; p >= 0; --p) {
    double v = b[p];
    for (int c = p + 1; c < 6; ++c) v = v - A[p][c] * d[c];
    d[p] = v / A[p][p];
  }
  return ok;
}

ATTPC_FIT_HD double fit_norm3(const double* v) {
#pragma clang fp contract(off)
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// the steps of the six difference quotients for the start q
ATTPC_FIT_HD void fit_deltas(const double q[6], double delta[6]) {
#pragma clang fp contract(off)
  const double dg = fit_norm3(q) * FIT_DELTA_MOMENTUM;
  delta[0] = dg;
  delta[1] = dg;
  delta[2] = dg;
  delta[3] = FIT_DELTA_POSITION;
  delta[4] = FIT_DELTA_POSITION;
  delta[5] = FIT_DELTA_POSITION;
}

// The start q from an estimate record; false: a value is not finite (NO_START)
ATTPC_FIT_HD bool fit_start(const attpc_track_estimate& e, const FitSpecies& sp, double q[6]) {
#pragma clang fp contract(off)
  const double gmag = FIT_P_PER_BRHO * sp.charge * e.brho / sp.mass;
  const double b = e.slope;
  const double w = sqrt(1.0 + b * b);
  const double st = 1.0 / w, ct = b / w;
  const double nx = (e.vx - e.cx) / e.radius, ny = (e.vy - e.cy) / e.radius;
  double tx = -ny, ty = nx;
  const double along = tx * (e.x_mean - e.vx) + ty * (e.y_mean - e.vy);
  if (along < 0.0) {
    tx = -tx;
    ty = -ty;
  }
  q[0] = gmag * st * tx;
  q[1] = gmag * st * ty;
  q[2] = gmag * ct;
  q[3] = e.vx / 1000.0;
  q[4] = e.vy / 1000.0;
  q[5] = e.vz / 1000.0;
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && fit_finite(q[k]);
  return ok;
}

// What the fit of a track starts from: 0 and q, or the status of the record without a fit.  `given`: the caller's start
// [6] in the place of the one made of the estimate, or nullptr.
ATTPC_FIT_HD int32_t fit_begin(const attpc_track_estimate& e, bool has_species, const FitSpecies& sp, const double* given,
                               double q[6]) {
  if (e.status & ATTPC_EST_EMPTY) return ATTPC_FIT_EMPTY;
  if (e.status & ATTPC_EST_FEW) return ATTPC_FIT_FEW;
  if (!has_species) return ATTPC_FIT_NO_START;
  bool ok = true;
  if (given) {
    for (int i = 0; i < 6; ++i) {
      q[i] = given[i];
      ok = ok && fit_finite(q[i]);
    }
  } else {
    ok = fit_start(e, sp, q);
  }
  return ok ? 0 : ATTPC_FIT_NO_START;
}

// a record without a fit
ATTPC_FIT_HD void fit_no_fit(int32_t status, int32_t n_points, attpc_track_fit* r) {
  const double nan = __builtin_nan("");
  r->status = status;
  r->evaluations = 0;
  r->n_points = n_points;
  r->n_inside = 0;
  r->steps = 0;
  r->end = 0;
  r->f = nan;
  r->lambda = nan;
  for (int k = 0; k < 3; ++k) {
    r->g[k] = nan;
    r->vertex[k] = nan;
  }
  r->ke = nan;
  r->brho = nan;
  r->path = nan;
  r->reserved[0] = 0.0;
  r->reserved[1] = 0.0;
}

// The iteration from the start q on n_points points; evaluate(q, delta) gives the 28 sums there in the contract's order
// of summation and trial 0.  On the device every lane of a track runs this with the same values.  `status`: the bits
// the record has already (CAPPED).
template <typename Evaluate>
ATTPC_FIT_HD void fit_iterate(const double start[6], const FitSpecies& sp, const attpc_fit_desc& d, int32_t n_points,
                              int32_t status, Evaluate&& evaluate, attpc_track_fit* r) {
#pragma clang fp contract(off)
  double q[6], delta[6];
  for (int k = 0; k < 6; ++k) q[k] = start[k];
  fit_deltas(q, delta);
  FitEval k = evaluate(q, delta);
  int32_t evaluations = 1;
  double lambda = FIT_LAMBDA0;
  bool converged = false, singular = false;
  while (evaluations < d.max_evaluations) {
    double step[6], qt[6];
    if (!fit_step(k.s, lambda, step)) {
      singular = true;
      break;
    }
    bool finite = true;
    for (int i = 0; i < 6; ++i) {
      qt[i] = q[i] + step[i];
      finite = finite && fit_finite(qt[i]);
    }
    const FitEval kt = evaluate(qt, delta);
    ++evaluations;
    if (kt.s[0] <= k.s[0] && finite) {  // (a NaN fails the comparison)
      for (int i = 0; i < 6; ++i) q[i] = qt[i];
      k = kt;
      lambda = FIT_LAMBDA_ACCEPT * lambda;
      if (fit_norm3(step) <= d.tolerance_momentum * fit_norm3(q) && fit_norm3(step + 3) <= d.tolerance_position) {
        converged = true;
        break;
      }
    } else {
      lambda = FIT_LAMBDA_REJECT * lambda;
    }
  }
  const double gmag = fit_norm3(q);
  r->status = status | (singular ? ATTPC_FIT_SINGULAR : 0) | (!converged && !singular ? ATTPC_FIT_NOT_CONVERGED : 0) |
              (k.trial.end == ATTPC_FIT_END_STEP_CAP ? ATTPC_FIT_STEP_CAP : 0);
  r->evaluations = evaluations;
  r->n_points = n_points;
  r->n_inside = k.trial.n_inside;
  r->steps = k.trial.steps;
  r->end = k.trial.end;
  r->f = k.s[0];
  r->lambda = lambda;
  for (int i = 0; i < 3; ++i) {
    r->g[i] = q[i];
    r->vertex[i] = q[3 + i] * 1000.0;
  }
  r->ke = sp.mass * (sqrt(1.0 + gmag * gmag) - 1.0);
  r->brho = gmag * sp.mass / (FIT_P_PER_BRHO * sp.charge);
  r->path = k.trial.path;
  r->reserved[0] = 0.0;
  r->reserved[1] = 0.0;
}

// data point j of n_used used rows: the used row it is taken from (the rule of CAPPED)
ATTPC_FIT_HD int64_t fit_point_row(int64_t j, int64_t n_used) {
  return n_used > ATTPC_FIT_MAX_POINTS ? j * n_used / ATTPC_FIT_MAX_POINTS : j;
}
// used row u of n_used: the data point it becomes, or -1
ATTPC_FIT_HD int32_t fit_row_point(int64_t u, int64_t n_used) {
  if (n_used <= ATTPC_FIT_MAX_POINTS) return (int32_t)u;
  const int64_t j = (u * ATTPC_FIT_MAX_POINTS + n_used - 1) / n_used;
  return j < ATTPC_FIT_MAX_POINTS && j * n_used / ATTPC_FIT_MAX_POINTS == u ? (int32_t)j : -1;
}

// One evaluation on the host in the contract's order: the seven trials one after the other into res [7][3 n], then
// eight accumulators, point i to accumulator i mod 8 in ascending i, then the xor tree over the eight.
inline FitEval fit_evaluate_lanes(const double q[6], const double delta[6], const FitSpecies& sp, const double* tab,
                                  const double* pts, int32_t n, const attpc_fit_desc& d, double length, double* res) {
#pragma clang fp contract(off)
  FitEval out;
  const int64_t stride = 3 * (int64_t)n;
  for (int k = 0; k < 7; ++k) {
    double qk[6];
    for (int i = 0; i < 6; ++i) qk[i] = q[i];
    if (k > 0) qk[k - 1] = qk[k - 1] + delta[k - 1];
    const FitTrial t = fit_trial(qk, sp, tab, pts, n, d.time_step, d.max_steps, length, res + k * stride);
    if (k == 0) out.trial = t;
  }
  double lane[FIT_LANES][FIT_SUMS], next[FIT_LANES][FIT_SUMS];
  for (int l = 0; l < FIT_LANES; ++l) {
    for (int a = 0; a < FIT_SUMS; ++a) lane[l][a] = 0.0;
    for (int32_t i = l; i < n; i += FIT_LANES) fit_point(res, stride, i, delta, lane[l]);
  }
  for (int off = FIT_LANES / 2; off > 0; off >>= 1) {
    for (int l = 0; l < FIT_LANES; ++l)
      for (int a = 0; a < FIT_SUMS; ++a) next[l][a] = lane[l][a] + lane[l ^ off][a];
    for (int l = 0; l < FIT_LANES; ++l)
      for (int a = 0; a < FIT_SUMS; ++a) lane[l][a] = next[l][a];
  }
  for (int a = 0; a < FIT_SUMS; ++a) out.s[a] = lane[0][a];
  return out;
}

}  // namespace attpc
