// straggle_host.hpp -- the kick of the track straggling (include/attpc_engine.h, "track straggling") as one piece of
// code for the device and the host: the checks of an attpc_straggle_desc, the step length and the kick of one recorded
// sample.  Plain C++, + - * / and sqrt only, the three normals are inputs: tracks.hip uses it on the device, abi.hip on
// the host, and tests/native/straggle_check.cpp compiles it alone (tests/test_straggling_cpu.py pins it bit for bit to
// tests/straggle_reference.py).
//
// The model, and what it is not.  First order, Gaussian per step: the direction gets a multiple-scattering kick of
// width theta0 (Rossi-Greisen, without Highland's logarithm, so that the variances of consecutive steps add and the
// result does not depend on the step length), the kinetic energy a Bohr fluctuation of variance Omega^2.  There is no
// single-scattering tail and no Landau tail, and Bohr's variance is too large at low velocity (it ignores the binding
// of the target electrons).  angular_scale and energy_scale exist so that a user can fit the lateral and the range
// straggling of their own SRIM or LISE tables.
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings sqrt and copysign for both sides)
#define ATTPC_STRAGGLE_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_STRAGGLE_HD inline
#endif

namespace attpc {

constexpr double STRAGGLE_C_LIGHT = 299792458.0;           // m / s
constexpr double STRAGGLE_HIGHLAND = 13.6;                 // MeV
constexpr double STRAGGLE_K = 2.605634303273153e-29;       // 4 pi (r_e m_e c^2)^2 in MeV^2 m^2 (detector/constants.py)
constexpr double STRAGGLE_KE_LIMIT = 1e-6;                 // MeV, detector/solver.py:14

// nullptr, or what is wrong with the settings
inline const char* straggle_desc_error(const attpc_straggle_desc& d) {
  // (a NaN fails every comparison)
  if (!(d.angular_scale >= 0.0) || __builtin_isinf(d.angular_scale)) return "angular_scale: finite and >= 0";
  if (!(d.energy_scale >= 0.0) || __builtin_isinf(d.energy_scale)) return "energy_scale: finite and >= 0";
  if (!(d.radiation_length > 0.0) || __builtin_isinf(d.radiation_length)) return "radiation_length: finite and > 0";
  if (!(d.electron_density > 0.0) || __builtin_isinf(d.electron_density)) return "electron_density: finite and > 0";
  if (d.stream >= 65536u) return "stream: < 2^16";
  return nullptr;
}

struct StraggleParams {  // what the kick reads of an attpc_straggle_desc
  double angular_scale, energy_scale, radiation_length, electron_density;
};

// the step length of a sample: gv2 = |gamma beta|^2 of the state at the previous recorded sample, h_sample in s
ATTPC_STRAGGLE_HD double straggle_step_length(double gv2, double h_sample) {
#pragma clang fp contract(off)
  return STRAGGLE_C_LIGHT * sqrt(gv2 / (1.0 + gv2)) * h_sample;
}

// The kick of one sample: g = gamma beta after the step (in and out), mass in MeV, z the charge number, ds in m,
// (n1, n2) the normals of the direction, n3 that of the energy.  A part whose scale is 0 is skipped: its normals are
// not read and the direction / the magnitude keeps its bits; with both scales 0 g is not touched at all.  True: the
// energy was clamped to KE_LIMIT -- the sample sits AT the limit, and its "ke" event function is exactly 0 by
// definition (m (gamma - 1) of the new g minus the limit is a rounding error of either sign), so that the next step
// ends the track through the ordinary event.
ATTPC_STRAGGLE_HD bool straggle_kick(double g[3], double mass, double z, double ds, double n1, double n2, double n3,
                                     const StraggleParams& p) {
#pragma clang fp contract(off)
  const bool angular = p.angular_scale > 0.0, energy = p.energy_scale > 0.0;
  if (!angular && !energy) return false;
  const double xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
  const double g2 = (xx + yy) + zz;
  const double gm = sqrt(g2);
  const double gamma2 = 1.0 + g2;
  const double gamma = sqrt(gamma2);
  double dir[3] = {g[0] / gm, g[1] / gm, g[2] / gm};  // u
  if (angular) {
    const double beta = gm / gamma;
    const double mom = mass * gm;
    const double theta0 = p.angular_scale * (STRAGGLE_HIGHLAND * fabs(z) / (beta * mom)) * sqrt(ds / p.radiation_length);
    // the branch-free orthonormal basis of Duff et al. (JCGT 6(1), 2017)
    const double ux = dir[0], uy = dir[1], uz = dir[2];
    const double sign = copysign(1.0, uz);
    const double a = -1.0 / (sign + uz);
    const double b = ux * uy * a;
    const double e1x = 1.0 + sign * ux * ux * a, e1y = sign * b, e1z = -sign * ux;
    const double e2x = b, e2y = sign + uy * uy * a, e2z = -uy;
    const double t1 = theta0 * n1, t2 = theta0 * n2;
    const double dx = (ux + t1 * e1x) + t2 * e2x;
    const double dy = (uy + t1 * e1y) + t2 * e2y;
    const double dz = (uz + t1 * e1z) + t2 * e2z;
    const double dm = sqrt((dx * dx + dy * dy) + dz * dz);
    dir[0] = dx / dm;
    dir[1] = dy / dm;
    dir[2] = dz / dm;
  }
  double mag = gm;
  bool clamped = false;
  if (energy) {
    const double ke = mass * (g2 / (gamma + 1.0));  // m (gamma - 1) without the cancellation
    const double beta2 = g2 / gamma2;
    const double omega2 = (p.energy_scale * p.energy_scale) * STRAGGLE_K * (z * z) * p.electron_density * ds * gamma2 *
                          (1.0 - 0.5 * beta2);
    const double moved = ke - sqrt(omega2) * n3;
    clamped = !(moved > STRAGGLE_KE_LIMIT);  // (a NaN ends at the limit)
    const double ke_new = clamped ? STRAGGLE_KE_LIMIT : moved;
    const double r = ke_new / mass;
    mag = sqrt(r * (r + 2.0));
  }
  g[0] = mag * dir[0];
  g[1] = mag * dir[1];
  g[2] = mag * dir[2];
  return clamped;
}

}  // namespace attpc
