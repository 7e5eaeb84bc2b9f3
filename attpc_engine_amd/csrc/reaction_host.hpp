// reaction_host.hpp -- the reaction reconstruction (include/attpc_engine.h, "reaction reconstruction") as one piece of
// code for the device and the host: the checks of an attpc_reaction_desc, the beam energy at a vertex, the ejectile's
// momentum from a fit or an estimate record, the missing mass and the centre-of-mass angle, the slot that is read, the
// record of one event and the cells of the spectra it counts in.  reaction.hip runs reaction_event with a lane per
// event and adds the cells with atomics, abi.hip uses the checks, and tests/native/reaction_check.cpp compiles this
// file alone and adds the cells in a plain loop (tests/test_reaction_cpu.py holds it to tests/reaction_reference.py
// byte for byte).
//
// f64 only; + - * / and sqrt, each rounded once in the order written here, never contracted into a fused
// multiply-add; the one angle is helix_atan2w of helix_host.hpp.
#pragma once
#include <stdint.h>

#include "attpc_engine.h"
#include "helix_host.hpp"

#if defined(__HIPCC__)  // (behind the HIP runtime header, which brings sqrt and floor for both sides)
#define ATTPC_REACTION_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define ATTPC_REACTION_HD inline
#endif

namespace attpc {

constexpr double REACTION_PI = 3.141592653589793;         // the upper edge of the angle's bins, and pi - theta
constexpr double REACTION_P_PER_BRHO = 299.792458;        // MeV/c per (T m) and unit charge, as the track fit

ATTPC_REACTION_HD bool reaction_finite(double v) { return v - v == 0.0; }

// the cells of the spectra of a desc: truth, truth_reconstructed, reconstructed, ex_response, outside[3]
ATTPC_REACTION_HD int64_t reaction_cells(int32_t n_ex, int32_t n_theta) {
  return 3 * (int64_t)n_ex * n_theta + (int64_t)n_ex * n_ex + 3;
}

// nullptr, or what is wrong with the settings (a NaN fails the comparisons)
inline const char* reaction_desc_error(const attpc_reaction_desc& d) {
  for (int i = 0; i < 4; ++i)
    if (!(d.masses[i] > 0.0) || !reaction_finite(d.masses[i])) return "masses: finite and > 0";
  if (!(d.beam_energy > 0.0) || !reaction_finite(d.beam_energy)) return "beam_energy: finite and > 0";
  if (d.has_target != 0 && d.has_target != 1) return "has_target: 0 or 1";
  if (d.has_target) {
    if (!reaction_finite(d.z_min) || !reaction_finite(d.z_max) || !(d.z_max > d.z_min)) return "z_min < z_max, finite";
    if (d.eloss_len < 2 || d.eloss_len > ATTPC_REACTION_MAX_ELOSS || !d.eloss) return "eloss: 2 .. 65536 nodes";
    for (int32_t i = 0; i < d.eloss_len; ++i)
      if (!reaction_finite(d.eloss[i])) return "eloss: finite";
  } else if (d.eloss_len != 0) {
    return "eloss_len: 0 without a target";
  }
  if (d.charge < 1) return "charge: >= 1";
  if (d.track < 0 || d.track >= ATTPC_MAX_SIM) return "track: 0 .. 7";
  if (d.observed_row != 2 && d.observed_row != 3) return "observed_row: 2 or 3";
  if (d.source != ATTPC_REACTION_FROM_FIT && d.source != ATTPC_REACTION_FROM_ESTIMATE) return "source: fit or estimate";
  if (d.n_ex < 1 || d.n_ex > ATTPC_REACTION_MAX_EX) return "n_ex: 1 .. 256";
  if (d.n_theta < 1 || d.n_theta > ATTPC_REACTION_MAX_THETA) return "n_theta: 1 .. 180";
  if (!reaction_finite(d.ex_lo) || !reaction_finite(d.ex_hi) || !(d.ex_hi > d.ex_lo)) return "ex_lo < ex_hi, finite";
  if (!(d.ex_inv_width == (double)d.n_ex / (d.ex_hi - d.ex_lo))) return "ex_inv_width: n_ex / (ex_hi - ex_lo)";
  if (!(d.theta_inv_width == (double)d.n_theta / REACTION_PI)) return "theta_inv_width: n_theta / pi";
  if (d.reserved != 0) return "reserved: 0";
  return nullptr;
}

struct ReactionParams {  // an attpc_reaction_desc as the kernel takes it (the table's pointer goes beside it)
  double masses[4];
  double beam_energy;
  double z_min, z_max;
  double ex_lo, ex_hi, ex_inv_width, theta_inv_width;
  int32_t has_target, eloss_len;
  int32_t charge, track, observed_row, source;
  int32_t n_ex, n_theta;
};

inline ReactionParams reaction_params(const attpc_reaction_desc& d) {
  ReactionParams c;
  for (int i = 0; i < 4; ++i) c.masses[i] = d.masses[i];
  c.beam_energy = d.beam_energy;
  c.z_min = d.z_min;
  c.z_max = d.z_max;
  c.ex_lo = d.ex_lo;
  c.ex_hi = d.ex_hi;
  c.ex_inv_width = d.ex_inv_width;
  c.theta_inv_width = d.theta_inv_width;
  c.has_target = d.has_target;
  c.eloss_len = d.eloss_len;
  c.charge = d.charge;
  c.track = d.track;
  c.observed_row = d.observed_row;
  c.source = d.source;
  c.n_ex = d.n_ex;
  c.n_theta = d.n_theta;
  return c;
}

// The projectile's kinetic energy at the vertex z (m): the look-up of eloss_lookup (kinematics.hip), linear in the
// table and extrapolating beyond its ends.  The node is floor(t) held to 0 .. eloss_len - 2, written without a
// conversion of a value outside the int range.
ATTPC_REACTION_HD double reaction_beam_ke(const ReactionParams& c, const double* eloss, double z) {
#pragma clang fp contract(off)
  if (!c.has_target) return c.beam_energy;
  const double t = (z - c.z_min) / (c.z_max - c.z_min) * (double)(c.eloss_len - 1);
  const int32_t last = c.eloss_len - 2;
  const int32_t i = !(t >= 0.0) ? 0 : (t >= (double)last ? last : (int32_t)t);
  const double f = t - (double)i;
  const double loss = eloss[i] + f * (eloss[i + 1] - eloss[i]);
  return c.beam_energy - loss;
}

struct ReactionValue {
  double beam_ke, ex, theta_cm;
  bool physical;  // M^2 > 0 and every value finite
};

// Missing mass and CM angle of the observed nucleus of row `row` (2 or 3) with the momentum (px, py, pz) in MeV/c, for
// the beam energy t_b.
ATTPC_REACTION_HD ReactionValue reaction_value(const ReactionParams& c, double t_b, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double m_t = c.masses[0], m_p = c.masses[1];
  const double m_e = c.masses[c.observed_row], m_r = c.masses[5 - c.observed_row];
  const double e = (t_b + m_p) + m_t;
  const double pb2 = t_b * (t_b + 2.0 * m_p);
  const double pb = sqrt(pb2);
  const double pt2 = px * px + py * py;
  const double p2 = pt2 + pz * pz;
  const double e_e = sqrt(p2 + m_e * m_e);
  const double de = e - e_e;
  const double m2 = de * de - ((pb2 + p2) - (2.0 * pb) * pz);
  const double ex = sqrt(m2) - m_r;
  const double beta = pb / e;
  const double gamma = e / sqrt(e * e - pb2);
  const double pt = sqrt(pt2);
  const double th = helix_atan2w(pt, gamma * (pz - beta * e_e));
  ReactionValue v;
  v.beam_ke = t_b;
  v.theta_cm = c.observed_row == 3 ? REACTION_PI - th : th;
  v.ex = ex;
  v.physical = m2 > 0.0 && reaction_finite(ex) && reaction_finite(v.theta_cm);
  if (!v.physical) {
    v.ex = __builtin_nan("");
    v.theta_cm = __builtin_nan("");
  }
  return v;
}

// the bin of v in n bins from lo to hi, -1: outside (below lo, at or above hi, NaN).  A value below hi whose product
// rounds to n is of the last bin.
ATTPC_REACTION_HD int32_t reaction_bin(double v, double lo, double hi, double inv_width, int32_t n) {
#pragma clang fp contract(off)
  if (!(v >= lo && v < hi)) return -1;
  const double b = floor((v - lo) * inv_width);
  return b >= (double)n ? n - 1 : (int32_t)b;
}

// the slot that is read: with pid the first whose position is the track, otherwise the track; -1: none
ATTPC_REACTION_HD int32_t reaction_slot(const ReactionParams& c, const attpc_pid_record* pid, int32_t n_sim) {
  if (!pid) return c.track < n_sim ? c.track : -1;
  for (int32_t s = 0; s < n_sim; ++s)
    if (pid[s].position == c.track) return s;
  return -1;
}

struct ReactionCells {  // the cells an event counts in, -1: none; indices into the spectra of reaction_cells()
  int64_t cell[4];
};

// One event: fits / estimates / pid are its n_sim records (the source's not nullptr, pid may be), p4_row the truth
// 4-vector (px, py, pz, E) of the observed row, vertex_z the truth vertex z in m, kin_status the kinematics status.
ATTPC_REACTION_HD ReactionCells reaction_event(const ReactionParams& c, const double* eloss, const attpc_track_fit* fits,
                                               const attpc_track_estimate* estimates, const attpc_pid_record* pid,
                                               int32_t n_sim, const double* p4_row, double vertex_z, int32_t kin_status,
                                               attpc_reaction_record* r) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  const int32_t slot = reaction_slot(c, pid, n_sim);
  int32_t status = 0;
  double px = nan, py = nan, pz = nan, z = nan;
  bool have = slot >= 0;
  if (have && c.source == ATTPC_REACTION_FROM_FIT) {
    const attpc_track_fit& f = fits[slot];
    have = !(f.status & (ATTPC_FIT_EMPTY | ATTPC_FIT_FEW | ATTPC_FIT_NO_START | ATTPC_FIT_NO_PID));
    const double m_e = c.masses[c.observed_row];
    px = m_e * f.g[0];
    py = m_e * f.g[1];
    pz = m_e * f.g[2];
    z = f.vertex[2] / 1000.0;
  } else if (have) {
    const attpc_track_estimate& e = estimates[slot];
    have = !(e.status & (ATTPC_EST_EMPTY | ATTPC_EST_FEW));
    const double pmag = REACTION_P_PER_BRHO * (double)c.charge * e.brho;
    const double b = e.slope;
    const double w = sqrt(1.0 + b * b);
    const double st = 1.0 / w, ct = b / w;
    px = pmag * st;
    py = 0.0;
    pz = pmag * ct;
    z = e.vz / 1000.0;
  }
  have = have && reaction_finite(px) && reaction_finite(py) && reaction_finite(pz) && reaction_finite(z);
  ReactionValue rec{nan, nan, nan, false};
  if (!have) {
    status |= ATTPC_REACTION_NO_TRACK;
  } else {
    if (c.has_target && !(z >= c.z_min && z <= c.z_max)) status |= ATTPC_REACTION_OUTSIDE_TARGET;
    rec = reaction_value(c, reaction_beam_ke(c, eloss, z), px, py, pz);
    if (!rec.physical) status |= ATTPC_REACTION_UNPHYSICAL;
  }
  ReactionValue truth{nan, nan, nan, false};
  if (kin_status == 0) truth = reaction_value(c, reaction_beam_ke(c, eloss, vertex_z), p4_row[0], p4_row[1], p4_row[2]);
  if (!truth.physical) {  // (a status 0 whose 4-vector gives no value has no truth either)
    status |= ATTPC_REACTION_NO_TRUTH;
    truth.beam_ke = nan;
  }
  r->status = status;
  r->slot = slot;
  r->beam_ke = rec.beam_ke;
  r->ex = rec.ex;
  r->theta_cm = rec.theta_cm;
  r->truth_beam_ke = truth.beam_ke;
  r->truth_ex = truth.ex;
  r->truth_theta_cm = truth.theta_cm;
  r->reserved = 0.0;

  const int64_t plane = (int64_t)c.n_ex * c.n_theta, outside = 3 * plane + (int64_t)c.n_ex * c.n_ex;
  ReactionCells k{{-1, -1, -1, -1}};
  const bool has_truth = !(status & ATTPC_REACTION_NO_TRUTH), good = status == 0;
  const int32_t te = reaction_bin(truth.ex, c.ex_lo, c.ex_hi, c.ex_inv_width, c.n_ex);
  const int32_t tt = reaction_bin(truth.theta_cm, 0.0, REACTION_PI, c.theta_inv_width, c.n_theta);
  const int32_t re = reaction_bin(rec.ex, c.ex_lo, c.ex_hi, c.ex_inv_width, c.n_ex);
  const int32_t rt = reaction_bin(rec.theta_cm, 0.0, REACTION_PI, c.theta_inv_width, c.n_theta);
  if (has_truth) {
    const bool in = te >= 0 && tt >= 0;
    k.cell[0] = in ? (int64_t)te * c.n_theta + tt : outside;
    if (in && good) k.cell[1] = plane + (int64_t)te * c.n_theta + tt;
  }
  if (good) {
    k.cell[2] = re >= 0 && rt >= 0 ? 2 * plane + (int64_t)re * c.n_theta + rt : outside + 1;
    k.cell[3] = te >= 0 && re >= 0 ? 3 * plane + (int64_t)te * c.n_ex + re : outside + 2;
  }
  return k;
}

// A batch on the host, sequentially: what reaction_kernel does, the cells added one after the other.
inline void reaction_records_host(const attpc_reaction_desc& d, int64_t n_events, int32_t n_sim, int32_t n_rows,
                                  const attpc_track_fit* fits, const attpc_track_estimate* estimates,
                                  const attpc_pid_record* pid, const double* p4, const double* vertex,
                                  const int32_t* kin_status, attpc_reaction_record* records, uint64_t* cells) {
  const ReactionParams c = reaction_params(d);
  for (int64_t e = 0; e < n_events; ++e) {
    const size_t first = (size_t)e * (size_t)n_sim;
    const ReactionCells k = reaction_event(c, d.eloss, fits ? fits + first : nullptr, estimates ? estimates + first : nullptr,
                                           pid ? pid + first : nullptr, n_sim,
                                           p4 + ((size_t)e * (size_t)n_rows + (size_t)d.observed_row) * 4, vertex[3 * e + 2],
                                           kin_status ? kin_status[e] : 0, &records[e]);
    for (int i = 0; i < 4; ++i)
      if (k.cell[i] >= 0) cells[k.cell[i]] += 1;
  }
}

#if defined(__HIPCC__)
// reaction.hip (the arguments live here and not in tracks_args.hpp: they hold a ReactionParams)
struct ReactionArgs {
  const attpc_track_fit* fits;            // [n_events][n_sim], or nullptr with the estimate source
  const attpc_track_estimate* estimates;  // [n_events][n_sim], or nullptr with the fit source
  const attpc_pid_record* pid;            // [n_events][n_sim], or nullptr: slot = track
  const double* p4;                       // [n_events][n_rows][4] the truth
  const double* vertex;                   // [n_events][3], m
  const int32_t* kin_status;              // [n_events], or nullptr: all 0
  const double* eloss;                    // [c.eloss_len] on the device, nullptr without a target
  attpc_reaction_record* records;         // [n_events]
  unsigned long long* cells;              // [reaction_cells(c.n_ex, c.n_theta)], added to
  ReactionParams c;
  uint32_t n_events;                      // > 0
  int32_t n_sim;                          // 1 .. ATTPC_MAX_SIM
  int32_t n_rows;                         // 4 .. ATTPC_MAX_ROWS
};
// a lane per event
void launch_reaction(hipStream_t s, const ReactionArgs& a);
#endif

}  // namespace attpc
