// pid_host.hpp -- the parts of the particle identification (include/attpc_engine.h, "particle identification") that are
// one piece of code for the device and the host: the checks of an attpc_pid_desc, the rule of one edge, the inside test
// of a polygon, which records are tested at all, the assignment walk over the slots of an event -- and a plain
// sequential form of one event on top of them.  pid.hip uses the shared parts on the device, abi.hip the checks on the
// host, and tests/native/pid_check.cpp compiles this file alone (tests/test_pid_cpu.py holds the sequential form to
// tests/pid_reference.py exactly).
//
// The arithmetic of the edge rule is two differences, two products and one more difference per side, each rounded once,
// never contracted into a fused multiply-add: no division, no transcendental, so numpy gives the same bits.
#pragma once
#include <stdint.h>

#include "attpc_engine.h"

#if defined(__HIPCC__)
#define ATTPC_PID_HD __host__ __device__ __forceinline__
#else
#define ATTPC_PID_HD inline
#endif

namespace attpc {

ATTPC_PID_HD bool pid_finite(double v) { return v - v == 0.0; }

// nullptr, or what is wrong with the gates (a NaN fails the comparisons)
inline const char* pid_desc_error(const attpc_pid_desc& d) {
  if (d.mode != ATTPC_PID_ANY && d.mode != ATTPC_PID_OWN) return "mode: ATTPC_PID_ANY or ATTPC_PID_OWN";
  if (d.reserved != 0) return "reserved: 0";
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) {
    const int32_t n = d.n_vertices[p];
    if (n != 0 && (n < 3 || n > ATTPC_PID_MAX_VERTICES)) return "n_vertices: 0 or 3 .. 32";
    for (int v = 0; v < n; ++v)
      if (!pid_finite(d.vertices[p][v][0]) || !pid_finite(d.vertices[p][v][1])) return "vertices: finite";
  }
  return nullptr;
}

// the record's point is tested at all: both coordinates finite and > 0 (a NaN fails the comparison)
ATTPC_PID_HD bool pid_testable(double brho, double dedx) {
  return brho > 0.0 && dedx > 0.0 && pid_finite(brho) && pid_finite(dedx);
}

// the edge from (x0, y0) to (x1, y1) counts for the point (x, y)
ATTPC_PID_HD bool pid_edge(double x, double y, double x0, double y0, double x1, double y1) {
#pragma clang fp contract(off)
  if ((y0 > y) == (y1 > y)) return false;
  const double a = (x1 - x0) * (y - y0);
  const double b = (x - x0) * (y1 - y0);
  const double d = a - b;
  return d != 0.0 && (d > 0.0) == (y1 > y0);
}

// the crossing number of the polygon v[0 .. n) (x at [2 i], y at [2 i + 1]), closing edge included, is odd
ATTPC_PID_HD bool pid_inside(const double* v, int32_t n, double x, double y) {
  bool inside = false;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t j = i + 1 < n ? i + 1 : 0;
    if (pid_edge(x, y, v[2 * i], v[2 * i + 1], v[2 * j], v[2 * j + 1])) inside = !inside;
  }
  return inside;
}

// The record of slot k from what the gates said of the event's slots: bit 8 j + p of `held` is set iff the gate of
// position p holds the point of slot j, bit j of `testable` iff slot j has a point.  The walk visits the slots 0 .. k
// in ascending order; a slot takes the lowest position of its mask that no earlier slot took.  species[p] is the
// detector species of position p (-1: none).  On the device lane k runs this for its own slot: every lane holds `held`.
ATTPC_PID_HD attpc_pid_record pid_assign_slot(uint64_t held, uint32_t testable, int k, const int32_t* species) {
  uint32_t taken = 0;
  attpc_pid_record r{-1, -1, 0, 0};
  for (int j = 0; j <= k; ++j) {
    const uint32_t mask = (uint32_t)(held >> (8 * j)) & 0xffu;
    const uint32_t free_bits = mask & ~taken;
    const int32_t position = free_bits ? __builtin_ctz(free_bits) : -1;
    if (position >= 0) taken |= 1u << position;
    if (j < k) continue;
    r.held = (int32_t)mask;
    if (!((testable >> j) & 1u)) {
      r.status = ATTPC_PID_NO_ESTIMATE;
      r.held = 0;
    } else if (mask == 0) {
      r.status = ATTPC_PID_NONE;
    } else {
      r.status = (position < 0 ? ATTPC_PID_TAKEN : 0) | ((mask & (mask - 1)) ? ATTPC_PID_AMBIGUOUS : 0);
      r.position = position;
      r.species = position >= 0 ? species[position] : -1;
    }
  }
  return r;
}

// One event, sequentially: the estimate records est[0 .. n_sim) against the gates of d -> out[0 .. n_sim).
inline void pid_event_host(const attpc_pid_desc& d, const attpc_track_estimate* est, int32_t n_sim, const int32_t* species,
                           attpc_pid_record* out) {
  uint64_t held = 0;
  uint32_t testable = 0;
  for (int k = 0; k < n_sim; ++k) {
    if (!pid_testable(est[k].brho, est[k].dedx)) continue;
    testable |= 1u << k;
    for (int p = 0; p < n_sim; ++p) {
      if (d.n_vertices[p] < 3 || (d.mode == ATTPC_PID_OWN && p != k)) continue;
      if (pid_inside(&d.vertices[p][0][0], d.n_vertices[p], est[k].brho, est[k].dedx)) held |= 1ull << (8 * k + p);
    }
  }
  for (int k = 0; k < n_sim; ++k) out[k] = pid_assign_slot(held, testable, k, species);
}

}  // namespace attpc
