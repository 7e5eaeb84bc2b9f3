// hypothesis_host.hpp -- the parts of the fit hypotheses (include/attpc_engine.h, "fit hypotheses") that are one piece
// of code for the device and the host: the check of an attpc_hypothesis_desc, the hypotheses of a layout, the candidate
// test, the fitted test, the walk over the slots of an event with its records -- and a plain sequential form of a batch
// on top of them.  fit.hip uses the candidate test in its instantiation over (track, hypothesis) pairs, hypothesis.hip
// the walk on the device (a lane per event), abi.hip the check and the layout on the host, and
// tests/native/hypothesis_check.cpp compiles this file alone (tests/test_hypothesis_cpu.py holds the sequential form
// to tests/hypothesis_reference.py exactly).
//
// f is only ever compared and copied: no arithmetic on it, so there is nothing to round and nothing to contract.
#pragma once
#include <stdint.h>

#include "attpc_engine.h"
#include "fit_host.hpp"  // (fit_no_fit: the record without a fit)

#if defined(__HIPCC__)
#define ATTPC_HYP_HD __host__ __device__ __forceinline__
#else
#define ATTPC_HYP_HD inline
#endif

namespace attpc {

// nullptr, or what is wrong with the settings
inline const char* hypothesis_desc_error(const attpc_hypothesis_desc& d) {
  if (d.candidates == 0) return "candidates: at least one position";
  if (d.candidates < 0 || d.candidates >> ATTPC_MAX_SIM) return "candidates: bits 0 .. 7";
  if (d.reserved != 0) return "reserved: 0";
  return nullptr;
}

struct HypLayout {                      // the hypotheses of a call's layout with the settings' mask
  int32_t n;                            // H
  int32_t candidates;                   // the settings' mask AND the positions < n_sim with a species
  int32_t first[ATTPC_MAX_SIM];         // hypothesis h: its first position (whose nucleus its fits take), -1 behind H
  int32_t positions[ATTPC_MAX_SIM];     // hypothesis h: the bit mask of its positions
  int32_t of_position[ATTPC_MAX_SIM];   // position p: its hypothesis, -1: none
  int32_t species[ATTPC_MAX_SIM];       // position p: its detector species, -1: none
};

// species[p]: the detector species of position p < n_sim, -1: none
inline HypLayout hypothesis_layout(const int32_t* species, int32_t n_sim, int32_t candidates) {
  HypLayout l{};
  for (int p = 0; p < ATTPC_MAX_SIM; ++p) l.first[p] = l.of_position[p] = l.species[p] = -1;
  int32_t with_species = 0;
  for (int p = 0; p < n_sim && p < ATTPC_MAX_SIM; ++p) {
    if (species[p] < 0) continue;
    l.species[p] = species[p];
    with_species |= 1 << p;
    int h = 0;
    while (h < l.n && l.species[l.first[h]] != species[p]) ++h;
    if (h == l.n) l.first[l.n++] = p;
    l.positions[h] |= 1 << p;
    l.of_position[p] = h;
  }
  l.candidates = candidates & with_species;
  return l;
}

// the candidates of a slot: `held` is its pid record's, nullptr without the particle identification
ATTPC_HYP_HD int32_t hypothesis_tried(const HypLayout& l, const attpc_pid_record* pid) {
  return pid ? (l.candidates & pid->held) : l.candidates;
}

ATTPC_HYP_HD bool hypothesis_finite(double f) { return f < __builtin_inf() && f > -__builtin_inf(); }  // (a NaN fails both)

// the record of a tried hypothesis can be compared
ATTPC_HYP_HD bool hypothesis_fitted(const attpc_track_fit& r) {
  return !(r.status & (ATTPC_FIT_EMPTY | ATTPC_FIT_FEW | ATTPC_FIT_NO_START)) && hypothesis_finite(r.f);
}

// One event: all [n_sim][l.n] the fit records of every (slot, hypothesis), pid [n_sim] or nullptr, estimates [n_sim]
// (their n_used is the n_points of a record without a fit) -> records [n_sim], fits [n_sim] and, if not nullptr,
// assigned [n_sim]: the positions as pid records, which is how the reaction reconstruction reads them.
ATTPC_HYP_HD void hypothesis_event(const HypLayout& l, int32_t n_sim, const attpc_track_fit* all, const attpc_pid_record* pid,
                                   const attpc_track_estimate* estimates, attpc_fit_hypothesis* records, attpc_track_fit* fits,
                                   attpc_pid_record* assigned) {
  const double nan = __builtin_nan("");
  int32_t taken = 0;
  for (int k = 0; k < n_sim; ++k) {
    attpc_fit_hypothesis r;
    r.position = r.species = -1;
    r.tried = hypothesis_tried(l, pid ? pid + k : nullptr);
    r.fitted = r.status = r.reserved = 0;
    r.f_next = nan;
    const attpc_track_fit* mine = all + (size_t)k * (size_t)l.n;
    int best = -1, choice = -1;  // the fitted position of the lowest f; the same among those not taken
    double f_best = nan, f_choice = nan;
    for (int p = 0; p < ATTPC_MAX_SIM; ++p) {
      r.f[p] = nan;
      if (!((r.tried >> p) & 1)) continue;
      const attpc_track_fit& rec = mine[l.of_position[p]];
      r.f[p] = rec.f;
      if (!hypothesis_fitted(rec)) continue;
      r.fitted |= 1 << p;
      if (best < 0 || rec.f < f_best) {
        best = p;
        f_best = rec.f;
      }
      if (!((taken >> p) & 1) && (choice < 0 || rec.f < f_choice)) {
        choice = p;
        f_choice = rec.f;
      }
    }
    if (r.tried == 0) r.status |= ATTPC_HYP_NO_CANDIDATE;
    if (r.fitted == 0) r.status |= ATTPC_HYP_NO_FIT;
    if (r.fitted != 0 && choice < 0) r.status |= ATTPC_HYP_TAKEN;
    if (choice >= 0) {
      taken |= 1 << choice;
      r.position = choice;
      r.species = l.species[choice];
      if (f_best < f_choice) r.status |= ATTPC_HYP_DISPLACED;
      bool other = false;
      for (int p = 0; p < ATTPC_MAX_SIM; ++p)
        if (((r.fitted >> p) & 1) && l.of_position[p] != l.of_position[choice] && (!other || r.f[p] < r.f_next)) {
          other = true;
          r.f_next = r.f[p];
        }
      fits[k] = mine[l.of_position[choice]];
    } else {
      attpc_track_fit none;
      const int32_t n_used = estimates[k].n_used;
      fit_no_fit(ATTPC_FIT_NO_PID, n_used < ATTPC_FIT_MAX_POINTS ? n_used : ATTPC_FIT_MAX_POINTS, &none);
      fits[k] = none;
    }
    records[k] = r;
    if (assigned) assigned[k] = attpc_pid_record{r.position, r.species, r.tried, 0};
  }
}

// A batch on the host, sequentially: what hypothesis_selection_kernel does.
inline void hypothesis_records_host(const HypLayout& l, int64_t n_events, int32_t n_sim, const attpc_track_fit* all,
                                    const attpc_pid_record* pid, const attpc_track_estimate* estimates,
                                    attpc_fit_hypothesis* records, attpc_track_fit* fits) {
  for (int64_t e = 0; e < n_events; ++e) {
    const size_t first = (size_t)e * (size_t)n_sim;
    hypothesis_event(l, n_sim, all + first * (size_t)l.n, pid ? pid + first : nullptr, estimates + first, records + first,
                     fits + first, nullptr);
  }
}

// hypothesis.hip
struct HypothesisArgs {
  HypLayout l;
  const attpc_track_fit* all;             // [n_events][n_sim][l.n]
  const attpc_pid_record* pid;            // [n_events][n_sim], or nullptr
  const attpc_track_estimate* estimates;  // [n_events][n_sim]
  attpc_fit_hypothesis* records;          // [n_events][n_sim]
  attpc_track_fit* fits;                  // [n_events][n_sim]
  attpc_pid_record* assigned;             // [n_events][n_sim] for reaction_kernel, or nullptr
  uint32_t n_events;
  int32_t n_sim;
};

}  // namespace attpc
