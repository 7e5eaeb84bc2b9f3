// fit.hip -- the track fit on the device: the label's points and the estimate record of every (event, position) -> one
// 128-byte attpc_track_fit (the contract is in include/attpc_engine.h, "track fit"; all of its arithmetic is
// fit_host.hpp, shared with the host).
//
// Eight lanes per track, eight tracks per wave, one wave per workgroup; a workgroup takes every gridDim.x-th group of
// eight tracks (in the instantiation of the fit hypotheses the eight items of a wave are (track, hypothesis) pairs, each
// with its own scratch regions).  Lane k = 0 .. 6 of a track integrates trial k of an evaluation (q, and q with parameter k - 1
// displaced); lane 7 has no trial.  Everything else -- the gather of the points, the 28 sums, the 6x6 step, the
// accept / stop rule -- all eight lanes of the track do together, and the iteration is uniform over them, since every
// lane holds the same sums.
//   Gather: the eight lanes walk the event's rows (or the position's thinned points) in tiles of eight, twice: the count
//   of the used rows, then a used row's rank from a ballot, which says the data point it becomes.  The points go, in
//   metres, to region 7 of the track's scratch.
//   Trial: a lane carries its state in registers and walks the points with one cursor; the residual of every point goes
//   to region k of the track's scratch.  The lanes of a track meet point i at different steps, so the products of J
//   cannot be formed in flight.
//   Sums: lane l takes the points i = l, l + 8, ..; it reads the seven residuals of a point, forms J and adds the 28
//   terms to its accumulators; an xor tree over the eight lanes (offsets 4, 2, 1) ends it.  That is the contract's
//   order of summation.
// The scratch is device memory: 8 regions x 2 048 points x 24 B = 384 KiB per track, 3 MiB per wave, far more than the
// 160 KiB of LDS of a CU; a track's regions are written and read by the same wave within microseconds, so they stay in
// L2.  The stopping-power tables are read from device memory too: a table is 11 KiB, the positions of a layout share a
// few of them, and every lane of a wave reads them at every stage of every step, which keeps them in the CU's cache;
// eight tables in LDS (90 KiB) would hold a CU to one workgroup.
#include "tracks_args.hpp"

#include <type_traits>

#include "estimate_host.hpp"
#include "fit_host.hpp"

namespace attpc {

namespace {

constexpr int64_t FIT_REGION = (int64_t)ATTPC_FIT_MAX_POINTS * 3;  // doubles of one region

struct FitRow {
  int32_t X, Y, Z;
  bool used;
};

// row r (valid: r is inside the span) for the label `target`, as the estimates select it
__device__ __forceinline__ FitRow fit_row(const FitArgs& a, int64_t r, bool valid, int64_t target) {
  FitRow row{0, 0, 0, false};
  if (!valid) return row;
  if (a.points) {
    const ThinPoint p = a.points[r];
    const bool ok = p.si > -2147483648ll && p.si < 2147483648ll;
    row.X = p.X;
    row.Y = p.Y;
    row.Z = p.Z;
    row.used = ok && (int64_t)p.X * p.X + (int64_t)p.Y * p.Y >= a.rb2;
    return row;
  }
  if (a.labels[r] != target) return row;
  const double* p = a.rows + r * 8;
  int64_t I;
  const bool ok = estimate_quantise(p[0], p[1], p[2], p[4], &row.X, &row.Y, &row.Z, &I);
  row.used = ok && (int64_t)row.X * row.X + (int64_t)row.Y * row.Y >= a.rb2;
  return row;
}

__device__ __forceinline__ double fit_group_add(double v) {
#pragma clang fp contract(off)
  for (int off = FIT_LANES / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, FIT_LANES);
  return v;
}

}  // namespace

// the argument block of an instantiation without the hypotheses
template <bool PID>
using FitSlotArgs = std::conditional_t<PID, FitPidArgs, FitArgs>;

// fit_kernel<false> is the fit of "track fit"; fit_kernel<true> is the same body behind the particle identification
// ("particle identification" in the header): the nucleus of slot s is that of the position its pid record names, and a
// slot without one gets the record without a fit, NO_PID.  fit_kernel<false, true> is the same body over the (track,
// hypothesis) pairs of "fit hypotheses": item = track * H + h is fitted as the nucleus of hypothesis h, so the eight
// groups of a wave hold the hypotheses of neighbouring tracks over the same points; an item that is no candidate of
// its slot gets the record without a fit, NO_PID, and leaves.
template <bool PID, bool HYP = false>
__global__ __launch_bounds__(64) void fit_kernel(std::conditional_t<HYP, FitHypArgs, FitSlotArgs<PID>> a) {
  const int lane = (int)threadIdx.x, k = lane & 7, group = lane & ~7;
  const uint32_t below = (1u << k) - 1u;
  uint64_t n_items = (uint64_t)a.n_events * (uint64_t)a.n_sim;
  if constexpr (HYP) n_items *= (uint64_t)a.hyp.n;
  for (uint64_t first = (uint64_t)blockIdx.x * 8; first < n_items; first += (uint64_t)gridDim.x * 8) {
    const uint64_t item = first + (uint64_t)(lane >> 3);
    if (item >= n_items) continue;  // (the eight lanes of an item together)
    uint64_t track = item;
    if constexpr (HYP) track = item / (uint64_t)a.hyp.n;
    const uint32_t e = (uint32_t)(track / (uint64_t)a.n_sim);
    const int s = (int)(track - (uint64_t)e * (uint64_t)a.n_sim);
    attpc_track_fit* out = a.records + item;
    const attpc_track_estimate est = a.estimates[track];
    int at = s;  // the position whose nucleus the track is taken for
    if constexpr (PID) at = a.pid[track].position;
    if constexpr (HYP) {
      const int h = (int)(item - track * (uint64_t)a.hyp.n);
      const bool candidate = (hypothesis_tried(a.hyp, a.pid ? a.pid + track : nullptr) & a.hyp.positions[h]) != 0;
      at = candidate ? a.hyp.first[h] : -1;
    }
    if constexpr (PID || HYP) {
      if (at < 0 || at >= a.n_sim) {
        attpc_track_fit none;
        fit_no_fit(ATTPC_FIT_NO_PID, est.n_used < ATTPC_FIT_MAX_POINTS ? est.n_used : ATTPC_FIT_MAX_POINTS, &none);
        if (k == 0) *out = none;
        continue;
      }
    }
    const FitPosition pos = a.position[at];
    attpc_track_fit rec;
    const int32_t est_points = est.n_used < ATTPC_FIT_MAX_POINTS ? est.n_used : ATTPC_FIT_MAX_POINTS;
    double start[6];
    const FitSpecies sp{pos.mass, pos.charge, pos.qm_b, pos.qm_e, pos.drag};
    const int32_t no_fit = fit_begin(est, pos.table >= 0, sp, a.start ? a.start + track * 6 : nullptr, start);
    if (no_fit) {
      fit_no_fit(no_fit, est_points, &rec);
      if (k == 0) *out = rec;
      continue;
    }
    // ---- gather ----
    double* const region = a.scratch + ((int64_t)blockIdx.x * 8 + (lane >> 3)) * 8 * FIT_REGION;
    double* const pts = region + 7 * FIT_REGION;
    const int64_t target = a.slot_label[s];
    int64_t lo = a.ev_start[e], hi = a.ev_start[e + 1];
    if (a.points) {  // the region of position s, behind the rows of the labels of the positions below it
      const attpc_thin_info* info = a.thin_info + (size_t)e * (size_t)a.n_sim;
      for (int t = 0; t < s; ++t) lo += info[t].n_rows;
      hi = lo + info[s].n_points;
    }
    int64_t n_used = 0;
    for (int64_t base = lo; base < hi; base += 8) {
      const FitRow row = fit_row(a, base + k, base + k < hi, target);
      n_used += __popc((uint32_t)(__ballot(row.used) >> group) & 0xffu);
    }
    int64_t count = 0;
    for (int64_t base = lo; base < hi; base += 8) {
      const FitRow row = fit_row(a, base + k, base + k < hi, target);
      const uint32_t bits = (uint32_t)(__ballot(row.used) >> group) & 0xffu;
      if (row.used) {
        const int32_t j = fit_row_point(count + __popc(bits & below), n_used);
        if (j >= 0) {  // (j < ATTPC_FIT_MAX_POINTS)
          pts[3 * j] = (double)row.X / 16000.0;
          pts[3 * j + 1] = (double)row.Y / 16000.0;
          pts[3 * j + 2] = (double)row.Z / 16000.0;
        }
      }
      count += __popc(bits);
    }
    const int32_t n = (int32_t)(n_used < ATTPC_FIT_MAX_POINTS ? n_used : ATTPC_FIT_MAX_POINTS);
    __threadfence();
    // ---- the iteration, uniform over the track's lanes ----
    const double* tab = a.dedx + (size_t)pos.table * ATTPC_DEDX_NODES;
    auto evaluate = [&](const double* q, const double* delta) {
      FitTrial t{0, 0, 0, 0.0};
      if (k < 7) {
        double qk[6];
        for (int i = 0; i < 6; ++i) qk[i] = i == k - 1 ? q[i] + delta[i] : q[i];
        t = fit_trial(qk, sp, tab, pts, n, a.d.time_step, a.d.max_steps, a.length, region + k * FIT_REGION);
      }
      __threadfence();
      FitEval out;
      out.trial.steps = __shfl(t.steps, 0, FIT_LANES);
      out.trial.end = __shfl(t.end, 0, FIT_LANES);
      out.trial.n_inside = __shfl(t.n_inside, 0, FIT_LANES);
      out.trial.path = __shfl(t.path, 0, FIT_LANES);
      for (int i = 0; i < FIT_SUMS; ++i) out.s[i] = 0.0;
      for (int32_t i = k; i < n; i += FIT_LANES) fit_point(region, FIT_REGION, i, delta, out.s);
#pragma unroll
      for (int i = 0; i < FIT_SUMS; ++i) out.s[i] = fit_group_add(out.s[i]);
      return out;
    };
    fit_iterate(start, sp, a.d, n, n_used > ATTPC_FIT_MAX_POINTS ? ATTPC_FIT_CAPPED : 0, evaluate, &rec);
    if (k == 0) *out = rec;
  }
}

uint32_t fit_workgroups(uint32_t n_events, int32_t n_sim, int32_t n_hyp) {
  const uint64_t groups = ((uint64_t)n_events * (uint64_t)n_sim * (uint64_t)n_hyp + 7) / 8;
  return (uint32_t)(groups < FIT_MAX_WORKGROUPS ? groups : FIT_MAX_WORKGROUPS);
}

void launch_fit_hypotheses(hipStream_t s, const FitArgs& a, const HypLayout& hyp, const attpc_pid_record* pid) {
  FitHypArgs with;
  static_cast<FitArgs&>(with) = a;
  with.pid = pid;
  with.hyp = hyp;
  hipLaunchKernelGGL((fit_kernel<false, true>), dim3(fit_workgroups(a.n_events, a.n_sim, hyp.n)), dim3(64), 0, s, with);
}

void launch_fit(hipStream_t s, const FitArgs& a, const attpc_pid_record* pid) {
  if (pid) {
    FitPidArgs with;
    static_cast<FitArgs&>(with) = a;
    with.pid = pid;
    hipLaunchKernelGGL(fit_kernel<true>, dim3(fit_workgroups(a.n_events, a.n_sim)), dim3(64), 0, s, with);
  } else
    hipLaunchKernelGGL(fit_kernel<false>, dim3(fit_workgroups(a.n_events, a.n_sim)), dim3(64), 0, s, a);
}

}  // namespace attpc
