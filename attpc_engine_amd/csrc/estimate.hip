// estimate.hip -- track estimates of the trace rows on the device: an event's labelled Spyral rows -> one 128-byte
// record per position of layout->indices (the contract is in include/attpc_engine.h, "track estimates of the trace
// rows"; its closed form and quantisation are estimate_host.hpp, shared with the host).
//
// One workgroup of four waves per event, empty events included; the event's rows are contiguous.  Wave w takes the
// positions w and w + 4 on its own: no LDS, no atomics, no barrier.
//   Pass A walks the event's rows in tiles of 64, a lane per row: the label first, x, y, z and the integral only on a
//   match; a ballot of the used rows gives their count and the first and last of them.
//   Pass B walks the rows again from the start row in the direction of travel (sequence number q: row lo + q, or
//   hi - 1 - q for a backward track, so that an ascending lane is always the next row along the track) until m used
//   rows are in.  A used row's rank is the running count plus the popcount of the ballot below its lane; the rows of
//   rank < m are the segment.  The previous segment row's (X, Y) comes by a shuffle from the previous set lane of the
//   segment's ballot, carried across tiles; S from an integer wave prefix sum plus the carry.  Every lane keeps the
//   fourteen sums of its own rows in registers; they are reduced over the wave once, with integer adds.
// The second pass reads the rows of the first again (72 B per row of the label, out of L2).  All lanes evaluate the
// closed form (it is wave-uniform); lane 0 stores the record.
//
// estimate_kernel<true, *> is the same body on thinned points (thin.hip, "thinned track points" in the header): the
// rows of position s are the points of its region of the chunk's point buffer -- every one of them matches --, a point
// is out of range at |SI| >= 2^31, and RANGE is set from the start if thinning dropped a row of the label.
//
// estimate_kernel<*, true> is the same body again with the geometric circle fit behind the Kasa circle ("geometric
// circle fit" in the header; its arithmetic is circle_host.hpp, shared with the host).  Pass B knows every segment
// row's rank, so it parks the row's (u, v) there as one packed word (|u|, |v| <= 10 240 fit int16) in the wave's own
// 8 KiB of LDS: 2 048 points x 4 B x 4 waves = 32 KiB static, in these two instantiations only (with CIRCLE false
// nothing of it is instantiated: those two kernels are instruction for instruction what they were without it).  An
// evaluation is then a lane-strided walk over the parked points (rank i in lane i mod 64, ascending) and nine xor-tree
// reductions; the iteration is wave-uniform, since every lane holds the same sums.  No barrier: a wave reads only what
// it wrote, and the LDS operations of one wave complete in order.
//
// estimate_kernel<*, *, true> is the same body once more with the helix slope behind the circle ("helix slope" in the
// header; its arithmetic is helix_host.hpp, shared with the host).  Once the circle (a, b, R) is in every lane, pass C
// walks the rows as pass B does: a segment lane computes its quantised turning angle about the centre (written
// arctangent: selects, two divisions, no libm), takes the previous segment row's angle as pass B takes (X, Y), gets the
// wrap j, the turn count K by the integer wave prefix plus the carry, and the unwrapped angle; a ballot covers the cap;
// four integer sums, reduced once.  No f64 sum, nothing parked: the rows are read a third time out of L2.  With HELIX
// false nothing of it is instantiated: those four kernels are instruction for instruction what they were.
#include "tracks_args.hpp"

#include "circle_host.hpp"
#include "estimate_host.hpp"
#include "helix_host.hpp"

namespace attpc {

constexpr int EST_THREADS = 256;
constexpr int EST_WAVES = EST_THREADS / 64;

namespace {

struct EstRow {
  int32_t X, Y, Z;
  int64_t I;
  bool match, used, out_of_range;
};

// row r of the chunk for the label `target` (valid: r is a row of the event); POINTS: point r of the point buffer
// (valid: r is a point of the position's region)
template <bool POINTS>
__device__ __forceinline__ EstRow est_row(const EstimateArgs& a, int64_t r, bool valid, int64_t target) {
  EstRow row{0, 0, 0, 0, false, false, false};
  if constexpr (POINTS) {
    row.match = valid;
    if (valid) {
      const ThinPoint p = a.points[r];
      // (estimate_quantise of the point row: the coordinates are in range by construction, SI is an integer)
      const bool ok = p.si > -2147483648ll && p.si < 2147483648ll;
      row.X = ok ? p.X : 0;
      row.Y = ok ? p.Y : 0;
      row.Z = ok ? p.Z : 0;
      row.I = ok ? p.si : 0;
      row.out_of_range = !ok;
      row.used = ok && (int64_t)row.X * row.X + (int64_t)row.Y * row.Y >= a.rb2;
    }
    return row;
  }
  row.match = valid && a.labels[r] == target;
  if (row.match) {
    const double* p = a.rows + r * 8;
    const bool ok = estimate_quantise(p[0], p[1], p[2], p[4], &row.X, &row.Y, &row.Z, &row.I);
    row.out_of_range = !ok;
    row.used = ok && (int64_t)row.X * row.X + (int64_t)row.Y * row.Y >= a.rb2;
  }
  return row;
}

struct EstSpan {
  int64_t lo, hi;  // the rows to walk
  bool range;      // RANGE is set before any of them is read
};

// the event's rows; POINTS: the region of position s, behind the rows of the labels of the positions below it
template <bool POINTS>
__device__ __forceinline__ EstSpan est_span(const EstimateArgs& a, uint32_t e, int s, int64_t ev_lo, int64_t ev_hi) {
  if constexpr (POINTS) {
    const attpc_thin_info* info = a.thin_info + (size_t)e * (size_t)a.n_sim;
    int64_t lo = ev_lo;
    for (int t = 0; t < s; ++t) lo += info[t].n_rows;
    return EstSpan{lo, lo + info[s].n_points, info[s].n_dropped != 0};
  }
  return EstSpan{ev_lo, ev_hi, false};
}

__device__ __forceinline__ int64_t est_wave_add(int64_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// inclusive prefix of v over the wave
__device__ __forceinline__ int32_t est_wave_inclusive(int32_t v, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const int32_t up = __shfl_up(v, off);
    v += lane >= off ? up : 0;
  }
  return v;
}

__device__ __forceinline__ double est_wave_add(double v) {
#pragma clang fp contract(off)
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// one evaluation of the circle fit on the wave's m parked points
__device__ __forceinline__ CircleSums est_circle_evaluate(const uint32_t* parked, int32_t m, int lane, double a, double b,
                                                          double R) {
  CircleSums k = circle_zero();
  for (int32_t i = lane; i < m; i += 64) {
    const uint32_t word = parked[i];
    circle_point((int16_t)(word & 0xffffu), (int16_t)(word >> 16), a, b, R, &k);
  }
  return CircleSums{est_wave_add(k.f),  est_wave_add(k.uu), est_wave_add(k.uv), est_wave_add(k.vv), est_wave_add(k.u),
                    est_wave_add(k.v),  est_wave_add(k.gu), est_wave_add(k.gv), est_wave_add(k.g)};
}

// CIRCLE: the wave's ATTPC_EST_MAX_FIT words of LDS (static, in the instantiations that ask for them only)
template <bool CIRCLE>
__device__ __forceinline__ uint32_t* est_parked(int wave) {
  if constexpr (CIRCLE) {
    __shared__ uint32_t parked[EST_WAVES][ATTPC_EST_MAX_FIT];
    return parked[wave];
  }
  return nullptr;
}

}  // namespace

template <bool POINTS, bool CIRCLE, bool HELIX>
__global__ __launch_bounds__(EST_THREADS) void estimate_kernel(EstimateArgs a) {
  const uint32_t e = blockIdx.x;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t ev_lo = a.ev_start[e], ev_hi = a.ev_start[e + 1];
  const uint64_t below = (1ull << lane) - 1ull;  // the lanes below this one
  [[maybe_unused]] uint32_t* const parked = est_parked<CIRCLE>(wave);
  for (int s = wave; s < a.n_sim; s += EST_WAVES) {
    attpc_track_estimate rec;
    attpc_track_estimate* out = a.records + (size_t)e * (size_t)a.n_sim + (size_t)s;
    const int64_t target = a.slot_label[s];
    // ---- pass A: counts, the first and last used row ----
    int32_t n_rows = 0, n_used = 0;
    const EstSpan span = est_span<POINTS>(a, e, s, ev_lo, ev_hi);
    const int64_t lo = span.lo, hi = span.hi;
    bool range = span.range;
    int64_t first = -1, last = -1;
    int32_t rho_first = 0, rho_last = 0;  // X^2 + Y^2 <= 2 * 5120^2
    if (target >= 0) {
      for (int64_t base = lo; base < hi; base += 64) {
        const EstRow row = est_row<POINTS>(a, base + lane, base + lane < hi, target);
        const uint64_t bm = __ballot(row.match), bu = __ballot(row.used);
        if (bm == 0ull) continue;
        n_rows += __popcll(bm);
        range = range || __ballot(row.out_of_range) != 0ull;
        if (bu == 0ull) continue;
        n_used += __popcll(bu);
        const int32_t rho = row.X * row.X + row.Y * row.Y;
        const int l0 = __ffsll((long long)bu) - 1, l1 = 63 - __clzll((long long)bu);
        if (first < 0) {
          first = base + l0;
          rho_first = __shfl(rho, l0);
        }
        last = base + l1;
        rho_last = __shfl(rho, l1);
      }
    }
    if (n_used < a.min_points) {  // (uniform over the wave, as everything above)
      estimate_no_fit(n_rows, n_used, range, &rec);
      if (lane == 0) *out = rec;
      continue;
    }
    const int32_t direction = rho_first <= rho_last ? 1 : -1;
    int32_t m = (n_used + 1) / 2 > a.min_points ? (n_used + 1) / 2 : a.min_points;
    const bool capped = m > ATTPC_EST_MAX_FIT;
    m = capped ? ATTPC_EST_MAX_FIT : m;
    // ---- pass B: the segment's sums ----
    const int64_t n = hi - lo;
    const int64_t q0 = direction > 0 ? first - lo : hi - 1 - last;  // the start row: rank 0, lane 0 of the first tile
    const EstRow origin = est_row<POINTS>(a, direction > 0 ? first : last, true, target);
    int64_t su = 0, sv = 0, suu = 0, suv = 0, svv = 0, suuu = 0, suvv = 0, svvv = 0, svuu = 0;
    int64_t ss = 0, sw = 0, sss = 0, ssw = 0, si = 0;
    int32_t count = 0, arc = 0;                  // segment rows so far, S of the last of them
    int32_t prev_x = origin.X, prev_y = origin.Y;  // (X, Y) of the last of them
    for (int64_t qb = q0; qb < n && count < m; qb += 64) {
      const int64_t q = qb + lane;
      const EstRow row = est_row<POINTS>(a, direction > 0 ? lo + q : hi - 1 - q, q < n, target);
      const uint64_t bu = __ballot(row.used);
      if (bu == 0ull) continue;
      const bool seg = row.used && count + __popcll(bu & below) < m;
      const uint64_t bs = __ballot(seg);  // (never empty: count < m and the tile has a used row)
      const uint64_t before = bs & below;
      const int src = before ? 63 - __clzll((long long)before) : lane;
      const int32_t from_x = __shfl(row.X, src), from_y = __shfl(row.Y, src);
      const int32_t px = before ? from_x : prev_x, py = before ? from_y : prev_y;
      const int32_t d = seg ? estimate_step(row.X - px, row.Y - py) : 0;  // (rank 0: the origin itself, d = 0)
      const int32_t incl = est_wave_inclusive(d, lane);
      if (seg) {
        const int64_t u = row.X - origin.X, v = row.Y - origin.Y, w = row.Z - origin.Z, S = arc + incl;
        if constexpr (CIRCLE)  // (the rank is < m <= ATTPC_EST_MAX_FIT)
          parked[count + __popcll(bu & below)] = ((uint32_t)u & 0xffffu) | ((uint32_t)v << 16);
        su += u;
        sv += v;
        suu += u * u;
        suv += u * v;
        svv += v * v;
        suuu += u * u * u;
        suvv += u * v * v;
        svvv += v * v * v;
        svuu += v * u * u;
        ss += S;
        sw += w;
        sss += S * S;
        ssw += S * w;
        si += row.I;
      }
      const int top = 63 - __clzll((long long)bs);
      arc += __shfl(incl, 63);
      prev_x = __shfl(row.X, top);
      prev_y = __shfl(row.Y, top);
      count += __popcll(bs);
    }
    EstimateSums k;
    k.m = m;
    k.x0 = origin.X;
    k.y0 = origin.Y;
    k.z0 = origin.Z;
    k.su = est_wave_add(su);
    k.sv = est_wave_add(sv);
    k.suu = est_wave_add(suu);
    k.suv = est_wave_add(suv);
    k.svv = est_wave_add(svv);
    k.suuu = est_wave_add(suuu);
    k.suvv = est_wave_add(suvv);
    k.svvv = est_wave_add(svvv);
    k.svuu = est_wave_add(svuu);
    k.ss = est_wave_add(ss);
    k.sw = est_wave_add(sw);
    k.sss = est_wave_add(sss);
    k.ssw = est_wave_add(ssw);
    k.si = est_wave_add(si);
    k.arc = arc;
    rec.n_rows = n_rows;
    rec.n_used = n_used;
    rec.n_fit = m;
    rec.status = (range ? ATTPC_EST_RANGE : 0) | (capped ? ATTPC_EST_CAPPED : 0);
    rec.direction = direction;
    rec.reserved = 0;
    if constexpr (HELIX) {
      // step 6 up to the circle, which stays in registers: (a, b, R) in every lane
      double ca, cb, cR;
      bool circle;
      if constexpr (CIRCLE)
        circle = helix_step6(k, a.magnetic_field, true, a.circle_tolerance, a.circle_max_evaluations,
                             [&](double ta, double tb, double tr) { return est_circle_evaluate(parked, m, lane, ta, tb, tr); },
                             &rec, &ca, &cb, &cR);
      else
        circle = helix_step6(k, a.magnetic_field, false, 0.0, 0, [](double, double, double) { return circle_zero(); }, &rec,
                             &ca, &cb, &cR);
      if (!circle) {
        rec.status |= ATTPC_EST_NO_HELIX;
      } else {
        // ---- pass C: the segment's turning angles about the centre, walked as pass B walks ----
        const double p0x = -ca, p0y = -cb;
        int64_t sp = 0, spp = 0, spw = 0, sww = 0;
        int32_t done = 0, turns = 0, prev_phi = 0;  // segment rows so far, K and phi_q of the last of them
        bool no_helix = false;
        for (int64_t qb = q0; qb < n && done < m; qb += 64) {
          const int64_t q = qb + lane;
          const EstRow row = est_row<POINTS>(a, direction > 0 ? lo + q : hi - 1 - q, q < n, target);
          const uint64_t bu = __ballot(row.used);
          if (bu == 0ull) continue;
          const bool seg = row.used && done + __popcll(bu & below) < m;
          const uint64_t bs = __ballot(seg);
          const uint64_t before = bs & below;
          const int src = before ? 63 - __clzll((long long)before) : lane;
          bool bad;
          const int32_t phi = helix_phi(p0x, p0y, (double)(row.X - origin.X) - ca, (double)(row.Y - origin.Y) - cb, &bad);
          const int32_t from_phi = __shfl(phi, src);
          const int32_t j = seg ? helix_wrap(before ? from_phi : prev_phi, phi) : 0;  // (rank 0: phi = 0 against 0)
          const int32_t K = turns + est_wave_inclusive(j, lane);
          const int32_t unwrapped = phi + HELIX_TURN * K;  // (|K| <= 2047: below 2^30)
          const bool over = seg && (bad || unwrapped >= HELIX_CAP || unwrapped <= -HELIX_CAP);
          no_helix = no_helix || __ballot(over) != 0ull;
          if (seg) {
            const int64_t P = over ? 0 : unwrapped, w = row.Z - origin.Z;
            sp += P;
            spp += P * P;
            spw += P * w;
            sww += w * w;
          }
          turns = __shfl(K, 63);
          prev_phi = __shfl(phi, 63 - __clzll((long long)bs));
          done += __popcll(bs);
        }
        const HelixSums h{est_wave_add(sp), est_wave_add(spp), est_wave_add(spw), est_wave_add(sww), no_helix};
        helix_closed_form(k, h, a.helix_regressor, a.magnetic_field, ca, cb, cR, &rec);
      }
    } else if constexpr (CIRCLE) {
      // (the iteration is uniform over the wave: every lane holds the same sums)
      estimate_closed_form_circle(k, a.magnetic_field, a.circle_tolerance, a.circle_max_evaluations,
                                  [&](double ta, double tb, double tr) { return est_circle_evaluate(parked, m, lane, ta, tb, tr); },
                                  &rec);
    } else {
      estimate_closed_form(k, a.magnetic_field, &rec);
    }
    if (lane == 0) *out = rec;
  }
}

// (the instantiations of the helix slope first, then the refining ones: the two others then lie in the code object as
//  they did without them)
void launch_helix_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a, bool points, bool circle) {
  if (points && circle)
    hipLaunchKernelGGL((estimate_kernel<true, true, true>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
  else if (circle)
    hipLaunchKernelGGL((estimate_kernel<false, true, true>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
  else if (points)
    hipLaunchKernelGGL((estimate_kernel<true, false, true>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((estimate_kernel<false, false, true>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
}

void launch_circle_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a, bool points) {
  if (points)
    hipLaunchKernelGGL((estimate_kernel<true, true, false>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((estimate_kernel<false, true, false>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
}

void launch_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a) {
  hipLaunchKernelGGL((estimate_kernel<false, false, false>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
}

void launch_point_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a) {
  hipLaunchKernelGGL((estimate_kernel<true, false, false>), dim3(n_events), dim3(EST_THREADS), 0, s, a);
}

}  // namespace attpc
