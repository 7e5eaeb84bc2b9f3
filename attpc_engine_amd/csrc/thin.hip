// thin.hip -- thinned track points on the device: an event's labelled Spyral rows -> one charge-weighted centroid per
// run of equal z bin for every position of layout->indices (the contract is in include/attpc_engine.h, "thinned track
// points"; its bin and centroid are thin_host.hpp, its quantisation estimate_host.hpp, both shared with the host).
//
// One workgroup of four waves per event, empty events included; wave w takes the positions w and w + 4.
//   Pass 1 reads the labels only and counts every position's rows; the counts meet in LDS behind the kernel's one
//   barrier.  The region of position s in the chunk's point buffer starts at the event's first row plus the rows of the
//   positions below s: a label has no more points than rows, so the regions cannot meet.
//   Pass 2 walks the event's rows in tiles of 64, a lane per row: the label first, the row only on a match.  A lane is
//   a HEAD if its bin differs from that of the participating lane in front of it (ballot and shuffle; the open run's bin
//   in front of the tile's first) or if it is row 4096 of the open run.  The seven sums of a point come from one
//   segmented inclusive scan over the wave (shuffles, six steps; lanes that take no part hold the neutral element, so
//   a segment is simply head .. next head - 1); the lane in front of the next head holds its segment's sums and writes
//   the point, with the three 64-bit divisions of C(S) -- once per point.  The run that is open at the end of a tile is
//   carried in wave-uniform registers and written by lane 0 when the next head, or the end of the rows, closes it.
// No atomics, no scratch; the row reads of pass 2 are the kernel's traffic (40 B per row of the label, 8 B per row for
// the labels of each pass).
#include "tracks_args.hpp"

#include "estimate_host.hpp"
#include "thin_host.hpp"

namespace attpc {

constexpr int THIN_THREADS = 256;
constexpr int THIN_WAVES = THIN_THREADS / 64;

namespace {

struct ThinSums {  // step 4
  int64_t w, sx, sy, sz, si;
  double amp;
  int32_t n;
};

__device__ __forceinline__ ThinSums thin_add(const ThinSums& a, const ThinSums& b) {
  return ThinSums{a.w + b.w, a.sx + b.sx, a.sy + b.sy, a.sz + b.sz, a.si + b.si, fmax(a.amp, b.amp), a.n + b.n};
}

__device__ __forceinline__ ThinSums thin_from_lane(const ThinSums& v, int src) {
  return ThinSums{__shfl(v.w, src), __shfl(v.sx, src), __shfl(v.sy, src), __shfl(v.sz, src), __shfl(v.si, src),
                  __shfl(v.amp, src), __shfl(v.n, src)};
}

// inclusive scan of v over the lanes seg0 .. lane of every lane
__device__ __forceinline__ ThinSums thin_segmented_scan(ThinSums v, int lane, int seg0) {
  for (int off = 1; off < 64; off <<= 1) {
    const ThinSums up{__shfl_up(v.w, off), __shfl_up(v.sx, off), __shfl_up(v.sy, off), __shfl_up(v.sz, off),
                      __shfl_up(v.si, off), __shfl_up(v.amp, off), __shfl_up(v.n, off)};
    if (lane - off >= seg0) v = thin_add(v, up);
  }
  return v;
}

// steps 5 and 6: the point of the sums
__device__ __forceinline__ void thin_store(ThinPoint* out, const ThinSums& k, int32_t bin, int32_t split) {
  ThinPoint p;
  p.X = (int32_t)thin_centroid(k.sx, k.w);
  p.Y = (int32_t)thin_centroid(k.sy, k.w);
  p.Z = (int32_t)thin_centroid(k.sz, k.w);
  p.n = k.n;
  p.si = k.si;
  p.amplitude = k.amp;
  p.bin = bin;
  p.split = split;
  *out = p;
}

}  // namespace

__global__ __launch_bounds__(THIN_THREADS) void thin_kernel(ThinArgs a) {
  __shared__ int32_t label_rows[ATTPC_MAX_SIM];
  const uint32_t e = blockIdx.x;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t lo = a.ev_start[e], hi = a.ev_start[e + 1];
  const uint64_t below = (1ull << lane) - 1ull;  // the lanes below this one
  // ---- pass 1: the rows of every position's label ----
  for (int s = wave; s < a.n_sim; s += THIN_WAVES) {
    const int64_t target = a.slot_label[s];
    int32_t count = 0;
    if (target >= 0)
      for (int64_t base = lo; base < hi; base += 64)
        count += __popcll(__ballot(base + lane < hi && a.labels[base + lane] == target));
    if (lane == 0) label_rows[s] = count;
  }
  block_sync();
  // ---- pass 2: the points ----
  for (int s = wave; s < a.n_sim; s += THIN_WAVES) {
    const int64_t target = a.slot_label[s];
    int64_t start = lo;
    for (int t = 0; t < s; ++t) start += label_rows[t];
    ThinPoint* region = a.points + start;
    // the open run (everything here is uniform over the wave)
    bool open = false, from_split = false;  // from_split: it began at a split
    int32_t open_bin = 0;
    ThinSums carry{0, 0, 0, 0, 0, __builtin_nan(""), 0};
    int32_t n_started = 0, n_dropped = 0, n_split = 0;  // n_started: points begun; the open run is point n_started - 1
    if (target >= 0) {
      for (int64_t base = lo; base < hi; base += 64) {
        const int64_t r = base + lane;
        const bool match = r < hi && a.labels[r] == target;
        if (__ballot(match) == 0ull) continue;
        int32_t X = 0, Y = 0, Z = 0;
        int64_t I = 0;
        double amplitude = __builtin_nan("");
        bool part = false;
        if (match) {
          const double* p = a.rows + r * 8;
          part = estimate_quantise(p[0], p[1], p[2], p[4], &X, &Y, &Z, &I);
          amplitude = part ? p[3] : amplitude;
        }
        n_dropped += __popcll(__ballot(match && !part));
        const uint64_t bp = __ballot(part);
        if (bp == 0ull) continue;
        const int32_t bin = thin_bin(Z, a.step);
        // heads: a change of bin against the participating lane in front ...
        const uint64_t before = bp & below;
        const int32_t from = __shfl(bin, before ? 63 - __clzll((long long)before) : lane);
        const bool natural = part && (before ? bin != from : !open || bin != open_bin);
        const uint64_t bn = __ballot(natural);
        // ... and row 4096 of the open run, which can only be among the lanes in front of the first change of bin
        const uint64_t leading = bn ? (bn & (~bn + 1ull)) - 1ull : ~0ull;
        const bool split = part && open && ((leading >> lane) & 1ull) && carry.n + __popcll(before) == ATTPC_THIN_MAX_RUN;
        const uint64_t bs = __ballot(split);  // (one lane at most: the first head of the tile then)
        const uint64_t heads = bn | bs;
        const uint64_t upto = heads & (below | (1ull << lane));
        const int seg0 = upto ? 63 - __clzll((long long)upto) : 0;  // this lane's head, lane 0 in front of the first
        const int64_t w = I > 1 ? I : 1;
        ThinSums v{0, 0, 0, 0, 0, amplitude, 0};
        if (part) v = ThinSums{w, w * X, w * Y, w * Z, I, amplitude, 1};
        v = thin_segmented_scan(v, lane, seg0);
        if (heads == 0ull) {  // (the open run goes on: without one the first participating lane is a head)
          carry = thin_add(carry, thin_from_lane(v, 63));
          continue;
        }
        const int first = __ffsll((long long)heads) - 1;
        const int n_heads = __popcll(heads);
        if (open) {  // the first head closes the open run: its sums and the lanes in front of that head
          ThinSums total = carry;
          if (first > 0) total = thin_add(carry, thin_from_lane(v, first - 1));
          if (lane == 0) thin_store(region + (n_started - 1), total, open_bin, bs != 0ull);
          if (bs != 0ull) n_split += from_split ? 1 : 2;
        }
        // a lane in front of a later head closes its segment
        const int32_t seg_bin = __shfl(bin, seg0);
        if (lane < 63 && lane >= first && ((heads >> (lane + 1)) & 1ull))
          thin_store(region + (n_started + __popcll(upto) - 1), v, seg_bin, 0);
        // the last head's segment stays open
        carry = thin_from_lane(v, 63);
        open_bin = __shfl(seg_bin, 63);
        from_split = bs != 0ull && n_heads == 1;
        open = true;
        n_started += n_heads;
      }
      if (open && lane == 0) thin_store(region + (n_started - 1), carry, open_bin, 0);
    }
    if (lane == 0) a.info[(size_t)e * (size_t)a.n_sim + (size_t)s] = attpc_thin_info{label_rows[s], n_started, n_dropped, n_split};
  }
}

void launch_thin(hipStream_t s, uint32_t n_events, const ThinArgs& a) {
  hipLaunchKernelGGL(thin_kernel, dim3(n_events), dim3(THIN_THREADS), 0, s, a);
}

}  // namespace attpc
