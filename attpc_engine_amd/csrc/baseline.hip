// baseline.hip -- Spyral's Fourier baseline removal on the device: kept trace rows -> y rows in the traces' own layout,
// which the peak kernels of peaks.hip read as they are (the contract is in include/attpc_engine.h, "Fourier baseline").
//
// One wave per trace row, as in peaks.hip (a workgroup IS one wave): a lane loads 8 consecutive samples (16 bytes, the
// 1 KiB row coalesced), the edge fix is applied there, and the row goes through 1 KiB of LDS into the layout of the
// transform: lane l holds samples 64 r + l in register r.  The peak mask is decided in integers on wave-wide sums, the
// masked samples are replaced by the mean of the others, and
//   baseline = Re(IDFT_512(DFT_512(b) * F))
// is computed in f64 with 8 complex points per lane: radix 8 three times, decimation in frequency forward and
// decimation in time back, so that the permuted order of the spectrum is never undone -- F comes from the host already
// in that order and already divided by 512.  With n = 64 n2 + 8 n1 + n0 and k = k0 + 8 k1 + 64 k2:
//   forward  lane (n1, n0) over n2 -> k0, times W512^((8 n1 + n0) k0); lane (k0, n0) over n1 -> k1, times W64^(n0 k1);
//            lane (k0, k1) over n0 -> k2
//   inverse  the same three steps from the last to the first with the conjugate factors
// A lane pair (a, b) is lane 8 a + b.  Between the steps the points change lanes through LDS, real and imaginary parts
// in arrays of their own; entry (k0, n1, n0) sits at 72 k0 + 8 n1 + n0 and entry (k0, k1, n0) at 72 k0 + 9 k1 + n0, so
// that the reading lanes of a 32-lane half address 32 different 8-byte slots of ds_read_b64's 64-dword bank row.  (A
// ds_write banks by 32 dwords: an 8-byte write of 32 lanes takes two cycles whatever the layout, and these, 32
// different locations spread evenly over the banks, are no worse than a write to consecutive addresses.)
// The twiddle factors are a table of the host (cos and sin of 2 pi j / 512): no sincos here.
//
// A row's y and baseline depend on its 512 samples and on F alone: every row has a transform of its own (no second row
// in the imaginary part) with one order of operations.  Contraction into fused multiply-adds is left on: the contract
// of this stage is a tolerance on the baseline; the one rounding to an integer is a plain rint of the finished value.
#include "tracks_args.hpp"

namespace attpc {

constexpr int BL_LDS = 576;  // 72 * 7 + 9 * 7 + 7 + 1 entries

__device__ __forceinline__ int bl_wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ long long bl_wave_sum(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// X[m] = sum_n x[n] W4^(n m), W4 = -i (INV: +i), in place and in natural order
template <bool INV>
__device__ __forceinline__ void bl_dft4(double& r0, double& i0, double& r1, double& i1, double& r2, double& i2, double& r3,
                                        double& i3) {
  const double cr0 = r0 + r2, ci0 = i0 + i2, dr0 = r0 - r2, di0 = i0 - i2;
  const double cr1 = r1 + r3, ci1 = i1 + i3, tr = r1 - r3, ti = i1 - i3;
  const double dr1 = INV ? -ti : ti, di1 = INV ? tr : -tr;  // (tr, ti) * -i (INV: * i)
  r0 = cr0 + cr1, i0 = ci0 + ci1;
  r2 = cr0 - cr1, i2 = ci0 - ci1;
  r1 = dr0 + dr1, i1 = di0 + di1;
  r3 = dr0 - dr1, i3 = di0 - di1;
}

// X[k] = sum_n x[n] W8^(n k), W8 = exp(-2 pi i / 8) (INV: the conjugate), in place and in natural order
template <bool INV>
__device__ __forceinline__ void bl_dft8(double (&re)[8], double (&im)[8]) {
  constexpr double H = 0.70710678118654752440;
  double ar[4], ai[4], br[4], bi[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    ar[n] = re[n] + re[n + 4];
    ai[n] = im[n] + im[n + 4];
    br[n] = re[n] - re[n + 4];
    bi[n] = im[n] - im[n + 4];
  }
  {  // b[n] *= W8^n
    const double r1 = br[1], i1 = bi[1], r2 = br[2], i2 = bi[2], r3 = br[3], i3 = bi[3];
    br[1] = INV ? (r1 - i1) * H : (r1 + i1) * H;
    bi[1] = INV ? (r1 + i1) * H : (i1 - r1) * H;
    br[2] = INV ? -i2 : i2;
    bi[2] = INV ? r2 : -r2;
    br[3] = INV ? -(r3 + i3) * H : (i3 - r3) * H;
    bi[3] = INV ? (r3 - i3) * H : -(r3 + i3) * H;
  }
  bl_dft4<INV>(ar[0], ai[0], ar[1], ai[1], ar[2], ai[2], ar[3], ai[3]);
  bl_dft4<INV>(br[0], bi[0], br[1], bi[1], br[2], bi[2], br[3], bi[3]);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    re[2 * m] = ar[m], im[2 * m] = ai[m];
    re[2 * m + 1] = br[m], im[2 * m + 1] = bi[m];
  }
}

// (re, im) *= W512^j (INV: its conjugate); t = (cos, sin) of 2 pi j / 512
template <bool INV>
__device__ __forceinline__ void bl_twiddle(double& re, double& im, const double2 t) {
  const double s = INV ? t.y : -t.y;
  const double r = re * t.x - im * s;
  im = re * s + im * t.x;
  re = r;
}

__global__ __launch_bounds__(64) void baseline_kernel(const int16_t* __restrict__ samples, const double2* __restrict__ twiddle,
                                                       const double* __restrict__ filter, int16_t* __restrict__ y,
                                                       double* __restrict__ baseline) {
  __shared__ __attribute__((aligned(16))) short xs[ATTPC_NUM_TB];
  __shared__ double lre[BL_LDS], lim[BL_LDS];
  const int64_t row = blockIdx.x;
  const int lane = (int)threadIdx.x, hi = lane >> 3, lo = lane & 7;
  {  // step a: the row with Spyral's edge fix, into the layout of the transform
    uint4 v = reinterpret_cast<const uint4*>(samples + row * ATTPC_NUM_TB)[lane];
    if (lane == 0) v.x = (v.x & 0xffff0000u) | (v.x >> 16);           // x[0] = x[1]
    if (lane == 63) v.w = (v.w & 0x0000ffffu) | (v.w << 16);          // x[511] = x[510]
    reinterpret_cast<uint4*>(xs)[lane] = v;
  }
  block_sync();
  int x[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) x[r] = xs[64 * r + lane];
  // step b: masked iff 512 x - S > 0 and 4 (512 x - S)^2 > 9 (512 Q - S^2), all in integers
  int part = 0, part_sq = 0;  // (8 * 4095^2 < 2^31)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    part += x[r];
    part_sq += x[r] * x[r];
  }
  const long long S = bl_wave_sum(part), Q = bl_wave_sum((long long)part_sq);
  const long long bound = 9ll * (512ll * Q - S * S);
  uint32_t masked = 0u;
  int rest = 0, n_rest = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const long long d = 512ll * x[r] - S;
    const bool m = d > 0 && 4ll * d * d > bound;
    masked |= m ? 1u << r : 0u;
    rest += m ? 0 : x[r];
    n_rest += m ? 0 : 1;
  }
  // step c: the mean of the others in their place (one rounding; some sample is always at or below the mean)
  const double mean = (double)bl_wave_sum(rest) / (double)bl_wave_sum(n_rest);
  double re[8], im[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    re[r] = (masked >> r & 1u) ? mean : (double)x[r];
    im[r] = 0.0;
  }
  // step d, forward
  bl_dft8<false>(re, im);
#pragma unroll
  for (int k = 1; k < 8; ++k) bl_twiddle<false>(re[k], im[k], twiddle[(lane * k) & (ATTPC_NUM_TB - 1)]);
#pragma unroll
  for (int k = 0; k < 8; ++k) lre[72 * k + lane] = re[k], lim[72 * k + lane] = im[k];
  block_sync();
#pragma unroll
  for (int n = 0; n < 8; ++n) re[n] = lre[72 * hi + 8 * n + lo], im[n] = lim[72 * hi + 8 * n + lo];
  bl_dft8<false>(re, im);
#pragma unroll
  for (int k = 1; k < 8; ++k) bl_twiddle<false>(re[k], im[k], twiddle[8 * lo * k]);
  block_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) lre[72 * hi + 9 * k + lo] = re[k], lim[72 * hi + 9 * k + lo] = im[k];
  block_sync();
#pragma unroll
  for (int n = 0; n < 8; ++n) re[n] = lre[72 * hi + 9 * lo + n], im[n] = lim[72 * hi + 9 * lo + n];
  bl_dft8<false>(re, im);
  // the filter (real, in this order, with the 1 / 512 of the inverse) and back
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double f = filter[64 * k + lane];
    re[k] *= f;
    im[k] *= f;
  }
  bl_dft8<true>(re, im);
#pragma unroll
  for (int n = 1; n < 8; ++n) bl_twiddle<true>(re[n], im[n], twiddle[8 * n * lo]);
  block_sync();
#pragma unroll
  for (int n = 0; n < 8; ++n) lre[72 * hi + 9 * lo + n] = re[n], lim[72 * hi + 9 * lo + n] = im[n];
  block_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) re[k] = lre[72 * hi + 9 * k + lo], im[k] = lim[72 * hi + 9 * k + lo];
  bl_dft8<true>(re, im);
#pragma unroll
  for (int n = 0; n < 8; ++n) bl_twiddle<true>(re[n], im[n], twiddle[((8 * n + lo) * hi) & (ATTPC_NUM_TB - 1)]);
  block_sync();
#pragma unroll
  for (int n = 0; n < 8; ++n) lre[72 * hi + 8 * n + lo] = re[n], lim[72 * hi + 8 * n + lo] = im[n];
  block_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) re[k] = lre[72 * k + lane], im[k] = lim[72 * k + lane];
  bl_dft8<true>(re, im);  // re[r]: the baseline at sample 64 r + lane
  // step e
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (baseline) baseline[row * ATTPC_NUM_TB + 64 * r + lane] = re[r];
    int v = x[r] - (int)rint(re[r]);
    v = v < -4095 ? -4095 : (v > 4095 ? 4095 : v);
    xs[64 * r + lane] = (short)v;
  }
  block_sync();
  reinterpret_cast<uint4*>(y + row * ATTPC_NUM_TB)[lane] = reinterpret_cast<const uint4*>(xs)[lane];
}

void launch_baseline(hipStream_t s, uint32_t n_rows, const int16_t* samples, const double2* twiddle, const double* filter,
                     int16_t* y, double* baseline) {
  hipLaunchKernelGGL(baseline_kernel, dim3(n_rows), dim3(64), 0, s, samples, twiddle, filter, y, baseline);
}

}  // namespace attpc
