// trace_pack.hip -- the kept pad-trace rows of a chunk as losslessly packed records, format "for64-bitplane-v1" (the
// contract is in include/attpc_engine.h, "packed pad traces"; tests/trace_pack_reference.py restates it in numpy).
// The kernels read the int16 [rows][512] samples the trace write pass left in HBM; nothing in traces.hip knows of them.
//
// Both passes: one wave per row, TP_WAVES waves per workgroup, grid-stride over the rows, no LDS.  Lane l loads sample
// l of each of the row's eight blocks of 64 -- 128 contiguous bytes per block across the wave -- so the eight values
// it holds are exactly one bit position of the eight blocks' plane words.
//   trace_pack_size_kernel   per block the minimum and the maximum over the wave: the pair (v, 4095 - v) sits in one
//                            register as two u16 and a packed 16-bit minimum reduces both at once, six xor steps per
//                            block; the base is the minimum, lowered to 4096 - 2^w where the contract says so.
//                            Leaves the row's eight headers (16 bytes, kept for the write pass) and its
//                            record size.
//   (a scan of the sizes -- peaks.hip's -- gives the chunk-relative offsets; the host reads their total)
//   trace_pack_write_kernel  reads the headers back, builds plane k of block b as __ballot(bit k of v - base) in loops
//                            whose bounds are wave-uniform, hands word n of the record to lane n mod 64 (words 0 and 1
//                            are the headers), and stores the record with one 8-byte store per lane and round of 64
//                            words (98 words at most: two rounds), coalesced.  The wave then rebases its row's offset
//                            by the bytes of the chunks before (the caller's row_start is absolute within a call).
// A record is written at [row_start[r], row_start[r] + size) with size from the same headers the scan summed, so the
// stores stay inside the `total` bytes the host sized the buffer for.
#include "tracks_args.hpp"

namespace attpc {

constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / 64;
constexpr int TP_BLOCKS = ATTPC_NUM_TB / 64;

typedef unsigned short tp_u16x2 __attribute__((ext_vector_type(2)));

// the eight samples of lane `lane`: v[b] = row[64 b + lane]
__device__ __forceinline__ void tp_load_row(const int16_t* __restrict__ row, int lane, uint32_t (&v)[TP_BLOCKS]) {
  const unsigned short* p = reinterpret_cast<const unsigned short*>(row) + lane;
#pragma unroll
  for (int b = 0; b < TP_BLOCKS; ++b) v[b] = p[64 * b];
}

__global__ __launch_bounds__(TP_THREADS) void trace_pack_size_kernel(uint32_t n_rows, const int16_t* __restrict__ samples,
                                                                      uint4* __restrict__ headers,
                                                                      uint32_t* __restrict__ sizes) {
  const int lane = (int)threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)TP_WAVES + (threadIdx.x >> 6));
  const uint32_t stride = gridDim.x * (uint32_t)TP_WAVES;
  for (uint32_t row = wave; row < n_rows; row += stride) {
    uint32_t v[TP_BLOCKS];
    tp_load_row(samples + (size_t)row * ATTPC_NUM_TB, lane, v);
    uint32_t h[TP_BLOCKS];
    uint32_t planes = 0u;
#pragma unroll
    for (int b = 0; b < TP_BLOCKS; ++b) {
      tp_u16x2 m = {(unsigned short)v[b], (unsigned short)(4095u - v[b])};
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)__builtin_bit_cast(uint32_t, m), off);
        m = __builtin_elementwise_min(m, __builtin_bit_cast(tp_u16x2, other));
      }
      const uint32_t lo = m.x, hi = 4095u - (uint32_t)m.y;
      const uint32_t w = 32u - (uint32_t)__clz((int)(hi - lo));  // bit_length: __clz(0) = 32
      const uint32_t base = min(lo, 4096u - (1u << w));         // (the contract's base: minimum + 2^w - 1 may not pass 4095)
      h[b] = (base | (w << 12)) & 0xffffu;
      planes += w;
    }
    if (lane == 0) {
      headers[row] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
      sizes[row] = 16u + 8u * planes;
    }
  }
}

__global__ __launch_bounds__(TP_THREADS) void trace_pack_write_kernel(uint32_t n_rows, const int16_t* __restrict__ samples,
                                                                       const uint4* __restrict__ headers,
                                                                       int64_t* __restrict__ row_start, int64_t base,
                                                                       unsigned char* __restrict__ bytes) {
  const int lane = (int)threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)TP_WAVES + (threadIdx.x >> 6));
  const uint32_t stride = gridDim.x * (uint32_t)TP_WAVES;
  for (uint32_t row = wave; row < n_rows; row += stride) {
    uint32_t v[TP_BLOCKS];
    tp_load_row(samples + (size_t)row * ATTPC_NUM_TB, lane, v);
    const uint4 hq = headers[row];
    const uint32_t hw[4] = {(uint32_t)__builtin_amdgcn_readfirstlane(hq.x), (uint32_t)__builtin_amdgcn_readfirstlane(hq.y),
                            (uint32_t)__builtin_amdgcn_readfirstlane(hq.z), (uint32_t)__builtin_amdgcn_readfirstlane(hq.w)};
    const int64_t at = row_start[row];  // chunk-relative: nobody but this wave touches the entry
    unsigned long long first = 0ull, second = 0ull;  // words lane and 64 + lane of the record
    if (lane == 0) first = (unsigned long long)hw[0] | ((unsigned long long)hw[1] << 32);
    if (lane == 1) first = (unsigned long long)hw[2] | ((unsigned long long)hw[3] << 32);
    uint32_t n = 2u;  // words so far (wave-uniform)
#pragma unroll
    for (int b = 0; b < TP_BLOCKS; ++b) {
      const uint32_t h = (hw[b >> 1] >> (16 * (b & 1))) & 0xffffu;
      const uint32_t d = v[b] - (h & 0xfffu), w = h >> 12;
      for (uint32_t k = 0; k < w; ++k, ++n) {
        const unsigned long long plane = __ballot((d >> k) & 1u);
        if (n < 64u) first = (uint32_t)lane == n ? plane : first;
        else second = (uint32_t)lane == n - 64u ? plane : second;
      }
    }
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(bytes + at);  // (at and the buffer: multiples of 8)
    if ((uint32_t)lane < n) rec[lane] = first;
    if ((uint32_t)lane + 64u < n) rec[lane + 64] = second;
    if (lane == 0) {
      row_start[row] = at + base;
      if (row == n_rows - 1u) row_start[n_rows] += base;
    }
  }
}

void launch_trace_pack_size(hipStream_t s, uint32_t workgroups, uint32_t n_rows, const int16_t* samples, uint4* headers,
                            uint32_t* sizes) {
  hipLaunchKernelGGL(trace_pack_size_kernel, dim3(workgroups), dim3(TP_THREADS), 0, s, n_rows, samples, headers, sizes);
}

void launch_trace_pack_write(hipStream_t s, uint32_t workgroups, uint32_t n_rows, const int16_t* samples, const uint4* headers,
                             int64_t* row_start, int64_t base, unsigned char* bytes) {
  hipLaunchKernelGGL(trace_pack_write_kernel, dim3(workgroups), dim3(TP_THREADS), 0, s, n_rows, samples, headers, row_start,
                     base, bytes);
}

uint32_t trace_pack_workgroups(uint32_t n_rows, uint32_t limit) {
  const uint32_t need = (n_rows + (uint32_t)TP_WAVES - 1u) / (uint32_t)TP_WAVES;
  return need < 1u ? 1u : (need < limit ? need : limit);
}

}  // namespace attpc
