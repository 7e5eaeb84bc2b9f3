// maps.hip -- run maps: pad and time-bucket hit maps accumulated over the events of a resident run (the contract is in
// include/attpc_engine.h, section "run maps").
//
// Behind a chunk's scatter and its summary kernels (summary.hip) -- and, for a selected map, the predicate on their
// records (select.hip) -- the chunk's rows still lie where the scatter left them and summary_fill_kernel has grouped
// the launch's segments by event (seg_start / seg_list).  maps_event_kernel reads the rows once more:
//   - persistent workgroups, one per compute unit; every wave of a workgroup takes events of its own, so a compute
//     unit has 16 events in flight and nothing but the sums is shared between waves: no barrier between events;
//   - a workgroup keeps a whole map of its own in LDS (MapsShared, 150 KiB of the CU's 160 KiB: one workgroup per CU),
//     a wave two bitmaps of the event it has in hand: a row is the first of its event on a pad / in a time bucket iff
//     the word that atomicOr returns had the bit clear, which makes the distinct counts without a pass over the
//     bitmaps; the wave clears them behind the event;
//   - an event that failed the selection is skipped before one of its rows is read;
//   - at the end of the launch a workgroup adds its non-zero cells to the chunk's map in HBM with u64 atomics.
// Every term is an integer, so neither the order of the workgroups nor that of the rows shows in the result.
// A chunk is scattered again when its buffers were too small, and the host learns that only later: the chunk's map is a
// buffer of its slot's own, zeroed in front of every launch, and maps_fold_kernel adds it to the call's totals only once
// the host has accepted the chunk.  A launch that ran out of room (CTRL_OVERFLOW) left segment slots unwritten: the
// event kernel returns at once then, as the summary kernels do, and leaves the zeroed map alone.
#include "tracks_args.hpp"

namespace attpc {

constexpr int MP_THREADS = 1024;                  // threads of maps_event_kernel
constexpr int MP_WAVES = MP_THREADS / 64;         // ... each wave takes events of its own
constexpr int MP_PAD_WORDS = ATTPC_NUM_PADS / 32; // words of an event's pad bitmap
constexpr int MP_TB_WORDS = ATTPC_NUM_TB / 32;    // ... and of its time-bucket bitmap
constexpr int MP_NO_SLOT = 15;

struct MapsEventBits {                            // of the event a wave has in hand
  uint32_t pad[MP_PAD_WORDS];
  uint32_t tb[MP_TB_WORDS];
};
struct MapsShared {
  unsigned long long pad_charge[ATTPC_NUM_PADS];  // 80 KiB
  unsigned long long tb_charge[ATTPC_NUM_TB];
  uint32_t pad_events[ATTPC_NUM_PADS];            // 40 KiB
  uint32_t tb_events[ATTPC_NUM_TB];
  uint32_t tb_rows[ATTPC_NUM_TB];
  MapsEventBits bits[MP_WAVES];                   // 21 KiB
  uint32_t n_hit;
  uint32_t pad_to_8;
};
static_assert(sizeof(MapsShared) <= 163840, "LDS of a CU");
static_assert(sizeof(MapsShared) % 8 == 0 && sizeof(MapsEventBits) % 4 == 0, "cleared in 8-byte / 4-byte words");
// The u32 cells cannot wrap inside one launch.  An event adds at most 1 to a cell of pad_events / tb_events, and a cell
// of tb_rows gets at most one row per pad and event from a scattered chunk (its (pad, time bucket) cells are distinct):
// launch_maps_events refuses a launch in which a workgroup's share of the events, times ATTPC_NUM_PADS, passes this
// bound.  A host cloud may repeat a cell; attpc_cloud_maps takes at most as many rows as the bound in all.
constexpr uint64_t MP_MAX_ROWS_PER_WORKGROUP = 0xffffffffull;

// What a wave wrote to LDS is seen by its other lanes' later LDS instructions: a wave's LDS instructions execute in
// the order they were issued; this keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(MP_THREADS) void maps_event_kernel(MapsArgs a) {
  __shared__ MapsShared sh;
  if (launch_overflowed(a.chunk.ctrl)) return;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  {
    unsigned long long* words = reinterpret_cast<unsigned long long*>(&sh);
    for (int i = t; i < (int)(sizeof(MapsShared) / 8); i += MP_THREADS) words[i] = 0ull;
  }
  block_sync();

  const uint32_t n_segs = launch_segments(a.chunk);
  const uint64_t nib_lo = a.slot_nibbles[0], nib_hi = a.slot_nibbles[1];
  const double min_q = a.min_electrons;
  const uint32_t mask = a.track_mask;
  MapsEventBits& bits = sh.bits[wave];
  uint32_t n_hit = 0u;  // events of this wave with a counted row (the same in every lane)

  // the waves of the launch take the events in turn, one event a wave: nothing of an event is shared between waves but
  // the sums, so there is no barrier in this loop and a CU has MP_WAVES events' loads in flight
  for (uint32_t ev = blockIdx.x * MP_WAVES + wave; ev < a.n_events; ev += gridDim.x * MP_WAVES) {
    if (a.passed != nullptr && a.passed[(size_t)a.event0 + ev] == 0) continue;
    int64_t k0 = a.seg_start[ev], k1 = a.seg_start[ev + 1];
    if (k0 < 0) k0 = 0;
    if (k1 > (int64_t)n_segs) k1 = (int64_t)n_segs;
    bool counted_any = false;
    for (int64_t k = k0; k < k1; ++k) {
      const uint32_t s = a.seg_list[k];
      if (s >= n_segs) continue;
      const Segment sg = a.chunk.segments[s];
      if (sg.count <= 0 || sg.offset < 0 || sg.offset + (int64_t)sg.count > a.chunk.row_capacity) continue;
      const double* __restrict__ rows = a.chunk.points + sg.offset * 3;
      const int64_t* __restrict__ labs = a.chunk.labels + sg.offset;
      for (int i = lane; i < sg.count; i += 64) {
        const double padf = rows[(size_t)3 * i], tau = rows[(size_t)3 * i + 1], q = rows[(size_t)3 * i + 2];
        const long long lab = labs[i];
        int slot = MP_NO_SLOT;
        if (lab >= 0 && lab < 16) slot = (int)((nib_lo >> (4 * (int)lab)) & 15ull);
        else if (lab >= 16 && lab < ATTPC_MAX_ROWS) slot = (int)((nib_hi >> (4 * ((int)lab - 16))) & 15ull);
        if (slot >= a.n_sim) slot = ATTPC_MAX_SIM;  // a label in no position: the mask's last bit
        if (!(q >= min_q) || !((mask >> slot) & 1u)) continue;
        const unsigned long long charge = (unsigned long long)(long long)q;
        const uint32_t pad = (uint32_t)(int)padf;
        const uint32_t tb = (uint32_t)(int)tau;  // tau >= 0: floor
        counted_any = true;
        if (pad < (uint32_t)ATTPC_NUM_PADS) {
          const uint32_t bit = 1u << (pad & 31u);
          if (!(atomicOr(&bits.pad[pad >> 5], bit) & bit)) atomicAdd(&sh.pad_events[pad], 1u);
          atomicAdd(&sh.pad_charge[pad], charge);
        }
        if (tb < (uint32_t)ATTPC_NUM_TB) {
          const uint32_t bit = 1u << (tb & 31u);
          if (!(atomicOr(&bits.tb[tb >> 5], bit) & bit)) atomicAdd(&sh.tb_events[tb], 1u);
          atomicAdd(&sh.tb_rows[tb], 1u);
          atomicAdd(&sh.tb_charge[tb], charge);
        }
      }
    }
    if (__any(counted_any)) {  // (an event without a counted row left the bitmaps clear)
      n_hit += 1u;
      wave_lds_order();  // every row of the event has been counted
      uint32_t* words = reinterpret_cast<uint32_t*>(&bits);
      for (int i = lane; i < (int)(sizeof(MapsEventBits) / 4); i += 64) words[i] = 0u;
      wave_lds_order();  // the wave's next event finds its bitmaps clear
    }
  }
  if (lane == 0 && n_hit) atomicAdd(&sh.n_hit, n_hit);
  block_sync();

  // ---- this workgroup's non-zero cells to the chunk's map ----
  unsigned long long* out = a.map;
  for (int p = t; p < ATTPC_NUM_PADS; p += MP_THREADS) {
    if (sh.pad_events[p]) atomicAdd(&out[MAPS_PAD_EVENTS + p], (unsigned long long)sh.pad_events[p]);
    if (sh.pad_charge[p]) atomicAdd(&out[MAPS_PAD_CHARGE + p], sh.pad_charge[p]);
  }
  for (int b = t; b < ATTPC_NUM_TB; b += MP_THREADS) {
    if (sh.tb_events[b]) atomicAdd(&out[MAPS_TB_EVENTS + b], (unsigned long long)sh.tb_events[b]);
    if (sh.tb_rows[b]) atomicAdd(&out[MAPS_TB_ROWS + b], (unsigned long long)sh.tb_rows[b]);
    if (sh.tb_charge[b]) atomicAdd(&out[MAPS_TB_CHARGE + b], sh.tb_charge[b]);
  }
  if (t == 0 && sh.n_hit) atomicAdd(&out[MAPS_N_HIT], (unsigned long long)sh.n_hit);
}

// total[i] += map[i], i < MAPS_CELLS: one writer per cell, the launches of a stream run one after the other
__global__ __launch_bounds__(256) void maps_fold_kernel(const unsigned long long* __restrict__ map,
                                                       unsigned long long* __restrict__ total) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < (uint32_t)MAPS_CELLS; i += gridDim.x * 256u) {
    const unsigned long long v = map[i];
    if (v) total[i] += v;
  }
}

bool launch_maps_events(hipStream_t s, const MapsArgs& a, uint32_t max_workgroups) {
  if (max_workgroups == 0 || a.n_events == 0) return false;
  const uint32_t n_workgroups = (uint32_t)std::min<uint64_t>(max_workgroups, ((uint64_t)a.n_events + MP_WAVES - 1) / MP_WAVES);
  // a workgroup's share of the launch, at one row per pad and event, stays below 2^32 (the u32 cells of MapsShared)
  const uint64_t per_round = (uint64_t)n_workgroups * MP_WAVES;
  const uint64_t share = (((uint64_t)a.n_events + per_round - 1) / per_round) * MP_WAVES;
  if (share * (uint64_t)ATTPC_NUM_PADS > MP_MAX_ROWS_PER_WORKGROUP) return false;
  hipLaunchKernelGGL(maps_event_kernel, dim3(n_workgroups), dim3(MP_THREADS), 0, s, a);
  return true;
}

void launch_maps_fold(hipStream_t s, const unsigned long long* map, unsigned long long* total) {
  hipLaunchKernelGGL(maps_fold_kernel, dim3((MAPS_CELLS + 255) / 256), dim3(256), 0, s, map, total);
}

}  // namespace attpc
