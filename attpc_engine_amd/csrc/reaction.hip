// reaction.hip -- the reaction reconstruction on the device: per event the record of its one observed track and of its
// truth -> one 64-byte attpc_reaction_record, and the event's counts in the call's spectra (the contract is in
// include/attpc_engine.h, "reaction reconstruction"; the arithmetic, the slot, the status and the cells are
// reaction_host.hpp, shared with the host).
//
// One lane per event.  A lane reads at most n_sim 16-byte pid records, one 128-byte source record, 32 bytes of truth and
// two nodes of the table, and writes 64 bytes: the kernel is bound by its launch, not by its arithmetic (some 120 f64
// operations per event).  An event adds 1 to at most four u64 cells with atomics that return nothing.  A narrow state
// sends most lanes of a wave to one cell; that is a few hundred thousand atomics per chunk at the most, behind a fit
// kernel that takes milliseconds, so equal cells are not pre-aggregated within a wave (profiles/r35_reaction.md).
#include "tracks_args.hpp"

#include "reaction_host.hpp"

namespace attpc {

__global__ __launch_bounds__(256) void reaction_kernel(ReactionArgs a) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_events) return;
  const size_t first = (size_t)e * (size_t)a.n_sim;
  attpc_reaction_record r;
  const ReactionCells k = reaction_event(
      a.c, a.eloss, a.fits ? a.fits + first : nullptr, a.estimates ? a.estimates + first : nullptr,
      a.pid ? a.pid + first : nullptr, a.n_sim, a.p4 + ((size_t)e * (size_t)a.n_rows + (size_t)a.c.observed_row) * 4,
      a.vertex[3 * (size_t)e + 2], a.kin_status ? a.kin_status[e] : 0, &r);
  a.records[e] = r;
  const int64_t n_cells = reaction_cells(a.c.n_ex, a.c.n_theta);
  for (int i = 0; i < 4; ++i)
    if (k.cell[i] >= 0 && k.cell[i] < n_cells) atomicAdd(a.cells + k.cell[i], 1ull);
}

void launch_reaction(hipStream_t s, const ReactionArgs& a) {
  hipLaunchKernelGGL(reaction_kernel, dim3((a.n_events + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace attpc
