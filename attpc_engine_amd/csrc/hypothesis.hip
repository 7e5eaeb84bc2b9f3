// hypothesis.hip -- the selection of the fit hypotheses on the device: per event the fit records of every (slot,
// hypothesis) pair -> one 96-byte attpc_fit_hypothesis and one chosen 128-byte attpc_track_fit per slot (the contract is
// in include/attpc_engine.h, "fit hypotheses"; the candidate test, the fitted test, the walk and the record are
// hypothesis_host.hpp, shared with the host).
//
// One lane per event: the walk over the slots of an event is sequential, since a slot takes what no earlier slot took.
// A lane reads at most 64 records of 128 bytes and 8 pid records and writes 8 x (96 + 128 + 16) bytes; comparisons and
// copies only.  The kernel stands behind a fit launch that takes milliseconds and is bound by its launch.
#include "tracks_args.hpp"

#include "hypothesis_host.hpp"

namespace attpc {

__global__ __launch_bounds__(256) void hypothesis_selection_kernel(HypothesisArgs a) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_events) return;
  const size_t first = (size_t)e * (size_t)a.n_sim;
  hypothesis_event(a.l, a.n_sim, a.all + first * (size_t)a.l.n, a.pid ? a.pid + first : nullptr, a.estimates + first,
                   a.records + first, a.fits + first, a.assigned ? a.assigned + first : nullptr);
}

void launch_hypothesis_select(hipStream_t s, const HypothesisArgs& a) {
  hipLaunchKernelGGL(hypothesis_selection_kernel, dim3((a.n_events + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace attpc
