// pid.hip -- the particle identification on the device: the estimate records of every event against the gates of the
// positions -> one 16-byte attpc_pid_record per (event, slot) (the contract is in include/attpc_engine.h, "particle
// identification"; the edge rule, the inside test and the assignment walk are pid_host.hpp, shared with the host).
//
// One wave per workgroup and per event; a workgroup takes every gridDim.x-th event.  Lane 8 k + p tests the point of
// slot k against the gate of position p, at most 32 edges; a ballot gives every lane the eight masks at once, and lane
// k < n_sim walks the slots 0 .. k and writes the record of its own slot, so the n_sim records of an event leave as one
// run of 16-byte stores.  The gates (4 KiB, filled at configure time) are staged into LDS once per workgroup, a gate at
// a stride of 33 vertices so that the eight gates the lanes of a slot read start in different banks.
#include "tracks_args.hpp"

#include "pid_host.hpp"

namespace attpc {

namespace {

constexpr int PID_STRIDE = 2 * (ATTPC_PID_MAX_VERTICES + 1);  // doubles from a gate to the next in LDS

}  // namespace

__global__ __launch_bounds__(64) void pid_kernel(PidArgs a) {
  __shared__ double gates[ATTPC_MAX_SIM * PID_STRIDE];
  __shared__ int32_t n_vertices[ATTPC_MAX_SIM];
  __shared__ int32_t species[ATTPC_MAX_SIM];
  const int lane = (int)threadIdx.x, k = lane >> 3, p = lane & 7;
  for (int i = lane; i < ATTPC_MAX_SIM * ATTPC_PID_MAX_VERTICES * 2; i += 64)
    gates[(i >> 6) * PID_STRIDE + (i & 63)] = a.gates->vertices[i];
  if (lane < ATTPC_MAX_SIM) {
    n_vertices[lane] = a.gates->n_vertices[lane];
    species[lane] = a.species[lane];
  }
  __syncthreads();
  const int32_t n = n_vertices[p];
  const bool gate = k < a.n_sim && p < a.n_sim && n >= 3 && (a.mode == ATTPC_PID_ANY || p == k);
  for (uint32_t e = blockIdx.x; e < a.n_events; e += gridDim.x) {
    const size_t first = (size_t)e * (size_t)a.n_sim;
    double x = 0.0, y = 0.0;
    if (k < a.n_sim) {
      const attpc_track_estimate* est = a.estimates + first + k;
      x = est->brho;
      y = est->dedx;
    }
    const bool testable = k < a.n_sim && pid_testable(x, y);
    const bool holds = gate && testable && pid_inside(gates + p * PID_STRIDE, n, x, y);
    const uint64_t held = __ballot(holds);
    const uint64_t tested = __ballot(testable && p == 0);  // bit 8 k: slot k has a point
    if (lane < a.n_sim) {  // (lane k' = lane walks the slots 0 .. k')
      uint32_t testable_bits = 0;
      for (int j = 0; j < ATTPC_MAX_SIM; ++j) testable_bits |= (uint32_t)((tested >> (8 * j)) & 1u) << j;
      a.records[first + lane] = pid_assign_slot(held, testable_bits, lane, species);
    }
  }
}

uint32_t pid_workgroups(uint32_t n_events) { return n_events < PID_MAX_WORKGROUPS ? n_events : PID_MAX_WORKGROUPS; }

void launch_pid(hipStream_t s, const PidArgs& a) {
  hipLaunchKernelGGL(pid_kernel, dim3(pid_workgroups(a.n_events)), dim3(64), 0, s, a);
}

}  // namespace attpc
