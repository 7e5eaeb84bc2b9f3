// host_threads.hpp -- how many worker threads a host-only loop over rows takes (unpack_host.cpp, trace_pack_host.cpp):
// one rule for every n_threads argument of include/attpc_engine.h.  Plain C++17, no HIP.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#if defined(__linux__)
#include <sched.h>
#endif

namespace attpc {

// CPUs this process may really use: the hardware threads, cut down to the scheduler affinity mask and to the CPU
// quota of its control group (a GPU box hands a job 16 of its 256 hardware threads through cpu.max: twice as many
// expansion threads as that only take turns)
inline int usable_cpus() {
  static const int cached = [] {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
#if defined(__linux__)
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    long long quota = -1, period = -1;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
      char word[32] = {0};
      if (std::fscanf(f, "%31s %lld", word, &period) == 2 && std::strcmp(word, "max") != 0) quota = std::atoll(word);
      std::fclose(f);
    } else {  // cgroup v1
      if (FILE* q = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        if (std::fscanf(q, "%lld", &quota) != 1) quota = -1;
        std::fclose(q);
      }
      if (FILE* q = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
        if (std::fscanf(q, "%lld", &period) != 1) period = -1;
        std::fclose(q);
      }
    }
    if (quota > 0 && period > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
#endif
    return n;
  }();
  return cached;
}

inline int pick_threads(int n_threads, int64_t n, int64_t rows_per_thread) {
  // default: up to 32 threads, never more than the CPUs the process may use (half of them on a machine of its own:
  // the other hardware thread of a core adds nothing to a loop of streaming stores); tools/deliver_sweep.py
  if (n_threads <= 0) {
    const int cpus = usable_cpus();
    n_threads = std::min(32, std::max(1, cpus >= 64 ? cpus / 2 : cpus));
  }
  return (int)std::min<int64_t>(n_threads, std::max<int64_t>(1, n / rows_per_thread));
}

}  // namespace attpc
