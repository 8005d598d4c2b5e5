// The kernel-free part of the C-ABI units' host side: the stream cast, the device-array type, and the few functions
// through which the agent unit (api.hip) reaches the replay unit (api_replay.hip) and the RCCL unit (api_comm.hip).
// api_replay.hip and api_comm.hip include this and not host.h, which carries the agent's kernel headers.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/spprl.h"
#include "common.h"

namespace spp {

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

template <typename T>
struct DevArray {
  T* ptr = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    n = count;
    return hipMalloc(&ptr, sizeof(T) * std::max<size_t>(count, 1));
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
  }
};

// ---- defined in api_replay.hip: the ring of a replay handle (replay.h), and the gather of the rows idx[0, B) into
// the feature-major staging arrays [.][Bp] (act null: not staged)
struct ReplayDev;
const ReplayDev& replay_dev(sppReplayHandle r);
void launch_replay_stage(const ReplayDev& d, const int64_t* idx, int B, int Bp, float* S, float* S2, float* act,
                         float* AENV, float* R, float* DN, hipStream_t st);

// ---- defined in api_comm.hip: librccl resolved; the in-place average of the buffers (pointer, floats) over comm
bool comm_loaded();
sppStatus comm_allreduce_mean(const std::vector<std::pair<float*, int64_t>>& bufs, int world, void* comm,
                              hipStream_t st);

}  // namespace spp
