// The one-slot block reduction that optim.hip and onp.hip share (included by both, so `inline`).
#pragma once
#include "common.h"

namespace spp {

// Deterministic block reduction of per-tile partial sums (double accumulate).
__device__ inline double block_sum(const float* part, int ntiles, int stride, int slot) {
  __shared__ double red[256];
  double s = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += blockDim.x) s += (double)part[(int64_t)t * stride + slot];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

}  // namespace spp
