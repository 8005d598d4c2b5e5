#pragma once
#include "common.h"

namespace spp {

// The HBM replay ring (rltoolkit/buffer/replay_buffer.py: MetaReplayBuffer's obs-index ring + the
// BufferAcMOffPolicy timestep arrays).  Observations are stored once per obs slot, row-major.  Everything
// else a timestep holds is ONE 64-B-aligned record of rw 32-bit words, so a sampled transition reads one
// record segment and two obs rows instead of seven scattered arrays (8-B obs / next indices, 4-B reward,
// 1-B done, the action and ACM rows, each touching its own 64-B line):
//   word 0  obs slot            word 1  next-obs slot        word 2  reward (fp32 bits)
//   word 3  done (bit 0) | end (bit 8)
//   words 4 .. 4 + ac - 1            the ACM (env) action  (within the first 64 B for ac <= 12)
//   words 4 + ac .. 4 + ac + aout - 1 the actor output the buffer stores as "action"
// obs_idx keeps the obs slot of every timestep as its own array too: the obs statistics read every live
// row through it in order (replay_buffer.py:83-96), where a contiguous index stream is the right layout.
struct ReplayDev {
  float* obs;        // [cap][ob]
  int64_t* obs_idx;  // [cap]
  uint32_t* rec;     // [cap][rw]
  int64_t cap;
  int ob, aout, ac;
  int rw;            // record words: 4 + ac + aout rounded up to 16 (a multiple of 64 B)
  const int* acm_cols;  // AcMTrainer.acm_ob_idx (acm.py:94-99, 260-264): the ob columns of acm_cat, or null
};
constexpr int kRecAcm = 4;  // first ACM word
__host__ __device__ inline int rec_words(int aout, int ac) { return (kRecAcm + ac + aout + 15) / 16 * 16; }
__host__ __device__ inline int rec_act(const ReplayDev& r) { return kRecAcm + r.ac; }  // first action word

// Device helpers that the on-policy kernels (onp_rollout.hip) share with replay.hip / stats.hip.
// fkey(): the order-preserving uint32 image of a float (the radix selects' keys); funkey(): its inverse.
__device__ __forceinline__ uint32_t fkey(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// MemoryMeta.normalize / denormalize (rltoolkit/buffer/memory.py:76-127) elementwise
// over [rows][ob], the same fp32 operation order as the fused device helpers:
//   min-max : (x - mid) / (hi - mid + 1e-8)     |  mid + x * (hi - lo) / 2
//   z-score : clamp((x - mean) / (std + 1e-8), -10, 10)  |  (std + 1e-8) * x + mean
__device__ __forceinline__ float obs_norm1(float v, int j, const float* lo, const float* hi, const float* mean,
                                           const float* std, int min_max, int inverse) {
  if (min_max) {
    const float l = lo[j], h = hi[j];
    const float mid = fadd_rn(h, l) * 0.5f;
    return inverse ? fadd_rn(mid, fmul_rn(v, fsub_rn(h, l) * 0.5f))
                   : fdiv_rn(fsub_rn(v, mid), fadd_rn(fsub_rn(h, mid), 1e-8f));
  }
  return inverse ? fadd_rn(fmul_rn(fadd_rn(std[j], 1e-8f), v), mean[j])
                 : fminf(fmaxf(fdiv_rn(fsub_rn(v, mean[j]), fadd_rn(std[j], 1e-8f)), -10.f), 10.f);
}

}  // namespace spp
