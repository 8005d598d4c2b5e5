// Vanilla PPO's rollout step and running observation normaliser (rltoolkit/algorithms/a2c/a2c.py:144-184,
// buffer/memory.py:283-302).
//
//  k_onp_rollout_act  one launch per rollout step: standardize_and_clip of the raw observations, the policy's
//                     standard-normal draws (Philox / Box-Muller, the values sppRandNormal writes), the actor's
//                     forward from the CANONICAL flat parameters (no packed images: always current), action and
//                     Independent-Normal log-prob with k_onp_act's arithmetic (basic_model.py:32-51).
//                     One 64-lane workgroup per env row, lane j = hidden unit j: the row's work (ob x 64 +
//                     64 x 64 + 64 x aout MACs) is a latency chain, not throughput, so there is no MFMA tile to
//                     fill.  fc1 / fc2: lane j holds row j of the weight matrix in registers and takes the inputs by
//                     v_readlane; fc3: lane k holds column k, one wave sum per output.  No LDS but the noise staging.
//  k_onp_obs_stats    Memory.update_obs_mean_std: column mean and ddof-1 std over the iteration's observations
//                     (each rollout's first observation + every next observation) in fp64, blended into the running
//                     mean / std, and the exact 1st / 99th np.percentile of the frames' obs rows by a 4-pass 8-bit
//                     radix select per order statistic (fkey / funkey, replay.h), max / min into the running pair.
//                     One workgroup per column; plain [rows][ob] arrays.
#pragma once
// (included by api_onp.hip after onp.hip; obs_norm1, fkey / funkey: replay.h; philox, kLogSqrt2PiO: common.h)
#include "layout.h"

namespace spp {

struct OnpRolloutArgs {
  const float* obs;         // [E][ob] raw observations
  const float *mean, *std;  // [ob] running statistics, or both null (no normalisation)
  const float* P;           // canonical actor parameters (log_scale first)
  const float* lim;         // [aout]
  uint64_t seed, offset;    // the Philox stream of sppRandNormal(out, E * aout, seed, offset)
  int E, deterministic;
  float *act, *lp;          // [E][aout], [E] (lp may be null)
  float *xn, *noise;        // [E][ob] normalised obs, [E][aout] draws; nullable
};

__device__ __forceinline__ float lane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

template <int OB, int AOUT>
__global__ __launch_bounds__(64) void k_onp_rollout_act(OnpRolloutArgs p) {
  static_assert(OB <= 64 && AOUT <= 64, "one lane per input / output");
  constexpr int NG = (AOUT + 3) / 4 + 1;  // Philox groups of four a row's AOUT draws can touch
  __shared__ float nz[4 * NG];
  const int e = blockIdx.x, lane = threadIdx.x;
  const float* P = p.P;
  constexpr NetLayout L = onp_actor_layout(OB, AOUT);  // (log_scale = P[0, AOUT))
  const float *W1 = P + L.w(0), *b1 = P + L.b(0), *W2 = P + L.w(1), *b2 = P + L.b(1), *W3 = P + L.w(2), *b3 = P + L.b(2);
  // every weight this lane needs, in flight before the first use
  float w1[OB], w2[64], w3[AOUT];
#pragma unroll
  for (int i = 0; i < OB; ++i) w1[i] = W1[lane * OB + i];
#pragma unroll
  for (int k = 0; k < 64; ++k) w2[k] = W2[lane * 64 + k];
#pragma unroll
  for (int o = 0; o < AOUT; ++o) w3[o] = W3[o * 64 + lane];
  const float bb1 = b1[lane], bb2 = b2[lane];
  // element j of the [E][AOUT] noise = normal j % 4 of Philox group j / 4 (k_rand_normal): this row's groups
  const int64_t j0 = (int64_t)e * AOUT, g0 = j0 >> 2;
  if (!p.deterministic && lane < NG) {
    const u32x4 r = philox(p.seed, p.offset, (uint64_t)(g0 + lane));
    float a, b, c, d;
    box_muller(r.x, r.y, a, b);
    box_muller(r.z, r.w, c, d);
    nz[4 * lane + 0] = a;
    nz[4 * lane + 1] = b;
    nz[4 * lane + 2] = c;
    nz[4 * lane + 3] = d;
  }
  float x = 0.f;
  if (lane < OB) {
    x = p.obs[(int64_t)e * OB + lane];
    if (p.mean) x = obs_norm1(x, lane, nullptr, nullptr, p.mean, p.std, 0, 0);  // standardize_and_clip
    if (p.xn) p.xn[(int64_t)e * OB + lane] = x;
  }
  float a1 = bb1;
#pragma unroll
  for (int i = 0; i < OB; ++i) a1 = fmaf(w1[i], lane_f(x, i), a1);
  const float h1 = tanhf(a1);
  float a2 = bb2;
#pragma unroll
  for (int k = 0; k < 64; ++k) a2 = fmaf(w2[k], lane_f(h1, k), a2);
  const float h2 = tanhf(a2);
  float z = 0.f;
#pragma unroll
  for (int o = 0; o < AOUT; ++o) {
    const float s = wave_sum(w3[o] * h2);
    if (lane == o) z = s;
  }
  __syncthreads();  // the draws
  float lpt = 0.f;
  if (lane < AOUT) {
    const float sc = expf(P[lane]);
    const float mu = fmul_rn(tanhf(z + b3[lane]), p.lim[lane]);
    const float eps = p.deterministic ? 0.f : nz[(int)(j0 - 4 * g0) + lane];
    const float a = p.deterministic ? mu : fadd_rn(mu, fmul_rn(sc, eps));
    const float d = fsub_rn(a, mu);
    lpt = fsub_rn(fsub_rn(fdiv_rn(-fmul_rn(d, d), 2.f * fmul_rn(sc, sc)), logf(sc)), kLogSqrt2PiO);
    p.act[j0 + lane] = a;
    if (p.noise) p.noise[j0 + lane] = eps;
  }
  float lp = 0.f;  // the outputs' terms in order
#pragma unroll
  for (int o = 0; o < AOUT; ++o) lp += lane_f(lpt, o);
  if (lane == 0 && p.lp) p.lp[e] = lp;
}

struct OnpStatsArgs {
  const float* start;  // [n_start][ob] the rollouts' first observations
  const float* next;   // [n_next][ob] every frame's next observation
  const float* obs;    // [n_obs][ob] every frame's observation (the percentiles' rows)
  int64_t n_start, n_next, n_obs;
  int ob, have_minmax;
  double alpha;
  float *mean, *std, *max_obs, *min_obs;  // [ob] running statistics, updated in place
};

__global__ __launch_bounds__(256) void k_onp_obs_stats(OnpStatsArgs a) {
  __shared__ double red[2][256];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[2];  // the select's prefix and remaining rank
  const int c = blockIdx.x, t = threadIdx.x, ob = a.ob;
  // ---- moments of start | next about the first row (a constant column gives exactly 0)
  const int64_t n = a.n_start + a.n_next;
  auto row = [&](int64_t i) { return i < a.n_start ? a.start[i * ob + c] : a.next[(i - a.n_start) * ob + c]; };
  if (n > 0) {
    const double piv = (double)row(0);
    double s = 0.0, ss = 0.0;
    for (int64_t i = t; i < n; i += 256) {
      const double d = (double)row(i) - piv;
      s += d;
      ss += d * d;
    }
    red[0][t] = s;
    red[1][t] = ss;
    __syncthreads();
    if (t == 0) {
      s = ss = 0.0;
      for (int k = 0; k < 256; ++k) {  // a fixed order
        s += red[0][k];
        ss += red[1][k];
      }
      const double mu = s / (double)n;
      const double var = fmax(ss - s * mu, 0.0) / (double)(n - 1);  // torch.std: unbiased (n = 1: nan)
      a.mean[c] = (float)((1.0 - a.alpha) * (piv + mu) + a.alpha * (double)a.mean[c]);
      a.std[c] = (float)((1.0 - a.alpha) * sqrt(var) + a.alpha * (double)a.std[c]);
    }
  }
  // ---- np.percentile(obs, 99 / 1, axis=0), linear: order statistics floor((m - 1) q) and the next
  const int64_t m = a.n_obs;
  if (m <= 0) return;
  float res[2];
  for (int k = 0; k < 2; ++k) {
    const double q = k == 0 ? 0.99 : 0.01;
    const int64_t lo = (int64_t)floor((double)(m - 1) * q);
    float v[2];
    for (int u = 0; u < 2; ++u) {
      const int64_t rank = min(lo + u, m - 1);
      __syncthreads();
      if (t == 0) {
        sel[0] = 0u;
        sel[1] = (uint32_t)rank;
      }
      for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0u;
        __syncthreads();
        const uint32_t prefix = sel[0];
        const uint32_t mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int64_t i = t; i < m; i += 256) {
          const uint32_t key = fkey(a.obs[i * ob + c]);
          if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t == 0) {
          uint32_t r = sel[1], b = 0;
          while (b < 255u && r >= hist[b]) r -= hist[b++];
          sel[0] = prefix | (b << shift);
          sel[1] = r;
        }
        __syncthreads();
      }
      v[u] = funkey(sel[0]);
    }
    res[k] = (float)np_lerp((double)v[0], (double)v[1], np_frac(m, q));  // numpy _lerp
  }
  if (t == 0) {
    a.max_obs[c] = a.have_minmax ? fmaxf(res[0], a.max_obs[c]) : res[0];
    a.min_obs[c] = a.have_minmax ? fminf(res[1], a.min_obs[c]) : res[1];
  }
}

}  // namespace spp
