// Small-batch ("team") forms of the DDPG phase kernels (gfx950) for the vanilla DDPG handles (SPP_ALGO_DDPG,
// rltoolkit/algorithms/ddpg/ddpg.py:239-271): the reference workload is one env, B = 100, 50 grad steps every
// 50 frames, i.e. 4 tiles.  k_ddpg_critic_phase / k_ddpg_actor_phase give each 32-sample tile to one wave;
// here a tile gets a workgroup of TW waves that share the tile's LDS image, built from sac_team.h's blocks
// (dense_team, dense_lds_team, dense1_ksplit, actor_trunk_team, critic_forward_team) under the same
// discipline: every wave computes the replicated per-sample scalars identically (uniform barrier sequence), a
// team barrier separates a layer's last image read from the next write, wave 0 alone writes replicated values
// to HBM.  One tile per workgroup, grid = min(tiles, CUs) (api.hip's ddpg_team).
//
// Same math as the one-wave kernels with ACMC == false and custom_loss == 0 (ddpg.hip); the summation order
// of the q reduction, of the one-block layers and of the fused fc3 weight gradient differs (wave partials in
// fixed order), so the two forms agree within fp32 rounding, not bit for bit.
#pragma once
#include "sac_team.h"
#include "ddpg.hip"

namespace spp {

// waves per tile: the critic phase and the rollout action run 8 (two per SIMD); the actor phase 4 (at 8 its
// live state -- the parked pre-activation tile next to two layers' fragments -- spills 100 VGPRs to scratch)
constexpr int kTeamDCritic = 8, kTeamDActor = 4, kTeamDAct = 8;

// Deterministic head (ddpg_head), team form: every wave reads the fc3 pre-activation tile u from image rows
// [0, AOUT), the team synchronises, every wave writes the same a_d = denormalize(tanh(u) * lim) to those
// rows.  Returns team-synchronised; u keeps the pre-activation.
template <class C>
__device__ __forceinline__ void ddpg_head_team(const SacArgs& p, const Lane& L, f32x16 (&u)[1]) {
  lds_load<1>(u, L.img);
  team_sync();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int ur = ru(q), j = ur + L.h4;
    const bool ok = j < C::AOUT;
    const int jj = ok ? j : 0;
    const float ad = denorm<true>(p, L.tbl, jj, fmul_rn(tanhf(u[0][q]), actor_lim<true>(p, L.tbl, jj)));
    if (ok) L.bl[ur * 32] = ad;
  }
  team_sync();
}

// ============================================================================ critic phase, team form
// ddpg.py:239-258 (targets through the target actor and the target critic) and :303-313 (critic forward, MSE
// backward) -> the critic's weight-gradient operands; fc3's weight gradient fused (TW partial slots per
// workgroup, each wave's own units, zeros elsewhere: k_dw_reduce sums them).
template <class C, int TW = kTeamDCritic>
__global__ __launch_bounds__(TW * 64, 1) void k_ddpg_critic_team(SacArgs p, BAcmScratch) {
  static_assert(!C::ACMC && !C::BF && C::NB_AOUT == 1 && C::NB_CA == 1 && C::OB <= 32,
                "team critic phase: vanilla fp32 shapes");
  __shared__ float img[kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  constexpr int NOW = 8 / TW;
  constexpr int UW = 32 * NOW;  // fc3 units per wave
  __shared__ float red[TW][64];
  __shared__ float s_dq[TW][32];
  __shared__ float part[TW][16][64];
  load_table(p, tbl);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ob0 = NOW * w;
  const int ntiles = p.Bp / 32;
  float w3a = 0.f, b3a = 0.f;  // fused fc3 grads of unit UW*w + lane % UW (bias: wave 0)
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const Lane L = make_lane(img, img + kSmallRow * 32, tbl, p.Bp, tile * 32 + (lane & 31));
    const int b = L.b;
    const bool valid = b < p.B;
    uint32_t d0 = 0, d1 = 0;
    // ---- a' = mu_targ(s')   (ddpg.py:243-244)
    actor_trunk_team<C, false, TW, C::AOUT>(p.actor_targ, p.S2, C::OB * L.ld4, L, w, nullptr, nullptr, part, d0, d1);
    {
      f32x16 u[1];
      ddpg_head_team<C>(p, L, u);
    }
    f32x16 tin[C::NB_CIN];
    load_cat_gl<C::NB_OB, C::NB_CA>(tin, p.S2, C::OB * L.ld4, C::OB, L.ld4, L.vo, img, C::AOUT);
    team_sync();
    // ---- y = r + gamma (1 - d) Q_targ(s', a')   (:245-248)
    const float qt = critic_forward_team<C, false, false, TW>(p.targ[0], tin, L, w, nullptr, nullptr, red, d0, d1);
    const float notdone = 1.f - p.DN[b];
    const float y = fadd_rn(p.R[b], fmul_rn(fmul_rn(p.gamma, notdone), qt));
    // ---- critic forward (H1 stored, h2 in the image), MSE grad   (:303-313)
    uint32_t m1 = 0, m2 = 0;
    f32x16 xin[C::NB_CIN];
    load_cat_gg<C::NB_OB, C::NB_CA>(xin, p.S, C::OB, p.ACT, C::CA, L.ld4, L.vo);
    const CriticDev& Q = p.critic[0];
    const float q = critic_forward_team<C, true, true, TW>(Q, xin, L, w, p.H1[0], nullptr, red, m1, m2);
    const float diff = fsub_rn(q, y);
    const float dq = valid ? fmul_rn(2.f * diff, p.inv_B) : 0.f;
    const float lq = (valid && L.h == 0) ? diff * diff : 0.f;
    // fc3 weight gradient of this wave's units (dW3 = dq . h2^T, db3 = sum dq): h2 rows UW*w .. are this
    // wave's own image rows (k_sac_critic_team)
    if (L.h == 0) s_dq[w][L.s] = dq;
    SPP_XLANE_SYNC();
    {
      constexpr int NS = 32 * UW / 64;
      const int u = UW * w + lane % UW;
      const int s0 = NS * (lane / UW);
      const float* row = img + u * 32;
      float acc = 0.f;
#pragma unroll 8
      for (int j = 0; j < NS; ++j) {
        const int s2 = s0 + ((j + u) & (NS - 1));
        acc = fmaf(row[s2], s_dq[w][s2], acc);
      }
      if constexpr (UW == 32) acc += __shfl_xor(acc, 32, 64);
      w3a += acc;
    }
    b3a += wave_sum(L.h == 0 ? dq : 0.f);
    SPP_XLANE_SYNC();  // own rows rewritten below
    // delta2 = dq * w3 * relu'(h2), own blocks, staged in the image and stored feature-major
    const rsrc_t d2r = rsrc(p.D2[0]);
    const float* w3 = tbl + Q.tw3;
#pragma unroll 1
    for (int k = 0; k < NOW; ++k) {
      const int ob = ob0 + k;
      float tv[16];
      tvals(w3, ob, L.h4, tv);
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2) {
        const int ur = 32 * ob + ru(q2);
        const float v = getown(m2, k, q2) ? dq * tv[q2] : 0.f;
        L.bl[ur * 32] = v;
        fm_st_op(d2r, ur, L.ld4, L.vo, v);
      }
    }
    team_sync();
    // delta1 = (W2^T delta2) * relu'(h1), own blocks
    const rsrc_t d1r = rsrc(p.D1[0]);
    dense_lds_team<NOW, 8, false>(Q.W2T, ob0, img, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2)
        fm_st_op(d1r, 32 * ob + ru(q2), L.ld4, L.vo, getown(m1, ob - ob0, q2) ? acc[q2] : 0.f);
    });
    const float s0 = wave_sum(lq);
    if (w == 0 && lane == 0) p.part[tile * kParts + 0] = s0;
  }
  // this wave's fc3 partials [256 weights | bias]: units UW*w .. (from lanes 0 .. UW-1), zeros elsewhere
  float* o0 = p.W3P[0] + ((int64_t)blockIdx.x * TW + w) * p.w3p_stride;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int idx = lane + 64 * k;
    const bool own = idx / UW == w;
    const float va = __shfl(w3a, idx % UW, 64);
    o0[idx] = own ? va : 0.f;
  }
  if (lane == 0) o0[256] = w == 0 ? b3a : 0.f;
}

// ============================================================================ actor phase, team form
// ddpg.py:260-271: loss = -Q(s, mu(s)).mean(), backward through the updated critic's action input, the
// head's lim * (1 - t^2) and the actor -> ADH / AD2 / AD1 for the k_dw jobs; part slot 2 = sum(-q), slot 3 = 0.
template <class C, int TW = kTeamDActor>
__global__ __launch_bounds__(TW * 64, 1) void k_ddpg_actor_team(SacArgs p, BAcmScratch) {
  static_assert(!C::ACMC && !C::BF && C::NB_AOUT == 1 && C::NB_CA == 1, "team actor phase: vanilla fp32 shapes");
  __shared__ float img[kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  constexpr int NOW = 8 / TW;
  __shared__ float red[TW][64];
  __shared__ float part[TW][16][64];
  load_table(p, tbl);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ob0 = NOW * w;
  const int ntiles = p.Bp / 32;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const Lane L = make_lane(img, img + kSmallRow * 32, tbl, p.Bp, tile * 32 + (lane & 31));
    const int b = L.b;
    const bool valid = b < p.B;
    // ---- a = mu(s)   (ddpg.py:262)
    uint32_t a1 = 0, a2 = 0;
    actor_trunk_team<C, true, TW, C::AOUT>(p.actor, p.S, C::OB * L.ld4, L, w, p.AH1, p.AH2, part, a1, a2);
    f32x16 u[1];  // the fc3 pre-activation, kept through the critic section
    ddpg_head_team<C>(p, L, u);
    // ---- q = Q(s, a)   (:263-264), own-block masks kept for the backward
    uint32_t k1 = 0, k2 = 0;
    const CriticDev& Q = p.critic[0];
    float q;
    {
      f32x16 cin[C::NB_CIN];
      load_cat_gl<C::NB_OB, C::NB_CA>(cin, p.S, C::OB * L.ld4, C::OB, L.ld4, L.vo, img, C::AOUT);
      team_sync();
      q = critic_forward_team<C, false, false, TW>(Q, cin, L, w, nullptr, nullptr, red, k1, k2);
    }
    const float dqv = valid ? -p.inv_B : 0.f;
    // ---- back through the critic to its action input
    const float* w3 = tbl + Q.tw3;
#pragma unroll 1
    for (int k = 0; k < NOW; ++k) {
      const int ob = ob0 + k;
      float tv[16];
      tvals(w3, ob, L.h4, tv);
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2) L.bl[(32 * ob + ru(q2)) * 32] = getown(k2, k, q2) ? dqv * tv[q2] : 0.f;
    }
    team_sync();
    dense_lds_team<NOW, 8, false>(Q.W2T, ob0, img, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2) L.bl[(32 * ob + ru(q2)) * 32] = getown(k1, ob - ob0, q2) ? acc[q2] : 0.f;
    });
    team_sync();
    // d loss / d a (one block, split over the waves by input blocks; every wave the same tile)
    const f32x16 dca = dense1_ksplit<false, TW>(Q.W1Ta, img, nullptr, part, w);
    // ---- head backward: lim * (1 - t^2) (identity denormalisation scale, no custom loss)
    const float ddpg_part = (valid && L.h == 0) ? -q : 0.f;
#pragma unroll
    for (int q2 = 0; q2 < 16; ++q2) {
      const int j = ru(q2) + L.h4;
      const bool ok = j < C::AOUT;
      const int jj = ok ? j : 0;
      const float t = tanhf(u[0][q2]);
      const float lim = actor_lim<true>(p, L.tbl, jj);
      float g_a = 0.f;
      g_a += dca[q2] * denorm_scale<true>(p, L.tbl, jj);
      u[0][q2] = ok ? g_a * lim * (1.f - t * t) : 0.f;
    }
    if (w == 0) {
      const rsrc_t adhr = rsrc(p.ADH);
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2)
        if (ru(q2) + L.h4 < C::AOUT) fm_st(adhr, ru(q2), L.ld4, L.vo, u[0][q2]);
    }
    // ---- dh2 = fc3^T du * relu'(h2) (own blocks); dh1 = W2^T dh2 * relu'(h1)
    // (dense1_ksplit returned team-synchronised: the image is free to write)
    const rsrc_t ad2r = rsrc(p.AD2), ad1r = rsrc(p.AD1);
    dense_team<C::NB_AOUT, C::RV_AOUT, NOW>(p.actor.WhT, ob0, u, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2) {
        const int ur = 32 * ob + ru(q2);
        const float v = getown(a2, ob - ob0, q2) ? acc[q2] : 0.f;
        L.bl[ur * 32] = v;
        fm_st_op(ad2r, ur, L.ld4, L.vo, v);
      }
    });
    team_sync();
    dense_lds_team<NOW, 8, false>(p.actor.W2T, ob0, img, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q2 = 0; q2 < 16; ++q2)
        fm_st_op(ad1r, 32 * ob + ru(q2), L.ld4, L.vo, getown(a1, ob - ob0, q2) ? acc[q2] : 0.f);
    });
    const float pq = wave_sum(ddpg_part);
    if (w == 0 && lane == 0) {
      p.part[tile * kParts + 2] = pq;
      p.part[tile * kParts + 3] = 0.f;
    }
  }
}

// ============================================================================ rollout action, team form
// k_ddpg_policy_act's plain branch (DDPG.noise_action / initial_act / process_action, ddpg.py:171-180,
// 371-383) with the actor trunk of each 32-env tile split over a TW-wave workgroup; every wave computes the
// per-env action, wave 0 writes it.  Same arithmetic as the one-wave form.
template <class C, int TW = kTeamDAct>
__global__ __launch_bounds__(TW * 64, 1) void k_ddpg_policy_act_team(SacArgs p, ActArgs a, BAcmScratch) {
  static_assert(!C::ACMC && C::NB_AOUT == 1 && C::AOUT == C::AC, "team act: vanilla shapes");
  __shared__ float img[kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  __shared__ float part[TW][16][64];
  load_table(p, tbl);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ntiles = (a.E + 31) / 32;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int e = tile * 32 + (lane & 31);
    const bool valid = e < a.E;
    const int er = valid ? e : 0;
    Lane L = make_lane(img, img + kSmallRow * 32, tbl, 1, er * C::OB);  // row-major obs: ld = 1
    f32x16 u[1];
    if (a.mode != 0) {
      uint32_t d0 = 0, d1 = 0;
      actor_trunk_team<C, false, TW, C::AOUT>(p.actor, a.obs, a.E * C::OB * 4, L, w, nullptr, nullptr, part, d0, d1);
      lds_load<1>(u, img);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = ru(q) + L.h4;
      if (j < C::AOUT) {
        const float lim = actor_lim<true>(p, L.tbl, j);
        float act;
        if (a.mode == 0) {
          act = valid ? a.eps[er * C::AOUT + j] : 0.f;  // action_space.sample() drawn by the caller
        } else {
          act = fmul_rn(tanhf(u[0][q]), lim);
          if (a.mode == 1 && a.noise) act = fadd_rn(act, a.act_noise * (valid ? a.noise[er * C::AOUT + j] : 0.f));
          act = fminf(fmaxf(act, -lim), lim);
        }
        if (valid && w == 0) {
          a.target_out[er * C::AOUT + j] = act;
          a.env_out[er * C::AOUT + j] = act;  // process_action: identity
        }
      }
    }
    team_sync();  // the next tile's trunk rewrites the image the head was read from
  }
}

}  // namespace spp
