// SAC_AcM per-sample kernels (gfx950).  One wave = 32 samples; one workgroup
// = 4 waves (one per SIMD), each with a private 32 KiB LDS image [256][32]
// (rows 192..255 double as the SMALL image of the 64-wide ACM layers), plus a
// 16 KiB per-workgroup table of bias / fc3 vectors shared by the 4 waves.
//
//  k_sac_critic_phase   rltoolkit/acm/off_policy/sac_acm.py:30-58 (targets) and
//                       :114-131 (both critics' forward + backward) -> per-sample
//                       operands of the critic weight gradients
//  k_sac_actor_phase    sac_acm.py:60-87 + :137-145 (actor loss through the
//                       frozen ACM and both updated critics) -> actor grad operands
//  k_policy_act         ddpg_acm.py:40-50, off_policy.py:50-54, :89-106 (rollout)
//  k_acm_regress        acm.py:246-258 (ACM regression forward + backward)
#pragma once
#include "sac_kernels.h"

namespace spp {

constexpr float kLog2 = 0.69314718055994530942f;
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;  // math.log(math.sqrt(2*pi))

template <int OB_, int AOUT_, int AC_, bool ACMC_, bool BF_ = false>
struct Cfg {
  static constexpr int OB = OB_, AOUT = AOUT_, AC = AC_;
  static constexpr bool ACMC = ACMC_;
  static constexpr bool BF = BF_;  // bf16 MFMA MLP layers (fp32 accumulation, epilogues and targets)
  // the critics' fc3 weight gradient fused into k_sac_critic_phase (else h2 / dq go to HBM for a k_dw job);
  // bf16 sets: SPP_BF16_FUSE3 (api.hip's build_dw makes the same choice through sac_fuse3())
  static constexpr bool F3 = !BF_ || SPP_BF16_FUSE3;
  static constexpr int NB_OB = blocks_of(OB);
  static constexpr int NB_AOUT = blocks_of(AOUT);
  static constexpr int NB_H2 = blocks_of(2 * AOUT);      // heads output blocks (natural rows mu | logsig)
  static constexpr int NB_PAIR = (AOUT + 15) / 16;        // heads in pairing layout
  static constexpr int CA = ACMC ? AC : AOUT;             // critic action-input width
  static constexpr int NB_CA = blocks_of(CA);
  static constexpr int NB_CIN = NB_OB + NB_CA;
  static constexpr int NB_ACMIN = NB_OB + NB_AOUT;
  static constexpr uint64_t RV_X = rv_nat(OB, NB_OB);
  static constexpr uint64_t RV_H = rv_nat(256, 8);
  static constexpr uint64_t RV_CIN = rv_cat(OB, NB_OB, CA, NB_CA);
  static constexpr uint64_t RV_ACMIN = rv_cat(OB, NB_OB, AOUT, NB_AOUT);
  static constexpr uint64_t RV_Z1 = rv_nat(64, 2);
  static constexpr uint64_t RV_Z2 = rv_nat(32, 1);
  static constexpr uint64_t RV_AC = rv_nat(AC, 1);
  static constexpr uint64_t RV_CA = rv_nat(CA, NB_CA);
  static constexpr uint64_t RV_PAIR = rv_pair(AOUT, NB_PAIR);
  // Input blocks of the 256-wide layers produced in registers inside the consumer's MFMA loop (dense_gen)
  // instead of staged through the LDS image (SPP_GEN_INPUTS, common.h): the fp32 sets whose critic input is
  // one observation block and one action block.  The wide-input sets (111-dim observations, NB_CIN = 5)
  // spill VGPRs to scratch with the generators' state and keep the staged path.
  static constexpr bool kGenOk = !BF_ && NB_OB == 1 && NB_CA == 1;
  static constexpr bool GEN_CD2 = kGenOk && (SPP_GEN_INPUTS & 1);   // critic phase: delta2 -> W2^T
  static constexpr bool GEN_AD2 = kGenOk && (SPP_GEN_INPUTS & 2);   // actor phase: delta2 -> W2^T
  static constexpr bool GEN_CFC1 = kGenOk && (SPP_GEN_INPUTS & 4);  // critic_forward: fc1 -> fc2
  // the stage split's trunk kernels only (selected per call site: with the actor's generator beside the
  // critics' the one-kernel phases spill); the narrow heads those kernels exist for
  static constexpr bool GEN_AFC1 = kGenOk && NB_PAIR <= 2 && (SPP_GEN_INPUTS & 8);   // k_sac_trunk_fwd_gen: fc1 -> fc2
  static constexpr bool GEN_AWHT = kGenOk && NB_PAIR <= 2 && (SPP_GEN_INPUTS & 16);  // k_sac_actor_trunk_bwd_gen: Wh^T -> W2^T
  static_assert(AC <= 32, "env action dim <= 32");
  static_assert(2 * AOUT <= 256 && OB + AOUT <= 256, "dims");
};

constexpr int kWavesPerWG = 4;

constexpr int kLdsPerWave = 256 * 32;  // BIG [256][32] floats
constexpr int kSmallRow = 192;         // SMALL [64][32] = BIG rows 192..255

// Fill the per-workgroup LDS constant table (all threads), then barrier.
__device__ __forceinline__ void load_table(const SacArgs& p, float* tbl) {
  for (int s = 0; s < p.nseg; ++s) {
    const TabSeg g = p.seg[s];
    for (int i = threadIdx.x; i < g.npad; i += blockDim.x) tbl[g.off + i] = i < g.n ? g.src[i] : 0.f;
  }
  __syncthreads();
}
// Natural-order table vector at (block ob, register q) of this lane half.
__device__ __forceinline__ float tval(const float* t, int ob, int q, int h4) { return t[32 * ob + ru(q) + h4]; }
// All 16 table values of output block ob for this lane half (v[q] = tval(t, ob, q, h4)) as 4
// broadcast ds_read_b128, read before any use: an LDS read inside a select is turned into a
// branch with its own wait, i.e. one LDS round trip per element.
__device__ __forceinline__ void tvals(const float* t, int ob, int h4, float (&v)[16]) {
  const float4* p = reinterpret_cast<const float4*>(t + 32 * ob + h4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 x = p[2 * k];
    v[4 * k + 0] = x.x;
    v[4 * k + 1] = x.y;
    v[4 * k + 2] = x.z;
    v[4 * k + 3] = x.w;
  }
}

__device__ __forceinline__ void setbits(uint64_t& lo, uint64_t& hi, int ob, uint32_t bits) {
  if (ob < 4) lo |= (uint64_t)bits << (16 * ob);
  else hi |= (uint64_t)bits << (16 * (ob - 4));
  asm volatile("" : "+v"(lo), "+v"(hi));  // materialise now: no sinking of 16 live floats per block
}
__device__ __forceinline__ bool getbit(uint64_t lo, uint64_t hi, int ob, int q) {
  const uint64_t w = ob < 4 ? (lo >> (16 * ob)) : (hi >> (16 * (ob - 4)));
  return (w >> q) & 1;
}

// memory.py:107-121 (denormalize) and :76-87 / utils.py:62-73 (normalize, force=True)
// TB: read the kernel's LDS table T (make_args puts the limits at t_lim / t_alim and the
// normaliser vectors at t_n0 / t_n1) instead of the global arrays (per-slot global loads are one
// round trip each).  Every kernel set reads the table (TB = true); the global form stays for
// reference.
template <bool TB>
__device__ __forceinline__ float nv0(const SacArgs& p, const float* T, int j) {
  if constexpr (TB) return T[p.t_n0 + j];
  else return p.min_max ? p.lo[j] : p.mean[j];
}
template <bool TB>
__device__ __forceinline__ float nv1(const SacArgs& p, const float* T, int j) {
  if constexpr (TB) return T[p.t_n1 + j];
  else return p.min_max ? p.hi[j] : p.std[j];
}
template <bool TB>
__device__ __forceinline__ float denorm(const SacArgs& p, const float* T, int j, float x) {
  const float n0 = nv0<TB>(p, T, j), n1 = nv1<TB>(p, T, j);
  if (p.min_max) {  // n0 = lo, n1 = hi
    const float mid = fadd_rn(n1, n0) * 0.5f, delta = fsub_rn(n1, n0) * 0.5f;
    return fadd_rn(mid, fmul_rn(x, delta));
  }
  return fadd_rn(fmul_rn(fadd_rn(n1, 1e-8f), x), n0);  // n0 = mean, n1 = std
}
template <bool TB>
__device__ __forceinline__ float denorm_scale(const SacArgs& p, const float* T, int j) {
  const float n0 = nv0<TB>(p, T, j), n1 = nv1<TB>(p, T, j);
  if (p.min_max) return fsub_rn(n1, n0) * 0.5f;
  return fadd_rn(n1, 1e-8f);
}
template <bool TB>
__device__ __forceinline__ float normalize(const SacArgs& p, const float* T, int j, float x) {
  const float n0 = nv0<TB>(p, T, j), n1 = nv1<TB>(p, T, j);
  if (p.min_max) {
    const float mid = fadd_rn(n1, n0) * 0.5f;
    return fdiv_rn(fsub_rn(x, mid), fadd_rn(fsub_rn(n1, mid), 1e-8f));
  }
  return fminf(fmaxf(fdiv_rn(fsub_rn(x, n0), fadd_rn(n1, 1e-8f)), -10.f), 10.f);
}
template <bool TB>
__device__ __forceinline__ float actor_lim(const SacArgs& p, const float* T, int j) {
  if constexpr (TB) return T[p.t_lim + j];
  else return p.actor_lim[j];
}
template <bool TB>
__device__ __forceinline__ float acm_lim(const SacArgs& p, const float* T, int u) {
  if constexpr (TB) return T[p.t_alim + u];
  else return p.acm_lim[u];
}
__device__ __forceinline__ float softplus_t(float x) {  // torch softplus(beta=1, threshold=20)
  return x > 20.f ? x : log1pf(expf(x));
}

// Transcendentals of the squash / log-prob epilogues.  F (the bf16 kernel sets, BASELINE configs[4]:
// bf16 MLP): the hardware forms (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp), far inside the bf16
// tolerance; these epilogues are VALU-latency bound on the 111-wide Ant heads.  fp32 sets: libm.
template <bool F>
__device__ __forceinline__ float t_exp(float x) {
  if constexpr (F) return __expf(x);
  else return expf(x);
}
template <bool F>
__device__ __forceinline__ float t_rcp(float x) {
  if constexpr (F) return __builtin_amdgcn_rcpf(x);
  else return 1.f / x;
}
template <bool F>
__device__ __forceinline__ float t_tanh(float x) {
  if constexpr (F) return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f);
  else return tanhf(x);
}
template <bool F>
__device__ __forceinline__ float t_softplus(float x) {
  if constexpr (F) return x > 20.f ? x : __logf(1.f + __expf(x));
  else return softplus_t(x);
}

// Pairing-layout tile of the actor heads from the LDS image rows [0, 2*AOUT)
// pairing layout: block ib, register r<8 (mu) / r+8 (logsig), half h -> j = 16*ib + 8*h + r
template <class C>
__device__ __forceinline__ void load_pair(f32x16 (&t)[C::NB_PAIR], const float* lds) {
  SPP_XLANE_SYNC();
  const int lane = lane_id(), h8 = 8 * (lane >> 5);
  const float* pl = lds + h8 * 32 + (lane & 31);
#pragma unroll
  for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j0 = 16 * ib + (r & 7);
      t[ib][r] = (j0 + h8 < C::AOUT) ? pl[((r < 8) ? j0 : C::AOUT + j0) * 32] : 0.f;
    }
}

// The same tile from a feature-major global array HD [2*AOUT][ld] (rows mu | logsig) at the lane's pairing
// offset vp; slots j >= AOUT hold 0, as load_pair's do (the bounded resource alone would not give that: slot j
// of the mu rows lands in the logsig rows).
template <class C>
__device__ __forceinline__ void load_pair_gl(f32x16 (&t)[C::NB_PAIR], const float* HD, int ld4, uint32_t vp) {
  const rsrc_t hr = rsrc_n(HD, 2 * C::AOUT * ld4);
  const int h8 = 8 * (lane_id() >> 5);
#pragma unroll
  for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j0 = 16 * ib + r;
      const bool ok = j0 + h8 < C::AOUT;
      const float mu = fm_ldb(hr, j0, ld4, vp);
      const float ls = fm_ldb(hr, C::AOUT + j0, ld4, vp);
      t[ib][r] = ok ? mu : 0.f;
      t[ib][r + 8] = ok ? ls : 0.f;
    }
}

// Concatenated input tile: blocks [0, NB0) natural from global X (F0 units),
// blocks [NB0, NB0+NB1) natural from the LDS image rows [0, F1).
template <int NB0, int NB1>
__device__ __forceinline__ void load_cat_gl(f32x16 (&t)[NB0 + NB1], const float* X, int nbytes, int F0, int ld4,
                                            uint32_t vo, const float* lds, int F1) {
  SPP_XLANE_SYNC();
  const int lane = lane_id(), h4 = 4 * (lane >> 5);
  const float* l = lds + h4 * 32 + (lane & 31);
  f32x16 g[NB0];
  gm_load<NB0>(g, X, nbytes, F0, ld4, vo);
#pragma unroll
  for (int ib = 0; ib < NB0; ++ib) t[ib] = g[ib];
#pragma unroll
  for (int ib = 0; ib < NB1; ++ib)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u0 = 32 * ib + ru(r);
      t[NB0 + ib][r] = (u0 + h4 < F1) ? l[u0 * 32] : 0.f;
    }
}
// Concatenated input tile from two global feature-major arrays.
template <int NB0, int NB1>
__device__ __forceinline__ void load_cat_gg(f32x16 (&t)[NB0 + NB1], const float* X0, int F0, const float* X1, int F1,
                                            int ld4, uint32_t vo) {
  f32x16 g0[NB0], g1[NB1];
  gm_load<NB0>(g0, X0, F0 * ld4, F0, ld4, vo);
  gm_load<NB1>(g1, X1, F1 * ld4, F1, ld4, vo);
#pragma unroll
  for (int ib = 0; ib < NB0; ++ib) t[ib] = g0[ib];
#pragma unroll
  for (int ib = 0; ib < NB1; ++ib) t[NB0 + ib] = g1[ib];
}

// Per-tile lane context: LDS images, sample column offsets.
// Global 2-D arrays X[row][ld] are addressed through buffer resources:
// byte offset row*ld4 (wave-uniform soffset) + vo (this lane's column, voffset).
struct Lane {
  int h, s, h4;
  float* img;             // BIG image base of this wave
  const float* tbl;       // per-workgroup LDS table
  int b, ld4;             // sample index, row stride in bytes
  uint32_t vo, vp;        // 4*(4h*ld + b) (natural layout), 4*(8h*ld + b) (pairing layout)
  float *bl, *sl;         // BIG / SMALL image at this lane: image[urow*32] = unit (urow + 4h), sample s
  float* pl;              // BIG at the pairing offset: pl[j0*32] = row j0 + 8h
};
__device__ __forceinline__ Lane make_lane(float* big, float* small, const float* tbl, int ld, int b) {
  Lane L;
  L.img = big;
  L.tbl = tbl;
  int lane = lane_id();
  asm volatile("" : "+v"(lane));  // keep lane-derived values inside the tile loop (no LICM + spill)
  int ld4 = 4 * ld;
  asm volatile("" : "+s"(ld4));   // likewise the row strides (no hoisted per-row offsets)
  L.h = lane >> 5;
  L.s = lane & 31;
  L.h4 = 4 * L.h;
  L.ld4 = ld4;
  L.b = b;
  L.vo = (uint32_t)(L.h4 * ld4 + 4 * b);
  L.vp = (uint32_t)(8 * L.h * ld4 + 4 * b);
  L.bl = big + L.h4 * 32 + L.s;
  L.sl = small + L.h4 * 32 + L.s;
  L.pl = big + 8 * L.h * 32 + L.s;
  return L;
}

// ---- generators of dense_gen's input blocks (mlp.h: called in NP parts per block, in order)
// delta2 = dq * w3 * relu'(h2) of a critic, rank one per sample: register q of block ib is
// mask bit (ib, q) ? dq * w3[unit] : 0.  Part 0 reads the block's 16 table values, the other parts
// spread the registers; st(unit row, value) stores the weight-gradient operand (or does nothing).
template <int NP, typename St>
struct Delta2Gen {
  const float* w3;
  int h4;
  uint64_t lo, hi;
  float dq;
  St st;
  float tv[16];
  template <int P>
  __device__ __forceinline__ void operator()(int ib, IC<P>, f32x16& x) {
    if constexpr (P == 0) {
      tvals(w3, ib, h4, tv);
    } else {
#pragma unroll
      for (int q = gen_q0(P, NP); q < gen_q0(P + 1, NP); ++q) {
        const float v = getbit(lo, hi, ib, q) ? dq * tv[q] : 0.f;
        x[q] = v;
        st(32 * ib + ru(q), v);
      }
    }
  }
};
// relu(fc1) of a register-input first layer (dense_impl's chain: bias tile, then the register quads in
// flat order) as the input of fc2.  Part 0 runs block ib's MFMA chain and then requests block ib+1's
// fragments into the same registers, so their L2 latency sits under the consumer's MFMAs; the other
// parts spread the ReLU, the mask bits and st(unit row, value), the h1 operand store (or nothing).
template <int NBI, uint64_t RV, int NP, typename St>
struct Fc1Gen {
  static constexpr int NQ = rv_total(RV, NBI);
  static constexpr int OBSTRIDE = NBI * 4 * 64 * 16;  // bytes per output block
  const f32x16 (&in)[NBI];
  rsrc_t wr;
  uint32_t l16;
  const float* biasL;
  int h;
  uint64_t &mlo, &mhi;
  St st;
  float4 cur[NQ];
  f32x16 acc;
  uint32_t bits;
  __device__ __forceinline__ void request(int ob) {
    const int wn = ob * OBSTRIDE;
    static_for<0, NQ>([&](auto Q) {
      constexpr int q = Q;
      cur[q] = wfrag(wr, l16, wn + (q_ib(RV, NBI, q) * 4 + q_rq(RV, NBI, q)) * 1024);
    });
  }
  template <int P>
  __device__ __forceinline__ void operator()(int ib, IC<P>, f32x16& x) {
    if constexpr (P == 0) {
      acc = bias_tile(biasL, ib, h);
      static_for<0, NQ>([&](auto Q) {
        constexpr int q = Q;
        constexpr int kb = q_ib(RV, NBI, q);
        constexpr int rq = q_rq(RV, NBI, q);
        acc = mfma(cur[q].x, in[kb][4 * rq + 0], acc);
        acc = mfma(cur[q].y, in[kb][4 * rq + 1], acc);
        acc = mfma(cur[q].z, in[kb][4 * rq + 2], acc);
        acc = mfma(cur[q].w, in[kb][4 * rq + 3], acc);
      });
      request(ib + 1 < 8 ? ib + 1 : ib);  // (the last block re-reads its own: no branch in the MFMA loop)
      bits = 0;
    } else {
#pragma unroll
      for (int q = gen_q0(P, NP); q < gen_q0(P + 1, NP); ++q) {
        const float v = fmaxf(acc[q], 0.f);
        x[q] = v;
        st(32 * ib + ru(q), v);
        bits |= (uint32_t)(v > 0.f) << q;
      }
      if constexpr (P == NP - 1) setbits(mlo, mhi, ib, bits);
    }
  }
};

// dh2 = Wh^T dheads * relu'(h2) of the actor trunk's backward, a register-input layer without a bias
// (dense_impl's chain with a null bias table: zero16(), then the register quads in flat order), as the
// input of W2^T.  Parts as Fc1Gen: part 0 runs block ib's MFMA chain and requests block ib+1's
// fragments; the other parts spread the h2 mask select and st(unit row, value), the AD2 operand store.
template <int NBI, uint64_t RV, int NP, typename St>
struct WhTGen {
  static constexpr int NQ = rv_total(RV, NBI);
  static constexpr int OBSTRIDE = NBI * 4 * 64 * 16;  // bytes per output block
  const f32x16 (&in)[NBI];
  rsrc_t wr;
  uint32_t l16;
  uint64_t lo, hi;
  St st;
  float4 cur[NQ];
  f32x16 acc;
  __device__ __forceinline__ void request(int ob) {
    const int wn = ob * OBSTRIDE;
    static_for<0, NQ>([&](auto Q) {
      constexpr int q = Q;
      cur[q] = wfrag(wr, l16, wn + (q_ib(RV, NBI, q) * 4 + q_rq(RV, NBI, q)) * 1024);
    });
  }
  template <int P>
  __device__ __forceinline__ void operator()(int ib, IC<P>, f32x16& x) {
    if constexpr (P == 0) {
      acc = zero16();
      static_for<0, NQ>([&](auto Q) {
        constexpr int q = Q;
        constexpr int kb = q_ib(RV, NBI, q);
        constexpr int rq = q_rq(RV, NBI, q);
        acc = mfma(cur[q].x, in[kb][4 * rq + 0], acc);
        acc = mfma(cur[q].y, in[kb][4 * rq + 1], acc);
        acc = mfma(cur[q].z, in[kb][4 * rq + 2], acc);
        acc = mfma(cur[q].w, in[kb][4 * rq + 3], acc);
      });
      request(ib + 1 < 8 ? ib + 1 : ib);  // (the last block re-reads its own: no branch in the MFMA loop)
    } else {
#pragma unroll
      for (int q = gen_q0(P, NP); q < gen_q0(P + 1, NP); ++q) {
        const float v = getbit(lo, hi, ib, q) ? acc[q] : 0.f;
        x[q] = v;
        st(32 * ib + ru(q), v);
      }
    }
  }
};

// Actor trunk: x -> relu(L1) -> relu(L2) -> heads into LDS rows [0, NHR): SAC
// (mu | logsig), NHR = 2*AOUT; DDPG fc3 pre-activation, NHR = AOUT (NBH blocks).
// ST: store h1 / h2 feature-major (H1g, H2g).  Returns the ReLU masks.
// HG: the heads go feature-major to HDg [NHR][ld] at the sample's own column instead of into the image.
// GEN: fc1's blocks are produced in registers under fc2's MFMAs (Fc1Gen, as critic_forward's); fc1 does not
// touch the image.  Off by default: a flag of the call site, not of the kernel set (Cfg::GEN_AFC1).
template <class C, bool ST, int NBH = C::NB_H2, int NHR = 2 * C::AOUT, bool HG = false, bool GEN = false>
__device__ __forceinline__ void actor_trunk(const ActorDev& A, const float* X, int xbytes, const Lane& L, float* H1g,
                                            float* H2g,
                                            uint64_t& m1lo, uint64_t& m1hi, uint64_t& m2lo, uint64_t& m2hi,
                                            float* HDg = nullptr) {
  if constexpr (GEN) {
    static_assert(!C::BF, "fp32 sets");
    f32x16 x[C::NB_OB];
    gm_load<C::NB_OB>(x, X, xbytes, C::OB, L.ld4, L.vo);
    const rsrc_t h1r = rsrc(H1g), h2r = rsrc(H2g);
    const int ld4 = L.ld4;
    const uint32_t vo = L.vo;
    auto st1 = [=](int ur, float v) {
      if constexpr (ST) op_st<C::BF>(h1r, ur, ld4, vo, v);
    };
    Fc1Gen<C::NB_OB, C::RV_X, 8, decltype(st1)> g{x, rsrc(A.W1), 16u * lane_id(), L.tbl + A.tb1, L.h, m1lo, m1hi, st1};
    g.request(0);
    SPP_TP(1);
    dense_gen<8>(A.W2, L.tbl + A.tb2, g, [&](int ob, const f32x16& acc) {
      uint32_t bits = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        const float v = fmaxf(acc[q], 0.f);
        L.bl[ur * 32] = v;
        if constexpr (ST) op_st<C::BF>(h2r, ur, L.ld4, L.vo, v);
        bits |= (uint32_t)(v > 0.f) << q;
      }
      setbits(m2lo, m2hi, ob, bits);
    });
  } else {
    {
      f32x16 x[C::NB_OB];
      gm_load<C::NB_OB>(x, X, xbytes, C::OB, L.ld4, L.vo);
      const rsrc_t hr = rsrc(H1g);
      dense<C::NB_OB, C::RV_X, C::BF>(A.W1, 8, x, L.tbl + A.tb1, [&](int ob, const f32x16& acc) {
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ur = 32 * ob + ru(q);
          const float v = fmaxf(acc[q], 0.f);
          L.bl[ur * 32] = v;
          if constexpr (ST) op_st<C::BF>(hr, ur, L.ld4, L.vo, v);
          bits |= (uint32_t)(v > 0.f) << q;
        }
        setbits(m1lo, m1hi, ob, bits);
      });
    }
    SPP_TP(1);
    {
      const rsrc_t hr = rsrc(H2g);
      dense_lds<8, C::BF>(A.W2, L.img, L.tbl + A.tb2, [&](int ob, const f32x16& acc) {
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ur = 32 * ob + ru(q);
          const float v = fmaxf(acc[q], 0.f);
          L.bl[ur * 32] = v;
          if constexpr (ST) op_st<C::BF>(hr, ur, L.ld4, L.vo, v);
          bits |= (uint32_t)(v > 0.f) << q;
        }
        setbits(m2lo, m2hi, ob, bits);
      });
    }
  }
  SPP_TP(2);
  {
    dense_lds<NBH, C::BF>(A.Wh, L.img, L.tbl + A.tbh, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        if (ur + L.h4 < NHR) {
          if constexpr (HG) fm_st(rsrc(HDg), ur, L.ld4, L.vo, acc[q]);
          else L.bl[ur * 32] = acc[q];
        }
      }
    });
  }
  SPP_TP(3);
}

// ACM forward (basic_model.py:118-126): in [s | a_d] -> tanh 64 -> tanh 32 -> tanh(ac)*lim.
// ST: store z1 / z2 / t3 feature-major; output c into SMALL rows [0, AC).
template <class C, bool ST>
__device__ __forceinline__ void acm_forward(const SacArgs& p, const f32x16 (&xin)[C::NB_ACMIN], const Lane& L,
                                            float* Z1g, float* Z2g, float* T3g) {
  float* small = L.sl - L.h4 * 32 - L.s;
  const rsrc_t z1r = rsrc(Z1g), z2r = rsrc(Z2g), t3r = rsrc(T3g);
  dense<C::NB_ACMIN, C::RV_ACMIN, C::BF>(p.acm.W1, 2, xin, L.tbl + p.acm.tb1, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ur = 32 * ob + ru(q);
      const float v = tanhf(acc[q]);
      L.sl[ur * 32] = v;
      if constexpr (ST) fm_st(z1r, ur, L.ld4, L.vo, v);
    }
  });
  f32x16 z1[2];
  lds_load<2>(z1, small);
  dense<2, C::RV_Z1, C::BF>(p.acm.W2, 1, z1, L.tbl + p.acm.tb2, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float v = tanhf(acc[q]);
      L.sl[ru(q) * 32] = v;
      if constexpr (ST) fm_st(z2r, ru(q), L.ld4, L.vo, v);
    }
  });
  f32x16 z2[1];
  lds_load<1>(z2, small);
  float limv[16];  // before the layer: a load behind the epilogue's buffer stores waits per element
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int u = ru(q) + L.h4;
    limv[q] = acm_lim<true>(p, L.tbl, u < C::AC ? u : 0);
  }
  dense<1, C::RV_Z2, C::BF>(p.acm.W3, 1, z2, L.tbl + p.acm.tb3, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = ru(q) + L.h4;
      if (u < C::AC) {
        const float t = tanhf(acc[q]);
        L.sl[ru(q) * 32] = t * limv[q];
        if constexpr (ST) fm_st(t3r, ru(q), L.ld4, L.vo, t);
      }
    }
  });
}

// Critic forward through L2 with q = w3 . relu(h2) + b3 reduced per sample.
// ST: store h1 / h2 feature-major.
// H2L: h2 goes to the wave's LDS image (the caller's fused layer-3 weight gradient reads it there) instead
// of to HBM.
template <class C, bool ST, int R = 30, bool H2L = false>
__device__ __forceinline__ float critic_forward(const CriticDev& Q, const f32x16 (&xin)[C::NB_CIN], const Lane& L,
                                                float* H1g, float* H2g, uint64_t& m1lo, uint64_t& m1hi,
                                                uint64_t& m2lo, uint64_t& m2hi) {
  const rsrc_t h1r = rsrc(H1g), h2r = rsrc(H2g);
  float qp = 0.f;
  const float* w3 = L.tbl + Q.tw3;
  auto epi2 = [&](int ob, const f32x16& acc) {
    uint32_t bits = 0;
    float tv[16];
    tvals(w3, ob, L.h4, tv);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float v = fmaxf(acc[q], 0.f);
      if constexpr (H2L) L.bl[(32 * ob + ru(q)) * 32] = v;  // the image's h1 reads are done (dense_lds)
      else if constexpr (ST) op_st<C::BF>(h2r, 32 * ob + ru(q), L.ld4, L.vo, v);
      qp = fmaf(v, tv[q], qp);
      bits |= (uint32_t)(v > 0.f) << q;
    }
    setbits(m2lo, m2hi, ob, bits);
  };
  if constexpr (C::GEN_CFC1) {
    // fc1's blocks are produced in registers under fc2's MFMAs (Fc1Gen): the layer does not touch the image
    const int ld4 = L.ld4;
    const uint32_t vo = L.vo;
    auto st1 = [=](int ur, float v) {
      if constexpr (ST) op_st<C::BF>(h1r, ur, ld4, vo, v);
    };
    Fc1Gen<C::NB_CIN, C::RV_CIN, 8, decltype(st1)> g{xin, rsrc(Q.W1), 16u * lane_id(), L.tbl + Q.tb1, L.h, m1lo, m1hi, st1};
    g.request(0);
    SPP_TP(R);
    dense_gen<8>(Q.W2, L.tbl + Q.tb2, g, epi2);
  } else {
    dense<C::NB_CIN, C::RV_CIN, C::BF>(Q.W1, 8, xin, L.tbl + Q.tb1, [&](int ob, const f32x16& acc) {
      uint32_t bits = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        const float v = fmaxf(acc[q], 0.f);
        L.bl[ur * 32] = v;
        if constexpr (ST) op_st<C::BF>(h1r, ur, L.ld4, L.vo, v);
        bits |= (uint32_t)(v > 0.f) << q;
      }
      setbits(m1lo, m1hi, ob, bits);
    });
    SPP_TP(R);
    dense_lds<8, C::BF>(Q.W2, L.img, L.tbl + Q.tb2, epi2);
  }
  SPP_TP(R + 1);
  return qp + __shfl_xor(qp, 32, 64) + *Q.b3;
}

// Squash (sac/models.py:37-52) of the pairing-layout heads tile with eps [aout][Bp].
// Writes a_d = denormalize(tanh(u)*lim) into LDS rows [0, AOUT); returns logpi.
template <class C, bool BRF = false>
__device__ __forceinline__ float squash_write(const SacArgs& p, const f32x16 (&hd)[C::NB_PAIR],
                                              const float* __restrict__ EPS, const Lane& L) {
  float lp = 0.f, corr = 0.f;
  const int h8 = 8 * L.h;
  // all eps reads first (one latency for the block, not one per output).  The loads may be
  // issued for every lane, so they go through a resource bounded to the [AOUT][Bp] array:
  // the pairing layout's unused slots (j >= AOUT) read 0 instead of past the array.
  const rsrc_t er = rsrc_n(EPS, C::AOUT * L.ld4);
  float ev[C::NB_PAIR][8];
#pragma unroll
  for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
    for (int r = 0; r < 8; ++r) ev[ib][r] = 16 * ib + r < C::AOUT ? fm_ldb(er, 16 * ib + r, L.ld4, L.vp) : 0.f;
  // BRF (critic phase): no per-slot branch (a branch holding a table load and its use costs one
  // LDS round trip per slot); slots j >= AOUT compute on index 0 and are dropped.  The actor
  // phase keeps the branches (its branch-free live ranges spill).
  constexpr bool kBranchFree = BRF;
#pragma unroll
  for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j0 = 16 * ib + r;
      if (j0 >= C::AOUT) continue;  // no lane holds a slot of this row (unrolled: folded away)
      const int j = j0 + h8;
      const bool ok = j < C::AOUT;
      if (kBranchFree || ok) {
        const int jj = ok ? j : 0;
        constexpr bool F = C::BF;
        const float mu = hd[ib][r];
        const float ls = fminf(fmaxf(hd[ib][r + 8], -20.f), 2.f);
        const float sc = t_exp<F>(ls);
        const float e = ev[ib][r];
        const float u = fadd_rn(mu, fmul_rn(e, sc));
        float lpj;
        if constexpr (F) {  // Normal(mu, sc).log_prob(u) with u - mu = e sc, log sc = ls
          lpj = -0.5f * e * e - ls - kLogSqrt2Pi;
        } else {  // the reference's operation order
          const float d = fsub_rn(u, mu);
          const float var = fmul_rn(sc, sc);
          lpj = fsub_rn(fsub_rn(fdiv_rn(-fmul_rn(d, d), 2.f * var), logf(sc)), kLogSqrt2Pi);
        }
        const float cj = 2.f * fsub_rn(fsub_rn(kLog2, u), t_softplus<F>(-2.f * u));
        lp += ok ? lpj : 0.f;
        corr += ok ? cj : 0.f;
        const float a = fmul_rn(t_tanh<F>(u), actor_lim<true>(p, L.tbl, jj));
        const float ad = denorm<true>(p, L.tbl, jj, a);
        if (ok) L.pl[j0 * 32] = ad;
      }
    }
  SPP_XLANE_SYNC();
  const float tot = lp + __shfl_xor(lp, 32, 64);
  const float tc = corr + __shfl_xor(corr, 32, 64);
  return fsub_rn(tot, tc);
}

// ============================================================================ wave pairs
// PAIR forms of the phase kernels (k_sac_critic_phase<C, true, true>, k_sac_actor_phase<C, true, true, true>): a
// tile's two critics are independent up to 32 q values, so the two waves of a pair (waves 2j and 2j + 1 of the
// grid, both in one workgroup) take one critic each (the wave's role c) and the unit of work is half a tile.
//   pair j = global wave >> 1, P = 2 gridDim pairs, iteration k = 0 .. K - 1 works on tile j + k P,
//   K = ceil(ntiles / P): from kernel arguments only, so every wave of every workgroup runs K iterations and
//   reaches the one barrier of each; a pair whose tile is past the end skips the work, not the barrier.
// The q values cross through an LDS slot [pair in workgroup][k & 1][c][32]: written before the barrier, the
// partner's read behind it; the next write to the same parity is two barriers later, behind the partner's read.
struct PairMap {
  int c, j, P, K;
};
__device__ __forceinline__ PairMap pair_map(int ntiles) {
  const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerWG + (threadIdx.x >> 6)));
  const int P = 2 * (int)gridDim.x;
  return {gw & 1, gw >> 1, P, (ntiles + P - 1) / P};
}
using PairSlot = float[kWavesPerWG / 2][2][2][32];

// The soft-min twin target y (sac_acm.py:50-56) of one sample: one expression for every form of the critic phase.
__device__ __forceinline__ float sac_target_y(const SacArgs& p, int b, float q1t, float q2t, float alpha, float lp2) {
  const float notdone = 1.f - p.DN[b];
  return fadd_rn(p.R[b], fmul_rn(p.gamma * notdone, fsub_rn(fminf(q1t, q2t), alpha * lp2)));
}

// ============================================================================ critic phase
// STAGED (the stage split): the target action comes from k_sac_trunk_fwd / k_sac_squash_stage; the kernel starts
// at the target critics, from their action input (p.SCA) and log pi' (p.SLP).
// PAIR (with STAGED): wave pairs, above.  Wave c runs target critic c, then critic c's forward and backward.  Its
// two fc3 accumulator sets are the slabs of the unpaired kernel's waves j (even k) and j + P (odd k): with
// W = 2 P waves, those walk tiles j, j + W, .. and j + P, j + P + W, .. in this order, so every slab holds the same
// sums of the same tiles in the same order, and is written by one wave.
template <class C, bool STAGED = false, bool PAIR = false>
__global__ __launch_bounds__(256, 1) void k_sac_critic_phase(SacArgs p) {
  static_assert(STAGED || !PAIR, "the pair form starts at the target critics");
  static_assert(C::F3 || !PAIR, "the pair form keeps the fused fc3 slabs");
  __shared__ __attribute__((aligned(16))) float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  __shared__ __attribute__((aligned(16))) float s_dq[kWavesPerWG][32];  // the tile's d loss / dq, for the fused layer-3 weight gradient
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  const float alpha = *p.alpha;
  float w3a[4] = {0.f, 0.f, 0.f, 0.f}, w3b[4] = {0.f, 0.f, 0.f, 0.f}, b3a = 0.f, b3b = 0.f;  // fused fc3 grads
  const PairMap pm = PAIR ? pair_map(ntiles) : PairMap{};
  int tile = PAIR ? pm.j : blockIdx.x * kWavesPerWG + w;
  for (int k = 0; PAIR ? k < pm.K : tile < ntiles; ++k, tile += PAIR ? pm.P : gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    const int b = L.b;
    const bool valid = b < p.B;
    uint64_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    float lp2;
    f32x16 tin[C::NB_CIN];
    float q1t, q2t;
    if constexpr (PAIR) {
      const bool active = tile < ntiles;  // wave-uniform, and the same for both waves of the pair
      __shared__ PairSlot s_q;  // (here: only the pair forms hold it)
      float* slot = &s_q[w >> 1][k & 1][0][0];
      float qt = 0.f;
      if (active) {
        SPP_TP(0);
        load_cat_gg<C::NB_OB, C::NB_CA>(tin, p.S2, C::OB, p.SCA, C::CA, L.ld4, L.vo);
        lp2 = p.SLP[b];
        SPP_TP(5);
        qt = critic_forward<C, false, 6>(p.targ[pm.c], tin, L, nullptr, nullptr, d0, d1, d2, d3);
        if (L.h == 0) slot[32 * pm.c + L.s] = qt;
      }
      __syncthreads();  // every wave of the workgroup, K times
      if (!active) continue;
      const float qo = slot[32 * (pm.c ^ 1) + L.s];
      q1t = pm.c ? qo : qt;
      q2t = pm.c ? qt : qo;
    } else if constexpr (STAGED) {
      SPP_TP(0);
      load_cat_gg<C::NB_OB, C::NB_CA>(tin, p.S2, C::OB, p.SCA, C::CA, L.ld4, L.vo);
      lp2 = p.SLP[b];
    } else {
      // ---- target action: a' ~ pi(s'), a'_d, logpi'   (sac_acm.py:44-45)
      SPP_TP(0);
      actor_trunk<C, false>(p.actor, p.S2, C::OB * L.ld4, L, nullptr, nullptr, d0, d1, d2, d3);
      {
        f32x16 hd[C::NB_PAIR];
        load_pair<C>(hd, big);
        lp2 = squash_write<C, true>(p, hd, p.EPS1, L);
      }
      SPP_TP(4);
      // ---- critic-target input: [s' | ACM(s', a'_d)] or [s' | a'_d]   (:46-48)
      if constexpr (C::ACMC) {
        f32x16 xin[C::NB_ACMIN];
        load_cat_gl<C::NB_OB, C::NB_AOUT>(xin, p.S2, C::OB * L.ld4, C::OB, L.ld4, L.vo, big, C::AOUT);
        acm_forward<C, false>(p, xin, L, nullptr, nullptr, nullptr);
        load_cat_gl<C::NB_OB, C::NB_CA>(tin, p.S2, C::OB * L.ld4, C::OB, L.ld4, L.vo, small, C::AC);
      } else {
        load_cat_gl<C::NB_OB, C::NB_CA>(tin, p.S2, C::OB * L.ld4, C::OB, L.ld4, L.vo, big, C::AOUT);
      }
    }
    // ---- soft-min twin target (:50-56)
    if constexpr (!PAIR) {
      SPP_TP(5);
      q1t = critic_forward<C, false, 6>(p.targ[0], tin, L, nullptr, nullptr, d0, d1, d2, d3);
      q2t = critic_forward<C, false, 8>(p.targ[1], tin, L, nullptr, nullptr, d0, d1, d2, d3);
    }
    const float y = sac_target_y(p, b, q1t, q2t, alpha, lp2);
    // ---- both critics (PAIR: this wave's): forward, MSE grad, backward to weight-gradient operands (:117-131)
    float lq0 = 0.f, lq1 = 0.f;
    const int i0 = PAIR ? pm.c : 0, i1 = PAIR ? pm.c + 1 : 2;
#pragma unroll 1
    for (int i = i0; i < i1; ++i) {
      // the fc3 accumulator set: critic i's (PAIR: the slab of even / of odd iterations)
      const bool seta = PAIR ? (k & 1) == 0 : i == 0;
      uint64_t m1lo = 0, m1hi = 0, m2lo = 0, m2hi = 0;
      f32x16 xin[C::NB_CIN];
      load_cat_gg<C::NB_OB, C::NB_CA>(xin, p.S, C::OB, C::ACMC ? p.AENV : p.ACT, C::CA, L.ld4, L.vo);
      const CriticDev& Q = p.critic[i];
      SPP_TP(10);
      const float q = critic_forward<C, true, 11, C::F3>(Q, xin, L, p.H1[i], C::F3 ? nullptr : p.H2[i], m1lo, m1hi,
                                                        m2lo, m2hi);
      const float diff = fsub_rn(q, y);
      const float dq = valid ? fmul_rn(2.f * diff, p.inv_B) : 0.f;  // d mse / dq
      const float lqi = (valid && L.h == 0) ? diff * diff : 0.f;
      if (i == 0) lq0 = lqi; else lq1 = lqi;
      if constexpr (!C::F3) {
        if (L.h == 0) p.DQ[i][b] = dq;  // (h2 is stored by critic_forward: the k_dw job dW3 = dq . h2^T)
      } else {
      // fc3's weight gradient, fused (sac_acm.py:117-131; dW3 = dq . h2^T, db3 = sum dq): h2 is in the image;
      // lane l sums units l + 64k over the tile's 32 samples (rotated column order: conflict-free rows)
      // into registers that carry over the wave's tiles; the per-wave partials are reduced in a fixed order
      // by k_dw_reduce (no h2 / dq written to HBM and read back)
      if (L.h == 0) s_dq[w][L.s] = dq;
      SPP_XLANE_SYNC();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int u = lane + 64 * k;
        const float* row = big + u * 32;
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
          const int s2 = (j + u) & 31;
          acc = fmaf(row[s2], s_dq[w][s2], acc);
        }
        if (seta) w3a[k] += acc;
        else w3b[k] += acc;
      }
      const float dsum = wave_sum(L.h == 0 ? dq : 0.f);
      if (seta) b3a += dsum;
      else b3b += dsum;
      SPP_XLANE_SYNC();  // the image rows are rewritten by the delta2 staging below
      }
      const rsrc_t d2r = rsrc(p.D2[i]);
      const float* w3 = tbl + Q.tw3;
      // delta1 = (W2^T delta2) * relu'(h1)
      const rsrc_t d1r = rsrc(p.D1[i]);
      auto epi1 = [&](int ob, const f32x16& acc) {
#pragma unroll
        for (int q2 = 0; q2 < 16; ++q2)
          op_st<C::BF>(d1r, 32 * ob + ru(q2), L.ld4, L.vo, getbit(m1lo, m1hi, ob, q2) ? acc[q2] : 0.f);
      };
      if constexpr (C::GEN_CD2) {
        // delta2 = dq * w3 * relu'(h2): produced in registers under the W2^T MFMAs, stored feature-major
        const int ld4 = L.ld4;
        const uint32_t vo = L.vo;
        auto st2 = [=](int ur, float v) { op_st<C::BF>(d2r, ur, ld4, vo, v); };
        Delta2Gen<8, decltype(st2)> g{w3, L.h4, m2lo, m2hi, dq, st2, {}};
        SPP_TP(13);
        dense_gen<8>(Q.W2T, nullptr, g, epi1);
      } else {
        // delta2 = dq * w3 * relu'(h2): staged through the LDS image, stored feature-major
#pragma unroll 1
        for (int ob = 0; ob < 8; ++ob) {
          float tv[16];
          tvals(w3, ob, L.h4, tv);
#pragma unroll
          for (int q2 = 0; q2 < 16; ++q2) {
            const int ur = 32 * ob + ru(q2);
            const float v = getbit(m2lo, m2hi, ob, q2) ? dq * tv[q2] : 0.f;
            L.bl[ur * 32] = v;
            op_st<C::BF>(d2r, ur, L.ld4, L.vo, v);
          }
        }
        SPP_TP(13);
        dense_lds<8, C::BF>(Q.W2T, big, nullptr, epi1);
      }
    }
    SPP_TP(14);
    const float s0 = wave_sum(lq0), s1 = wave_sum(lq1);
    if (lane == 0) {
      if (!PAIR || pm.c == 0) p.part[tile * kParts + 0] = s0;
      if (!PAIR || pm.c == 1) p.part[tile * kParts + 1] = s1;
    }
    SPP_TP(15);
  }
  // this wave's fc3 partials [256 weights | bias] per critic (every wave writes, tiles or not)
  // PAIR: slabs j and j + P of this wave's critic
  if constexpr (C::F3) {
    const int64_t wg = (int64_t)blockIdx.x * kWavesPerWG + w;
    float* o0 = PAIR ? p.W3P[pm.c] + (int64_t)pm.j * p.w3p_stride : p.W3P[0] + wg * p.w3p_stride;
    float* o1 = PAIR ? p.W3P[pm.c] + (int64_t)(pm.j + pm.P) * p.w3p_stride : p.W3P[1] + wg * p.w3p_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o0[lane + 64 * k] = w3a[k];
      o1[lane + 64 * k] = w3b[k];
    }
    if (lane == 0) {
      o0[256] = b3a;
      o1[256] = b3b;
    }
  }
  SPP_TP_FLUSH();
}

// ============================================================================ actor phase
// Scratch for the frozen-ACM backward (feature-major, same-lane re-read).
struct AcmScratch {
  float *Z1, *Z2, *T3;
  // wide heads (NB_PAIR > 2): the actor phase runs as two kernels; the first hands the second
  // d loss / d a_d [AOUT][Bp] (GAD) and the trunk's ReLU masks [tile][4][64 lanes] (MASK)
  float* GAD;
  uint64_t* MASK;
  // min-critic split (SPLIT kernels below): the forward kernel hands the compacted critic backward
  //   SEL  [Bp]            per sample: bit 0 = critic 1 takes the gradient, bit 1 = critic 2 (3 = exact tie,
  //                        0 = dead: b >= B, or no order between q1 and q2)
  //   CM   [2][Bp][2][4]   each critic's fc1 / fc2 ReLU masks, 32 B per (sample, lane half)
  //   CNT  [ntiles]        samples of the tile in list 1 | in list 2 << 16 (wave ballots)
  // k_minq_scan / k_minq_scatter turn the counts into
  //   OFF  [ntiles][2]     list positions of the tile's first entries (exclusive prefix sums)
  //   NG   [2]             lengths of the two lists
  //   LIST [2][Bp]         sample indices, ascending
  // and the compacted backward stores d q_i / d (critic action input) at the sample's own column of
  //   DCA  [2][CA][Bp]
  uint8_t* SEL;
  uint64_t* CM;
  uint32_t *CNT, *OFF;
  int* NG;
  int* LIST[2];
  float* DCA[2];
};

// d a_d through the frozen ACM (basic_model.py:118-126 backward): dca -> image rows [0, AOUT).
// PRE: every scratch value of the three layers is requested up front: buffer loads cannot be
// moved across the epilogues' LDS stores (no alias proof), so loads issued inside an
// epilogue run as one round trip each.  (Kernels whose registers are taken keep the per-element loads.)
template <class C, bool PRE>
__device__ __forceinline__ void acm_backward(const SacArgs& p, const AcmScratch& z, const Lane& L, float* small,
                                             const f32x16 (&dca)[C::NB_CA]) {
  constexpr bool kPre = PRE;
  float t3v[16], limv[16], z2v[16], z1v[2][16];
  const rsrc_t t3r = rsrc_n(z.T3, C::AC * L.ld4);  // rows >= AC read 0
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int u = ru(q) + L.h4;
    t3v[q] = fm_ldb(t3r, ru(q), L.ld4, L.vo);
    limv[q] = acm_lim<true>(p, L.tbl, u < C::AC ? u : 0);
  }
  if constexpr (kPre) {
#pragma unroll
    for (int q = 0; q < 16; ++q) z2v[q] = fm_ld(rsrc(z.Z2), ru(q), L.ld4, L.vo);
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int q = 0; q < 16; ++q) z1v[ob][q] = fm_ld(rsrc(z.Z1), 32 * ob + ru(q), L.ld4, L.vo);
  }
  auto z2at = [&](int q) {
    if constexpr (kPre) return z2v[q];
    else return fm_ld(rsrc(z.Z2), ru(q), L.ld4, L.vo);
  };
  auto z1at = [&](int ob, int q) {
    if constexpr (kPre) return ob ? z1v[1][q] : z1v[0][q];
    else return fm_ld(rsrc(z.Z1), 32 * ob + ru(q), L.ld4, L.vo);
  };
  f32x16 dp3[1];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int u = ru(q) + L.h4;
    const float t = t3v[q];
    dp3[0][q] = u < C::AC ? dca[0][q] * limv[q] * (1.f - t * t) : 0.f;
  }
  SPP_TPN(23);  // ACM bwd input
  dense<1, C::RV_AC, C::BF>(p.acm.W3T, 1, dp3, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float zz = z2at(q);
      L.sl[ru(q) * 32] = acc[q] * (1.f - zz * zz);
    }
  });
  SPP_TPN(24);  // ACM W3T
  f32x16 dp2[1];
  lds_load<1>(dp2, small);
  dense<1, C::RV_Z2, C::BF>(p.acm.W2T, 2, dp2, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float zz = z1at(ob, q);
      L.sl[(32 * ob + ru(q)) * 32] = acc[q] * (1.f - zz * zz);
    }
  });
  SPP_TPN(25);  // ACM W2T
  f32x16 dp1[2];
  lds_load<2>(dp1, small);
  dense<2, C::RV_Z1, C::BF>(p.acm.W1Ta, C::NB_AOUT, dp1, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ur = 32 * ob + ru(q);
      if (ur + L.h4 < C::AOUT) L.bl[ur * 32] = acc[q];
    }
  });
}
// d (critic action input) -> d a_d in the image rows [0, AOUT): through the ACM, or as it is
template <class C, bool PRE>
__device__ __forceinline__ void dca_to_dad(const SacArgs& p, const AcmScratch& z, const Lane& L, float* small,
                                           const f32x16 (&dca)[C::NB_CA]) {
  if constexpr (C::ACMC) {
    acm_backward<C, PRE>(p, z, L, small, dca);
  } else {
#pragma unroll
    for (int ib = 0; ib < C::NB_CA; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ib + ru(q);
        if (ur + L.h4 < C::AOUT) L.bl[ur * 32] = dca[ib][q];
      }
  }
}

// Heads backward in the pairing layout (squash, denorm, custom loss, logpi) for narrow heads (NB_PAIR <= 2):
// hd holds the heads (PARK: they are read back from the ADH rows instead) and returns d loss / d heads, which
// is also stored to ADH; d loss / d a_d is read from the image rows [0, AOUT).  Returns the custom-loss partial.
template <class C, bool PARK>
__device__ __forceinline__ float heads_backward(const SacArgs& p, const Lane& L, f32x16 (&hd)[C::NB_PAIR], bool valid,
                                                float g_lp) {
  constexpr bool kParkHeads = PARK;
  float dist_part = 0.f;
  const float cl_scale = valid ? p.custom_loss * 2.f * p.inv_B / (float)C::AOUT : 0.f;
  const int h8 = 8 * L.h;
  {
    // Branch-free over the pairing slots: every lane loads through resources bounded to the
    // arrays (slots j >= AOUT read 0) and computes; results of those slots are dropped.  Per-slot
    // branches would put each load and its use in one block, i.e. one round trip per slot.
    const rsrc_t adhr = rsrc_n(p.ADH, 2 * C::AOUT * L.ld4);
    const rsrc_t epsr = rsrc_n(p.EPS2, C::AOUT * L.ld4);
    const rsrc_t s2r = rsrc_n(p.S2, C::OB * L.ld4);
    const bool closs = p.custom_loss != 0.f;
    SPP_XLANE_SYNC();  // d loss / d a_d was written in the natural layout (other lanes' rows)
#pragma unroll
    for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j0 = 16 * ib + r;
        const int j = j0 + h8;
        const bool ok = j < C::AOUT;
        const int jj = ok ? j : 0;
        const float mu = kParkHeads ? fm_ldb(adhr, j0, L.ld4, L.vp) : hd[ib][r];
        const float lsr = kParkHeads ? fm_ldb(adhr, C::AOUT + j0, L.ld4, L.vp) : hd[ib][r + 8];
        const float e = fm_ldb(epsr, j0, L.ld4, L.vp);
        const float s2 = closs ? fm_ldb(s2r, j0, L.ld4, L.vp) : 0.f;
        const float ls = fminf(fmaxf(lsr, -20.f), 2.f);
        const float sc = expf(ls);
        const float u = fadd_rn(mu, fmul_rn(e, sc));
        const float d = fsub_rn(u, mu);
        const float t = tanhf(u);
        const float lim = actor_lim<true>(p, L.tbl, jj);
        const float a = fmul_rn(t, lim);
        float g_ad = L.pl[j0 * 32];  // from the critics through the ACM
        float g_a = 0.f;
        if (closs) {
          if (p.norm_closs) {
            const float df = fsub_rn(a, normalize<true>(p, L.tbl, jj, s2));
            g_a += cl_scale * df;
            dist_part += (valid && ok) ? df * df : 0.f;
          } else {
            const float df = fsub_rn(denorm<true>(p, L.tbl, jj, a), s2);
            g_ad += cl_scale * df;
            dist_part += (valid && ok) ? df * df : 0.f;
          }
        }
        g_a += g_ad * denorm_scale<true>(p, L.tbl, jj);
        const float var = fmul_rn(sc, sc);
        const float sig_m2u = 1.f / (1.f + expf(2.f * u));  // sigmoid(-2u)
        const float gu = g_a * lim * (1.f - t * t) + g_lp * (-d / var + 2.f - 4.f * sig_m2u);
        const float gmu = gu + g_lp * d / var;
        const float gsc = gu * e + g_lp * (d * d / (var * sc) - 1.f / sc);
        const float gls = (lsr >= -20.f && lsr <= 2.f) ? gsc * sc : 0.f;
        hd[ib][r] = ok ? gmu : 0.f;
        hd[ib][r + 8] = ok ? gls : 0.f;
      }
    // stores after all of the loop's loads (a buffer store would order every later load behind it)
#pragma unroll
    for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j0 = 16 * ib + r;
        if (j0 + h8 < C::AOUT) {
          fm_st(rsrc(p.ADH), j0, L.ld4, L.vp, hd[ib][r]);
          fm_st(rsrc(p.ADH), C::AOUT + j0, L.ld4, L.vp, hd[ib][r + 8]);
        }
      }
  }
  return dist_part;
}

// The chosen critics' action-input gradients of the min-critic split, read back at the sample's own column:
// dca = 0; dca += critic 1's; dca += critic 2's, as the one-kernel phase sums them: there the critic
// that lost the min adds the exact +0 its zero delta2 gives.  Rows >= CA are not read by anything.
template <class C>
__device__ __forceinline__ void load_dca(const AcmScratch& z, const Lane& L, f32x16 (&dca)[C::NB_CA]) {
  const int sel = z.SEL[L.b];
  const rsrc_t r1 = rsrc_n(z.DCA[0], C::CA * L.ld4), r2 = rsrc_n(z.DCA[1], C::CA * L.ld4);
#pragma unroll
  for (int ib = 0; ib < C::NB_CA; ++ib)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ur = 32 * ib + ru(q);
      float v1 = 0.f, v2 = 0.f;
      if (ur < C::CA) {  // (rows ur + 4h >= CA of the upper lane half read 0 through the bounded resource)
        v1 = fm_ldb(r1, ur, L.ld4, L.vo);
        v2 = fm_ldb(r2, ur, L.ld4, L.vo);
      }
      v1 = (sel & 1) ? v1 : 0.f;
      v2 = (sel & 2) ? v2 : 0.f;
      dca[ib][q] = fadd_rn(fadd_rn(0.f, v1), v2);
    }
}

// Actor trunk backward from d loss / d heads in the pairing layout: dh2 = Wh^T dheads * relu'(h2),
// dh1 = W2^T dh2 * relu'(h1), both stored feature-major (AD2 / AD1, the weight-gradient operands).
template <class C>
__device__ __forceinline__ void actor_trunk_backward(const SacArgs& p, const Lane& L, const f32x16 (&hd)[C::NB_PAIR],
                                                     uint64_t a1lo, uint64_t a1hi, uint64_t a2lo, uint64_t a2hi) {
  dense<C::NB_PAIR, C::RV_PAIR, C::BF>(p.actor.WhT, 8, hd, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ur = 32 * ob + ru(q);
      const float v = getbit(a2lo, a2hi, ob, q) ? acc[q] : 0.f;
      L.bl[ur * 32] = v;
      op_st<C::BF>(rsrc(p.AD2), ur, L.ld4, L.vo, v);
    }
  });
  dense_lds<8, C::BF>(p.actor.W2T, L.img, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      op_st<C::BF>(rsrc(p.AD1), 32 * ob + ru(q), L.ld4, L.vo, getbit(a1lo, a1hi, ob, q) ? acc[q] : 0.f);
  });
}
// The same with dh2's blocks produced in registers under the W2^T MFMAs (WhTGen): no LDS image at all.
template <class C>
__device__ __forceinline__ void actor_trunk_backward_gen(const SacArgs& p, const Lane& L,
                                                         const f32x16 (&hd)[C::NB_PAIR], uint64_t a1lo, uint64_t a1hi,
                                                         uint64_t a2lo, uint64_t a2hi) {
  static_assert(!C::BF, "fp32 sets");
  const rsrc_t d2r = rsrc(p.AD2);
  const int ld4 = L.ld4;
  const uint32_t vo = L.vo;
  auto st2 = [=](int ur, float v) { op_st<C::BF>(d2r, ur, ld4, vo, v); };
  WhTGen<C::NB_PAIR, C::RV_PAIR, 8, decltype(st2)> g{hd, rsrc(p.actor.WhT), 16u * lane_id(), a2lo, a2hi, st2};
  g.request(0);
  dense_gen<8>(p.actor.W2T, nullptr, g, [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      op_st<C::BF>(rsrc(p.AD1), 32 * ob + ru(q), L.ld4, L.vo, getbit(a1lo, a1hi, ob, q) ? acc[q] : 0.f);
  });
}

// SPLIT (the min-critic split, fp32 sets): the kernel ends after q = min(Q1, Q2) and hands the rest of the
// phase to k_sac_minq_backward (the chosen critic's backward, samples regrouped by critic) and
// k_sac_actor_heads<C, true> (everything after it, in the original sample order).
// STAGED (the stage split, with SPLIT): a, logpi and the critics' input come from k_sac_trunk_fwd /
// k_sac_squash_stage (p.SCA, p.SLP; the trunk kernel has stored the trunk's masks); the kernel is the critics.
// PAIR (with STAGED; wave pairs, above the critic phase): wave c runs critic c and stores its masks; behind the
// exchange the role-0 wave does what one wave does for the tile: q = min, the partials, SEL and the counts.
template <class C, bool SPLIT = false, bool STAGED = false, bool PAIR = false>
__global__ __launch_bounds__(256, 1) void k_sac_actor_phase(SacArgs p, AcmScratch z) {
  static_assert(SPLIT || !STAGED, "the stage split cuts the split phase");
  static_assert(STAGED || !PAIR, "the pair form is the staged kernel's");
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  const float alpha = *p.alpha;
  const PairMap pm = PAIR ? pair_map(ntiles) : PairMap{};
  int tile = PAIR ? pm.j : blockIdx.x * kWavesPerWG + w;
  for (int k = 0; PAIR ? k < pm.K : tile < ntiles; ++k, tile += PAIR ? pm.P : gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    const int b = L.b;
    const bool valid = b < p.B;
    const float g_lp = valid ? alpha * p.inv_B : 0.f;  // d loss / d logpi_b
    // ---- a, logpi = actor(s)  (sac_acm.py:137)
    uint64_t a1lo = 0, a1hi = 0, a2lo = 0, a2hi = 0;
    f32x16 hd[C::NB_PAIR];
    float lp;
    f32x16 cin[C::NB_CIN];
    constexpr bool kWide = C::NB_PAIR > 2;
    uint64_t ma0 = 0, ma1 = 0, ma2 = 0, ma3 = 0, mb0 = 0, mb1 = 0, mb2 = 0, mb3 = 0;
    float q1, q2;
    if constexpr (PAIR) {
      const bool active = tile < ntiles;  // wave-uniform, and the same for both waves of the pair
      __shared__ PairSlot s_q;  // (here: only the pair forms hold it)
      float* slot = &s_q[w >> 1][k & 1][0][0];
      if (active) {
        SPP_TP(26);
        load_cat_gg<C::NB_OB, C::NB_CA>(cin, p.S, C::OB, p.SCA, C::CA, L.ld4, L.vo);
        q1 = critic_forward<C, false>(p.critic[pm.c], cin, L, nullptr, nullptr, ma0, ma1, ma2, ma3);
        if (L.h == 0) slot[32 * pm.c + L.s] = q1;
        uint4* cm = reinterpret_cast<uint4*>(z.CM + (((int64_t)pm.c * ld + b) * 2 + L.h) * 4);
        cm[0] = make_uint4((uint32_t)ma0, (uint32_t)(ma0 >> 32), (uint32_t)ma1, (uint32_t)(ma1 >> 32));
        cm[1] = make_uint4((uint32_t)ma2, (uint32_t)(ma2 >> 32), (uint32_t)ma3, (uint32_t)(ma3 >> 32));
      }
      __syncthreads();  // every wave of the workgroup, K times
      if (!active || pm.c != 0) continue;
      q2 = slot[32 + L.s];
      lp = p.SLP[b];
    } else if constexpr (STAGED) {
      SPP_TP(26);
      load_cat_gg<C::NB_OB, C::NB_CA>(cin, p.S, C::OB, p.SCA, C::CA, L.ld4, L.vo);
      lp = p.SLP[b];
    } else {
      SPP_TP(26);
      actor_trunk<C, true>(p.actor, p.S, C::OB * L.ld4, L, p.AH1, p.AH2, a1lo, a1hi, a2lo, a2hi);
      SPP_TP(27);  // actor trunk
      load_pair<C>(hd, big);
      lp = squash_write<C>(p, hd, p.EPS2, L);  // a_d -> big rows [0, AOUT)
      SPP_TP(28);  // squash
      // Wide heads (Ant): park mu / raw log-std in the ADH rows the heads backward overwrites
      // (same lane, same element), instead of keeping NB_PAIR tiles live through the critics.
      // The split forward kernel parks them for k_sac_actor_heads whatever their width.
      constexpr bool kParkHeads = kWide || SPLIT;
      if constexpr (kParkHeads) {
#pragma unroll
        for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int j0 = 16 * ib + r;
            if (j0 + 8 * L.h < C::AOUT) {
              fm_st(rsrc(p.ADH), j0, L.ld4, L.vp, hd[ib][r]);
              fm_st(rsrc(p.ADH), C::AOUT + j0, L.ld4, L.vp, hd[ib][r + 8]);
            }
          }
      }
      // ---- critic input [s | ACM(s, a_d)] or [s | a_d]  (:67-72)
      if constexpr (C::ACMC) {
        f32x16 xin[C::NB_ACMIN];
        load_cat_gl<C::NB_OB, C::NB_AOUT>(xin, p.S, C::OB * L.ld4, C::OB, L.ld4, L.vo, big, C::AOUT);
        acm_forward<C, true>(p, xin, L, z.Z1, z.Z2, z.T3);
        load_cat_gl<C::NB_OB, C::NB_CA>(cin, p.S, C::OB * L.ld4, C::OB, L.ld4, L.vo, small, C::AC);
      } else {
        load_cat_gl<C::NB_OB, C::NB_CA>(cin, p.S, C::OB * L.ld4, C::OB, L.ld4, L.vo, big, C::AOUT);
      }
    }
    SPP_TP(29);  // ACM forward
    // ---- q = min(Q1, Q2)(s, c)  (:73-75), masks kept for the backward
    if constexpr (!PAIR) {
      q1 = critic_forward<C, false>(p.critic[0], cin, L, nullptr, nullptr, ma0, ma1, ma2, ma3);
      q2 = critic_forward<C, false>(p.critic[1], cin, L, nullptr, nullptr, mb0, mb1, mb2, mb3);
    }
    const float qmin = fminf(q1, q2);
    // torch.minimum backward: ties split the gradient in half
    const float gq = valid ? -p.inv_B : 0.f;
    const float dqa = q1 < q2 ? gq : (q1 == q2 ? 0.5f * gq : 0.f);
    const float dqb = q2 < q1 ? gq : (q1 == q2 ? 0.5f * gq : 0.f);
    SPP_TP(19);  // q min (the critic layers themselves: slots 30, 31)
    if constexpr (SPLIT) {
      // Hand over: who takes the gradient (dqa != 0: bit 0, dqb != 0: bit 1), both critics' masks, the
      // tile's list counts, the trunk's masks and the loss partials that need logpi / qmin.
      const int sel = valid ? (int)(q1 <= q2) | ((int)(q2 <= q1) << 1) : 0;
      if (L.h == 0) z.SEL[b] = (uint8_t)sel;
      if constexpr (!PAIR) {  // (PAIR: each wave has stored its critic's)
        uint4* cm0 = reinterpret_cast<uint4*>(z.CM + ((int64_t)b * 2 + L.h) * 4);
        uint4* cm1 = reinterpret_cast<uint4*>(z.CM + (((int64_t)ld + b) * 2 + L.h) * 4);
        cm0[0] = make_uint4((uint32_t)ma0, (uint32_t)(ma0 >> 32), (uint32_t)ma1, (uint32_t)(ma1 >> 32));
        cm0[1] = make_uint4((uint32_t)ma2, (uint32_t)(ma2 >> 32), (uint32_t)ma3, (uint32_t)(ma3 >> 32));
        cm1[0] = make_uint4((uint32_t)mb0, (uint32_t)(mb0 >> 32), (uint32_t)mb1, (uint32_t)(mb1 >> 32));
        cm1[1] = make_uint4((uint32_t)mb2, (uint32_t)(mb2 >> 32), (uint32_t)mb3, (uint32_t)(mb3 >> 32));
      }
      const int n1 = __popcll(__ballot(L.h == 0 && (sel & 1))), n2 = __popcll(__ballot(L.h == 0 && (sel & 2)));
      if constexpr (!STAGED) {
        uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
        mk[0] = a1lo;
        mk[64] = a1hi;
        mk[128] = a2lo;
        mk[192] = a2hi;
      }
      const float ps = wave_sum((valid && L.h == 0) ? fsub_rn(alpha * lp, qmin) : 0.f);
      const float pl = wave_sum((valid && L.h == 0) ? lp : 0.f);
      if (lane == 0) {
        z.CNT[tile] = (uint32_t)n1 | ((uint32_t)n2 << 16);
        p.part[tile * kParts + 2] = ps;
        p.part[tile * kParts + 4] = pl;
      }
      continue;
    }
    // ---- back through both critics to their action input
    f32x16 dca[C::NB_CA];
#pragma unroll
    for (int ib = 0; ib < C::NB_CA; ++ib) dca[ib] = zero16();
#pragma unroll 1
    for (int i = 0; i < 2; ++i) {
      const CriticDev& Q = p.critic[i];
      const uint64_t k0 = i ? mb0 : ma0, k1 = i ? mb1 : ma1, k2 = i ? mb2 : ma2, k3 = i ? mb3 : ma3;
      const float dqi = i ? dqb : dqa;
      const float* w3 = tbl + Q.tw3;
      auto epi1 = [&](int ob, const f32x16& acc) {
#pragma unroll
        for (int q = 0; q < 16; ++q) L.bl[(32 * ob + ru(q)) * 32] = getbit(k0, k1, ob, q) ? acc[q] : 0.f;
      };
      if constexpr (C::GEN_AD2) {
        auto st2 = [](int, float) {};
        Delta2Gen<8, decltype(st2)> g{w3, L.h4, k2, k3, dqi, st2, {}};
        SPP_TPN(20);  // (delta2 is produced under the W2T MFMAs)
        dense_gen<8>(Q.W2T, nullptr, g, epi1);
      } else {
#pragma unroll 1
        for (int ob = 0; ob < 8; ++ob) {
          float tv[16];
          tvals(w3, ob, L.h4, tv);
#pragma unroll
          for (int q = 0; q < 16; ++q) L.bl[(32 * ob + ru(q)) * 32] = getbit(k2, k3, ob, q) ? dqi * tv[q] : 0.f;
        }
        SPP_TPN(20);  // delta staging
        dense_lds<8, C::BF>(Q.W2T, big, nullptr, epi1);
      }
      SPP_TPN(21);  // W2T
      dense_lds<C::NB_CA, C::BF>(Q.W1Ta, big, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
        for (int ib = 0; ib < C::NB_CA; ++ib)
          if (ib == ob) dca[ib] += acc;
      });
      SPP_TPN(22);  // W1Ta
    }
    SPP_TP(31);  // critics backward
    // ---- through the frozen ACM to d a_d  (basic_model.py:118-126 backward)
    // (Wide-head configs keep the per-element scratch loads: their registers are taken.)
    dca_to_dad<C, !kWide>(p, z, L, small, dca);
    SPP_TP(16);  // ACM backward
    if constexpr (kWide) {
      // Wide heads: the heads and trunk backward run in k_sac_actor_heads (a second kernel with
      // the whole register file: in one kernel the live ranges spill to scratch, and spilled
      // phase kernels have returned wrong results).  Hand over d a_d and the masks.
      const rsrc_t gr = rsrc(z.GAD);
#pragma unroll
      for (int ib = 0; ib < C::NB_AOUT; ++ib)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ur = 32 * ib + ru(q);
          if (ur + L.h4 < C::AOUT) fm_st(gr, ur, L.ld4, L.vo, L.bl[ur * 32]);
        }
      uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
      mk[0] = a1lo;
      mk[64] = a1hi;
      mk[128] = a2lo;
      mk[192] = a2hi;
      const float ps = wave_sum((valid && L.h == 0) ? fsub_rn(alpha * lp, qmin) : 0.f);
      const float pl = wave_sum((valid && L.h == 0) ? lp : 0.f);
      if (lane == 0) {
        p.part[tile * kParts + 2] = ps;
        p.part[tile * kParts + 4] = pl;
      }
      continue;
    }
    // ---- heads backward in the pairing layout (squash, denorm, custom loss, logpi)
    float sac_part = (valid && L.h == 0) ? fsub_rn(alpha * lp, qmin) : 0.f;
    const float dist_part = heads_backward<C, false>(p, L, hd, valid, g_lp);
    SPP_TP(17);  // heads backward
    // ---- dh2 = Wh^T dheads * relu'(h2); dh1 = W2^T dh2 * relu'(h1)
    actor_trunk_backward<C>(p, L, hd, a1lo, a1hi, a2lo, a2hi);
    SPP_TP(18);  // trunk backward
    const float ps = wave_sum(sac_part);
    const float pd = wave_sum(dist_part);
    const float pl = wave_sum((valid && L.h == 0) ? lp : 0.f);
    if (lane == 0) {
      p.part[tile * kParts + 2] = ps;
      p.part[tile * kParts + 3] = pd;
      p.part[tile * kParts + 4] = pl;
    }
  }
  SPP_TP_FLUSH();
}

// Heads backward for wide heads (NB_PAIR > 2; k_sac_actor_heads): the heads are parked in the ADH rows, d loss / d a_d
// comes from z.GAD, or (IMG) from the image rows [0, AOUT), which the loop overwrites only behind its reads: block
// ib's results go to the rows it has just read and to rows >= AOUT.  hd returns d loss / d heads, also stored to ADH.
template <class C, bool IMG>
__device__ __forceinline__ float heads_backward_wide(const SacArgs& p, const AcmScratch& z, const Lane& L,
                                                     f32x16 (&hd)[C::NB_PAIR], bool valid, float g_lp) {
  float dist_part = 0.f;
  const float cl_scale = valid ? p.custom_loss * 2.f * p.inv_B / (float)C::AOUT : 0.f;
  const rsrc_t adhr = rsrc_n(p.ADH, 2 * C::AOUT * L.ld4);
  const rsrc_t epsr = rsrc_n(p.EPS2, C::AOUT * L.ld4);
  const rsrc_t s2r = rsrc_n(p.S2, C::OB * L.ld4);
  const rsrc_t gr = rsrc_n(z.GAD, C::AOUT * L.ld4);
  const bool closs = p.custom_loss != 0.f;
  const int h8 = 8 * L.h;
  if constexpr (IMG) SPP_XLANE_SYNC();  // d loss / d a_d was written in the natural layout (other lanes' rows)
  // one pairing block per iteration (not unrolled: a block's loads and math stay within the
  // iteration); results go to the LDS image in the pairing layout (rows j / AOUT + j)
#pragma unroll 1
  for (int ib = 0; ib < C::NB_PAIR; ++ib) {
    float mu[8], lsr[8], ev[8], s2v[8], gv[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j0 = 16 * ib + r;
      mu[r] = fm_ldb(adhr, j0, L.ld4, L.vp);
      lsr[r] = fm_ldb(adhr, C::AOUT + j0, L.ld4, L.vp);
      ev[r] = fm_ldb(epsr, j0, L.ld4, L.vp);
      s2v[r] = closs ? fm_ldb(s2r, j0, L.ld4, L.vp) : 0.f;
      if constexpr (IMG) gv[r] = j0 + h8 < C::AOUT ? L.pl[j0 * 32] : 0.f;
      else gv[r] = fm_ldb(gr, j0, L.ld4, L.vp);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j0 = 16 * ib + r;
      const int j = j0 + h8;
      const bool ok = j < C::AOUT;
      const int jj = ok ? j : 0;
      constexpr bool F = C::BF;
      const float e = ev[r];
      const float ls = fminf(fmaxf(lsr[r], -20.f), 2.f);
      const float sc = t_exp<F>(ls);
      const float u = fadd_rn(mu[r], fmul_rn(e, sc));
      const float d = fsub_rn(u, mu[r]);
      const float t = t_tanh<F>(u);
      const float lim = actor_lim<true>(p, L.tbl, jj);
      const float a = fmul_rn(t, lim);
      float g_ad = gv[r];  // from the critics through the ACM
      float g_a = 0.f;
      if (closs) {
        if (p.norm_closs) {
          const float df = fsub_rn(a, normalize<true>(p, L.tbl, jj, s2v[r]));
          g_a += cl_scale * df;
          dist_part += (valid && ok) ? df * df : 0.f;
        } else {
          const float df = fsub_rn(denorm<true>(p, L.tbl, jj, a), s2v[r]);
          g_ad += cl_scale * df;
          dist_part += (valid && ok) ? df * df : 0.f;
        }
      }
      g_a += g_ad * denorm_scale<true>(p, L.tbl, jj);
      const float var = fmul_rn(sc, sc);
      const float ivar = t_rcp<F>(var), isc = t_rcp<F>(sc);
      const float sig_m2u = t_rcp<F>(1.f + t_exp<F>(2.f * u));  // sigmoid(-2u)
      const float gu = g_a * lim * (1.f - t * t) + g_lp * (-d * ivar + 2.f - 4.f * sig_m2u);
      const float gmu = gu + g_lp * d * ivar;
      const float gsc = gu * e + g_lp * (d * d * ivar * isc - isc);
      const float gls = (lsr[r] >= -20.f && lsr[r] <= 2.f) ? gsc * sc : 0.f;
      if (ok) {  // slot j >= AOUT would land on row AOUT + j' of a valid slot's log-std
        L.pl[j0 * 32] = gmu;
        L.pl[(C::AOUT + j0) * 32] = gls;
      }
    }
  }
  load_pair<C>(hd, L.img);
  // the heads' gradient operands (dW of fc_prob / fc_scale), after every load above
#pragma unroll
  for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j0 = 16 * ib + r;
      if (j0 + h8 < C::AOUT) {
        fm_st(rsrc(p.ADH), j0, L.ld4, L.vp, hd[ib][r]);
        fm_st(rsrc(p.ADH), C::AOUT + j0, L.ld4, L.vp, hd[ib][r + 8]);
      }
    }
  return dist_part;
}

// ============================================================================ actor phase, wide heads
// k_sac_actor_heads: the heads backward (squash, denormalisation, custom loss, logpi, in the
// pairing layout) and the trunk backward of the actor phase for wide heads (Ant), after
// k_sac_actor_phase handed over d loss / d a_d (z.GAD) and the trunk's ReLU masks (z.MASK).  One
// pairing block at a time: the block's parked heads, eps, targets and d a_d are requested together
// (one round trip per block), the limit / normaliser vectors come from the LDS table, and the
// results stay in registers (the WhT layer's input tile) until every load has been issued.
//
// SPLIT (the min-critic split, any head width): the kernel is everything behind the critics' backward.  It
// sums the chosen critics' action-input gradients (z.DCA, selected by z.SEL), runs the frozen-ACM backward
// into the image, and then the heads backward of the set's width (d a_d is read from the image, not from
// z.GAD) and the trunk backward.
template <class C, bool SPLIT = false>
__global__ __launch_bounds__(256, 1) void k_sac_actor_heads(SacArgs p, AcmScratch z) {
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  const float alpha = *p.alpha;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    const bool valid = L.b < p.B;
    const float g_lp = valid ? alpha * p.inv_B : 0.f;
    constexpr bool kWide = C::NB_PAIR > 2;
    if constexpr (SPLIT) {
      f32x16 dca[C::NB_CA];
      load_dca<C>(z, L, dca);
      SPP_TP(31);  // critics backward (here: its results read back)
      dca_to_dad<C, true>(p, z, L, small, dca);
      SPP_TP(16);  // ACM backward
    }
    const uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
    const uint64_t a1lo = mk[0], a1hi = mk[64], a2lo = mk[128], a2hi = mk[192];
    float dist_part = 0.f;
    f32x16 hd[C::NB_PAIR];
    if constexpr (!kWide) {
      dist_part = heads_backward<C, true>(p, L, hd, valid, g_lp);
    } else {
      dist_part = heads_backward_wide<C, SPLIT>(p, z, L, hd, valid, g_lp);
    }
    SPP_TP(17);  // heads backward
    // ---- dh2 = Wh^T dheads * relu'(h2); dh1 = W2^T dh2 * relu'(h1)
    actor_trunk_backward<C>(p, L, hd, a1lo, a1hi, a2lo, a2hi);
    SPP_TP(18);  // trunk backward
    const float pd = wave_sum(dist_part);
    if (lane == 0) p.part[tile * kParts + 3] = pd;
  }
  SPP_TP_FLUSH();
}

// ============================================================================ actor phase, stage split
// k_sac_actor_heads<C, true> for narrow heads (NB_PAIR <= 2) cut in two at its hand-over point (the ADH rows):
//
//  k_sac_heads_stage      the per-sample stages: the chosen critics' gradients read back (z.SEL, z.DCA), the
//                         frozen-ACM backward, the heads backward; d loss / d heads goes to ADH (as before: it is
//                         the heads' weight-gradient operand) and the custom-loss partial to its slot.
//  k_sac_actor_trunk_bwd  d loss / d heads read back from ADH into the pairing tile, the trunk's masks from
//                         z.MASK, then Wh^T and W2^T with the AD2 / AD1 stores.
//
// The stages are libm transcendentals, three small dependent MFMA chains with LDS round trips between them and
// HBM read-backs: latency, not MFMA issue.  In the phase kernel they run one wave per SIMD (its register file and
// 32 KiB image) while the MFMA pipe idles.  The stage kernel keeps only what they touch (a per-wave image of
// 16 NB_PAIR heads / a_d rows and the ACM's 64 rows, and a table of the limit / normaliser vectors: the host
// passes an argument block whose table segments are those four, at offset 0), so several workgroups share a CU.
// Both kernels call the phase kernel's device functions on the same values in the same order: every array is
// bit-identical to k_sac_actor_heads<C, true>'s.
//
// The forward side of both phases is cut the same way, in three (ACT: the actor phase on S / EPS2 with the
// operand, mask and Z stores; else the critic phase's target action on S2 / EPS1):
//
//  k_sac_trunk_fwd<C, ACT>      actor_trunk; the heads epilogue stores mu / raw log-std feature-major (ACT: to the
//                               ADH rows, where the split forward kernel parks them; else to p.THD)
//  k_sac_squash_stage<C, ACT>   the squash from those rows and eps, the ACM forward; the critics' action input
//                               goes to p.SCA [CA][Bp] and log pi to p.SLP [Bp]
//  k_sac_actor_phase<C, true, true> / k_sac_critic_phase<C, true>   the rest of the phase from S | SCA and SLP
//
// The three trunk kernels have register hand-over forms (k_sac_trunk_fwd_gen<C, ACT>: Fc1Gen under fc2;
// k_sac_actor_trunk_bwd_gen: WhTGen under W2^T, no LDS at all), chosen per handle (SPP_ACTOR_GEN, api.hip); the
// generators run the staged layers' MFMA chains, so every array is bit-identical here too.

// floats: the ACM's three bias vectors (64 + 32 + 32) and actor_lim, acm_lim, n0, n1 (32 each: aout, ac <= 32)
constexpr int kStageTab = 256;

template <class C>
__global__ __launch_bounds__(256, 2) void k_sac_heads_stage(SacArgs p, AcmScratch z) {
  static_assert(C::NB_PAIR <= 2 && !C::BF, "narrow heads, fp32");
  constexpr int HR = 16 * C::NB_PAIR;  // pairing rows j0 + 8h < 16 NB_PAIR; natural rows u + 4h < AOUT <= HR
  constexpr int ROWS = HR + 64;        // + the ACM's SMALL image
  __shared__ __attribute__((aligned(16))) float smem[kWavesPerWG * ROWS * 32];
  __shared__ __attribute__((aligned(16))) float tbl[kStageTab];
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * ROWS * 32;
  float* small = big + HR * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  const float alpha = *p.alpha;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    const bool valid = L.b < p.B;
    const float g_lp = valid ? alpha * p.inv_B : 0.f;
    f32x16 dca[C::NB_CA];
    load_dca<C>(z, L, dca);
    SPP_TP(31);  // critics backward (here: its results read back)
    dca_to_dad<C, true>(p, z, L, small, dca);
    SPP_TP(16);  // ACM backward
    f32x16 hd[C::NB_PAIR];
    const float dist_part = heads_backward<C, true>(p, L, hd, valid, g_lp);
    SPP_TP(17);  // heads backward
    const float pd = wave_sum(dist_part);
    if (lane == 0) p.part[tile * kParts + 3] = pd;
  }
  SPP_TP_FLUSH();
}

template <class C>
__global__ __launch_bounds__(256, 1) void k_sac_actor_trunk_bwd(SacArgs p, AcmScratch z) {
  static_assert(C::NB_PAIR <= 2 && !C::BF, "narrow heads, fp32");
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  SPP_TP_INIT();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, nullptr, ld, tile * 32 + (lane & 31));
    const uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
    const uint64_t a1lo = mk[0], a1hi = mk[64], a2lo = mk[128], a2hi = mk[192];
    // d loss / d heads at the pairing slots (heads_backward's stores); slots j >= AOUT hold 0, as its tile does
    f32x16 hd[C::NB_PAIR];
    load_pair_gl<C>(hd, p.ADH, L.ld4, L.vp);
    SPP_TP(17);  // heads backward (here: its results read back)
    actor_trunk_backward<C>(p, L, hd, a1lo, a1hi, a2lo, a2hi);
    SPP_TP(18);  // trunk backward
  }
  SPP_TP_FLUSH();
}
// k_sac_actor_trunk_bwd with Wh^T's blocks handed to W2^T in registers (Cfg::GEN_AWHT): no LDS image, no table
template <class C>
__global__ __launch_bounds__(256, 1) void k_sac_actor_trunk_bwd_gen(SacArgs p, AcmScratch z) {
  static_assert(C::GEN_AWHT, "narrow heads, fp32, one observation block");
  SPP_TP_INIT();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(nullptr, nullptr, nullptr, ld, tile * 32 + (lane & 31));
    const uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
    const uint64_t a1lo = mk[0], a1hi = mk[64], a2lo = mk[128], a2hi = mk[192];
    f32x16 hd[C::NB_PAIR];
    load_pair_gl<C>(hd, p.ADH, L.ld4, L.vp);
    SPP_TP(17);  // heads backward (here: its results read back)
    actor_trunk_backward_gen<C>(p, L, hd, a1lo, a1hi, a2lo, a2hi);
    SPP_TP(18);  // trunk backward
  }
  SPP_TP_FLUSH();
}

// GEN: actor_trunk with fc1 handed to fc2 in registers
template <class C, bool ACT, bool GEN>
__device__ __forceinline__ void trunk_fwd_tiles(const SacArgs& p, const AcmScratch& z, float* smem, const float* tbl) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    uint64_t a1lo = 0, a1hi = 0, a2lo = 0, a2hi = 0;
    SPP_TP(ACT ? 26 : 0);
    if constexpr (ACT) {
      actor_trunk<C, true, C::NB_H2, 2 * C::AOUT, true, GEN>(p.actor, p.S, C::OB * L.ld4, L, p.AH1, p.AH2, a1lo, a1hi,
                                                             a2lo, a2hi, p.ADH);
      uint64_t* mk = z.MASK + (int64_t)tile * 4 * 64 + lane;
      mk[0] = a1lo;
      mk[64] = a1hi;
      mk[128] = a2lo;
      mk[192] = a2hi;
      SPP_TP(27);  // actor trunk
    } else {
      actor_trunk<C, false, C::NB_H2, 2 * C::AOUT, true, GEN>(p.actor, p.S2, C::OB * L.ld4, L, nullptr, nullptr, a1lo,
                                                              a1hi, a2lo, a2hi, p.THD);
    }
  }
}

template <class C, bool ACT>
__global__ __launch_bounds__(256, 1) void k_sac_trunk_fwd(SacArgs p, AcmScratch z) {
  static_assert(C::NB_PAIR <= 2 && !C::BF, "narrow heads, fp32");
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  SPP_TP_INIT();
  load_table(p, tbl);
  trunk_fwd_tiles<C, ACT, false>(p, z, smem, tbl);
  SPP_TP_FLUSH();
}
template <class C, bool ACT>
__global__ __launch_bounds__(256, 1) void k_sac_trunk_fwd_gen(SacArgs p, AcmScratch z) {
  static_assert(C::GEN_AFC1, "narrow heads, fp32, one observation block");
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  SPP_TP_INIT();
  load_table(p, tbl);
  trunk_fwd_tiles<C, ACT, true>(p, z, smem, tbl);
  SPP_TP_FLUSH();
}

template <class C, bool ACT>
__global__ __launch_bounds__(256, 2) void k_sac_squash_stage(SacArgs p, AcmScratch z) {
  static_assert(C::NB_PAIR <= 2 && !C::BF, "narrow heads, fp32");
  constexpr int HR = 16 * C::NB_PAIR;  // (as k_sac_heads_stage)
  constexpr int ROWS = HR + 64;
  __shared__ __attribute__((aligned(16))) float smem[kWavesPerWG * ROWS * 32];
  __shared__ __attribute__((aligned(16))) float tbl[kStageTab];
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * ROWS * 32;
  float* small = big + HR * 32;
  const int ntiles = p.Bp / 32;
  const int ld = p.Bp;
  const float* X = ACT ? p.S : p.S2;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    SPP_TP(ACT ? 26 : 0);
    f32x16 hd[C::NB_PAIR];
    load_pair_gl<C>(hd, ACT ? p.ADH : p.THD, L.ld4, L.vp);
    // (the critic phase squashes branch-free, the actor phase with the per-slot branches: as the phase kernels)
    const float lp = squash_write<C, !ACT>(p, hd, ACT ? p.EPS2 : p.EPS1, L);  // a_d -> big rows [0, AOUT)
    SPP_TP(ACT ? 28 : 4);  // squash
    if constexpr (C::ACMC) {
      f32x16 xin[C::NB_ACMIN];
      load_cat_gl<C::NB_OB, C::NB_AOUT>(xin, X, C::OB * L.ld4, C::OB, L.ld4, L.vo, big, C::AOUT);
      acm_forward<C, ACT>(p, xin, L, z.Z1, z.Z2, z.T3);
    }
    // the critics' action input, natural layout: c from SMALL rows [0, AC) (this lane's own stores), or a_d from
    // the image rows [0, AOUT) (written in the pairing layout: other lanes' rows)
    SPP_XLANE_SYNC();
    const float* src = C::ACMC ? L.sl : L.bl;
    const rsrc_t cr = rsrc(p.SCA);
#pragma unroll
    for (int ib = 0; ib < C::NB_CA; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ib + ru(q);
        if (ur < C::CA) {
          if (ur + L.h4 < C::CA) fm_st(cr, ur, L.ld4, L.vo, src[ur * 32]);
        }
      }
    if (L.h == 0) p.SLP[L.b] = lp;
    SPP_TP(ACT ? 29 : 5);  // ACM forward
  }
  SPP_TP_FLUSH();
}

// ============================================================================ actor phase, min-critic split
// k_sac_minq_backward: the critics' backward to their action input, for the critic(s) whose Q took the min only.
// The actor loss uses min(Q1, Q2), so per sample the other critic's upstream gradient is exactly 0 (an exact tie
// gives each 1/2), and its W2^T / W1^T a MFMAs multiply zeros.  Samples are the MFMA's N dimension and the two
// critics have different weights, so the zeros can only be skipped by regrouping the samples by critic over the
// whole batch: a group is 32 entries of one critic's list (k_minq_scatter), and the two lists give
// ceil(n1 / 32) + ceil(n2 / 32) groups where the one-kernel phase runs 2 * Bp / 32 critic tiles.  An MFMA output
// column depends on its own input column only, so a sample's values do not depend on the group or lane it lands
// in.  The results go to the sample's own column of z.DCA[critic]; k_sac_actor_heads<C, true> adds them.
template <class C>
__global__ __launch_bounds__(256, 1) void k_sac_minq_backward(SacArgs p, AcmScratch z) {
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  SPP_TP_INIT();
  load_table(p, tbl);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ld = p.Bp;
  const int n1 = z.NG[0], n2 = z.NG[1];  // <= B each
  const int g1 = (n1 + 31) >> 5, ngroups = g1 + ((n2 + 31) >> 5);
  for (int g = blockIdx.x * kWavesPerWG + w; g < ngroups; g += gridDim.x * kWavesPerWG) {
    const int i = g >= g1;  // this group's critic (wave-uniform)
    const int pos = 32 * (i ? g - g1 : g) + (lane & 31);
    const bool live = pos < (i ? n2 : n1);  // padding lanes of a list's last group: dq = 0, nothing stored
    const int b = live ? z.LIST[i][pos] : 0;
    const Lane L = make_lane(big, small, tbl, ld, b);
    const uint4* cm = reinterpret_cast<const uint4*>(z.CM + (((int64_t)i * ld + b) * 2 + L.h) * 4);
    const uint4 c01 = cm[0], c23 = cm[1];
    const int sel = z.SEL[b];
    const uint64_t k0 = live ? (uint64_t)c01.x | ((uint64_t)c01.y << 32) : 0;
    const uint64_t k1 = live ? (uint64_t)c01.z | ((uint64_t)c01.w << 32) : 0;
    const uint64_t k2 = live ? (uint64_t)c23.x | ((uint64_t)c23.y << 32) : 0;
    const uint64_t k3 = live ? (uint64_t)c23.z | ((uint64_t)c23.w << 32) : 0;
    // torch.minimum backward: ties split the gradient in half (list entries are samples b < B)
    const float gq = -p.inv_B;
    const float dqi = live ? (sel == 3 ? 0.5f * gq : gq) : 0.f;
    const CriticDev& Q = p.critic[i];
    const float* w3 = tbl + Q.tw3;
    auto epi1 = [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) L.bl[(32 * ob + ru(q)) * 32] = getbit(k0, k1, ob, q) ? acc[q] : 0.f;
    };
    if constexpr (C::GEN_AD2) {
      auto st2 = [](int, float) {};
      Delta2Gen<8, decltype(st2)> gen{w3, L.h4, k2, k3, dqi, st2, {}};
      SPP_TPN(20);  // (delta2 is produced under the W2T MFMAs)
      dense_gen<8>(Q.W2T, nullptr, gen, epi1);
    } else {
#pragma unroll 1
      for (int ob = 0; ob < 8; ++ob) {
        float tv[16];
        tvals(w3, ob, L.h4, tv);
#pragma unroll
        for (int q = 0; q < 16; ++q) L.bl[(32 * ob + ru(q)) * 32] = getbit(k2, k3, ob, q) ? dqi * tv[q] : 0.f;
      }
      SPP_TPN(20);  // delta staging
      dense_lds<8, C::BF>(Q.W2T, big, nullptr, epi1);
    }
    SPP_TPN(21);  // W2T
    const rsrc_t dr = rsrc(z.DCA[i]);
    dense_lds<C::NB_CA, C::BF>(Q.W1Ta, big, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        if (ur < C::CA) {
          if (live && ur + L.h4 < C::CA) fm_st(dr, ur, L.ld4, L.vo, acc[q]);
        }
      }
    });
    SPP_TPN(22);  // W1Ta
  }
  SPP_TP_FLUSH();
}

#ifndef SPP_KSET_TU  // non-template kernels live in the api.hip translation unit only
// The two lists of the min-critic split from the per-tile counts (AcmScratch): list i holds the samples whose
// selector has bit i, ascending (a stable partition by exclusive prefix sums; no atomics).
// k_minq_scan: one workgroup; thread t sums the counts of its run of consecutive tiles, the runs' sums are
// scanned in LDS, and the thread walks its run again to write each tile's two list positions.
constexpr int kMinqScanThreads = 1024;
__global__ __launch_bounds__(kMinqScanThreads) void k_minq_scan(const uint32_t* CNT, uint32_t* OFF, int* NG, int ntiles) {
  __shared__ uint32_t s1[kMinqScanThreads], s2[kMinqScanThreads];
  const int t = threadIdx.x;
  const int per = (ntiles + kMinqScanThreads - 1) / kMinqScanThreads;
  const int t0 = min(t * per, ntiles), t1 = min(t0 + per, ntiles);
  uint32_t a1 = 0, a2 = 0;
  for (int k = t0; k < t1; ++k) {
    const uint32_t c = CNT[k];
    a1 += c & 0xffffu;
    a2 += c >> 16;
  }
  s1[t] = a1;
  s2[t] = a2;
  __syncthreads();
  for (int o = 1; o < kMinqScanThreads; o <<= 1) {  // inclusive scan of the runs' sums
    const uint32_t u1 = t >= o ? s1[t - o] : 0u, u2 = t >= o ? s2[t - o] : 0u;
    __syncthreads();
    s1[t] += u1;
    s2[t] += u2;
    __syncthreads();
  }
  uint32_t o1 = s1[t] - a1, o2 = s2[t] - a2;
  for (int k = t0; k < t1; ++k) {
    const uint32_t c = CNT[k];
    OFF[2 * k] = o1;
    OFF[2 * k + 1] = o2;
    o1 += c & 0xffffu;
    o2 += c >> 16;
  }
  if (t == kMinqScanThreads - 1) {
    NG[0] = (int)s1[t];
    NG[1] = (int)s2[t];
  }
}
// k_minq_scatter: one thread per sample (a wave covers two tiles); a sample's rank within its tile comes from
// the wave ballot, so each list is ascending in the sample index.
__global__ __launch_bounds__(256) void k_minq_scatter(const uint8_t* SEL, const uint32_t* OFF, int* L1, int* L2, int Bp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int sel = b < Bp ? SEL[b] : 0;
  const int sh = threadIdx.x & 32;  // this tile's half of the ballot
  const uint32_t below = (1u << (threadIdx.x & 31)) - 1u;
  const uint32_t m1 = (uint32_t)(__ballot(sel & 1) >> sh), m2 = (uint32_t)(__ballot(sel & 2) >> sh);
  if (sel & 1) L1[OFF[2 * (b >> 5)] + __popc(m1 & below)] = b;
  if (sel & 2) L2[OFF[2 * (b >> 5) + 1] + __popc(m2 & below)] = b;
}
#endif  // SPP_KSET_TU

// ============================================================================ rollout action
struct ActArgs {
  int E, mode, denorm_out;
  float act_noise;
  const float *obs, *eps, *noise;  // row-major [E][ob], [E][aout]
  float *target_out, *env_out;     // [E][aout], [E][ac]
  int plain;  // vanilla SAC (sac.py + DDPG.noise_action, ddpg.py:171-176): no ACM, env action = actor action
};

template <class C>
__global__ __launch_bounds__(256, 1) void k_policy_act(SacArgs p, ActArgs a) {
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = (a.E + 31) / 32;
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const int e = tile * 32 + (lane & 31);
    const bool valid = e < a.E;
    const int er = valid ? e : 0;
    // row-major obs: element (unit u, env e) = obs[e*OB + u] -> ld = 1, offset 4h + e*OB
    Lane L = make_lane(big, small, tbl, 1, er * C::OB);
    const bool use_actor = a.mode == 1 || a.mode == 2;
    if (use_actor) {
      uint64_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
      actor_trunk<C, false>(p.actor, a.obs, a.E * C::OB * 4, L, nullptr, nullptr, d0, d1, d2, d3);
    }
    f32x16 hd[C::NB_PAIR];
    if (use_actor) load_pair<C>(hd, big);
    const int h8 = 8 * L.h;
#pragma unroll
    for (int ib = 0; ib < C::NB_PAIR; ++ib)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j0 = 16 * ib + r;
        const int j = j0 + h8;
        if (j < C::AOUT) {
          const float lim = actor_lim<true>(p, L.tbl, j);
          float act;
          if (a.plain && (a.mode == 0 || a.mode == 3)) {
            act = valid ? a.eps[er * C::AOUT + j] : 0.f;  // action_space.sample() drawn by the caller (ddpg.py:178-180)
          } else if (a.plain) {  // DDPG.noise_action: a + act_noise * N(0,1), clip to [-lim, lim]
            const float mu = hd[ib][r];
            float u = mu;
            if (a.mode == 1 && a.eps) {
              const float ls = fminf(fmaxf(hd[ib][r + 8], -20.f), 2.f);
              u = fadd_rn(mu, fmul_rn(valid ? a.eps[er * C::AOUT + j] : 0.f, expf(ls)));
            }
            act = fmul_rn(tanhf(u), lim);
            if (a.mode == 1 && a.noise) act = fadd_rn(act, a.act_noise * (valid ? a.noise[er * C::AOUT + j] : 0.f));
            act = fminf(fmaxf(act, -lim), lim);
          } else if (a.mode == 0) {
            act = valid ? lim * a.eps[er * C::AOUT + j] : 0.f;  // off_policy.py:50-54
          } else if (a.mode == 3) {
            act = valid ? a.eps[er * C::AOUT + j] : 0.f;  // caller's action (on-policy process_action)
          } else {
            const float mu = hd[ib][r];
            float u = mu;
            if (a.mode == 1 && a.eps) {
              const float ls = fminf(fmaxf(hd[ib][r + 8], -20.f), 2.f);
              u = fadd_rn(mu, fmul_rn(valid ? a.eps[er * C::AOUT + j] : 0.f, expf(ls)));
            }
            act = fmul_rn(tanhf(u), lim);
            if (a.mode == 1 && a.noise) act += fmul_rn(a.act_noise * (valid ? a.noise[er * C::AOUT + j] : 0.f), lim);
            act = fminf(fmaxf(act, -1.1f * lim), 1.1f * lim);  // ddpg_acm.py:43-45
          }
          if (a.denorm_out && !a.plain) act = denorm<true>(p, L.tbl, j, act);
          L.pl[j0 * 32] = act;
          if (valid) a.target_out[er * C::AOUT + j] = act;
          if (valid && a.plain) a.env_out[er * C::AOUT + j] = act;  // process_action: identity (ddpg.py:371-384)
        }
      }
    if (a.plain) continue;
    // env action = ACM(cat(obs, a))  (off_policy.py:89-106)
    f32x16 xin[C::NB_ACMIN];
    load_cat_gl<C::NB_OB, C::NB_AOUT>(xin, a.obs, a.E * C::OB * 4, C::OB, L.ld4, L.vo, big, C::AOUT);
    acm_forward<C, false>(p, xin, L, nullptr, nullptr, nullptr);
    if (L.h == 0 && valid)
      for (int u = 0; u < C::AC; ++u) a.env_out[er * C::AC + u] = small[u * 32 + L.s];
  }
}

// ============================================================================ ACM regression
// acm.py:246-258: forward + MSE backward; writes the dW operands feature-major.
struct AcmRegArgs {
  int B, Bp;
  const float *x, *y;                   // row-major [B][2ob], [B][ac]
  float *XT, *Z1, *Z2, *P1, *P2, *P3;  // feature-major [.][Bp]
  float* part;                          // [ntiles]
};

template <class C>
__global__ __launch_bounds__(256, 1) void k_acm_regress(SacArgs p, AcmRegArgs g) {
  __shared__ float smem[kWavesPerWG * kLdsPerWave];
  __shared__ __attribute__((aligned(16))) float tbl[kTabMax];
  load_table(p, tbl);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* big = smem + w * kLdsPerWave;
  float* small = big + kSmallRow * 32;
  const int ntiles = g.Bp / 32;
  const int ld = g.Bp;
  constexpr int IN = 2 * C::OB;
  constexpr int NB_IN = blocks_of(IN);
  constexpr uint64_t RV_IN = rv_nat(IN, NB_IN);
  for (int tile = blockIdx.x * kWavesPerWG + w; tile < ntiles; tile += gridDim.x * kWavesPerWG) {
    const Lane L = make_lane(big, small, tbl, ld, tile * 32 + (lane & 31));
    const int b = L.b;
    const bool valid = b < g.B;
    const int br = valid ? b : 0;
    f32x16 xin[NB_IN];
#pragma unroll
    for (int ib = 0; ib < NB_IN; ++ib)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ur = 32 * ib + ru(r);
        const int u = ur + L.h4;
        xin[ib][r] = (u < IN && valid) ? g.x[br * IN + u] : 0.f;
      }
    // stores after all loads (a buffer store orders every later load behind it)
#pragma unroll
    for (int ib = 0; ib < NB_IN; ++ib)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ur = 32 * ib + ru(r);
        if (ur + L.h4 < IN) fm_st(rsrc(g.XT), ur, L.ld4, L.vo, xin[ib][r]);
      }
    dense<NB_IN, RV_IN, C::BF>(p.acm.W1, 2, xin, tbl + p.acm.tb1, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        const float v = tanhf(acc[q]);
        L.sl[ur * 32] = v;
        fm_st(rsrc(g.Z1), ur, L.ld4, L.vo, v);
      }
    });
    f32x16 z1[2];
    lds_load<2>(z1, small);
    dense<2, C::RV_Z1, C::BF>(p.acm.W2, 1, z1, tbl + p.acm.tb2, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float v = tanhf(acc[q]);
        L.sl[ru(q) * 32] = v;
        fm_st(rsrc(g.Z2), ru(q), L.ld4, L.vo, v);
      }
    });
    f32x16 z2[1];
    lds_load<1>(z2, small);
    float lsum = 0.f;
    f32x16 p3[1];
    const float sc = 2.f / ((float)g.B * (float)C::AC);
    float limv[16], yv[16];  // requested before the layer (see above)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = ru(q) + L.h4;
      const int uu = u < C::AC ? u : 0;
      limv[q] = acm_lim<true>(p, L.tbl, uu);
      yv[q] = g.y[br * C::AC + uu];
    }
    dense<1, C::RV_Z2, C::BF>(p.acm.W3, 1, z2, tbl + p.acm.tb3, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int u = ru(q) + L.h4;
        float v = 0.f;
        if (u < C::AC && valid) {
          const float t = tanhf(acc[q]);
          const float lim = limv[q];
          const float df = fsub_rn(fmul_rn(t, lim), yv[q]);
          lsum += df * df;
          v = sc * df * lim * (1.f - t * t);
        }
        p3[0][q] = v;
        if (u < C::AC) fm_st(rsrc(g.P3), ru(q), L.ld4, L.vo, v);
      }
    });
    dense<1, C::RV_AC, C::BF>(p.acm.W3T, 1, p3, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float zz = z2[0][q];
        const float v = acc[q] * (1.f - zz * zz);
        L.sl[ru(q) * 32] = v;
        fm_st(rsrc(g.P2), ru(q), L.ld4, L.vo, v);
      }
    });
    f32x16 p2[1];
    lds_load<1>(p2, small);
    dense<1, C::RV_Z2, C::BF>(p.acm.W2T, 2, p2, nullptr, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int ur = 32 * ob + ru(q);
        const float zz = ob == 0 ? z1[0][q] : z1[1][q];
        fm_st(rsrc(g.P1), ur, L.ld4, L.vo, acc[q] * (1.f - zz * zz));
      }
    });
    const float ls = wave_sum(lsum);
    if (lane == 0) g.part[tile] = ls;
  }
}

#ifndef SPP_KSET_TU  // non-template kernels live in the api.hip translation unit only
// ============================================================================ staging
// Row-major caller batch (sample_batch layout) -> feature-major padded scratch.
struct StageArgs {
  int B, Bp, ob, aout, ac;
  const float *obs, *next_obs, *act, *rew, *acm;
  const int8_t* done;
  const float *eps1, *eps2;  // [B][aout] or NULL
  float *S, *S2, *ACT, *AENV, *R, *DN, *EPS1, *EPS2;
};
__global__ void k_stage_batch(StageArgs a) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.Bp) return;
  const bool v = b < a.B;
  const int64_t ld = a.Bp;
  for (int f = 0; f < a.ob; ++f) {
    a.S[f * ld + b] = v ? a.obs[b * a.ob + f] : 0.f;
    a.S2[f * ld + b] = v ? a.next_obs[b * a.ob + f] : 0.f;
  }
  for (int f = 0; f < a.aout; ++f) {
    if (a.act) a.ACT[f * ld + b] = v ? a.act[b * a.aout + f] : 0.f;
    if (a.eps1) a.EPS1[f * ld + b] = v ? a.eps1[b * a.aout + f] : 0.f;
    if (a.eps2) a.EPS2[f * ld + b] = v ? a.eps2[b * a.aout + f] : 0.f;
  }
  for (int f = 0; f < a.ac; ++f) a.AENV[f * ld + b] = v ? a.acm[b * a.ac + f] : 0.f;
  a.R[b] = v ? a.rew[b] : 0.f;
  a.DN[b] = v ? (float)a.done[b] : 0.f;
}

// The staged batch's sample_batch tail (replay_buffer.py:247-249) and DDPG_AcM.make_unbiased_update
// (acm/off_policy/ddpg_acm.py:59-73) on the feature-major staging arrays [ob][Bp]: with `norm`, the staged
// obs and next obs are normalised in place (the buffer's obs_norm); with `act_next`, the critic's action
// operand becomes the (normalised) next obs.  Columns b >= B (padding) stay zero.
__global__ void k_stage_post(float* S, float* S2, float* ACT, int ob, int B, int Bp, const float* lo, const float* hi,
                             const float* mean, const float* std, int min_max, int norm, int act_next) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)ob * B) return;
  const int f = (int)(i / B), b = (int)(i - (int64_t)f * B);
  const int64_t o = (int64_t)f * Bp + b;
  float s2 = S2[o];
  if (norm) {
    S[o] = obs_norm1(S[o], f, lo, hi, mean, std, min_max, 0);
    s2 = obs_norm1(s2, f, lo, hi, mean, std, min_max, 0);
    S2[o] = s2;
  }
  if (act_next) ACT[o] = s2;
}

// Caller eps [B][aout] -> feature-major [aout][Bp] (zero padded).
__global__ void k_eps_copy_fm(const float* eps, float* E, int aout, int B, int Bp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)aout * Bp) return;
  const int64_t j = i / Bp, b = i % Bp;
  E[i] = b < B ? eps[b * aout + j] : 0.f;
}

// Feature-major [aout][Bp] -> row-major [B][aout] (read-back of the staged eps).
__global__ void k_eps_read_fm(const float* E, float* eps, int aout, int B, int Bp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)aout * B) return;
  const int64_t b = i / aout, j = i % aout;
  eps[i] = E[j * Bp + b];
}

// Device-side Gaussian eps straight into the feature-major layout (zero padded).
// Box-Muller with the hardware transcendentals (v_log_f32, v_sqrt_f32, v_sin/cos_f32 of 2 pi v in
// revolutions): the policy noise needs the N(0, 1) law, not libm-exact values.
__device__ __forceinline__ void box_muller_hw(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float u = u01(a), v = u01(b);
  const float r = __builtin_amdgcn_sqrtf(-2.f * 0.69314718055994531f * __builtin_amdgcn_logf(u));
  n0 = r * __builtin_amdgcn_cosf(v);
  n1 = r * __builtin_amdgcn_sinf(v);
}
// eps [aout][Bp] (padding columns b >= B zero): one philox block -> 4 normals -> one 16-B store
// (Bp is a multiple of 32, so a quad never crosses a row).
__global__ void k_eps_fm(float* E, int aout, int B, int Bp, uint64_t seed, uint64_t ctr, float* E2, uint64_t ctr2) {
  if (blockIdx.y) {  // (a second array in the same launch: the update's two rsample draws)
    E = E2;
    ctr = ctr2;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // quad index; aout * Bp < 2^31 (host check)
  if (4 * i >= aout * Bp) return;
  const u32x4 r = philox(seed, ctr, (uint64_t)i);
  float4 v;
  box_muller_hw(r.x, r.y, v.x, v.y);
  box_muller_hw(r.z, r.w, v.z, v.w);
  const int col = (4 * i) % Bp;
  v.x = col < B ? v.x : 0.f;
  v.y = col + 1 < B ? v.y : 0.f;
  v.z = col + 2 < B ? v.z : 0.f;
  v.w = col + 3 < B ? v.w : 0.f;
  *reinterpret_cast<float4*>(E + 4 * (int64_t)i) = v;
}

#endif  // SPP_KSET_TU

// ============================================================================ debug dense
// One layer on a [B][K] row-major batch with a natural bias b (NULL -> 0).
// K <= 224: register-input dense (ob-major image); K == 256: dense_lds from the
// LDS image (ib-major image), NBO compile-time.  KQ > 0 (NBI == 1): only the first
// KQ register quads of the input block carry units, as in the 3..24-wide first layers.
template <int NBI, int NBO, int KQ = 0>
__global__ __launch_bounds__(64) void k_debug_dense(const float4* Wf, const float* bias, const float* x, float* y,
                                                    int B, int K, int N, int act) {
  __shared__ float img[256 * 32];
  __shared__ __attribute__((aligned(16))) float tb[256];
  const int lane = threadIdx.x & 63, h = lane >> 5, s = lane & 31;
  for (int i = lane; i < 256; i += 64) tb[i] = (bias && i < N) ? bias[i] : 0.f;
  const int64_t b = (int64_t)blockIdx.x * 32 + s;
  f32x16 in[NBI];
#pragma unroll
  for (int ib = 0; ib < NBI; ++ib)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * ib + unit_of(r, h);
      in[ib][r] = (u < K && b < B) ? x[b * K + u] : 0.f;
      img[(32 * ib + ru(r) + 4 * h) * 32 + s] = in[ib][r];
    }
  __syncthreads();
  auto epi = [&](int ob, const f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * ob + unit_of(q, h);
      float v = acc[q];
      if (act == 1) v = fmaxf(v, 0.f);
      if (act == 2) v = tanhf(v);
      if (u < N && b < B) y[b * N + u] = v;
    }
  };
  if constexpr (NBI == 8)
    dense_lds<NBO>(Wf, img, tb, epi);  // tb holds zeros without a bias
  else
    dense<NBI, KQ ? (uint64_t)KQ : rv_nat(32 * NBI, NBI)>(Wf, (N + 31) / 32, in, tb, epi);
}

}  // namespace spp
