// Weight gradients as split-K MFMA GEMMs over the batch:
//   dW[n][k] = sum_b A[n][b] * X[k][b],   db[n] = sum_b A[n][b]
// A = per-sample layer-output gradients (delta) and X = layer inputs, both
// feature-major [rows][Bp] as written by the per-sample kernels.
//
// One work item = (job, sample range).  A workgroup of 4 waves owns the whole
// <=256x256 output of its item: wave w holds the 128x128 quadrant
// (n blocks 4*(w>>1).., k blocks 4*(w&1)..) as 16 accumulator tiles.  The
// operands need no LDS: the sum over samples is order-free, so lane half h
// takes samples [b+8h, b+8h+8) of its row as two float4 and feeds them to 8
// consecutive MFMA k-steps for both A and X (same sample<->k map on both
// sides).  Each lane streams its 4 A rows and 4 X rows straight from HBM
// through an R-deep register ring (loads for step t+R-1 issued before step
// t's MFMAs; R from dw_ring, deeper for thin tile sets).  Partial slabs are
// summed in a fixed order by k_dw_reduce (deterministic, no atomics).
//
// Operand element types are per job (DwJob::a_bf / x_bf): the bf16 kernel sets store the
// activations and deltas they hand to this kernel as bf16 [rows][Bp] (half the bytes written
// and read back; the bf16 MFMA rounds fp32 operands to bf16 with the same conversion), while
// staged inputs (s, a), the per-sample dq and the head deltas stay fp32.  A bf16 operand
// row-step is one 16-B load of the lane half's 8 samples, fed to the MFMA as is.
#include "common.h"
#include "internal.h"

namespace spp {

constexpr int kDwThreads = 256;

// Steps (16 samples each) in flight for an NI x NJ tile set: the R-1 steps ahead should carry
// >= ~8K cycles of MFMA work (HBM latency under load), within ~168 VGPRs of operand ring.
// fp32: 8 x 64-cycle 32x32x2 MFMAs per block pair and step (4x4: R = 2); bf16: one 32-cycle
// 32x32x16 per block pair and step, so the ring runs as deep as the registers allow (bf16
// operand rows take one float4 per step, fp32 rows two).
template <int NI, int NJ, bool BF = false, bool ABF = false, bool XBF = false>
constexpr int dw_ring() {
  constexpr int cyc = NI * NJ * (BF ? 32 : 512);
  constexpr int want = 1 + (8192 + cyc - 1) / cyc;
  constexpr int cap = 168 / (4 * (NI * (ABF ? 1 : 2) + NJ * (XBF ? 1 : 2)));
  constexpr int r = want < cap ? want : cap;
  return r < 2 ? 2 : (r > 8 ? 8 : r);
}

// One step = 16 samples: lane half h takes samples [16t + 8h, +8) of each of
// its rows as two adjacent float4 (a full 64 B run per row and half), i.e. 8
// MFMA k-steps per row pair.
__device__ __forceinline__ bf16x8 pack8(const float4& a, const float4& b) {
  bf16x8 r;
  r[0] = (__bf16)a.x; r[1] = (__bf16)a.y; r[2] = (__bf16)a.z; r[3] = (__bf16)a.w;
  r[4] = (__bf16)b.x; r[5] = (__bf16)b.y; r[6] = (__bf16)b.z; r[7] = (__bf16)b.w;
  return r;
}

// BF: one v_mfma_f32_32x32x16_bf16 per (row block, column block) per 16-sample step: lane half
// h's 8 samples are exactly the MFMA's k = 8h + j slots on both operands (bf16 agents, mlp_bf16).
__device__ __forceinline__ bf16x8 as_bf8(const float4& a) { return __builtin_bit_cast(bf16x8, a); }
// sum of the 8 bf16 of a 16-B operand word (the bias gradient of a bf16 delta row)
__device__ __forceinline__ float sum_bf8(const float4& a) {
  const uint32_t w[4] = {__builtin_bit_cast(uint32_t, a.x), __builtin_bit_cast(uint32_t, a.y),
                         __builtin_bit_cast(uint32_t, a.z), __builtin_bit_cast(uint32_t, a.w)};
  float s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    s[i] = __builtin_bit_cast(float, w[i] << 16) + __builtin_bit_cast(float, w[i] & 0xffff0000u);
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// ABF / XBF: the A / X operand rows are bf16 (BF only); row pointers are then __bf16* cast to float*.
// Operand loads use the default cache policy: nt loads were measured slower (both lane
// halves of a wave reuse each L1 line).
__device__ __forceinline__ float4 dw_ld(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <int NI, int NJ, bool DB, bool BF = false, bool ABF = false, bool XBF = false>
__device__ __forceinline__ void dw_tile(const float* const (&ap)[4], const float* const (&xp)[4], int nsteps,
                                        f32x16 (&acc)[4][4], float (&bs)[4]) {
  constexpr int R = dw_ring<NI, NJ, BF, ABF, XBF>();
  float4 ra[R][NI][2], rx[R][NJ][2];
  const float* a0[NI];
  const float* x0[NJ];
  static_for<0, NI>([&](auto I) { a0[I] = ap[I]; });
  static_for<0, NJ>([&](auto J) { x0[J] = xp[J]; });
  auto load = [&](auto SL, int t) {
    constexpr int sl = decltype(SL)::value;
    static_for<0, NI>([&](auto I) {
      if constexpr (ABF) {
        ra[sl][I][0] = dw_ld(reinterpret_cast<const float*>(reinterpret_cast<const __bf16*>(a0[I]) + 16 * t));
      } else {
        ra[sl][I][0] = dw_ld(a0[I] + 16 * t);
        ra[sl][I][1] = dw_ld(a0[I] + 16 * t + 4);
      }
    });
    static_for<0, NJ>([&](auto J) {
      if constexpr (XBF) {
        rx[sl][J][0] = dw_ld(reinterpret_cast<const float*>(reinterpret_cast<const __bf16*>(x0[J]) + 16 * t));
      } else {
        rx[sl][J][0] = dw_ld(x0[J] + 16 * t);
        rx[sl][J][1] = dw_ld(x0[J] + 16 * t + 4);
      }
    });
  };
  static_for<0, R - 1>([&](auto S) {
    if ((int)S < nsteps) load(S, (int)S);
  });
#pragma unroll 1
  for (int t0 = 0; t0 < nsteps; t0 += R) {
    static_for<0, R>([&](auto U) {
      constexpr int u = U;
      constexpr int sn = (u + R - 1) % R;
      if (t0 + u >= nsteps) return;
      const int tn = t0 + u + R - 1;
      if (tn < nsteps) load(IC<sn>{}, tn);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (BF) {
        static_for<0, NI>([&](auto I) {
          if constexpr (DB && ABF) {
            bs[I] += sum_bf8(ra[u][I][0]);
          } else if constexpr (DB) {
            const float4 a0 = ra[u][I][0], a1 = ra[u][I][1];
            bs[I] += ((a0.x + a0.y) + (a0.z + a0.w)) + ((a1.x + a1.y) + (a1.z + a1.w));
          }
          const bf16x8 av = ABF ? as_bf8(ra[u][I][0]) : pack8(ra[u][I][0], ra[u][I][1]);
          static_for<0, NJ>([&](auto J) {
            const bf16x8 xv = XBF ? as_bf8(rx[u][J][0]) : pack8(rx[u][J][0], rx[u][J][1]);
            acc[I][J] = mfma16(av, xv, acc[I][J]);
          });
        });
      } else {
        static_for<0, NI>([&](auto I) {
          static_for<0, 2>([&](auto P) {
            const float4 av = ra[u][I][P];
            if constexpr (DB) bs[I] += (av.x + av.y) + (av.z + av.w);
            static_for<0, NJ>([&](auto J) {
              const float4 xv = rx[u][J][P];
              acc[I][J] = mfma(av.x, xv.x, acc[I][J]);
              acc[I][J] = mfma(av.y, xv.y, acc[I][J]);
              acc[I][J] = mfma(av.z, xv.z, acc[I][J]);
              acc[I][J] = mfma(av.w, xv.w, acc[I][J]);
            });
          });
        });
      }
    });
  }
}

// 256 x 256 fp32 jobs (the hidden-layer weight gradients of the critics and the actor): the
// workgroup's operand rows are staged through LDS so every A / X byte leaves HBM once per item.
// (In dw_tile each A row is streamed by the two waves that share its row blocks and each X row by
// the two that share its column blocks: twice the bytes, ~4.9 TB/s at the MFMA rate.)
// Step = 32 samples = one 128-B line per row; the step's 512 rows ([A (256) | X (256)] x 128 B = 64 KiB)
// arrive by LDS-DMA (global_load_lds_dwordx4: 8 rows per wave-instruction, 16 per wave, no VGPR
// destination), one step ahead, into the other of two LDS buffers.  The LDS image is lane-linear
// (row r at 128 r bytes); the 16-B slot q of row r holds piece q ^ ((r >> 1) & 7) of the row (the
// swizzle is applied on the global SOURCE address and undone on the read), which makes the MFMA
// operand reads (lane c reads row c of its block, ds_read_b128) bank-conflict free.
// SPP_DW_TIMING (tools/build_variant.py only; the results are WRONG on purpose, the variants are timed, never shipped
// or tested): bit 0 drops the per-step DMA issue of k_dw_big and k_dw_big8 after the first two steps, bit 1 their
// per-step wait and barrier.  What each costs the two loops: DESIGN.md §8, round 15.
#ifndef SPP_DW_TIMING
#define SPP_DW_TIMING 0
#endif
typedef __attribute__((address_space(1))) void glob_void;
typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ void dw_big_lds(const DwJob& J, int b_begin, int nsteps, int nb0, int kb0, bool db,
                                           f32x16 (&acc)[4][4], float (&bs)[4]) {
  __shared__ __attribute__((aligned(16))) float lds[2][512 * 32];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
  const int64_t ld = J.Bp;
  // instruction k of wave w: rows 128 w + 8 k + (lane >> 3), slot lane & 7 <- piece (lane & 7) ^ ((row >> 1) & 7)
  //   = (lane & 7) ^ ((lane >> 4) & 3) ^ (4 (k & 1))
  const int pe = (lane & 7) ^ ((lane >> 4) & 3);
  // wave-uniform row base (SGPRs) + one 32-bit per-lane offset per instruction parity
  // wave-uniform values forced into SGPRs (the job fields may arrive in VGPRs)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const float* wsel = wu < 2 ? J.A : J.X0;
  const uint64_t wbits = (uint64_t)(size_t)wsel;
  const uint64_t wbu = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wbits) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wbits >> 32)) << 32);
  const int64_t ldu = (int64_t)__builtin_amdgcn_readfirstlane((int)ld);  // Bp < 2^31
  const int bbu = __builtin_amdgcn_readfirstlane(b_begin);
  const float* wb = opaque(reinterpret_cast<const float*>((size_t)wbu) + (int64_t)(128 * (wu & 1)) * ldu + bbu);
  const uint32_t off0 = (uint32_t)((lane >> 3) * ld + 4 * pe), off1 = off0 ^ 16u;  // pe ^ 4: 16 floats
  // The DMA is issued by inline asm: for the builtin the compiler cannot tell the LDS-DMA's
  // destination from the buffer being read and waits vmcnt(0) before every ds_read, which serialises
  // the next step's loads with this step's MFMAs.  Here the only wait is the explicit one before the
  // step's closing barrier (the loop holds no other vector-memory loads whose counts it could skew).
  auto issue = [&](int t, int buf) {
    const uint32_t dst = (uint32_t)(size_t)(lds_void*)&lds[buf][(128 * wu) * 32];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float* src = opaque(wb + ((int64_t)(8 * k) * ldu + 32 * t)) + ((k & 1) ? off1 : off0);
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(src), "s"(dst + 1024u * k)
                   : "memory");
    }
  };
  // Operand registers are double-buffered across the step's two sub-steps (16 samples each): the
  // reads of the next sub-step are in flight while the current one's 128 MFMAs issue, so no LDS
  // latency is exposed.  A step's sub-step 1 reads are complete (lgkmcnt) before the step's closing
  // barrier, after which buffer t & 1 may be refilled by DMA for step t + 2.
  const int sw = (c >> 1) & 7;  // the read-side swizzle of rows 32 b + c
  auto rd = [&](const float* L, int s, float4 (&ra)[4][2], float4 (&rx)[4][2]) {
    const int q0 = (4 * s + 2 * h) ^ sw, q1 = (4 * s + 2 * h + 1) ^ sw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* pa = L + (32 * (nb0 + i) + c) * 32;
      const float* px = L + (256 + 32 * (kb0 + i) + c) * 32;
      ra[i][0] = *reinterpret_cast<const float4*>(pa + 4 * q0);
      ra[i][1] = *reinterpret_cast<const float4*>(pa + 4 * q1);
      rx[i][0] = *reinterpret_cast<const float4*>(px + 4 * q0);
      rx[i][1] = *reinterpret_cast<const float4*>(px + 4 * q1);
    }
  };
  auto mm = [&](const float4 (&ra)[4][2], const float4 (&rx)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float4 av = ra[i][p];
        if (db) bs[i] += (av.x + av.y) + (av.z + av.w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 xv = rx[j][p];
          acc[i][j] = mfma(av.x, xv.x, acc[i][j]);
          acc[i][j] = mfma(av.y, xv.y, acc[i][j]);
          acc[i][j] = mfma(av.z, xv.z, acc[i][j]);
          acc[i][j] = mfma(av.w, xv.w, acc[i][j]);
        }
      }
  };
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nsteps > 1) issue(1, 1);
  float4 ra0[4][2], rx0[4][2], ra1[4][2], rx1[4][2];
  rd(lds[0], 0, ra0, rx0);
#pragma unroll 1
  for (int t = 0; t < nsteps; ++t) {
    rd(lds[t & 1], 1, ra1, rx1);
    mm(ra0, rx0);
    if (t + 1 < nsteps) {
#if !(SPP_DW_TIMING & 2)
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // my DMA for t + 1 landed, my reads of t done
      __syncthreads();  // every wave's DMA landed and every wave is done reading buffer t & 1
#endif
#if !(SPP_DW_TIMING & 1)
      if (t + 2 < nsteps) issue(t + 2, t & 1);
#endif
      rd(lds[(t + 1) & 1], 0, ra0, rx0);
    }
    mm(ra1, rx1);
  }
}

// dw_big_lds for a workgroup of 8 waves, two on each SIMD (k_dw_big8): while one wave of a SIMD issues DMA, reads LDS
// or waits at the step's barrier, its partner's MFMAs keep the matrix pipe busy.  The LDS image, the swizzle, the two
// buffers and the barrier per step are dw_big_lds's; per wave:
//   output   4 row blocks x 2 column blocks (128 accumulator registers): waves w and w + 4, which share a SIMD, hold the
//            two column halves of dw_big_lds's quadrant w, so every 32 x 32 block sees the same MFMA chain in the same
//            order and the bias sums come from the waves with column blocks 0-1 by the same expression
//   DMA      8 of the step's 64 instructions: rows 64 w .. 64 w + 63 of [A | X]
//   reads    12 ds_read_b128 per sub-step (4 A rows, 2 X rows, two 16-B slots each), as two quarter-steps of 6
// The two waves of a SIMD are kept out of phase by where they issue the DMA for step t + 2 behind step t's barrier:
// waves 0-3 at once (their partners run the step's last 32 MFMAs meanwhile), waves 4-7 after those MFMAs (beside
// their partners').  Either way the DMA follows the barrier that ends every wave's reads of the buffer, and is waited for
// before the next one.  Every barrier's trip count comes from nsteps alone.
__device__ __forceinline__ void dw_big8_lds(const DwJob& J, int b_begin, int nsteps, int nb0, int kb0, bool db,
                                            f32x16 (&acc)[4][2], float (&bs)[4]) {
  __shared__ __attribute__((aligned(16))) float lds[2][512 * 32];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
  const int64_t ld = J.Bp;
  // instruction k of wave w: rows 64 w + 8 k + (lane >> 3), slot lane & 7 <- piece (lane & 7) ^ ((row >> 1) & 7)
  //   = (lane & 7) ^ ((lane >> 4) & 3) ^ (4 (k & 1))
  const int pe = (lane & 7) ^ ((lane >> 4) & 3);
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const float* wsel = wu < 4 ? J.A : J.X0;
  const uint64_t wbits = (uint64_t)(size_t)wsel;
  const uint64_t wbu = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wbits) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wbits >> 32)) << 32);
  const int64_t ldu = (int64_t)__builtin_amdgcn_readfirstlane((int)ld);  // Bp < 2^31
  const int bbu = __builtin_amdgcn_readfirstlane(b_begin);
  const float* wb = opaque(reinterpret_cast<const float*>((size_t)wbu) + (int64_t)(64 * (wu & 3)) * ldu + bbu);
  const uint32_t off0 = (uint32_t)((lane >> 3) * ld + 4 * pe), off1 = off0 ^ 16u;  // pe ^ 4: 16 floats
  const bool late = wu >= 4;  // the SIMD's second wave
  auto issue = [&](int t, int buf) {
    const uint32_t dst = (uint32_t)(size_t)(lds_void*)&lds[buf][(64 * wu) * 32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float* src = opaque(wb + ((int64_t)(8 * k) * ldu + 32 * t)) + ((k & 1) ? off1 : off0);
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(src), "s"(dst + 1024u * k)
                   : "memory");
    }
  };
  // A step is read in 4 quarter-steps of 8 samples per lane half: quarter v = one 16-B slot per row, piece
  // 4 (v >> 1) + 2 h + (v & 1) of the row, which is the order in which dw_big_lds's sub-steps (two slots each) feed
  // them to the MFMAs.  The operand registers are double-buffered across quarter-steps: the 6 reads of the next are
  // in flight under the current one's 32 MFMAs.
  const int sw = (c >> 1) & 7;  // the read-side swizzle of rows 32 b + c
  auto rd = [&](const float* L, int v, float4 (&ra)[4], float4 (&rx)[2]) {
    const int q = (4 * (v >> 1) + 2 * h + (v & 1)) ^ sw;
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = *reinterpret_cast<const float4*>(L + (32 * (nb0 + i) + c) * 32 + 4 * q);
#pragma unroll
    for (int j = 0; j < 2; ++j) rx[j] = *reinterpret_cast<const float4*>(L + (256 + 32 * (kb0 + j) + c) * 32 + 4 * q);
  };
  auto mm = [&](const float4 (&ra)[4], const float4 (&rx)[2]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 av = ra[i];
      if (db) bs[i] += (av.x + av.y) + (av.z + av.w);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 xv = rx[j];
        acc[i][j] = mfma(av.x, xv.x, acc[i][j]);
        acc[i][j] = mfma(av.y, xv.y, acc[i][j]);
        acc[i][j] = mfma(av.z, xv.z, acc[i][j]);
        acc[i][j] = mfma(av.w, xv.w, acc[i][j]);
      }
    }
  };
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nsteps > 1) issue(1, 1);
  float4 ra0[4], rx0[2], ra1[4], rx1[2];
  rd(lds[0], 0, ra0, rx0);
#pragma unroll 1
  for (int t = 0; t < nsteps; ++t) {
    const float* L = lds[t & 1];
    rd(L, 1, ra1, rx1);
    mm(ra0, rx0);
    rd(L, 2, ra0, rx0);
    mm(ra1, rx1);
    rd(L, 3, ra1, rx1);
    mm(ra0, rx0);
    if (t + 1 < nsteps) {
#if !(SPP_DW_TIMING & 2)
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // my DMA for t + 1 landed, my reads of t done
      __syncthreads();  // every wave's DMA landed and every wave is done reading buffer t & 1
#endif
#if !(SPP_DW_TIMING & 1)
      if (!late && t + 2 < nsteps) issue(t + 2, t & 1);
#endif
      rd(lds[(t + 1) & 1], 0, ra0, rx0);
    }
    mm(ra1, rx1);
#if !(SPP_DW_TIMING & 1)
    if (late && t + 2 < nsteps) issue(t + 2, t & 1);  // behind step t's barrier: t + 2 < nsteps implies it ran
#endif
  }
}

// 256 x 256 jobs with bf16 A and X rows (the bf16 sets' hidden-layer weight gradients): the same LDS-DMA staging
// with a 64-sample step, which is again one 128-B line per row (8 slots of 8 bf16, the same swizzle): the rows are
// addressed as 4-byte words (ld = Bp / 2, the step 32 words), so the DMA issue is dw_big_lds's.  A step holds 4
// k-steps of v_mfma_f32_32x32x16_bf16; k-step s reads one 16-B slot per row, slot 2s + h (lane half h takes
// samples 8h..8h+7 of the k-step on both operands, as dw_tile's bf16 form), double-buffered across the k-steps.
// Per item the k-steps run in sample order, as in k_dw<true>.  Needs b_begin and the item's range multiples of 64.
__device__ __forceinline__ void dw_big_lds16(const DwJob& J, int b_begin, int nsteps, int nb0, int kb0, bool db,
                                             f32x16 (&acc)[4][4], float (&bs)[4]) {
  __shared__ __attribute__((aligned(16))) float lds[2][512 * 32];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, c = lane & 31;
  const int64_t ld = J.Bp / 2;  // words per bf16 row
  const int pe = (lane & 7) ^ ((lane >> 4) & 3);
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const float* wsel = wu < 2 ? J.A : J.X0;
  const uint64_t wbits = (uint64_t)(size_t)wsel;
  const uint64_t wbu = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wbits) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(wbits >> 32)) << 32);
  const int64_t ldu = (int64_t)__builtin_amdgcn_readfirstlane((int)ld);
  const int bbu = __builtin_amdgcn_readfirstlane(b_begin / 2);  // first sample's word
  const float* wb = opaque(reinterpret_cast<const float*>((size_t)wbu) + (int64_t)(128 * (wu & 1)) * ldu + bbu);
  const uint32_t off0 = (uint32_t)((lane >> 3) * ld + 4 * pe), off1 = off0 ^ 16u;
  auto issue = [&](int t, int buf) {
    const uint32_t dst = (uint32_t)(size_t)(lds_void*)&lds[buf][(128 * wu) * 32];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float* src = opaque(wb + ((int64_t)(8 * k) * ldu + 32 * t)) + ((k & 1) ? off1 : off0);
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(src), "s"(dst + 1024u * k)
                   : "memory");
    }
  };
  const int sw = (c >> 1) & 7;
  auto rd = [&](const float* L, int s, float4 (&ra)[4], float4 (&rx)[4]) {
    const int q = (2 * s + h) ^ sw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const float4*>(L + (32 * (nb0 + i) + c) * 32 + 4 * q);
      rx[i] = *reinterpret_cast<const float4*>(L + (256 + 32 * (kb0 + i) + c) * 32 + 4 * q);
    }
  };
  auto mm = [&](const float4 (&ra)[4], const float4 (&rx)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (db) bs[i] += sum_bf8(ra[i]);
      const bf16x8 av = as_bf8(ra[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(av, as_bf8(rx[j]), acc[i][j]);
    }
  };
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nsteps > 1) issue(1, 1);
  float4 ra0[4], rx0[4], ra1[4], rx1[4];
  rd(lds[0], 0, ra0, rx0);
#pragma unroll 1
  for (int t = 0; t < nsteps; ++t) {
    const float* L = lds[t & 1];
    rd(L, 1, ra1, rx1);
    mm(ra0, rx0);
    rd(L, 2, ra0, rx0);
    mm(ra1, rx1);
    rd(L, 3, ra1, rx1);
    mm(ra0, rx0);
    if (t + 1 < nsteps) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // my DMA for t + 1 landed, my reads of t done
      __syncthreads();  // every wave's DMA landed and every wave is done reading buffer t & 1
      if (t + 2 < nsteps) issue(t + 2, t & 1);
      rd(lds[(t + 1) & 1], 0, ra0, rx0);
    }
    mm(ra1, rx1);
  }
}

// Partial (or final) result of an item's (nb0, kb0) quadrant; rows >= nrow2 go to the second output
// (dW2 / db2).
// NJ: column blocks the wave holds (k_dw_big8: 2).
template <int NJ = 4>
__device__ __forceinline__ void dw_store(const DwJob& J, int split, int part, int nb0, int kb0, int ni, int nj,
                                         bool db, const f32x16 (&acc)[4][NJ], const float (&bs)[4]) {
  // recomputed here, not carried over the tile loop: the prologue's per-row indices, kept live across the
  // MFMA loop for these stores, were what spilled to scratch
  int tid = threadIdx.x;
  asm volatile("" : "+v"(nb0), "+v"(kb0), "+v"(ni), "+v"(nj), "+v"(split), "+v"(part), "+v"(tid));
  const int lane = tid & 63, h = lane >> 5, c = lane & 31;
  const int N = J.N, K = J.K0 + J.K1;
  const bool direct = J.nsplit * J.wsplit == 1;
  float* slab = direct ? nullptr : J.slab + (int64_t)(split * J.wsplit + part) * J.slab_stride;
  // row n's destination: one 64-bit row pointer live at a time (rows outer, the row's column blocks inner:
  // precomputing every (row, column) address is what spilled this kernel's VGPRs)
  auto row_w = [&](int n) -> float* {
    if (!direct) return slab + (int64_t)n * K;
    return n < J.nrow2 ? J.dW + (int64_t)n * K : J.dW2 + (int64_t)(n - J.nrow2) * K;
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= ni) break;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = 32 * (nb0 + i) + unit_of(q, h);
      if (n >= N) continue;
      float* rowp = row_w(n);
      asm volatile("" : "+v"(rowp));  // keep the row pointer from being hoisted across the unrolled rows
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (j >= nj) break;
        const int k = 32 * (kb0 + j) + c;
        if (k < K) rowp[k] = acc[i][j][q];
      }
    }
    if (db) {
      const float tot = bs[i] + __shfl_xor(bs[i], 32, 64);
      const int n = 32 * (nb0 + i) + c;
      if (h == 0 && n < N) {
        if (!direct) slab[(int64_t)N * K + n] = tot;
        else if (n < J.nrow2) J.db[n] = tot;
        else J.db2[n - J.nrow2] = tot;
      }
    }
  }
}

// BFK: the bf16 job sets (every job of a launch has the agent's bf16 flag); one kernel per
// precision so each gets its own register allocation.
template <bool BFK>
__global__ __launch_bounds__(kDwThreads, 1) void k_dw(const DwJob* __restrict__ jobs, const int* __restrict__ item_job,
                                                      const int* __restrict__ item_split) {
  const int item = blockIdx.x;
  const DwJob J = jobs[item_job[item]];
  const int split = item_split[item];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int64_t ld = J.Bp;
  // Waves whose output quadrant would be empty take part of the samples instead:
  //   wsplit 4 (N, K <= 128): all 4 waves on quadrant (0, 0), a quarter of the samples each;
  //   wsplit 2 (one side <= 128): 2 quadrants along the wide side, 2 sample halves each.
  const int N = J.N, K = J.K0 + J.K1;
  const bool wsp = J.wsplit > 1;
  int nb0 = 4 * (w >> 1), kb0 = 4 * (w & 1), part = 0;
  if (J.wsplit == 4) {
    nb0 = kb0 = 0;
    part = w;
  } else if (J.wsplit == 2) {
    if (N <= 128) {
      nb0 = 0;
      part = w >> 1;
    } else {
      kb0 = 0;
      part = w & 1;
    }
  }
  int b_begin = split * J.split_len;
  int b_end = min(b_begin + J.split_len, J.Bp);
  if (wsp) {  // parts of whole 32-sample units
    const int q = (((b_end - b_begin + J.wsplit - 1) / J.wsplit) + 31) & ~31;
    b_begin = min(b_begin + part * q, b_end);
    b_end = min(b_begin + q, b_end);
  }
  const int nsteps = (b_end - b_begin) / 16;  // ranges are multiples of 32 samples
  const int ni = min(4, max(0, (N + 31) / 32 - nb0));
  const int nj = min(4, max(0, (K + 31) / 32 - kb0));
  if (ni == 0 || nj == 0) return;
  const bool db = J.db != nullptr && kb0 == 0;
  // per-lane row pointers at this item's first sample; rows past N / K are
  // clamped to row 0 (their outputs are never stored)
  const float* ap[4];
  const float* xp[4];
  const int esa = J.a_bf ? 2 : 4, esx = J.x_bf ? 2 : 4;  // operand element sizes
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int n = 32 * (nb0 + i) + c;
    n = n < N ? n : 0;
    ap[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(J.A) +
                                           esa * ((int64_t)n * ld + b_begin + 8 * h));
    int k = 32 * (kb0 + i) + c;
    k = k < K ? k : 0;
    const float* xr = k < J.K0 ? J.X0 : J.X1;
    const int64_t kr = k < J.K0 ? k : k - J.K0;
    xp[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(xr) + esx * (kr * ld + b_begin + 8 * h));
  }
  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero16();
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  // operand types: 0 fp32 MFMA; bf16 MFMA with (A, X) element types fp32/fp32, bf16/fp32,
  // bf16/bf16, fp32/bf16.  The bf16 forms instantiate 1, 2 and 4 blocks per side only (a 3-block
  // side runs as 4 with its last row block clamped to row 0 and never stored): 4 x 9 shapes.
  const int mode = BFK ? 1 + J.a_bf + 2 * J.x_bf : 0;
#define SPP_DW_T(I, J_, ...)                                                    \
  if (db) dw_tile<I, J_, true, ##__VA_ARGS__>(ap, xp, nsteps, acc, bs);         \
  else dw_tile<I, J_, false, ##__VA_ARGS__>(ap, xp, nsteps, acc, bs);
#define SPP_DW_CASE(I, J_)                                                      \
  case (I) * 8 + (J_): SPP_DW_T(I, J_) break;
#define SPP_DW_CASE16(I, J_)                                                    \
  case (I) * 8 + (J_):                                                          \
    switch (mode) {                                                             \
      case 1: SPP_DW_T(I, J_, true) break;                                      \
      case 2: SPP_DW_T(I, J_, true, true) break;                                \
      case 4: SPP_DW_T(I, J_, true, true, true) break;                          \
      default: SPP_DW_T(I, J_, true, false, true) break;                        \
    }                                                                           \
    break;
  if constexpr (!BFK) {
    switch (ni * 8 + nj) {
      SPP_DW_CASE(1, 1) SPP_DW_CASE(1, 2) SPP_DW_CASE(1, 3) SPP_DW_CASE(1, 4)
      SPP_DW_CASE(2, 1) SPP_DW_CASE(2, 2) SPP_DW_CASE(2, 3) SPP_DW_CASE(2, 4)
      SPP_DW_CASE(3, 1) SPP_DW_CASE(3, 2) SPP_DW_CASE(3, 3) SPP_DW_CASE(3, 4)
      SPP_DW_CASE(4, 1) SPP_DW_CASE(4, 2) SPP_DW_CASE(4, 3) SPP_DW_CASE(4, 4)
    }
  } else {
    const int ni4 = ni == 3 ? 4 : ni, nj4 = nj == 3 ? 4 : nj;
    switch (ni4 * 8 + nj4) {
      SPP_DW_CASE16(1, 1) SPP_DW_CASE16(1, 2) SPP_DW_CASE16(1, 4)
      SPP_DW_CASE16(2, 1) SPP_DW_CASE16(2, 2) SPP_DW_CASE16(2, 4)
      SPP_DW_CASE16(4, 1) SPP_DW_CASE16(4, 2) SPP_DW_CASE16(4, 4)
    }
  }
#undef SPP_DW_CASE
#undef SPP_DW_CASE16
#undef SPP_DW_T
  dw_store(J, split, part, nb0, kb0, ni, nj, db, acc, bs);
}

// 256 x 256 fp32 items (host: DwJob N = K0 = 256, K1 = 0, wsplit = 1, not bf16), listed first in a
// phase's item table: their own kernel, so the LDS-DMA path gets the kernel's whole register budget
// (double-buffered operands) and k_dw's thin / mid items carry no 128 KiB static LDS.
__global__ __launch_bounds__(kDwThreads, 1) void k_dw_big(const DwJob* __restrict__ jobs,
                                                          const int* __restrict__ item_job,
                                                          const int* __restrict__ item_split) {
  const int item = blockIdx.x;
  const DwJob J = jobs[item_job[item]];
  const int split = item_split[item];
  const int w = threadIdx.x >> 6;
  const int nb0 = 4 * (w >> 1), kb0 = 4 * (w & 1);
  const int b_begin = split * J.split_len;
  const int b_end = min(b_begin + J.split_len, J.Bp);
  const int nsteps = (b_end - b_begin) / 32;  // ranges are multiples of 32 samples
  const bool db = J.db != nullptr && kb0 == 0;
  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero16();
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  if (nsteps > 0) dw_big_lds(J, b_begin, nsteps, nb0, kb0, db, acc, bs);
  dw_store(J, split, 0, nb0, kb0, 4, 4, db, acc, bs);
}

// 256 x 256 bf16-operand items (host: as k_dw_big's, both operands bf16, item ranges multiples of 64 samples).
__global__ __launch_bounds__(kDwThreads, 1) void k_dw_big16(const DwJob* __restrict__ jobs,
                                                            const int* __restrict__ item_job,
                                                            const int* __restrict__ item_split) {
  const int item = blockIdx.x;
  const DwJob J = jobs[item_job[item]];
  const int split = item_split[item];
  const int w = threadIdx.x >> 6;
  const int nb0 = 4 * (w >> 1), kb0 = 4 * (w & 1);
  const int b_begin = split * J.split_len;
  const int b_end = min(b_begin + J.split_len, J.Bp);
  const int nsteps = (b_end - b_begin) / 64;  // ranges are multiples of 64 samples (host: lds_big)
  const bool db = J.db != nullptr && kb0 == 0;
  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero16();
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  if (nsteps > 0) dw_big_lds16(J, b_begin, nsteps, nb0, kb0, db, acc, bs);
  dw_store(J, split, 0, nb0, kb0, 4, 4, db, acc, bs);
}

// Fixed-order reduction of the split slabs: one thread per element of a job's [N*K | N] image,
// slabs summed in split order.  A job has few elements (<= 64K) against 128-256 slabs, so the
// walk is latency-bound: one element per thread (4x the threads of a float4 walk) and 16
// slabs' loads in flight.
__global__ void k_dw_reduce(const DwJob* __restrict__ jobs) {
  const DwJob J = jobs[blockIdx.y];
  const int nslab = J.nsplit * J.wsplit;
  if (nslab == 1) return;
  const int N = J.N, K = J.K0 + J.K1;
  const int64_t nw = (int64_t)N * K;
  const int64_t total = nw + (J.db ? N : 0);
  const int G = dw_red_group(nslab, nw + N);  // lanes per element (as the host sized the grid; a power of 2 dividing 64)
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t e = gid / G;
  const int g = (int)(gid % G);
  if (e >= total) return;  // whole groups: e is the same for the G lanes of a group
  const float* p = J.slab + e;
  float s = 0.f;
  if (G == 1) {
    int sp = 0;
    for (; sp + 16 <= nslab; sp += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = p[(int64_t)(sp + u) * J.slab_stride];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; sp < nslab; ++sp) s += p[(int64_t)sp * J.slab_stride];
  } else {
    // lane g sums slabs g, g + G, ... (16 loads per round trip), then a fixed butterfly over the group; lane 0's
    // operand order is the same on every run, and only lane 0 writes
    for (int sp = g; sp < nslab; sp += 16 * G) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = sp + u * G < nslab ? p[(int64_t)(sp + u * G) * J.slab_stride] : 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (g != 0) return;
  }
  if (e < nw) {
    const int n = (int)(e / K), k = (int)(e % K);
    if (n < J.nrow2) J.dW[(int64_t)n * K + k] = s;
    else J.dW2[(int64_t)(n - J.nrow2) * K + k] = s;
  } else {
    const int n = (int)(e - nw);
    if (n < J.nrow2) J.db[n] = s;
    else J.db2[n - J.nrow2] = s;
  }
}

// k_dw_big's items on 8 waves, two per SIMD (dw_big8_lds; at most 256 registers per wave): wave w holds column blocks
// 2 (w >> 2) .. + 1 of k_dw_big's quadrant w & 3.  Same items, slabs and results as k_dw_big, bit for bit.
// A template (of nothing) that the launch function names after k_dw<>, so that it is emitted behind every other kernel
// of the unit and those keep the place in the code object that they had without it.
constexpr int kDwBig8Threads = 512;
template <int = 0>
__global__ __launch_bounds__(kDwBig8Threads, 1) void k_dw_big8(const DwJob* __restrict__ jobs,
                                                               const int* __restrict__ item_job,
                                                               const int* __restrict__ item_split) {
  const int item = blockIdx.x;
  const DwJob J = jobs[item_job[item]];
  const int split = item_split[item];
  const int w = threadIdx.x >> 6;
  const int nb0 = 4 * ((w >> 1) & 1), kb0 = 4 * (w & 1) + 2 * (w >> 2);
  const int b_begin = split * J.split_len;
  const int b_end = min(b_begin + J.split_len, J.Bp);
  const int nsteps = (b_end - b_begin) / 32;  // ranges are multiples of 32 samples
  const bool db = J.db != nullptr && kb0 == 0;
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  if (nsteps > 0) dw_big8_lds(J, b_begin, nsteps, nb0, kb0, db, acc, bs);
  dw_store<2>(J, split, 0, nb0, kb0, 4, 2, db, acc, bs);
}

// Thin fp32 jobs (host: plan_dw's thin_ok -- wsplit == 2 with one side a single 32-block: the first-layer weight
// gradients D1 x [s | a]^T, AD1 x s^T and the head rows x h2^T), listed last in a phase's item table: HBM-bound items
// whose operand rows k_dw streams 16 B per row and instruction.  Here the rows arrive by LDS-DMA as whole 128-B lines, 8
// rows per wave-instruction (dw_big_lds's image: lane-linear, row R of a part at 128 R bytes, its 16-B slot q holding
// piece q ^ ((R >> 1) & 7)).  Two forms, the same slabs bit for bit:
//   split (the default)   a workgroup of 4 waves owns ONE sample part of an item (blockIdx = 2 item + part), 72 KiB of
//            LDS, so a CU holds two workgroups whose barriers are independent: one's MFMAs run under the other's LDS
//            reads, waits and barriers.  Measured: 0.173 ms per Hopper launch against
//            0.212 ms for the joint form, whose two waves per SIMD meet at the same barriers.
//   joint (-DSPP_DW_THIN_SPLIT=0, tools/build_variant.py)   a workgroup of 8 waves owns both parts of an item, 144 KiB.
//   LDS      [2 buffers][parts][288 rows][128 B]: rows 0..255 the wide side's (A when N > 128, else [X0 | X1]), rows
//            256..287 the narrow side's; only groups of 8 rows that hold a live row are fetched, and a lane of such a
//            group past the last live row fetches that last row again (its LDS row is never read)
//   DMA      wave w fetches the wide rows of its own blocks, and one narrow group of 8 rows
//   MFMA     wave w holds block(s) 8 / kDwThinWaves * w .. of the wide side x the narrow block, one accumulator per
//            part: per 32-sample step a chain of 16 v_mfma_f32_32x32x2_f32 per (block, part), in dw_tile's order
//            (16-sample step t, P = 0, 1, e = 0..3: lane half h feeds sample 16 t + 8 h + 4 P + e), so every 32 x 32
//            block of every slab holds what k_dw<false> writes, bit for bit; bias sums by dw_tile's expression in the
//            same order, from the waves with column block 0; stores through dw_store
//   step t   ds_read the step's operands into registers | lgkmcnt(0), barrier: buffer t & 1 is free | DMA of step
//            t + 2 into it | the step's MFMAs | vmcnt(what step t + 2 issued): this wave's rows of step t + 1 landed
//            (issued a whole step earlier), barrier: every wave's did.  Two steps are in flight beside the one in
//            registers.
// Every barrier's trip count comes from the workgroup's own step count alone: the split form's is its part's (an empty
// part, the ragged last item's, runs no step and stores its all-zero slab); the joint form's is part 0's, which is never
// the shorter one, and a shorter or empty part 1 skips its DMA, reads and MFMAs and reaches every barrier.
#ifndef SPP_DW_THIN_SPLIT
#define SPP_DW_THIN_SPLIT 1
#endif
#ifndef SPP_DW_THIN_WAVES
#define SPP_DW_THIN_WAVES (SPP_DW_THIN_SPLIT ? 4 : 8)
#endif
// SPP_DW_THIN_TIMING (tools/build_variant.py only, as SPP_DW_TIMING: bits 0 and 1 give WRONG results on purpose, the
// variants are timed, never shipped or tested): bit 0 drops the DMA issue after the first two steps, bit 1 replaces a
// step's MFMAs by one multiply-add per operand word, bit 2 marks the DMA loads nt.
#ifndef SPP_DW_THIN_TIMING
#define SPP_DW_THIN_TIMING 0
#endif
constexpr int kDwThinWaves = SPP_DW_THIN_WAVES;
constexpr int kDwThinThreads = 64 * kDwThinWaves;
constexpr int kDwThinRows = 288;
constexpr bool kDwThinSplit = SPP_DW_THIN_SPLIT != 0;  // a workgroup per (item, part), two workgroups per CU
static_assert(kDwThinWaves == 4 || kDwThinWaves == 8, "k_dw_thin: 4 or 8 waves");
template <int = 0>
__global__ __launch_bounds__(kDwThinThreads, kDwThinSplit ? 2 : 1) void k_dw_thin(const DwJob* __restrict__ jobs,
                                                               const int* __restrict__ item_job,
                                                               const int* __restrict__ item_split) {
  __shared__ __attribute__((aligned(16))) float lds[2][kDwThinSplit ? 1 : 2][kDwThinRows * 32];
  constexpr int NW = kDwThinWaves, BPW = 8 / NW, WG = 32 / NW;  // blocks and 8-row DMA groups of the wide side per wave
  const int item = kDwThinSplit ? blockIdx.x >> 1 : blockIdx.x;
  const int mypart = kDwThinSplit ? blockIdx.x & 1 : 0;
  const DwJob J = jobs[item_job[item]];
  const int split = item_split[item];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, c = lane & 31;
  const int wu = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = J.N, K = J.K0 + J.K1;
  const bool wideA = N > 128;  // k_dw's wsplit == 2 rule: the waves spread along the side that is wider than 128
  const int nwide = wideA ? N : K, nnar = wideA ? K : N;
  // the two parts' sample ranges, as k_dw's (whole 32-sample units)
  const int i_begin = split * J.split_len;
  const int s_end = min(i_begin + J.split_len, J.Bp);
  const int q = (((s_end - i_begin + 1) / 2) + 31) & ~31;
  const int b1 = min(i_begin + q, s_end);
  const int m0 = (b1 - i_begin) / 32, m1 = (min(b1 + q, s_end) - b1) / 32;  // m1 <= m0; m1 > 0: b1 = i_begin + q
  // split form: this workgroup's part runs as "part 0" below, and there is no part 1
  const int s_begin = mypart ? b1 : i_begin;
  const int n0 = __builtin_amdgcn_readfirstlane(mypart ? m1 : m0);
  const int n1 = __builtin_amdgcn_readfirstlane(kDwThinSplit ? 0 : m1);
  const int64_t ld = J.Bp;
  auto rowp = [&](bool a_side, int r) -> const float* {
    if (a_side) return J.A + (int64_t)r * ld;
    return r < J.K0 ? J.X0 + (int64_t)r * ld : J.X1 + (int64_t)(r - J.K0) * ld;
  };
  // DMA sources at part 0's first sample: lane l of a group fetches piece (l & 7) ^ ((R >> 1) & 7) of LDS row
  // R = 8 g + (l >> 3)
  const float* srcw[WG];
  int cw = 0;  // this wave's live wide groups
#pragma unroll
  for (int k = 0; k < WG; ++k) {
    const int R = 8 * (WG * wu + k) + (lane >> 3);
    srcw[k] = rowp(wideA, min(R, nwide - 1)) + s_begin + 4 * ((lane & 7) ^ ((R >> 1) & 7));
    cw += 8 * (WG * wu + k) < nwide;
  }
  const int gn = wu & 3;  // narrow group; 8 waves: of part wu >> 2, 4 waves: of both parts
  const int Rn = 8 * gn + (lane >> 3);
  const float* srcn = rowp(!wideA, min(Rn, nnar - 1)) + s_begin + 4 * ((lane & 7) ^ ((Rn >> 1) & 7));
  const bool nlive = 8 * gn < nnar;
  const int cnt0 = __builtin_amdgcn_readfirstlane(cw + (nlive && (NW == 4 || wu < 4)));   // DMAs of a step, part 0
  const int cnt1 = __builtin_amdgcn_readfirstlane(cw + (nlive && (NW == 4 || wu >= 4)));  // part 1
  auto glds = [&](const float* src, uint32_t dst) {
    // inline asm, as dw_big_lds's: the compiler neither counts these loads nor ties them to the LDS reads
    uint32_t keep;
#if SPP_DW_THIN_TIMING & 4
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
#else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
#endif
                 : "=&s"(keep)
                 : "v"(src), "s"(dst)
                 : "memory");
  };
  auto issue = [&](int t, int buf) {
#pragma unroll
    for (int p = 0; p < (kDwThinSplit ? 1 : 2); ++p) {
      if (p == 1 && t >= n1) break;
      const int so = __builtin_amdgcn_readfirstlane((p ? q : 0) + 32 * t);
      const uint32_t base = (uint32_t)(size_t)(lds_void*)&lds[buf][p][0];
#pragma unroll
      for (int k = 0; k < WG; ++k)
        if (8 * (WG * wu + k) < nwide) glds(srcw[k] + so, base + 1024u * (uint32_t)(WG * wu + k));
      if (nlive && (NW == 4 || (wu >> 2) == p)) glds(srcn + so, base + 1024u * (uint32_t)(32 + gn));
    }
  };
  auto issued = [&](int t) { return cnt0 + (t < n1 ? cnt1 : 0); };
  auto wait_vm = [&](int n) {  // s_waitcnt vmcnt(n), n wave-uniform
    static_for<0, 2 * WG + 3>([&](auto V) {
      if (n == (int)V) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((int)V) : "memory");
    });
  };
  auto barrier = [&]() {  // a bare s_barrier: __syncthreads' fence would drain the DMA in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // operand reads: LDS row offsets (floats) and swizzles of this lane's rows; rows past the last live one read row 0
  int offw[BPW], sww[BPW];
  bool blive[BPW], dbw[BPW];
#pragma unroll
  for (int bi = 0; bi < BPW; ++bi) {
    const int blk = BPW * wu + bi, r = 32 * blk + c, R = r < nwide ? r : 0;
    offw[bi] = 32 * R;
    sww[bi] = (R >> 1) & 7;
    blive[bi] = 32 * blk < nwide;
    dbw[bi] = J.db != nullptr && (wideA || blk == 0);
  }
  const int rn = c < nnar ? c : 0;
  const int offn = 32 * (256 + rn), swn = (rn >> 1) & 7;
  // i = 2 (16-sample step of the 32) + P: piece 4 (i >> 1) + 2 h + (i & 1) of the row
  auto rd = [&](const float* L, float4 (&wv)[BPW][4], float4 (&nv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = 4 * (i >> 1) + 2 * h + (i & 1);
      nv[i] = *reinterpret_cast<const float4*>(L + offn + 4 * (pc ^ swn));
#pragma unroll
      for (int bi = 0; bi < BPW; ++bi) wv[bi][i] = *reinterpret_cast<const float4*>(L + offw[bi] + 4 * (pc ^ sww[bi]));
    }
  };
  f32x16 acc[2][BPW];
  float bs[2][BPW];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int bi = 0; bi < BPW; ++bi) {
      acc[p][bi] = zero16();
      bs[p][bi] = 0.f;
    }
  float4 wv[2][BPW][4], nv[2][4];
  auto mm = [&](auto WA, auto NP) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < decltype(NP)::value; ++p)
#pragma unroll
        for (int bi = 0; bi < BPW; ++bi) {
          if (!blive[bi]) continue;
          const float4 av = decltype(WA)::value ? wv[p][bi][i] : nv[p][i];
          const float4 xv = decltype(WA)::value ? nv[p][i] : wv[p][bi][i];
          if (dbw[bi]) bs[p][bi] += (av.x + av.y) + (av.z + av.w);
#if SPP_DW_THIN_TIMING & 2
          acc[p][bi][i] += (av.x * xv.x + av.y * xv.y) + (av.z * xv.z + av.w * xv.w);
#else
          acc[p][bi] = mfma(av.x, xv.x, acc[p][bi]);
          acc[p][bi] = mfma(av.y, xv.y, acc[p][bi]);
          acc[p][bi] = mfma(av.z, xv.z, acc[p][bi]);
          acc[p][bi] = mfma(av.w, xv.w, acc[p][bi]);
#endif
        }
  };
  if (n0 > 0) {
    issue(0, 0);
    if (n0 > 1) issue(1, 1);
    wait_vm(n0 > 1 ? issued(1) : 0);
    barrier();
#pragma unroll 1
    for (int t = 0; t < n0; ++t) {
      const bool both = t < n1;
      rd(lds[t & 1][0], wv[0], nv[0]);
      if constexpr (!kDwThinSplit)
        if (both) rd(lds[t & 1][1], wv[1], nv[1]);
      barrier();  // every wave holds its operands of step t: buffer t & 1 is free
#if !(SPP_DW_THIN_TIMING & 1)
      if (t + 2 < n0) issue(t + 2, t & 1);
#endif
      if (wideA) {
        if (both) mm(IC<1>{}, IC<2>{});
        else mm(IC<1>{}, IC<1>{});
      } else {
        if (both) mm(IC<0>{}, IC<2>{});
        else mm(IC<0>{}, IC<1>{});
      }
      if (t + 1 < n0) {
        wait_vm(t + 2 < n0 && !(SPP_DW_THIN_TIMING & 1) ? issued(t + 2) : 0);  // this wave's rows of step t + 1 landed
        barrier();                                // every wave's did
      }
    }
  }
#pragma unroll
  for (int p = 0; p < (kDwThinSplit ? 1 : 2); ++p)
#pragma unroll
    for (int bi = 0; bi < BPW; ++bi) {
      if (!blive[bi]) continue;
      const int blk = BPW * wu + bi;
      f32x16 a1[4][1];
      a1[0][0] = acc[p][bi];
      const float b4[4] = {bs[p][bi], 0.f, 0.f, 0.f};
      dw_store<1>(J, split, kDwThinSplit ? mypart : p, wideA ? blk : 0, wideA ? 0 : blk, 1, 1, dbw[bi], a1, b4);
    }
}

}  // namespace spp
