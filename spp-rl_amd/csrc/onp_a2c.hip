// A2C's own update tail on the on-policy nets (onp.hip's tiles, OCfg, LDS table and dense<> blocks):
//  k_onp_td_adv         A2C.calculate_advantage (a2c.py:227-265) in one launch: the critic on x_next, then on x,
//                       q = r + gamma (1 - d) V(x'), adv = q - V(x), per-tile moment partials of adv
//  k_onp_td_moments     one workgroup: the partials -> {mean, std (ddof 1)} of adv
//  k_onp_pg_actor_grad  A2C.update_actor's backward (a2c.py:267-286; on_policy.py:100-124): k_onp_actor_grad's
//                       forward, log-prob and backward with the objective -logp * A / N, A normalised on the fly
//                       with A2C's (adv - mean) / (std + 1e-8)
// (included by api_onp.hip after onp.hip and ppo.hip: OnpArgs, onp_trunk, ppo_q)

namespace spp {

struct OnpA2cArgs {
  OnpArgs o;               // X = the observations; ACT, ADV, NXT as k_onp_actor_grad reads them
  const float *XN;         // [N][ob] next observations (td_adv)
  const float *REW, *DONE; // [N]
  float gamma;
  float *Q_OUT, *ADV_OUT;  // [N]; Q_OUT may be null
  const float* MOM;        // {mean, std} of ADV or null (pg_actor_grad)
  const float* DIST_ACT;   // [N][aout] the actions the distance is measured on, or null (= ACT)
};

template <class C>
__device__ __forceinline__ void onp_load_rows(f32x16 (&x)[C::NB_OB], const float* X, int br, bool valid, int h4) {
#pragma unroll
  for (int ib = 0; ib < C::NB_OB; ++ib)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * ib + ru(r) + h4;
      x[ib][r] = (u < C::OB && valid) ? X[(int64_t)br * C::OB + u] : 0.f;
    }
}

#define SPP_ONP_A2C_PROLOGUE                                                 \
  const OnpArgs& p = a.o;                                                    \
  __shared__ float smem[4 * 64 * 32];                                        \
  __shared__ __attribute__((aligned(16))) float tbl[1024];                   \
  onp_table(p, tbl);                                                         \
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5;    \
  const int h4 = 4 * h, s = lane & 31;                                       \
  float* img = smem + w * 64 * 32;                                           \
  float* bl = img + h4 * 32 + s;                                             \
  const int ntiles = p.Np / 32;

// Moment partials of a tile about its own first advantage (row 32 * tile is always a live row): slot 0 the pivot,
// 1 the rows, 2 sum (adv - pivot), 3 sum (adv - pivot)^2.  The differences are exact to half an ulp of themselves,
// so a mean far above the spread costs nothing; k_onp_td_moments joins the tiles in fp64.
template <class C>
__global__ __launch_bounds__(256) void k_onp_td_adv(OnpA2cArgs a) {
  SPP_ONP_A2C_PROLOGUE
  for (int tile = blockIdx.x * 4 + w; tile < ntiles; tile += gridDim.x * 4) {
    const int b = tile * 32 + s;
    const bool valid = b < p.N;
    const int br = valid ? b : 0;
    float vn;
    {
      f32x16 x[C::NB_OB], h1[2], h2[2];
      onp_load_rows<C>(x, a.XN, br, valid, h4);
      onp_trunk<C>(p.critic, x, tbl, img, bl, h1, h2);
      vn = onp_value<C>(p.critic, h2, tbl, h4);
    }
    float v;
    {
      f32x16 x[C::NB_OB], h1[2], h2[2];
      onp_load_rows<C>(x, p.X, br, valid, h4);
      onp_trunk<C>(p.critic, x, tbl, img, bl, h1, h2);
      v = onp_value<C>(p.critic, h2, tbl, h4);
    }
    const float q = ppo_q(a.REW[br], a.DONE[br], vn, a.gamma);
    const float adv = fsub_rn(q, v);
    if (valid && h == 0) {
      a.ADV_OUT[b] = adv;
      if (a.Q_OUT) a.Q_OUT[b] = q;
    }
    const float piv = __shfl(adv, 0, 64);
    const bool live = valid && h == 0;
    const float d = live ? fsub_rn(adv, piv) : 0.f;
    const float n = wave_sum(live ? 1.f : 0.f), s1 = wave_sum(d), s2 = wave_sum(d * d);
    if (lane == 0) {
      float* pt = p.part + (int64_t)tile * p.pstride;
      pt[0] = piv;
      pt[1] = n;
      pt[2] = s1;
      pt[3] = s2;
    }
  }
}

// {mean, std ddof 1} of the advantages from k_onp_td_adv's per-tile partials: each tile's mean and centred
// sum of squares in fp64, then the pairwise-update formula about the global mean (N = 1: std = NaN, as torch.std).
__global__ void k_onp_td_moments(const float* part, int ntiles, int stride, int N, float* mom) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  auto reduce = [&](double v) {
    red[t] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
  };
  double sm = 0.0;
  for (int i = t; i < ntiles; i += blockDim.x) {
    const float* pt = part + (int64_t)i * stride;
    sm += (double)pt[1] * (double)pt[0] + (double)pt[2];
  }
  const double mean = reduce(sm) / N;
  double m2 = 0.0;
  for (int i = t; i < ntiles; i += blockDim.x) {
    const float* pt = part + (int64_t)i * stride;
    const double n = pt[1], s1 = pt[2], s2 = pt[3];
    const double dm = (double)pt[0] + s1 / n - mean;
    m2 += (s2 - s1 * s1 / n) + n * dm * dm;
  }
  m2 = reduce(m2);
  if (t == 0) {
    mom[0] = (float)mean;
    mom[1] = (float)sqrt(fmax(m2, 0.0) / (double)(N - 1));
  }
}

// partials: [0] sum logp * A, [1] sum logp, [2] sum dist^2, [3 + j] sum d logp / d log_scale_j weighted by
// d loss / d logp = -A / N -- k_onp_actor_grad's slots, so k_onp_finish_actor (ent_coef 0) ends the step.
template <class C>
__global__ __launch_bounds__(256) void k_onp_pg_actor_grad(OnpA2cArgs a) {
  SPP_ONP_A2C_PROLOGUE
  const float invN = 1.f / (float)p.N;
  const float am = a.MOM ? a.MOM[0] : 0.f, ad = a.MOM ? fadd_rn(a.MOM[1], 1e-8f) : 1.f;
  const float* DA = a.DIST_ACT ? a.DIST_ACT : p.ACT;
  for (int tile = blockIdx.x * 4 + w; tile < ntiles; tile += gridDim.x * 4) {
    const int b = tile * 32 + s;
    const bool valid = b < p.N;
    const int br = valid ? b : 0;
    f32x16 x[C::NB_OB], h1[2], h2[2];
    onp_load_x<C>(x, p, br, valid, h4);
#pragma unroll
    for (int ib = 0; ib < C::NB_OB; ++ib)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (32 * ib + ru(r) + h4 < C::OB) p.XT[(int64_t)(32 * ib + ru(r) + h4) * p.Np + b] = x[ib][r];
    onp_trunk<C>(p.actor, x, tbl, img, bl, h1, h2);
    f32x16 t3[C::NB_AOUT];
    dense<2, C::RV_H>(p.actor.W3, C::NB_AOUT, h2, tbl + p.actor.tb3, [&](int ob, const f32x16& acc) {
#pragma unroll
      for (int ib = 0; ib < C::NB_AOUT; ++ib)
        if (ib == ob)
#pragma unroll
          for (int q = 0; q < 16; ++q) t3[ib][q] = tanhf(acc[q]);
    });
    // log_prob (torch Normal, summed over the action) and the data-only distance
    float lp = 0.f, dist = 0.f;
#pragma unroll
    for (int ib = 0; ib < C::NB_AOUT; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = 32 * ib + ru(q) + h4;
        if (j < C::AOUT) {
          const float sc = expf(p.log_scale[j]);
          const float mu = fmul_rn(t3[ib][q], p.lim[j]);
          const float ac = valid ? p.ACT[(int64_t)br * C::AOUT + j] : 0.f;
          const float d = fsub_rn(ac, mu);
          lp += fsub_rn(fsub_rn(fdiv_rn(-fmul_rn(d, d), 2.f * fmul_rn(sc, sc)), logf(sc)), kLogSqrt2PiO);
          if (p.NXT && valid) {
            const float e = fsub_rn(DA[(int64_t)br * C::AOUT + j], p.NXT[(int64_t)br * C::AOUT + j]);
            dist += e * e;
          }
        }
      }
    lp += __shfl_xor(lp, 32, 64);
    // A (a2c.py:274-277) and d loss / d logp
    float A = 0.f;
    if (valid) {
      A = p.ADV[br];
      if (a.MOM) A = fdiv_rn(fsub_rn(A, am), ad);
    }
    const float glp = -A * invN;
    f32x16 du3[C::NB_AOUT];
    float gls[C::NB_AOUT * 16];
#pragma unroll
    for (int ib = 0; ib < C::NB_AOUT; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = 32 * ib + ru(q) + h4;
        float g = 0.f, gl = 0.f;
        if (j < C::AOUT && valid) {
          const float sc = expf(p.log_scale[j]);
          const float var = fmul_rn(sc, sc);
          const float mu = fmul_rn(t3[ib][q], p.lim[j]);
          const float d = fsub_rn(p.ACT[(int64_t)br * C::AOUT + j], mu);
          const float gmu = glp * d / var;
          gl = glp * (d * d / var - 1.f);
          g = gmu * p.lim[j] * (1.f - t3[ib][q] * t3[ib][q]);
        }
        du3[ib][q] = g;
        gls[ib * 16 + q] = gl;
        if (j < C::AOUT) p.D3[(int64_t)j * p.Np + b] = g;
      }
    f32x16 d2[2];
    dense<C::NB_AOUT, C::RV_AOUT>(p.actor.W3T, 2, du3, nullptr, [&](int ob, const f32x16& acc) {
      const f32x16 hh = ob == 0 ? h2[0] : h2[1];
      f32x16 v;
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = acc[q] * (1.f - hh[q] * hh[q]);
      if (ob == 0) d2[0] = v;
      else d2[1] = v;
    });
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int u = 32 * ib + ru(q) + h4;
        p.H1[(int64_t)u * p.Np + b] = h1[ib][q];
        p.H2[(int64_t)u * p.Np + b] = h2[ib][q];
        p.D2[(int64_t)u * p.Np + b] = d2[ib][q];
      }
    dense<2, C::RV_H>(p.actor.W2T, 2, d2, nullptr, [&](int ob, const f32x16& acc) {
      const f32x16 hh = ob == 0 ? h1[0] : h1[1];
#pragma unroll
      for (int q = 0; q < 16; ++q)
        p.D1[(int64_t)(32 * ob + ru(q) + h4) * p.Np + b] = acc[q] * (1.f - hh[q] * hh[q]);
    });
    const bool live = valid && h == 0;
    const float sl = wave_sum(live ? lp * A : 0.f), sp = wave_sum(live ? lp : 0.f), sd = wave_sum(dist);
    if (lane == 0) {
      p.part[tile * p.pstride + 0] = sl;
      p.part[tile * p.pstride + 1] = sp;
      p.part[tile * p.pstride + 2] = sd;
    }
#pragma unroll
    for (int ib = 0; ib < C::NB_AOUT; ++ib)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float v = gls[ib * 16 + q];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        const int j = 32 * ib + ru(q) + h4;
        if (s == 0 && j < C::AOUT) p.part[tile * p.pstride + 3 + j] = v;
      }
  }
}
#undef SPP_ONP_A2C_PROLOGUE

}  // namespace spp
