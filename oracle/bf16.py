"""ORACLE (test infrastructure only): the linear layer of the bf16 kernel sets, restated.

``SAC_AcM(mlp_bf16=True)`` runs every MLP matmul as v_mfma_f32_32x32x16_bf16: both operands bf16, fp32
accumulation, fp32 bias / epilogue / targets / losses.  The ONE kind of rounding there is a single
round-to-nearest-even conversion of an fp32 value where it becomes an MFMA operand or is stored as one;
``rne`` restates it (``x.float().to(torch.bfloat16)``) and ``linear`` applies it at the same points, computing
everything else in the oracle's dtype (float64: a reference whose own summation error is negligible).

Where the kernels convert (spp-rl_amd/csrc; "R(.)" = one RNE fp32 -> bf16, everything else fp32):

  every forward / backward-data matmul is dense<.., C::BF> / dense_lds<.., C::BF> (mlp.h:531-554), i.e.
    dense16_impl      mlp.h:449   bin = to_bf16x8(in)        (mlp.h:403-408, ``(__bf16)t[..]``: RNE)
    dense16_lds_impl  mlp.h:510   b0, b1 = to_bf16x8(x)      (x read back from the fp32 LDS image)
    weights           optim.hip k_pack_matrix (PackJob::bf16): bf16 image = R(fp32 master), re-packed after
                      every Adam step; the bias / fc3 tables (load_table, sac.hip:56-62) are the fp32 master
  the two-tile critic phase (sac_bf.h, acm_critic sets) keeps the hand-off between layers as the bf16 operand
    itself: img16_put sac_bf.h:51-60 = R(fp32 epilogue value), the value dense16_lds_impl's reader would
    have converted; to_steps sac_bf.h:196-201 for register inputs.  Same roundings, same places.  That kernel
    is an A/B variant: it is compiled only with -DSPP_BF16_TWO_TILES=1 (common.h:14-21, kset.h:36-38; default 0),
    so the library the tests load runs the one-tile k_sac_critic_phase (sac.hip) for every bf16 set.
  weight-gradient operands: op_st<C::BF> (mlp.h:614-618 -> fm_st16 mlp.h:608-612, R(v)) stores H1, H2, D1,
    D2, AH1, AH2, AD1, AD2 as bf16; k_dw reads those as they are (as_bf8 dw.hip:55,120) and converts the
    fp32-sourced ones -- staged [s | a], DQ, ADH -- with pack8 (dw.hip:46-51,120-122: R).  The bias
    gradient sums the A rows it read: R(delta) for bf16 rows (sum_bf8 dw.hip:57-65,115), the fp32 delta for
    fp32 rows (dw.hip:117-118).

  matmul of the update                     forward / data-gradient operands        weight-gradient (k_dw job; csrc/api.hip)
  ---------------------------------------  --------------------------------------  -------------------------------------
  actor fc1      (target a', and a)        R(s) R(W1)          sac.hip:260          R(AD1) R(s)^T, db = sum R(AD1)  api.hip build_dw
  actor fc2                                R(h1) R(W2)         sac.hip:276          R(AD2) R(AH1)^T, sum R(AD2)     api.hip build_dw
  actor fc_prob | fc_scale                 R(h2) R(Wh)         sac.hip:291          R(ADH) R(AH2)^T, db = sum ADH   api.hip build_dw
    (two-tile target pass: sac_bf.h:272,281,291; bias added in fp32 sac_bf.h:301-302)
  actor heads^T . d heads                  R(ADH) R(Wh)        sac.hip:861,994      (delta AD2 = relu' . acc, op_st sac.hip:867,1000)
  actor W2^T . AD2                         R(AD2) R(W2)        sac.hip:871,1003     (delta AD1, op_st sac.hip:874,1006)
  ACM fc1 / fc2 / fc3 (frozen)             R(in) R(W)          sac.hip:309,320,336  none (z1, z2, t3 stay fp32: fm_st sac.hip:315,325,343)
  ACM W3^T / W2^T / W1a^T . delta          R(delta) R(W)       sac.hip:729,739,749  none
  critic / target fc1                      R([s|c]) R(W1)      sac.hip:358, sac_bf.h:248,254,345,389
                                                                                    R(D1) R([s|a])^T, sum R(D1)     api.hip critic_dw
  critic / target fc2                      R(h1) R(W2)         sac.hip:373, sac_bf.h:357,413
                                                                                    R(D2) R(H1)^T, sum R(D2)        api.hip critic_dw
  critic / target fc3                      fp32: q = w3 . h2 + b3, fmaf over the table's fp32 w3
                                           sac.hip:382,388, sac_bf.h:361,365,423,434
                                                                                    R(DQ) R(H2)^T, db = sum DQ      api.hip critic_dw
                                                                                    (bf16 sets build with SPP_BF16_FUSE3 = 0:
                                                                                    fc3 is a k_dw job, not fused, common.h:22)
  critic delta2 = dq w3 relu'(h2)          fp32 product        sac.hip:547,674, sac_bf.h:454
  critic W2^T . delta2                     R(D2) R(W2)         sac.hip:555,677, sac_bf.h:463  (D1 = relu' . acc, op_st sac.hip:558)
  critic W1a^T . delta1 (actor phase)      R(D1) R(W1)         sac.hip:682

Not rounded anywhere: accumulators, biases, every epilogue (relu, tanh, squash, log-prob), the target y, the
losses, DQ, ADH and the staged inputs.  The bf16 sets evaluate exp / log / tanh of the squash
with the hardware forms (sac.hip:143-165, ~1 ulp of fp32) and the Normal log-prob in its algebraic form
(sac.hip:428-429); both are fp32-level effects and are not restated.

``Mode`` names what a layer rounds: ``HIDDEN`` (bf16-stored delta), ``HEAD`` (fp32-stored delta: the bias
gradient sums the unrounded delta), ``CRITIC_FC3`` (fp32 forward and data gradient, bf16 weight-gradient
operands), ``EXACT`` (no rounding: F.linear).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

# fwd: forward operands; dx: data-gradient operands (delta, W); dw: weight-gradient operands (delta, x);
# db: the bias gradient sums the rounded delta
Mode = namedtuple("Mode", "fwd dx dw db")
EXACT = Mode(False, False, False, False)
HIDDEN = Mode(True, True, True, True)
HEAD = Mode(True, True, True, False)
CRITIC_FC3 = Mode(False, False, True, False)


def rne(x):
    """One fp32 -> bf16 round-to-nearest-even conversion of the fp32 value of x, in x's dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


class _Bf16Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, mode):
        ctx.mode = mode
        ctx.save_for_backward(x, w)
        if mode.fwd:
            x, w = rne(x), rne(w)
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        mode = ctx.mode
        dyr = rne(dy) if (mode.dx or mode.dw or mode.db) else dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dyr @ rne(w)) if mode.dx else (dy @ w)
        if ctx.needs_input_grad[1]:
            dw = (dyr.t() @ rne(x)) if mode.dw else (dy.t() @ x)
        if ctx.needs_input_grad[2]:
            db = (dyr if mode.db else dy).sum(0)
        return dx, dw, db, None


def linear(x, w, b, mode=None):
    """F.linear(x, w, b) with the bf16 kernel sets' operand roundings (mode None: F.linear itself)."""
    if mode is None:
        return F.linear(x, w, b)
    return _Bf16Linear.apply(x, w, b, mode)
