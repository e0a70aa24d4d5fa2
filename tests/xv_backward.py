"""The stages of the x-vector backward, restated for the stage pins of tests/test_gpu_backward_stages.py.  TEST
INFRASTRUCTURE (a plain module, not a conftest); proved on the CPU, without the engine, by tests/test_backward_stages_power.py.

Two kinds of restatement, as for the forward half (tests/xv_fold.py, oracle/conv_chain.c):

* bitwise -- the split-K slabs of the two data gradients that have no single chain, read from the arguments
  ``run_tdnn_backward`` (speakerguard_amd/csrc/sg_api.hip) hands ``launch_conv_gemm``:
    fc1 backward    A = demb (B, 512), W = fc1_wt (512, 3072), 16 chunks of 32, 2 per slab: slab z of ``dstats_part`` is the
                    fmaf chain over k = 64 z .. 64 z + 63;
    tdnn1 backward  A = dact1 (B F_1, 512), W = wb[0] (5 x 512, 32), tap step -1, 80 chunks, 8 per slab: slab z of ``dfeats`` is
                    tap z // 2 (source row t - z // 2; a row outside the utterance enters as zeros), channels 256 (z % 2) ..
                    + 255;
  and the ordered float32 sum ``0.f + s_0 + ... + s_{n-1}`` by which sum_cols_kernel, cmvn_bwd_kernel and pool_bwd_kernel
  (k_misc.hip) add the slabs.
* float64 -- the formulas of statistics pooling's backward, of the CMVN adjoint and of the tail, each with the same
  computation in float32 as the yardstick, and the judgement (``judge``: the per-utterance rule of tests/truth.py with a
  frame row as the block; ``cmvn_bound``: the a-priori elementwise bound of the CMVN adjoint).
"""
import numpy as np
import torch

import truth
import xv_fold
from oracle.conv_chain import conv_chain
from oracle.xv_plda import cmvn_window

FC1_SLABS, L1_SLABS = 8, 10  # kFc1BwdSplitK, kL1BwdSplitK (sg_internal.h)
FEAT, FEAT_PAD = 30, 32
EPS32 = truth.EPS32


# ------------------------------------------------------------------------------------------------------ bitwise stages
def ordered_sum(slabs):
    """float32 ``0.f + s_0 + s_1 + ...`` over the leading axis, one rounding per addition, in slab order"""
    slabs = np.asarray(slabs, np.float32)
    v = np.zeros(slabs.shape[1:], np.float32)
    for s in slabs:
        v = v + s
    return v


def fc1_bwd_slab(demb, fd, z):
    """slab z of fc1's data gradient: demb (B, 512) -> (B, 3072)"""
    demb = np.ascontiguousarray(demb, np.float32)
    wt = np.ascontiguousarray(fd.fc1_w.T)  # (512, 3072): the loader's fc1_wt
    k0 = z * (xv_fold.EMB // FC1_SLABS)
    k1 = k0 + xv_fold.EMB // FC1_SLABS
    return conv_chain(demb[:, k0:k1], wt[k0:k1], demb.shape[0], 1, 1, 1, 0, 0)


def tdnn1_bwd_slab(dact1, fd, B, F, z):
    """slab z of tdnn1's data gradient: dact1 (B * F_1, 512) -> (B * F, 32), one tap and one half of the channels"""
    F1 = xv_fold.layer_frames(F)[0]
    j, h = z // 2, z % 2
    half = xv_fold.COUT_PAD[0] // 2
    a = np.ascontiguousarray(np.asarray(dact1, np.float32)[:, h * half:(h + 1) * half])
    w = fd.wb[0][j * xv_fold.COUT_PAD[0] + h * half:j * xv_fold.COUT_PAD[0] + (h + 1) * half]
    return conv_chain(a, w, B, F1, F, 1, 0, -j)


def dgrad(dact, fd, layer, B, F, mask):
    """d(out) of tdnn `layer` (2..5), (B * F_l, C_pad) -> d(in) under the ReLU mask `mask` (B * F_{l-1}, 512): one chain"""
    l = layer - 1
    fl = xv_fold.layer_frames(F)
    return conv_chain(dact, fd.wb[l], B, fl[l], fl[l - 1], xv_fold.TAPS[l], -xv_fold.DIL[l], 0, mask=mask)


# ------------------------------------------------------------------------------------------------------ float64 stages
def pool_bwd(act5, dstats, dtype=torch.float64):
    """statistics pooling's backward: act5 (B, Tc, C) ReLU output, dstats (B, 2 C) = [d mean | d std] ->
    d act5 = relu'(act5) (d mean / Tc + d std (act5 - mean) / ((Tc - 1) std)), no std term where std == 0 (torch's
    std_backward), all in `dtype`; mean and the unbiased std are taken from act5 itself"""
    a = torch.as_tensor(np.asarray(act5)).to(dtype)
    d = torch.as_tensor(np.asarray(dstats)).to(dtype)
    Tc, C = a.shape[1], a.shape[2]
    mean = a.mean(1, keepdim=True)
    sd = a.std(1, keepdim=True)
    dmean, dstd = d[:, None, :C], d[:, None, C:]
    beta = torch.where(sd > 0, dstd / ((Tc - 1) * torch.where(sd > 0, sd, torch.ones_like(sd))), torch.zeros_like(sd))
    return ((a > 0).to(dtype) * (dmean / Tc + beta * (a - mean))).numpy()


def cmvn_matrix(F):
    """(F, F) float64: row t holds 1 / |window(t)| over window(t) -- CMVN is x - W x, its adjoint g - W^T g"""
    W = np.zeros((F, F))
    for t in range(F):
        s, e = cmvn_window(t, F)
        W[t, s:e] = 1.0 / (e - s)
    return W


def cmvn_adjoint(g, W=None):
    """g (B, F, 30) summed cotangent -> (the float64 adjoint g - m, the mean term m = W^T g)"""
    g = np.asarray(g, np.float64)
    W = cmvn_matrix(g.shape[1]) if W is None else W
    m = np.einsum("tu,btd->bud", W, g)
    return g - m, m


def cmvn_bound(g, m):
    """|got - truth| <= 2 eps32 (|v| + |m|), elementwise: the kernel rounds the mean term to float once (|m| eps32 / 2) and
    subtracts in float once (|v - m| eps32 / 2 <= (|v| + |m|) eps32 / 2), its double accumulation of <= 601 terms is nine
    orders below: (|v| + 2 |m|) eps32 / 2 at worst, so the factor 2 leaves between 2x (m dominates) and 4x (v dominates)"""
    return 2.0 * EPS32 * (np.abs(np.asarray(g, np.float64)) + np.abs(m))


def cmvn_misses(got, g, W=None):
    """elements of `got` (B, F, 30) outside the bound against the adjoint of g -> (count, worst error / bound)"""
    want, m = cmvn_adjoint(g, W)
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = cmvn_bound(g, m)
    bad = ~(err <= bound)
    return int(bad.sum()), float((err / np.maximum(bound, 1e-300)).max())


def cmvn_adjoint_fp32(g):
    """cmvn_bwd_kernel restated in numpy, both branches: g (B, F, 30) float32 -> float32.  F <= 300: one column mean,
    accumulated in double, divided by F in double, rounded to float, subtracted in float.  F > 300: per output frame u the
    double sum over the frames t whose window holds u of double(g[t]) / |window(t)|, rounded to float, subtracted in float."""
    g = np.asarray(g, np.float32)
    B, F, D = g.shape
    if F <= 300:
        mean = (g.astype(np.float64).sum(1, keepdims=True) / float(F)).astype(np.float32)
        return g - mean
    wins = np.array([cmvn_window(t, F) for t in range(F)])
    inside = (wins[:, :1] <= np.arange(F)[None]) & (np.arange(F)[None] < wins[:, 1:])  # [t, u]: window(t) holds u
    terms = g.astype(np.float64) / (wins[:, 1] - wins[:, 0]).astype(np.float64)[None, :, None]  # divided term by term
    acc = np.einsum("tu,btd->bud", inside.astype(np.float64), terms)  # (the order of a double sum is far below the bound)
    return g - acc.astype(np.float32)


def tail_grad(om, temb, y, loss, dtype=torch.float64):
    """d loss / d tdnn_emb by autograd of the oracle's tail (mean subtraction, LDA, detached length norm, PLDA transform,
    LLR against the enrolled table, loss) in `dtype`: temb (B, 512) -> (B, 512) float64.  `om`: an oracle.xv_plda.XvPlda of
    that dtype, `loss`: a truth.Loss."""
    t = torch.as_tensor(np.asarray(temb)).to(dtype).clone().requires_grad_(True)
    s = om.scoring_trials(om.enroll_embs, om.process_emb_batch(t))
    l = loss(s, torch.as_tensor(np.asarray(y), dtype=torch.int64))
    l.backward(torch.ones_like(l))
    return t.grad.double().numpy()


# ------------------------------------------------------------------------------------------------------ the judgement
def judge(got, yard, want, hop):
    """The per-utterance gradient rule of tests/truth.py (POLICY: C, FLOOR_UTT, FLOOR_BLOCK), `hop` entries (one frame row)
    per block: (list of (metric, utterance, value, bound) violated, one line of judged / yard / bound, the largest judged
    error over its bound)."""
    P = truth.POLICY
    B = np.asarray(got).shape[0]
    got, yard, want = (np.asarray(a, np.float64).reshape(B, -1) for a in (got, yard, want))
    fails, worst = [], {}
    for name, fn, floor in (("utt", truth.utt_error, P["FLOOR_UTT"]),
                            ("block", lambda a, b: truth.block_error(a, b, hop), P["FLOOR_BLOCK"])):
        j, y = fn(got, want), fn(yard, want)
        bound = P["C"] * np.maximum(y, floor)
        worst[name] = (float(j.max()), float(y.max()), float(bound.min()), float((j / bound).max()))
        fails += [(name, int(u), float(j[u]), float(bound[u])) for u in np.flatnonzero(~(j <= bound))]
    signs = truth.decided_sign(got, want)
    fails += [("decided_sign", int(u), int(signs[u]), 0) for u in np.flatnonzero(signs != 0)]
    line = ("utt judged %.2e yard %.2e bound >= %.2e (worst %.2f of it), block judged %.2e yard %.2e bound >= %.2e (worst %.2f "
            "of it), decided signs %d" % (worst["utt"] + worst["block"] + (int(signs.sum()),)))
    return fails, line, max(worst["utt"][3], worst["block"][3])
