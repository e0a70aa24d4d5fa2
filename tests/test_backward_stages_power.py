"""The tools of tests/test_gpu_backward_stages.py (tests/xv_backward.py), proved on the CPU before the engine is judged by them.

(a) The three float64 stage formulas -- statistics pooling's backward, the CMVN adjoint as the transposed window matrix,
    the tail -- equal float64 autograd of the oracle's own stages to 1e-12 of the largest entry.
(b) The slab restatement is self-consistent: the 10 tdnn1 slabs and the 8 fc1 slabs, summed in float64, are the float64
    contraction to float32 accumulation error (sqrt(K) eps32 of the largest entry, K = 2560 and 512: the random-walk bound of
    tests/test_layer_chain_power.py).
(c) The judgement accepts float32: the kernels' own arithmetic restated in numpy (pooling: the four frame-strided partial
    sums of pool_fwd_kernel and pool_bwd_kernel's alpha / beta; CMVN: both branches of cmvn_bwd_kernel; the tail: the
    oracle's per-utterance float32 path) against the float32 torch yard, at every frame count of the GPU grid, every F of the
    stand-alone CMVN cases and every back-end corner count.
(d) The judgement rejects planted defects, each planted in a copy of a restated result, never in a kernel.
"""
import copy

import numpy as np
import pytest
import torch

import plda_cases
import truth
import xv_backward as xb
import xv_fold
from conftest import log

CMVN_F = (32, 299, 300, 301, 451, 600, 601)  # the stand-alone cases of the GPU module
POOL_TC = (2, 71, 270, 368, 369, 384, 385)   # F5 of the GPU grid: 5040, 16123, 48000, 63680, 63840, 66240, 66400 samples
B, T = 3, 16000


@pytest.fixture(scope="module")
def weights():
    from speakerguard_amd import synth
    return synth.make_xv_weights(seed=0, D=200, n_spk=10)


@pytest.fixture(scope="module")
def fd(weights):
    return xv_fold.fold(weights["state_dict"])


@pytest.fixture(scope="module")
def om(weights):
    from oracle.xv_plda import XvPlda
    return XvPlda(weights)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def pool_case(Tc, seed=0, C=96):
    """a ReLU output (B, Tc, C) with dead channels, a channel alive in one frame only, and d stats"""
    rng = np.random.RandomState(seed + Tc)
    a = np.maximum(rng.standard_normal((B, Tc, C)) + 0.3, 0).astype(np.float32)
    a[:, :, 5] = 0
    a[:, :, 17] = 0
    a[:, 1:, 29] = 0
    a[:, 0, 29] = 0.7
    return a, rng.standard_normal((B, 2 * C)).astype(np.float32)


def pool_bwd_kernel_fp32(a, d, tc_minus=1, std_term=True, mask_ge=False):
    """pool_fwd_kernel's statistics (four frame-strided float32 partial sums, two passes) and pool_bwd_kernel's float32
    alpha + beta (v - mean); the keywords plant the defects of (d)"""
    a, d = np.asarray(a, np.float32), np.asarray(d, np.float32)
    Tc, C = a.shape[1], a.shape[2]
    f = np.float32

    def strided(v):
        parts = []
        for w in range(4):
            s = np.zeros((v.shape[0], C), np.float32)
            for t in range(w, Tc, 4):
                s = s + v[:, t]
            parts.append(s)
        return ((parts[0] + parts[1]) + parts[2]) + parts[3]
    mean = strided(a) / f(Tc)
    dev = a - mean[:, None]
    sd = np.sqrt(strided(dev * dev) / f(Tc - 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = np.where(sd > 0, d[:, C:] / (f(Tc - tc_minus) * sd), f(0)).astype(np.float32)
    if not std_term:
        beta = np.zeros_like(beta)
    alpha = d[:, :C] / f(Tc)
    on = (a >= 0) if mask_ge else (a > 0)
    return np.where(on, alpha[:, None] + beta[:, None] * (a - mean[:, None]), f(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ (a) the formulas
@pytest.mark.parametrize("Tc", (2, 71))
def test_pooling_formula_is_float64_autograd_of_the_oracles_pooling(Tc):
    a, d = pool_case(Tc)
    rng = np.random.RandomState(1)
    z = torch.from_numpy(np.where(a > 0, a, -np.abs(rng.standard_normal(a.shape))).astype(np.float64)).requires_grad_(True)
    h = torch.relu(z).transpose(1, 2)  # (B, C, Tc) as xvecTDNN.py:62 pools it
    stats = torch.cat((h.mean(dim=2), h.std(dim=2)), dim=1)
    (stats * torch.from_numpy(d.astype(np.float64))).sum().backward()
    got = xb.pool_bwd(a, d)
    assert rel(got, z.grad.numpy()) <= 1e-12
    assert not got[:, :, (5, 17)].any()


@pytest.mark.parametrize("F", (32, 301, 451))
def test_cmvn_adjoint_is_float64_autograd_of_the_oracles_cmvn(F):
    from oracle.xv_plda import cmvn_closed_form, cmvn_loop
    rng = np.random.RandomState(F)
    x = torch.from_numpy(rng.standard_normal((B, F, 30))).requires_grad_(True)
    g = rng.standard_normal((B, F, 30))
    y = cmvn_closed_form(x)
    assert rel(y[0].detach().numpy(), cmvn_loop(x[0].detach().float()).double().numpy()) <= 1e-4  # (the reference's loop, float32)
    (y * torch.from_numpy(g)).sum().backward()
    want, m = xb.cmvn_adjoint(g)
    assert rel(want, x.grad.numpy()) <= 1e-12
    assert np.allclose(g - m, want)


@pytest.mark.parametrize("kind", ("ce", "margin"))
def test_tail_gradient_is_float64_autograd_of_the_oracles_per_utterance_tail(om, kind):
    om64 = copy.deepcopy(om).double()
    rng = np.random.RandomState(4)
    temb = rng.standard_normal((B, 512)) * 3
    y = np.array([1, 7, 2])
    loss = truth.Loss(kind, clip_max=False)
    t = torch.from_numpy(temb).requires_grad_(True)
    emb = torch.stack([om64.process_emb(e) for e in t], 0)  # iv_plda.process_emb, one utterance at a time
    l = loss(om64.scoring_trials(om64.enroll_embs, emb), torch.from_numpy(y))
    l.backward(torch.ones_like(l))
    # tail_grad IS float64 autograd of the oracle's batched tail; the per-utterance path is the same arithmetic but for one
    # constant: it takes sqrt(D) of a float32 tensor (xvector_extract.py:33 keeps it a float), a relative 2.4e-8 at D = 200.
    # The length norm's scale enters the LLR squared and the gradient at most squared again, so 8 eps32 bounds the
    # difference (measured: 3.3e-9); a tail that differs in structure is off by its whole size
    err = rel(xb.tail_grad(om64, temb, y, loss), t.grad.numpy())
    log("power, tail gradient %s: batched vs per-utterance float64 autograd %.2e of max |g|" % (kind, err))
    assert err <= 8 * xb.EPS32


# ------------------------------------------------------------------------------------------------ (b) the slabs
def test_tdnn1_slabs_sum_to_the_float64_contraction(weights, fd):
    F = 41
    F1 = xv_fold.layer_frames(F)[0]
    rng = np.random.RandomState(7)
    dact1 = rng.standard_normal((B * F1, 512)).astype(np.float32)
    slabs = np.stack([xb.tdnn1_bwd_slab(dact1, fd, B, F, z) for z in range(xb.L1_SLABS)])
    assert not slabs[:, :, xb.FEAT:].view(np.uint32).any(), "pad columns 30, 31 are not +0"
    x = torch.zeros(B, 30, F, dtype=torch.float64, requires_grad=True)
    w = torch.from_numpy(np.asarray(weights["state_dict"]["tdnn1.weight"], np.float64))
    out = torch.nn.functional.conv1d(x, w)  # (B, 512, F1)
    (out * torch.from_numpy(dact1.astype(np.float64)).view(B, F1, 512).transpose(1, 2)).sum().backward()
    want = x.grad.transpose(1, 2).reshape(B * F, 30).numpy()
    got = slabs.astype(np.float64).sum(0)[:, :xb.FEAT]
    assert rel(got, want) <= np.sqrt(5 * 512) * xb.EPS32
    # rows outside the utterance contribute zero: the first j output rows of tap j's two slabs, in every utterance
    for z in range(xb.L1_SLABS):
        rows = slabs[z].reshape(B, F, 32)
        assert not rows[:, F1 + z // 2:].any() and not rows[:, :z // 2].any(), z


def test_fc1_slabs_sum_to_the_float64_contraction(fd):
    rng = np.random.RandomState(8)
    demb = rng.standard_normal((B, 512)).astype(np.float32)
    slabs = np.stack([xb.fc1_bwd_slab(demb, fd, z) for z in range(xb.FC1_SLABS)])
    want = demb.astype(np.float64) @ fd.fc1_w.astype(np.float64).T
    assert rel(slabs.astype(np.float64).sum(0), want) <= np.sqrt(512) * xb.EPS32
    for lo in (1500, 1536 + 1500):
        assert not slabs[:, :, lo:lo + 36].view(np.uint32).any(), "pad columns are not +0"
    assert rel(xb.ordered_sum(slabs), want) <= np.sqrt(512) * xb.EPS32


# ------------------------------------------------------------------------------------------------ (c) float32 passes
@pytest.mark.parametrize("Tc", POOL_TC)
def test_judgement_accepts_the_restated_pooling_kernel(Tc):
    a, d = pool_case(Tc)
    want, yard = xb.pool_bwd(a, d), xb.pool_bwd(a, d, torch.float32)
    got = pool_bwd_kernel_fp32(a, d)
    fails, line, _ = xb.judge(got, yard, want, a.shape[2])
    log("power, pooling backward Tc=%d: %s" % (Tc, line))
    assert not fails, fails
    assert not got[:, :, (5, 17)].view(np.uint32).any()


@pytest.mark.parametrize("F", CMVN_F)
def test_cmvn_bound_holds_for_the_restated_kernel_branches(F):
    """the bound is a condition on the kernel's arithmetic: its float32 restatement has to sit inside it, with room"""
    g = np.random.RandomState(100 + F).standard_normal((B, F, 30)).astype(np.float32)
    n, worst = xb.cmvn_misses(xb.cmvn_adjoint_fp32(g), g)
    log("power, CMVN adjoint F=%d (%s branch): restated kernel at %.2f of the bound" % (F, "register" if F <= 300 else "sliding", worst))
    assert n == 0 and worst <= 0.5, (n, worst)
    # a cotangent with a large common offset: the mean term dominates
    n, worst = xb.cmvn_misses(xb.cmvn_adjoint_fp32(g + np.float32(50)), g + np.float32(50))
    assert n == 0 and worst <= 0.5, (n, worst)


def corner_model(S):
    from oracle.xv_plda import XvPlda
    w = dict(plda_cases.xv_weights())
    w["enroll"] = w["enroll"][:S]
    return XvPlda(w)


@pytest.fixture(scope="module")
def corner_temb():
    m = corner_model(1)
    with torch.no_grad():
        feats = m.compute_feat(torch.from_numpy(plda_cases.waveforms()), flag=2)
        return m.tdnn_embedding(feats.transpose(1, 2)).numpy()


@pytest.mark.parametrize("kind", ("ce", "margin"))
@pytest.mark.parametrize("S", plda_cases.S_CASES)
def test_judgement_accepts_the_float32_tail_at_the_corner_counts(corner_temb, S, kind):
    m = corner_model(S)
    y = np.arange(plda_cases.B) % S
    loss = truth.Loss(kind, clip_max=False)
    want = xb.tail_grad(copy.deepcopy(m).double(), corner_temb, y, loss)
    yard = xb.tail_grad(m, corner_temb, y, loss, torch.float32)
    t = torch.from_numpy(corner_temb).clone().requires_grad_(True)
    l = loss(m.scoring_trials(m.enroll_embs, torch.stack([m.process_emb(e) for e in t], 0)), torch.from_numpy(y))
    l.backward(torch.ones_like(l))
    fails, line, _ = xb.judge(t.grad.numpy(), yard, want, 512)
    log("power, tail gradient S=%d %s: %s" % (S, kind, line))
    assert not fails, fails
    if S == 1 and kind == "ce":
        assert not want.any(), "one class: the cross-entropy is constant"


@pytest.mark.parametrize("kind", ("ce", "margin"))
def test_judgement_accepts_the_float32_tail_on_the_standard_weights(om, kind):
    """B = 5, ragged: the other tail case of the GPU module"""
    from speakerguard_amd import synth
    with torch.no_grad():
        feats = om.compute_feat(torch.from_numpy(synth.make_waveforms(5, 16123, seed=2000 + 5 + 16123)), flag=2)
        temb = om.tdnn_embedding(feats.transpose(1, 2)).numpy()
    y = np.arange(5) % 10
    loss = truth.Loss(kind, clip_max=False)
    want = xb.tail_grad(copy.deepcopy(om).double(), temb, y, loss)
    yard = xb.tail_grad(om, temb, y, loss, torch.float32)
    t = torch.from_numpy(temb).clone().requires_grad_(True)
    l = loss(om.scoring_trials(om.enroll_embs, torch.stack([om.process_emb(e) for e in t], 0)), torch.from_numpy(y))
    l.backward(torch.ones_like(l))
    fails, line, _ = xb.judge(t.grad.numpy(), yard, want, 512)
    log("power, tail gradient standard weights B=5 %s: %s" % (kind, line))
    assert not fails and np.abs(want).max() > 0, fails


# ------------------------------------------------------------------------------------------------ (d) planted defects
@pytest.mark.parametrize("Tc", (2, 71, 270))
@pytest.mark.parametrize("defect", ("Tc for Tc - 1", "std term dropped", "mask >= 0"))
def test_judgement_rejects_a_pooling_defect(Tc, defect):
    a, d = pool_case(Tc)
    want, yard = xb.pool_bwd(a, d), xb.pool_bwd(a, d, torch.float32)
    kw = {"Tc for Tc - 1": dict(tc_minus=0), "std term dropped": dict(std_term=False), "mask >= 0": dict(mask_ge=True)}[defect]
    fails, line, _ = xb.judge(pool_bwd_kernel_fp32(a, d, **kw), yard, want, a.shape[2])
    log("power, pooling backward Tc=%d with %s: %s" % (Tc, defect, line))
    assert fails, line


def planted_windows(F, defect):
    from oracle.xv_plda import cmvn_window
    W = np.zeros((F, F))
    for t in range(F):
        s, e = cmvn_window(t, F)
        n = e - s
        if defect == "shifted by one frame":
            s, e = cmvn_window(min(t + 1, F - 1), F)
        elif defect == "clamped at one end only":  # the start is clamped, the end is not moved back in
            s = max(t - 150, 0)
            e = min(s + 300, F)
            n = e - s
        elif defect == "|window| = 300":
            n = 300
        W[t, s:e] = 1.0 / n
    return W


@pytest.mark.parametrize("F,defect", [(451, "shifted by one frame"), (601, "shifted by one frame"), (451, "clamped at one end only"),
                                      (301, "clamped at one end only"), (32, "|window| = 300"), (299, "|window| = 300")])
def test_cmvn_bound_rejects_a_wrong_window(F, defect):
    g = np.random.RandomState(100 + F).standard_normal((B, F, 30)).astype(np.float32)
    wrong = xb.cmvn_adjoint(g, planted_windows(F, defect))[0].astype(np.float32)
    n, worst = xb.cmvn_misses(wrong, g)
    log("power, CMVN adjoint F=%d with the window %s: %d elements outside, worst %.1f x the bound" % (F, defect, n, worst))
    assert n > 0 and worst > 10


def slab_case(fd):
    F = 41
    F1 = xv_fold.layer_frames(F)[0]
    dact1 = np.random.RandomState(9).standard_normal((B * F1, 512)).astype(np.float32)
    return F, F1, dact1, np.stack([xb.tdnn1_bwd_slab(dact1, fd, B, F, z) for z in range(xb.L1_SLABS)])


@pytest.mark.parametrize("defect", ("one slab left out", "one slab added twice", "two slabs swapped"))
def test_slab_sum_checks_reject_a_wrong_sum(fd, defect):
    F, _, _, slabs = slab_case(fd)
    order = {"one slab left out": [0, 1, 2, 3, 4, 5, 6, 8, 9], "one slab added twice": [0, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9],
             "two slabs swapped": [0, 1, 2, 7, 4, 5, 6, 3, 8, 9]}[defect]
    right, wrong = xb.ordered_sum(slabs), xb.ordered_sum(slabs[order])
    assert xv_fold.bit_mismatch(right, xb.ordered_sum(slabs), F) is None
    msg = xv_fold.bit_mismatch(wrong, right, F, defect)
    assert msg is not None and "differ" in msg, msg
    # the flag-1 gradient is judged against the adjoint of the pinned sum: a slab lost or doubled inside cmvn_bwd_kernel's own
    # sum leaves the bound (a swap moves the last bit only: that is the bitwise check's to find)
    g = right.reshape(B, F, 32)[:, :, :30]
    n, worst = xb.cmvn_misses(xb.cmvn_adjoint_fp32(wrong.reshape(B, F, 32)[:, :, :30]), g)
    assert xb.cmvn_misses(xb.cmvn_adjoint_fp32(g), g)[0] == 0
    if defect != "two slabs swapped":
        assert n > 0 and worst > 10, (n, worst)


def test_slab_check_rejects_a_neighbouring_utterances_row_at_the_edge(fd):
    """tap 1, first output frame of utterance 1: its source row t - 1 lies before the utterance and enters as zeros; planted:
    the last row of utterance 0 instead (what an unguarded row index reads)"""
    from oracle.conv_chain import conv_chain
    F, F1, dact1, slabs = slab_case(fd)
    z = 2
    leak = conv_chain(np.ascontiguousarray(dact1[F1 - 1:F1, :256]), fd.wb[0][512:768], 1, 1, 1, 1, 0, 0)
    wrong = slabs[z].copy()
    assert not wrong[F].any()
    wrong[F] = leak[0]
    msg = xv_fold.bit_mismatch(wrong, slabs[z], F, "tdnn1 slab 2")
    assert msg is not None and "utterance 1 frame 0" in msg and "in 1 rows" in msg, msg


@pytest.mark.parametrize("kind", ("ce", "margin"))
def test_judgement_rejects_a_tail_without_the_plda_transform(corner_temb, kind):
    """(P A)^T folded into one matrix by the tail kernel: planted, A alone"""
    m = corner_model(28)
    y = np.arange(plda_cases.B) % 28
    loss = truth.Loss(kind, clip_max=False)
    want = xb.tail_grad(copy.deepcopy(m).double(), corner_temb, y, loss)
    yard = xb.tail_grad(m, corner_temb, y, loss, torch.float32)
    wrong = copy.deepcopy(m)
    wrong.plda_transform = torch.eye(m.plda_transform.shape[0])
    fails, line, _ = xb.judge(xb.tail_grad(wrong, corner_temb, y, loss, torch.float32), yard, want, 512)
    log("power, tail gradient S=28 %s with A for (P A): %s" % (kind, line))
    assert fails, line
