"""Every stage of the x-vector backward pinned in situ: the step's own launches, on the engine's own buffers.

tests/test_gpu_layers.py pins the forward half layer by layer; this module does the same for the backward half of
``sg_xv_loss_grad``.  One gradient call per (B, T) on CMVN-level features (flag 2) and one on raw features (flag 1); every
activation is read back through ``sg_xv_debug_activation`` and every buffer of the backward workspace through
``sg_xv_debug_gradient`` (demb, the 8 fc1 slabs, dact 1..5, the 10 tdnn1 slabs), once.  Every stage is then judged on the
engine's own upstream readback, so nothing upstream enters, over every element of every case (tests/xv_backward.py holds
the restatements; tests/test_backward_stages_power.py proves them and the judgement on the CPU).

Bitwise stages (``xv_fold.assert_same_bits``), as ``run_tdnn_backward`` (sg_api.hip) launches them -- the loader's
quad-packed transposed weights ``wbq``, the workspace strides, the launcher's choice of kernel:
  * fc1 backward: slab z of dstats_part = the fmaf chain of demb's columns [64 z, 64 z + 64) with those rows of the folded
    transposed fc1; pad columns 1500..1535 and 3036..3071 exactly +0.
  * dact l-1, l = 5, 4, 3, 2 = the chain of dact l with ``fd.wb[l-1]``, step -DIL, under the ReLU mask act l-1.
  * tdnn1's data gradient: slab z of dfeats = tap z // 2, channels [256 (z % 2), + 256) of dact 1, one chain per element, a
    source row outside the utterance entering as zeros; columns 30, 31 exactly +0.
  * the flag-2 gradient (launch_sum_cols) = the float32 sum 0.f + s0 + ... + s9 of the slab readbacks, in that order.

Float64 stages, by the rule of test_pool_and_split_k_fc1_... and the ``truth.POLICY`` constants (``xv_backward.judge``: per
utterance, utt_error <= C max(yard, FLOOR_UTT), block_error over one frame row <= C max(yard, FLOOR_BLOCK), no decided
sign wrong; the yard is the same formula in float32 torch on the CPU):
  * the tail's gradient: demb against float64 autograd of the oracle's tail from the engine's own tdnn_emb; CE and Margin on
    the standard weights at B = 5 and on the back-end corner model (tests/plda_cases.py) at S = 1, 27, 28, 64, 65.
  * statistics pooling's backward: dact 5 against relu'(act5) (dmean / Tc + dstd (act5 - mean) / ((Tc - 1) std)) with
    dmean | dstd the ordered float32 sum of the 8 slab readbacks and mean, std from the act5 readback (so pool_fwd_kernel's
    statistics are judged along); pad channels and dead channels exactly +0.
  * the CMVN adjoint, against the transposed (F, F) window matrix in float64 under ONE a-priori elementwise bound,
    |got - truth| <= 2 eps32 (|v| + |m|) (``xv_backward.cmvn_bound``): in situ the flag-1 gradient (cmvn_bwd_kernel<10>)
    against the adjoint of the ordered sum of that pass's slab readbacks, and on a flag-0 pass the dfeats_raw readback;
    stand-alone ``sg_xv_cmvn_backward`` (cmvn_bwd_kernel<0>) on seeded normal rows at F = 32, 299, 300, 301, 451, 600, 601.

The grid: 3 s at B = 1 (16 x 16 blocks; pooling backward's grid.z = 64), 2 (plain tiles), 4, 8, 16 (stream-K kinds 7, 6, 5) and
64 (kind 8, the B >= 64 pooling launch); (5, 16123) ragged; (3, 5040): F = 32, F5 = 2, the Tc - 1 = 1 edge; (2, 63680) and
(2, 63840): F = 398 / 399, the CMVN sliding branch (their tdnn5 outputs have 368 / 369 frames: both still inside the 384
frames pool_fwd_kernel holds in registers), and therefore also (2, 66240) and (2, 66400): F5 = 384 / 385, the last shape
held in registers and the first that is not.  One more case runs (2, 16000) after (8, 48000): the workspace is then larger
than the pass and the readback has to follow the pass's strides.  A forward-only call after a gradient call is refused.

Measured on an MI355X (profiles/backward_stage_pins_gpu_durations.txt, profiles/backward_stage_pins_parity.txt): 131 cases in
19.3 s; the slowest are the conv_chain restatements at 64 x 3 s -- tdnn3's data gradient 3.9 s (4.0 s inside the whole suite),
tdnn2's 2.9 s, tdnn5's 1.6 s -- every other case is under 0.5 s.  Every bitwise stage of every case: same bits, as read from
launch_conv_gemm's arguments, no slab order had to be restated.  Pooling backward: engine 1.1e-7 .. 2.9e-7 per utterance and
at most 1.8e-6 on a frame row against a float32 yard of 1e-7 / 2.4e-7 (both under the policy's floors, 6.1e-5 / 4.9e-4; at
Tc = 2 both sides 1.4e-6).  Tail gradient: engine 1.5e-7 .. 7.9e-6 against a yard of 3.8e-7 .. 7.0e-6.  CMVN adjoint: no element
outside the bound in any case, the worst at 0.47 of it (in situ, 64 x 3 s) and 0.44 (stand-alone, F = 301).
"""
import numpy as np
import pytest
import torch

import truth
import xv_backward as xb
import xv_fold
from conftest import log

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T3 = 48000
GRID = [(1, T3), (2, T3), (4, T3), (8, T3), (16, T3), (64, T3), (5, 16123), (3, 5040), (2, 63680), (2, 63840), (2, 66240), (2, 66400)]
CMVN_F = (32, 299, 300, 301, 451, 600, 601)
CE, MARGIN = truth.Loss("ce"), truth.Loss("margin", clip_max=False)


def _id(B, T):
    return "B%d_T%d" % (B, T)


@pytest.fixture(scope="module")
def hip(xv_weights):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=DEV, dither=0.0)


@pytest.fixture(scope="module")
def ora(xv_weights):
    from oracle.xv_plda import XvPlda
    return XvPlda(xv_weights)


@pytest.fixture(scope="module")
def fd(xv_weights):
    return xv_fold.fold(xv_weights["state_dict"])


def _np(t):
    return t.cpu().numpy()


def _features(ora, B, T):
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=2000 + B + T))
    with torch.no_grad():
        raw = ora.compute_feat(x, flag=1).contiguous()
        return raw, ora.cmvn(raw).contiguous()


def _run_pass(hip, ora, B, T):
    """One gradient call on CMVN-level features and one on raw features; everything read back once."""
    raw, feats = _features(ora, B, T)
    F = feats.shape[1]
    fl = xv_fold.layer_frames(F)
    assert F == xv_fold.num_frames(T)
    y = torch.arange(B) % 10
    x = feats.to(DEV)
    _, _, _, grad = hip.loss_grad(x, y, CE.spec(), flag=2)
    p = dict(B=B, T=T, F=F, fl=fl, grad2=_np(grad))
    p["acts"] = [xv_fold.pad_features(feats.numpy())]
    p["dact"] = [None]
    for l in range(1, 6):
        a, d = _np(hip.read_activation(l, B)), _np(hip.read_gradient("dact%d" % l))
        assert a.shape == d.shape == (B, fl[l - 1], xv_fold.COUT_PAD[l - 1]), (l, a.shape, d.shape)
        p["acts"].append(a.reshape(B * fl[l - 1], -1))
        p["dact"].append(d.reshape(B * fl[l - 1], -1))
    p["demb"], p["dstats"], p["dfeats"] = (_np(hip.read_gradient(k)) for k in ("demb", "dstats", "dfeats"))
    assert p["demb"].shape == (B, 512) and p["dstats"].shape == (xb.FC1_SLABS, B, xv_fold.STATS)
    assert p["dfeats"].shape == (xb.L1_SLABS, B, F, 32)
    from speakerguard_amd import _native as N
    with pytest.raises(N.NativeError):
        hip.read_gradient("dfeats_raw")  # a feature-level pass writes none
    _, _, _, grad1 = hip.loss_grad(raw.to(DEV), y, CE.spec(), flag=1)
    p["grad1"], p["dfeats1"] = _np(grad1), _np(hip.read_gradient("dfeats"))
    return p


@pytest.fixture(scope="module", params=GRID, ids=[_id(B, T) for B, T in GRID])
def p(request, hip, ora):
    """the readbacks of one (B, T): module-scoped, so that every stage of a shape runs before the next shape's pass"""
    return _run_pass(hip, ora, *request.param)


def _what(p, stage):
    return "backward stage pin, %s, B=%d T=%d" % (stage, p["B"], p["T"])


# ------------------------------------------------------------------------------------------------------ bitwise stages
def _check_fc1_slabs(p, fd):
    for z in range(xb.FC1_SLABS):
        xv_fold.assert_same_bits(p["dstats"][z], xb.fc1_bwd_slab(p["demb"], fd, z), 1, _what(p, "fc1 backward slab %d" % z))
    for lo in (xv_fold.COUT[4], xv_fold.POOL_C + xv_fold.COUT[4]):
        assert not p["dstats"][:, :, lo:lo + 36].view(np.uint32).any(), "pad columns %d.. of the fc1 slabs are not exactly +0" % lo


def _check_tdnn1_slabs(p, fd):
    B, F = p["B"], p["F"]
    for z in range(xb.L1_SLABS):
        xv_fold.assert_same_bits(p["dfeats"][z].reshape(B * F, 32), xb.tdnn1_bwd_slab(p["dact"][1], fd, B, F, z), F,
                                 _what(p, "tdnn1 data gradient slab %d (tap %d, channels %d..)" % (z, z // 2, 256 * (z % 2))))
    assert not p["dfeats"][:, :, :, xb.FEAT:].view(np.uint32).any(), "columns 30, 31 of the tdnn1 slabs are not exactly +0"


def _check_flag2_sum(p):
    B, F = p["B"], p["F"]
    want = xb.ordered_sum(p["dfeats"])[:, :, :xb.FEAT]
    xv_fold.assert_same_bits(p["grad2"].reshape(B * F, xb.FEAT), want.reshape(B * F, xb.FEAT), F, _what(p, "flag-2 gradient = ordered slab sum"))


def test_fc1_backward_slabs_are_the_restated_fmaf_chains(p, fd):
    _check_fc1_slabs(p, fd)
    log(_what(p, "fc1 backward, 8 slabs of (B, 3072)") + ": same bits")


@pytest.mark.parametrize("layer", (5, 4, 3, 2))
def test_data_gradient_in_situ_is_the_restated_fmaf_chain(p, fd, layer):
    """dact l-1 from the dact l readback: the step's own launch (wbq packing, workspace strides, the launcher's choice)"""
    mask = p["acts"][layer - 1]
    got = p["dact"][layer - 1]
    want = xb.dgrad(p["dact"][layer], fd, layer, p["B"], p["F"], mask)
    what = _what(p, "tdnn%d data gradient in situ (M=%d N=512 chunks=%d)"
                 % (layer, got.shape[0], xv_fold.TAPS[layer - 1] * xv_fold.COUT_PAD[layer - 1] // 32))
    xv_fold.assert_same_bits(got, want, p["fl"][layer - 2], what)
    assert np.abs(got).max() > 0, "an all-zero gradient pins nothing"
    log(what + ": same bits")


def test_tdnn1_data_gradient_slabs_are_the_restated_fmaf_chains(p, fd):
    _check_tdnn1_slabs(p, fd)
    assert np.abs(p["dfeats"]).max() > 0
    log(_what(p, "tdnn1 data gradient, 10 slabs of (B, F, 32)") + ": same bits")


def test_flag2_gradient_is_the_ordered_float32_sum_of_the_slabs(p):
    _check_flag2_sum(p)
    log(_what(p, "flag-2 gradient = 0.f + s0 + ... + s9") + ": same bits")


# ------------------------------------------------------------------------------------------------------ float64 stages
def test_pooling_backward_against_float64_on_the_engines_own_tdnn5(p):
    B, F5, C = p["B"], p["fl"][4], xv_fold.POOL_C
    a5 = p["acts"][5].reshape(B, F5, C)
    got = p["dact"][5].reshape(B, F5, C)
    dstats = xb.ordered_sum(p["dstats"])  # the pinned float32 sum, fed to the truth as is
    assert not got[:, :, xv_fold.COUT[4]:].view(np.uint32).any(), "pad channels of dact 5 are not exactly +0"
    dead = a5.max(1) == 0  # (B, C): channels whose every frame is zero, the zero deviations a ReLU output shows
    assert not (got.view(np.uint32) * dead[:, None, :]).any(), "a channel without deviation has a gradient"
    assert not got[a5 == 0].view(np.uint32).any(), "a frame the ReLU cut has a gradient"
    fails, lines = [], []
    for u in range(B):  # one utterance at a time: 64 x 270 x 1536 in float64 is 212 MB per temporary
        want, yard = xb.pool_bwd(a5[u:u + 1], dstats[u:u + 1]), xb.pool_bwd(a5[u:u + 1], dstats[u:u + 1], torch.float32)
        f, line, ratio = xb.judge(got[u:u + 1], yard, want, C)
        fails += [(m, u, v, b) for m, _, v, b in f]
        lines.append((ratio, u, line))
    ratio, u, line = max(lines)
    log(_what(p, "pooling backward (Tc=%d)" % F5) + ": the utterance nearest its bound, %d: %s%s"
        % (u, line, "; FAILED %s" % fails[:6] if fails else ""))
    assert not fails, fails[:8]


def _check_cmvn(got, slabs, what):
    g = xb.ordered_sum(slabs)[:, :, :xb.FEAT]  # bit-pinned (the flag-2 stage): adds no error of its own
    n, worst = xb.cmvn_misses(got, g)
    log("%s: %d of %d elements outside 2 eps32 (|v| + |m|), worst at %.2f of the bound" % (what, n, got.size, worst))
    assert np.isfinite(got).all() and n == 0, (n, worst)


def test_cmvn_adjoint_in_situ_flag1_gradient(p):
    assert p["dfeats1"].shape == p["dfeats"].shape and p["grad1"].shape == (p["B"], p["F"], xb.FEAT)
    _check_cmvn(p["grad1"], p["dfeats1"], _what(p, "CMVN adjoint in situ (flag 1, 10 slabs, F=%d, %s branch)"
                                                    % (p["F"], "register" if p["F"] <= 300 else "sliding")))


@pytest.mark.parametrize("B,T", [pytest.param(B, T, id=_id(B, T)) for B, T in ((3, 5040), (2, 63840))])
def test_cmvn_adjoint_in_situ_dfeats_raw_of_a_waveform_pass(hip, B, T):
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=2000 + B + T)).to(DEV)
    hip.loss_grad(x, torch.arange(B) % 10, CE.spec(), flag=0)
    raw, slabs = _np(hip.read_gradient("dfeats_raw")), _np(hip.read_gradient("dfeats"))
    F = xv_fold.num_frames(T)
    assert raw.shape == (B, F, xb.FEAT) and slabs.shape == (xb.L1_SLABS, B, F, 32)
    _check_cmvn(raw, slabs, "backward stage pin, CMVN adjoint in situ (flag 0, dfeats_raw), B=%d T=%d" % (B, T))


@pytest.mark.parametrize("F", CMVN_F)
def test_cmvn_adjoint_stand_alone(hip, F):
    g = np.random.RandomState(300 + F).standard_normal((3, F, xb.FEAT)).astype(np.float32)
    got = _np(hip.cmvn_backward(torch.from_numpy(g)))
    n, worst = xb.cmvn_misses(got, g)
    log("backward stage pin, CMVN adjoint stand-alone B=3 F=%d (%s branch): %d elements outside 2 eps32 (|v| + |m|), worst at "
        "%.2f of the bound" % (F, "register" if F <= 300 else "sliding", n, worst))
    assert np.isfinite(got).all() and n == 0, (n, worst)


def _tail_case(m, om, x, flag, y, loss, name):
    import copy
    temb = _np(m._forward(x, flag, want_tdnn=True)[3])
    m.loss_grad(x, torch.as_tensor(y), loss.spec(), flag=flag)
    got = _np(m.read_gradient("demb"))
    assert got.shape == temb.shape == (len(y), 512)
    want = xb.tail_grad(copy.deepcopy(om).double(), temb, y, loss)
    yard = xb.tail_grad(om, temb, y, loss, torch.float32)
    fails, line, _ = xb.judge(got, yard, want, 512)
    log("backward stage pin, tail gradient, %s %r: %s%s" % (name, loss, line, "; FAILED %s" % fails[:6] if fails else ""))
    assert np.isfinite(got).all() and not fails, fails[:8]
    return got, want


@pytest.mark.parametrize("loss", (CE, MARGIN), ids=("ce", "margin"))
def test_tail_gradient_against_float64_on_the_engines_own_tdnn_emb(hip, ora, loss):
    _, feats = _features(ora, 5, 16123)
    _tail_case(hip, ora, feats.to(DEV), 2, np.arange(5) % 10, loss, "standard weights B=5")


@pytest.fixture(scope="module")
def corner():
    import plda_cases as P
    from speakerguard_amd.model.xv_plda import xv_plda
    w = P.xv_weights()
    return w, xv_plda.from_weights(w, device=DEV, dither=0.0), torch.from_numpy(P.waveforms()).to(DEV)


@pytest.mark.parametrize("loss", (CE, MARGIN), ids=("ce", "margin"))
@pytest.mark.parametrize("S", (1, 27, 28, 64, 65))
def test_tail_gradient_at_the_back_end_corner_shapes(corner, S, loss):
    from oracle.xv_plda import XvPlda
    w, m, x = corner
    m.set_enroll(w["enroll"][:S])
    got, want = _tail_case(m, XvPlda(dict(w, enroll=w["enroll"][:S])), x, 0, np.arange(x.shape[0]) % S, loss, "corner model S=%d" % S)
    if S == 1 and loss is CE:
        assert not want.any() and not got.any(), "one class: the cross-entropy is constant"


# ------------------------------------------------------------------------------------------------------ the readback itself
def test_readback_follows_the_pass_when_the_workspace_is_larger(hip, ora, fd):
    """(2, 16000) after (8, 48000): the slabs lie at the pass's stride B F 32 / B 3072, not at the workspace's capacity"""
    _, big = _features(ora, 8, T3)
    hip.loss_grad(big.to(DEV), torch.arange(8) % 10, CE.spec(), flag=2)
    q = _run_pass(hip, ora, 2, 16000)
    _check_fc1_slabs(q, fd)
    _check_tdnn1_slabs(q, fd)
    _check_flag2_sum(q)
    for layer in (5, 2):
        xv_fold.assert_same_bits(q["dact"][layer - 1], xb.dgrad(q["dact"][layer], fd, layer, 2, q["F"], q["acts"][layer - 1]),
                                 q["fl"][layer - 2], _what(q, "tdnn%d data gradient after a larger pass" % layer))
    log(_what(q, "after (8, 48000): fc1 slabs, tdnn1 slabs, flag-2 sum, dact 4 and dact 1") + ": same bits")


def test_readback_is_refused_after_a_forward_only_call(hip, ora):
    from speakerguard_amd import _native as N
    _, feats = _features(ora, 2, 16000)
    x, y = feats.to(DEV), torch.arange(2)
    hip.loss_grad(x, y, CE.spec(), flag=2)
    assert hip.read_gradient("demb").shape == (2, 512)
    hip.make_decision(x, flag=2)
    for what in ("demb", "dact5", "dfeats"):
        with pytest.raises(N.NativeError):
            hip.read_gradient(what)
    hip.loss_grad(x, y, CE.spec(), flag=2)
    assert hip.read_gradient("dact3").shape[0] == 2
    hip.loss_grad(x, y, CE.spec(), flag=2, want_grad=False)
    with pytest.raises(N.NativeError):
        hip.read_gradient("demb")
