"""The tools of tests/test_gpu_an_stages.py, proved on the CPU before the engine is judged by them.

(a) The restatements chained -- the loader's fold (tests/an_fold.py), oracle/conv_chain.c per layer, the pre-filter chain, the
    pooling and head rules (tests/an_stages.py) -- ARE AudioNet: every layer within the float32 oracle's own distance of the
    float64 oracle (truth.POLICY), the gradient equal to float64 autograd to round-off, the pooling-backward and head rules
    equal to torch autograd of ``F.max_pool1d`` / ``x.max(2)`` on inputs with positive ties, zero ties and an odd length.
(b) The comparison has teeth: ``an_stages.simulate`` plays the engine with ONE operation replaced by a planted defect, and
    ``an_stages.mismatches`` -- the comparison the GPU test runs on the engine's readbacks, bit equality over every element --
    must name the stage that has it, on at least one case of the grid.
(c) The cases test something without the engine: ReLU masks 5 % .. 95 % active, non-zero gradients, positive tied pairs in
    the constant-in-time case; and the docstring's path table is what ``conv_plan`` picks, all four tile paths both ways.
"""
import copy
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import an_fold
import an_stages
import truth
from conftest import ROOT, log
from oracle.conv_chain import conv_chain, prefilter_chain

SMALL = ((3, 101), (5, 126), (2, 25), (2, 24))  # the grid's cases a planted defect is hunted on (plus the tied case)


@pytest.fixture(scope="module")
def sd():
    from speakerguard_amd import synth
    return synth.make_audionet_state_dict(seed=0, num_class=251)


@pytest.fixture(scope="module")
def fd(sd):
    return an_fold.fold(sd)


@pytest.fixture(scope="module")
def ora(sd):
    from oracle.audionet import AudioNet
    return AudioNet(sd)


_SIM = {}


def sim(fd, B, Fr, ties=False):
    """the restated pass of a case, computed once and left unchanged"""
    if (B, Fr, ties) not in _SIM:
        _SIM[(B, Fr, ties)] = an_stages.simulate(fd, an_stages.case_feats(B, Fr, ties))
    return _SIM[(B, Fr, ties)]


# ------------------------------------------------------------------------------------------ (a) the restatements are AudioNet
def test_layout_of_the_fold_and_the_frame_bookkeeping(sd, fd):
    for l in range(an_fold.CONVS):
        f = fd.wf[l].reshape(3, an_fold.CIN[l], an_fold.COUT[l])
        b = fd.wb[l].reshape(3, an_fold.COUT[l], an_fold.CIN[l])
        assert np.array_equal(f.view(np.uint32), b.transpose(0, 2, 1).view(np.uint32))
        assert fd.bias[l].shape == (an_fold.COUT[l],) and fd.bias[l].dtype == np.float32
    assert fd.w25.shape == (25,) and fd.w25.dtype == np.float32 and isinstance(fd.pre_bias, np.float32)
    assert an_fold.layer_frames(300) == ([300, 150, 150, 150, 75, 75, 37], [300, 150, 150, 150, 75, 75, 35])
    assert an_fold.layer_frames(126)[1] == [126, 63, 63, 63, 31, 31, 13] and an_fold.layer_frames(25)[0] == [25, 12, 12, 12, 6, 6, 3]
    assert an_fold.layer_frames(24)[1][-1] == 1 and an_fold.layer_frames(23) is None and an_fold.layer_frames(1) is None


@pytest.mark.parametrize("B,Fr", SMALL + (an_stages.TIES,))
def test_chained_restatements_are_the_float64_model(fd, ora, B, Fr):
    """Per layer and utterance: max |chain - fp64| <= C x (the fp32 oracle's largest error on that layer in the batch) +
    FLOOR_SCORE x max |fp64| of that utterance -- truth.POLICY's rule for a model output -- and d loss / d log-mel of the
    restated backward within FLOOR_UTT (relative L2 per utterance) of float64 autograd of cross-entropy on the same labels."""
    feats = torch.from_numpy(an_stages.case_feats(B, Fr).copy())
    rb = sim(fd, B, Fr)
    m64 = copy.deepcopy(ora).double()
    with torch.no_grad():
        o32 = ora.layers(feats)
    fin = feats.double().clone().requires_grad_(True)
    o64 = m64.layers(fin)
    got = [rb["pre"]] + [rb["pool"][l] if an_fold.POOL[l] else rb["act"][l] for l in range(an_fold.CONVS)]
    P = truth.POLICY
    for i, (g, w64, w32) in enumerate(zip(got, o64, o32), 1):
        w = w64.detach().numpy().transpose(0, 2, 1)
        assert g.shape == w.shape, (i, g.shape, w.shape)
        yard = np.abs(w32.numpy().transpose(0, 2, 1) - w).max()
        err = np.abs(g - w).reshape(B, -1).max(1)
        bound = P["C"] * yard + P["FLOOR_SCORE"] * np.abs(w).reshape(B, -1).max(1)
        log("AudioNet fold check layer %d (%d x %d frames): restated chain vs fp64 %.3e, fp32 oracle %.3e, worst error over its bound %.2f"
            % (i, B, Fr, err.max(), yard, (err / bound).max()))
        assert (err <= bound).all(), (i, err, bound)
    loss = F.cross_entropy(F.linear(o64[-1].max(2)[0], m64.p["fc.weight"], m64.p["fc.bias"]), torch.from_numpy(rb["y"]), reduction="none")
    loss.backward(torch.ones_like(loss))
    g64 = fin.grad.numpy().reshape(B, -1)
    rel = np.linalg.norm(rb["grad"].reshape(B, -1) - g64, axis=1) / np.linalg.norm(g64, axis=1)
    log("AudioNet fold check backward (%d x %d frames): restated chain vs fp64 autograd, relative L2 per utterance <= %.3e" % (B, Fr, rel.max()))
    assert (rel <= P["FLOOR_UTT"]).all(), rel
    assert an_stages.mismatches(rb, fd) == []  # the comparison accepts the pass it was derived from


def _tie_inputs(T):
    """(2, T, 6) ReLU-like activations: pairs with a positive tie, a zero tie, first larger, second larger, and noise"""
    rng = np.random.RandomState(T)
    a = np.maximum(rng.standard_normal((2, T, 6)), 0).astype(np.float32)
    a[:, 0:2, 0] = 1.5            # a positive tie
    a[:, 0:2, 1] = 0.0            # a zero tie
    a[:, 2:4, 0] = (2.0, 1.0)
    a[:, 2:4, 1] = (1.0, 2.0)
    a[0, :, 2] = 0.75             # a whole channel tied at a positive value: the head's maximum ties over every frame
    a[1, :, 2] = 0.0              # and at zero
    return a


@pytest.mark.parametrize("T", [8, 9, 2, 3])
def test_pooling_backward_rule_is_torch_autograd(T):
    a = _tie_inputs(max(T, 4))[:, :T]
    x = torch.from_numpy(a.transpose(0, 2, 1).copy()).requires_grad_(True)  # (B, C, T) pre-activations == activations where > 0
    y = F.max_pool1d(F.relu(x), 2, stride=2)
    d = torch.from_numpy(np.random.RandomState(1).standard_normal(tuple(y.shape)).astype(np.float32))
    y.backward(d)
    want = x.grad.numpy().transpose(0, 2, 1)
    assert np.array_equal(an_stages.pool_fwd(a), y.detach().numpy().transpose(0, 2, 1))
    got = an_stages.pool_bwd(a, np.ascontiguousarray(d.numpy().transpose(0, 2, 1)))
    assert np.array_equal(got, want)
    if T % 2:
        assert not got[:, -1].view(np.uint32).any(), "the dropped odd last frame gets +0"


@pytest.mark.parametrize("T", [9, 1])
def test_head_rule_is_torch_autograd(T):
    a = _tie_inputs(max(T, 4))[:, :T]
    x = torch.from_numpy(a.transpose(0, 2, 1).copy()).requires_grad_(True)
    emb = F.relu(x).max(2)[0]
    d = torch.from_numpy(np.random.RandomState(2).standard_normal(tuple(emb.shape)).astype(np.float32))
    emb.backward(d)
    want = x.grad.numpy().transpose(0, 2, 1)
    got = an_stages.head_dact(a, d.numpy())
    assert np.array_equal(got, want)
    assert np.array_equal(got != 0, an_stages.head_mask(a))


def test_prefilter_chain_is_the_reference_convolution_and_its_adjoint(fd, sd):
    """the C chain against conv2d in float64 (forward, with the folded weights) and the transposed form against the adjoint
    identity <P x, d> == <x, P^T d> in float64"""
    rng = np.random.RandomState(3)
    x = rng.standard_normal((2, 11, 32)).astype(np.float32)
    d = rng.standard_normal((2, 11, 32)).astype(np.float32)
    y = prefilter_chain(x, fd.w25, fd.pre_bias, False)
    w = torch.from_numpy(fd.w25.astype(np.float64).reshape(1, 1, 5, 5))
    want = F.conv2d(torch.from_numpy(x.astype(np.float64)).transpose(1, 2).unsqueeze(1), w, padding=2).squeeze(1).transpose(1, 2).numpy()
    assert np.abs(y - (want + float(fd.pre_bias))).max() < 25 * truth.EPS32 * np.abs(want).max()
    lin = prefilter_chain(x, fd.w25, 0.0, False).astype(np.float64)
    adj = prefilter_chain(d, fd.w25, 123.0, True).astype(np.float64)  # (the bias is ignored, as the kernel ignores it)
    assert abs((lin * d).sum() - (x * adj).sum()) < 1e-4 * np.abs(lin * d).sum()


# ------------------------------------------------------------------------------------------------ (b) planted defects
def _neighbour(step):
    """a tap row outside its utterance read from the neighbouring utterance (the batch as one long utterance) on the launches
    with this tap step; conv8 (no padding, Ta != Tc) has no such row"""
    def conv(a, w, B, Ta, Tc, taps, tap_step, tap_base=0, bias=None, mask=None):
        if tap_step == step and Ta == Tc:
            return conv_chain(a, w, 1, B * Ta, B * Tc, taps, tap_step, tap_base, bias=bias, mask=mask)
        return conv_chain(a, w, B, Ta, Tc, taps, tap_step, tap_base, bias=bias, mask=mask)
    return conv


def _pool_bwd(tie_second=False, no_mask=False, odd_pooled=False):
    def pool_bwd(act, dpool):
        T2 = act.shape[1] // 2
        a0, a1 = act[:, 0:2 * T2:2], act[:, 1:2 * T2:2]
        first = (a0 > a1) if tie_second else ~(a1 > a0)
        p0, p1 = (True, True) if no_mask else (a0 > 0, a1 > 0)
        out = np.zeros_like(act)
        out[:, 0:2 * T2:2] = np.where(first & p0, dpool, np.float32(0))
        out[:, 1:2 * T2:2] = np.where(~first & p1, dpool, np.float32(0))
        if odd_pooled and act.shape[1] % 2:  # the odd last frame joins the last pair
            last = act[:, -1]
            wins = (last > np.maximum(a0[:, -1], a1[:, -1])) & (last > 0)
            out[:, -1] = np.where(wins, dpool[:, -1], np.float32(0))
            out[:, -3:-1] = np.where(wins[:, None, :], np.float32(0), out[:, -3:-1])
        return out
    return pool_bwd


def _pool_fwd_odd(act):
    out = an_stages.pool_fwd(act)
    if act.shape[1] % 2:
        out[:, -1] = np.maximum(out[:, -1], act[:, -1])
    return out


def _head_last(act8):
    B, T8, C = act8.shape
    at = T8 - 1 - act8[:, ::-1].argmax(1)
    m = np.zeros(act8.shape, bool)
    b, c = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    m[b, at, c] = act8.max(1) > 0
    return m


def _head_no_mask(act8):
    m = np.zeros(act8.shape, bool)
    b, c = np.meshgrid(np.arange(act8.shape[0]), np.arange(act8.shape[2]), indexing="ij")
    m[b, act8.argmax(1), c] = True
    return m


def _ops(**kw):
    return SimpleNamespace(**dict(vars(an_stages.OPS), **kw))


def _prefilter(fwd_defect=0, unflipped=False):
    def prefilter(x, w25, bias=0.0, transpose=False):
        if transpose and unflipped:
            return prefilter_chain(x, w25, 0.0, False)
        return prefilter_chain(x, w25, bias, transpose, defect=fwd_defect)
    return prefilter


# defect -> (the operations of the engine double, the stage of stage_checks that must name it)
DEFECTS = {
    "edge tap row read from the neighbouring utterance, forward": (_ops(conv=_neighbour(1)), r"conv\d forward"),
    "edge tap row read from the neighbouring utterance, backward": (_ops(conv=_neighbour(-1)), r"conv\d data gradient"),
    "pooled tie goes to the second element": (_ops(pool_bwd=_pool_bwd(tie_second=True)), "pool backward"),
    "> 0 mask dropped in the pooling backward": (_ops(pool_bwd=_pool_bwd(no_mask=True)), "pool backward"),
    "> 0 mask dropped in the head": (_ops(head_mask=_head_no_mask), "head rule"),
    "odd last frame pooled instead of dropped, forward": (_ops(pool_fwd=_pool_fwd_odd), "pool after"),
    "odd last frame pooled instead of dropped, backward": (_ops(pool_bwd=_pool_bwd(odd_pooled=True)), "pool backward"),
    "pre-filter's mel edge clamped instead of zero-padded": (_ops(prefilter=_prefilter(fwd_defect=1)), "pre-filter"),
    "transposed pre-filter un-flipped": (_ops(prefilter=_prefilter(unflipped=True)), "pre-filter transposed"),
    "head's gradient at the last maximal frame": (_ops(head_mask=_head_last), "head rule"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_is_named_by_the_stage_comparison(fd, defect):
    ops, stage = DEFECTS[defect]
    caught = {}
    for B, Fr, ties in [(B, Fr, False) for B, Fr in SMALL] + [an_stages.TIES + (True,)]:
        bad = an_stages.mismatches(an_stages.simulate(fd, an_stages.case_feats(B, Fr, ties), ops=ops), fd)
        assert all(re.search(stage, n) for n in bad), (defect, (B, Fr, ties), bad)  # each stage stands on its own upstream readback
        if bad:
            caught[(B, Fr, "tied" if ties else "")] = bad
    log("planted defect '%s': caught on %s" % (defect, sorted(caught)))
    assert caught, "no case of the grid sees: " + defect


def test_a_weight_of_wb_taken_from_wfs_layout_is_caught(fd):
    """one entry of conv4's transposed weights replaced by the entry at the same offset of the forward layout"""
    wb = [w.copy() for w in fd.wb]
    wb[2].reshape(-1)[12345] = fd.wf[2].reshape(-1)[12345]
    assert wb[2].reshape(-1)[12345] != fd.wb[2].reshape(-1)[12345]
    for B, Fr in SMALL:
        bad = an_stages.mismatches(an_stages.simulate(fd, an_stages.case_feats(B, Fr), wb=wb), fd)
        assert bad == ["conv4 data gradient"], (B, Fr, bad)


def test_one_ulp_and_a_sign_of_zero_are_caught(fd):
    rb = dict(sim(fd, 2, 24))
    rb["dpre"] = rb["dpre"].copy()
    i = np.flatnonzero(rb["dpre"].reshape(-1) != 0)[0]
    rb["dpre"].reshape(-1)[i] = np.nextafter(rb["dpre"].reshape(-1)[i], np.float32(np.inf))
    assert set(an_stages.mismatches(rb, fd)) == {"conv2 data gradient", "pre-filter transposed"}
    rb = dict(sim(fd, 2, 24))
    rb["dact"] = list(rb["dact"])
    rb["dact"][0] = rb["dact"][0].copy()
    z = np.flatnonzero(rb["dact"][0].reshape(-1) == 0)[0]
    rb["dact"][0].reshape(-1)[z] = -0.0
    assert "pool backward below conv3" in an_stages.mismatches(rb, fd)


# -------------------------------------------------------------------------------------- (c) the cases, without the engine
@pytest.mark.parametrize("B,Fr", an_stages.GRID + (an_stages.TIES,))
def test_every_case_has_live_masks_and_gradients(fd, B, Fr):
    ties = (B, Fr) == an_stages.TIES
    rb = sim(fd, B, Fr, ties)
    failed = [d for d, ok in an_stages.conditions(rb) if not ok]
    assert failed == []
    assert (rb["scores"].argmax(1) != rb["y"]).all()
    if ties:
        for l in an_stages.POOLED:
            n = an_stages.positive_tied_pairs(rb["act"][l])
            log("constant-in-time case: positive tied pairs of conv%d per utterance %s" % (l + 2, n.tolist()))
            assert (n >= 1).all()
        assert (an_stages.tied_head_maxima(rb["act"][6]) >= 1).all(), "the head's maximum ties at a positive value"


def test_the_docstrings_path_table_is_what_conv_plan_picks():
    """the table in tests/test_gpu_an_stages.py against ``an_stages.conv_path``; that restatement against the launch table
    recorded from conv_plan itself at 3 x 16000 samples (100 frames); every tile path in both directions"""
    import test_gpu_an_stages as gpu
    doc = gpu.__doc__
    seen = set()
    for B, Fr in an_stages.GRID + (an_stages.TIES,):
        rows = an_stages.path_table(B, Fr)
        for d in ("fwd", "bwd"):
            line = "(%d, %d) %s: %s" % (B, Fr, d, " ".join(r[5] for r in rows if r[0] == d))
            assert line in doc, line
        seen |= {(r[0], r[5]) for r in rows}
    assert seen == {(d, p) for d in ("fwd", "bwd") for p in ("S16", "QUAD32", "QUAD64", "TILE_128x32")}
    rec = [l for l in open(os.path.join(ROOT, "tests", "native", "conv_launch_table.expected")) if l.startswith("audionet per layer B=3 T=16000 #")]
    assert len(rec) == 14
    kernel = {"S16": "conv_gemm_s16_kernel<", "TILE_128x32": "conv_gemm_kernel<128,32,4,1,"}
    for line, row in zip(rec, an_stages.path_table(3, 100)):
        assert kernel[row[5]] in line, (row, line)
    # the branch points themselves (conv_plan: 16 x 16 blocks up to 2800, QUAD32 from 8 chunks below 256 64-row tiles)
    assert an_stages.conv_path(5600, 128, 6) == "S16" and an_stages.conv_path(5601, 128, 6) == "QUAD64"
    assert an_stages.conv_path(16320, 128, 12) == "QUAD32" and an_stages.conv_path(16321, 128, 12) == "QUAD64"
    assert an_stages.conv_path(64, 128, 3) == "QUAD64" and an_stages.conv_path(10 ** 6, 64, 12) == "TILE_128x32"
