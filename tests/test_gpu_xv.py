"""GPU parity tests: the HIP path (through the C-ABI) against the oracle and the golden fixtures.

Run with ``pytest -m gpu`` on an MI355X.  Numbers measured by each test are appended to
``gpurun_out/parity_log.txt`` so one run documents the achieved tolerances.

Tolerance policy (north_star: "within a stated fp32 tolerance on the perturbation, bit-exact on
predicted speaker IDs and success flags"):
  * every arithmetic stage is fp32 on both sides but reduces in a different order, so stage
    outputs are compared with explicit rtol/atol written at each assert;
  * decisions and success flags must be EQUAL;
  * PGD perturbations: sign() turns round-off on near-zero gradient entries into +-step flips
    (SURVEY.md H3), so x_adv is compared as (fraction of samples that differ) and
    (max |diff| <= 2 * epsilon), both asserted.
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _vote(decisions):
    """attack/utils.py:118-125 resolve_prediction for one utterance: Counter.most_common(1), first seen wins a tie."""
    from collections import Counter
    return Counter(decisions).most_common(1)[0][0]

LOG = os.path.join(ROOT, "gpurun_out", "parity_log.txt")


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")
    print(msg)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip_model(xv_weights, dev):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=dev, dither=0.0)


@pytest.fixture(scope="module")
def oracle_model(xv_weights):
    from oracle.xv_plda import XvPlda
    return XvPlda(xv_weights, faithful=False)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------ front-end
@pytest.mark.parametrize("T", [48000, 52960, 16123])
def test_mfcc_matches_oracle(hip_model, dev, T):
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(3, T, seed=5))
    got = hip_model.compute_feat(x.to(dev), flag=1).cpu()
    want = kaldi_mfcc.mfcc_batch(x * 32768.0)
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    log("mfcc T=%d: max abs err %.3e (values up to %.1f)" % (T, err, want.abs().max().item()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=5e-3)


@pytest.mark.parametrize("tag", ["t48000", "t16123"])
def test_mfcc_matches_independent_implementation(hip_model, dev, tag):
    """HIP MFCC vs vectors from an INDEPENDENT implementation of torchaudio's Kaldi front-end (transformers.audio_utils
    + scipy DCT, tests/golden/frontend_xcheck.npz) -- the reference's own torchaudio==0.6.0 is not installable."""
    import hashlib
    from speakerguard_amd import synth
    g = load_golden("frontend_xcheck.npz")
    T, seed = (int(v) for v in g[tag + "_gen"])
    x = synth.make_waveforms(1, T, seed=seed)
    assert hashlib.sha256((x[0, 0] * 32768.0).astype(np.float32).tobytes()).hexdigest() == str(g[tag + "_x_sha256"])
    got = hip_model.compute_feat(torch.from_numpy(x).to(dev), flag=1).cpu().numpy()[0]
    want = g[tag + "_mfcc"]
    err = np.abs(got - want).max()
    log("mfcc vs independent implementation (%s): max abs err %.3e (values up to %.1f)" % (tag, err, np.abs(want).max()))
    assert got.shape == want.shape and err < 1e-3   # fp32 table rounding alone: 3e-4 (trap 1)


def test_float32_transforms_against_the_float64_counterpart(xv_weights, oracle_model, dev):
    """Round 6: the MFCC's 512-point transforms run in float32 by default -- the reference's own precision (torchaudio 0.6's
    kaldi.mfcc is float32 end to end, xv_plda.py:114-148) -- with the float64 form of rounds 1-5 behind sg_xv_configure.
    Both forms against each other and against the oracle: cepstra, decisions, d loss / d wav (the sign-mismatch statistic
    next to the float64 one)."""
    from oracle import attacks as oatk
    from oracle import kaldi_mfcc
    from speakerguard_amd import _native as N
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.model.xv_plda import xv_plda
    m = xv_plda.from_weights(xv_weights, device=dev, dither=0.0)
    with pytest.raises(N.NativeError, match="fft_bits"):
        m.configure_frontend(48)
    x = torch.from_numpy(synth.make_waveforms(3, 48000, seed=22))
    want = kaldi_mfcc.mfcc_batch(x * 32768.0)
    with torch.no_grad():
        y = oracle_model.make_decision(x)[0]
    xin = x.clone().requires_grad_(True)
    oatk.cross_entropy_loss(oracle_model.make_decision(xin)[1], y).backward(torch.ones(3))
    g_ref = xin.grad.numpy()
    got = {}
    for bits in (32, 64):
        m.configure_frontend(bits)
        feats = m.compute_feat(x.to(dev), flag=1).cpu()
        dec, scores, loss, grad = m.loss_grad(x.to(dev), y.to(dev), SEC4SR_CrossEntropy())
        g = grad.cpu().numpy()
        got[bits] = (feats, dec.cpu(), g)
        np.testing.assert_allclose(feats.numpy(), want.numpy(), rtol=1e-4, atol=5e-3)
        assert dec.cpu().tolist() == y.tolist()
        mism = float((np.sign(g) != np.sign(g_ref)).mean())
        err = np.abs(g - g_ref).max() / np.abs(g_ref).max()
        log("xv front-end with float%d transforms: cepstra max abs err vs oracle %.3e; d loss / d wav max err / max %.3e, sign mismatch %.3e"
            % (bits, (feats - want).abs().max().item(), err, mism))
        assert err < 3e-3 and mism < 5e-3
    m.configure_frontend(32)
    assert (got[32][0] - got[64][0]).abs().max().item() < 2e-4  # cepstra up to 33: float32 round-off of the spectrum
    assert float((np.sign(got[32][2]) != np.sign(got[64][2])).mean()) < 2e-3


def test_mfcc_int16_range_left_alone(hip_model, dev):
    """check_input_range: a batch already in int16 scale is NOT multiplied again (model/utils.py:11)."""
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=6)) * 32768.0
    got = hip_model.compute_feat(x.to(dev), flag=1).cpu()
    np.testing.assert_allclose(got.numpy(), kaldi_mfcc.mfcc_batch(x).numpy(), rtol=1e-4, atol=5e-3)


def test_mfcc_explicit_dither_noise(hip_model, dev):
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=7))
    F = kaldi_mfcc.num_frames(16000)
    g = torch.Generator().manual_seed(1)
    noise = kaldi_mfcc.dither_noise_from_uniform(torch.rand(2, F, 400, generator=g))
    got = hip_model.compute_feat(x.to(dev), flag=1, dither_noise=noise.to(dev).contiguous()).cpu()
    want = kaldi_mfcc.mfcc_batch(x * 32768.0, noise)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=5e-3)


def test_internal_dither_is_reproducible_and_changes_features(xv_weights, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=8)).to(dev) * 1e-3  # quiet: dither matters
    a = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=3)
    b = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=3)
    c = xv_plda.from_weights(xv_weights, device=dev, dither=0.0)
    fa, fb, fc = a.compute_feat(x), b.compute_feat(x), c.compute_feat(x)
    assert torch.equal(fa, fb)
    assert not torch.equal(fa, a.compute_feat(x)), "a second forward must draw fresh noise"
    assert (fa - fc).abs().max().item() > 1e-3


def test_device_noise_streams_match_the_philox_restatement(xv_weights, hip_model, dev):
    """SURVEY 8(a) rows A2 / A16 are "fp32 + RNG".  The reference's draws come from torch's process-global generator
    and cannot be reproduced by anyone; the engine's streams are a function of (seed, global utterance, frame /
    pair, sample) only, and oracle/philox.py -- Philox4x32-10, checked against the Random123 known-answer vectors on
    the CPU -- restates them.  NES normals: compared directly.  Dither: the features computed with the kernel's own
    draws equal the features computed from the restated noise handed in as an explicit tensor."""
    from oracle import kaldi_mfcc, philox
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=8)).to(dev)
    T, half, base = 16000, 3, (1 << 33) + 5  # a global example index beyond 32 bits exercises the high counter word
    _, z = hip_model.nes_queries(x, half, True, 0.001, 11, 4, None, want_noise=True, index_base=base)
    worst = 0.0
    for e in range(2):
        for p in range(half):
            want = philox.nes_normal(11, base + e, 4 + p, T)
            worst = max(worst, float(np.abs(z[e, p, 0].cpu().numpy() - want).max()))
    assert worst < 5e-6, worst  # same 24-bit uniforms; logf / cosf / sqrtf of two libms
    md = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=3)
    quiet = x * 1e-3  # quiet input: the dither moves the features visibly
    md.begin_batch(index_base=6)
    seed = md.noise_seed(md.dither_seed, 0)
    own = md.compute_feat(quiet, flag=1)
    F = kaldi_mfcc.num_frames(T)
    noise = torch.from_numpy(np.stack([philox.dither_noise(seed, 6 + b, F) for b in range(2)])).to(dev)  # chunk base + row
    fed = md.compute_feat(quiet, flag=1, dither_noise=noise.contiguous())
    silent = xv_plda.from_weights(xv_weights, device=dev, dither=0.0).compute_feat(quiet, flag=1)
    err = float((own - fed).abs().max())
    assert err < 2e-4 and float((own - silent).abs().max()) > 1e-2, err
    md._row_base = 4  # rows keyed as rows 4, 5 of a larger call (shard.QueryShardedModel)
    md._draw = 0
    own4 = md.compute_feat(quiet, flag=1)
    md._row_base = 0
    noise4 = torch.from_numpy(np.stack([philox.dither_noise(seed, 6 + 4 + b, F) for b in range(2)])).to(dev)
    err4 = float((own4 - md.compute_feat(quiet, flag=1, dither_noise=noise4.contiguous())).abs().max())
    assert err4 < 2e-4 and not torch.equal(own4, own)
    log("device noise vs Philox restatement: NES normals max |diff| %.2e; MFCC with own dither vs restated noise fed in %.2e"
        % (worst, max(err, err4)))


@pytest.mark.parametrize("tag", ["f300", "f331"])
def test_cmvn_matches_reference_fixture(hip_model, dev, tag):
    g = load_golden("xv_%s.npz" % tag)
    got = hip_model.cmvn(torch.from_numpy(g["feats"]).to(dev)).cpu().numpy()
    log("cmvn %s: max abs err vs reference %.3e" % (tag, np.abs(got - g["cmvn"]).max()))
    np.testing.assert_allclose(got, g["cmvn"], rtol=0, atol=2e-5)


# ------------------------------------------------------------------------------ from features: reference-pinned
@pytest.mark.parametrize("tag", ["f300", "f331"])
def test_forward_from_features_matches_reference_fixture(hip_model, dev, tag):
    g = load_golden("xv_%s.npz" % tag)
    feats = torch.from_numpy(g["feats"]).to(dev)
    B = feats.shape[0]
    dec, scores, emb, temb = hip_model._forward(feats, 1, want_emb=True, want_tdnn=True)
    for layer in range(1, 6):
        act = hip_model.read_activation(layer, B).cpu().numpy()  # (B, F_l, Cpad)
        C = g["relu%d_sub" % layer].shape[0]
        a = act[B - 1].T  # (Cpad, F_l) like the reference's (C, F)
        sub = a[::37, ::11][:C]
        ref = g["relu%d_sub" % layer]
        ctrue = 1500 if layer == 5 else 512
        ref_full_idx = np.arange(0, ctrue, 37)
        sub = a[ref_full_idx][:, ::11]
        log("relu%d %s: max abs err %.3e (max %.3f)" % (layer, tag, np.abs(sub - ref).max(), np.abs(ref).max()))
        np.testing.assert_allclose(sub, ref, rtol=2e-4, atol=2e-5)
        tot, tot_abs = g["relu%d_sum" % layer]
        assert abs(a[:ctrue].astype(np.float64).sum() - tot) <= 2e-5 * tot_abs
        if layer == 5:
            assert np.all(a[1500:] == 0), "padded channels must stay zero"
    np.testing.assert_allclose(temb.cpu().numpy(), g["tdnn_emb"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(emb.cpu().numpy(), g["emb"], rtol=1e-3, atol=3e-3)
    log("scores %s: max abs err %.3e" % (tag, np.abs(scores.cpu().numpy() - g["scores"]).max()))
    np.testing.assert_allclose(scores.cpu().numpy(), g["scores"], rtol=1e-3, atol=5e-2)
    assert dec.cpu().tolist() == g["decisions"].tolist()


@pytest.mark.parametrize("tag", ["f300", "f331"])
def test_loss_and_gradient_from_features_match_reference_fixture(hip_model, dev, tag):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    g = load_golden("xv_%s.npz" % tag)
    feats = torch.from_numpy(g["feats"]).to(dev)
    y = torch.from_numpy(g["y"]).to(dev)
    for name, spec, key in (("ce", SEC4SR_CrossEntropy(), "grad_ce"),
                            ("margin", SEC4SR_MarginLoss(False, 0., "CSI", None, False), "grad_margin")):
        dec, scores, loss, grad = hip_model.loss_grad(feats, y, spec, flag=1)
        np.testing.assert_allclose(loss.cpu().numpy(), g[name], rtol=1e-3, atol=5e-2)
        gs = np.abs(g[key]).max()
        err = np.abs(grad.cpu().numpy() - g[key]).max() / gs
        log("grad %s %s: max err / max|grad| = %.3e" % (name, tag, err))
        np.testing.assert_allclose(grad.cpu().numpy(), g[key], rtol=0, atol=2e-3 * gs)
        assert dec.cpu().tolist() == g["decisions"].tolist()


def test_cmvn_level_gradient_matches_oracle(hip_model, oracle_model, dev):
    from oracle import attacks as oatk
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    g = load_golden("xv_f300.npz")
    cm = torch.from_numpy(g["cmvn"])
    y = torch.from_numpy(g["y"])
    xin = cm.clone().requires_grad_(True)
    _, sc = oracle_model.make_decision(xin, flag=2)
    oatk.cross_entropy_loss(sc, y).backward(torch.ones(2))
    _, _, _, grad = hip_model.loss_grad(cm.to(dev), y.to(dev), SEC4SR_CrossEntropy(), flag=2)
    gs = xin.grad.abs().max().item()
    np.testing.assert_allclose(grad.cpu().numpy(), xin.grad.numpy(), rtol=0, atol=2e-3 * gs)


def test_threshold_decisions_and_margin_variants(xv_weights, dev):
    from speakerguard_amd.attack.utils import SEC4SR_MarginLoss
    from speakerguard_amd.model.xv_plda import xv_plda
    g = load_golden("xv_thresh.npz")
    thr = g["meta"]["threshold"]
    m = xv_plda.from_weights(xv_weights, threshold=thr, device=dev, dither=0.0)
    feats = torch.from_numpy(g["feats"]).to(dev)
    dec, scores = m.make_decision(feats, flag=1)
    assert dec.cpu().tolist() == g["decisions"].tolist()
    y = torch.from_numpy(g["y"]).to(dev)
    for task in ("CSI", "OSI"):
        for targeted in (False, True):
            for clip in (False, True):
                spec = SEC4SR_MarginLoss(targeted, 0.5, task, thr, clip)
                _, _, loss, _ = m.loss_grad(feats, y, spec, flag=1, want_grad=False)
                np.testing.assert_allclose(loss.cpu().numpy(), g["margin_%s_%d_%d" % (task, targeted, clip)],
                                           rtol=1e-3, atol=5e-2, err_msg="%s %s %s" % (task, targeted, clip))
    # SV: a single enrolled speaker
    m.set_enroll(xv_weights["enroll"][:1])
    ysv = torch.from_numpy(g["ysv"]).to(dev)
    for targeted in (False, True):
        spec = SEC4SR_MarginLoss(targeted, 0.5, "SV", thr, False)
        _, sc, loss, _ = m.loss_grad(feats, ysv, spec, flag=1, want_grad=False)
        assert sc.shape == (3, 1)
        np.testing.assert_allclose(loss.cpu().numpy(), g["margin_SV_%d" % targeted], rtol=1e-3, atol=5e-2)


def test_enroll_embs_argument_is_a_per_call_override(xv_weights, oracle_model, dev):
    """iv_plda.py:155-165: forward/score/make_decision(x, enroll_embs=e) score against e for THAT call only;
    the model's enrolled set, num_spks and every later call are unchanged (it used to stick)."""
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    m = xv_plda.from_weights(xv_weights, device=dev, dither=0.0)
    x = torch.from_numpy(synth.make_waveforms(3, 16000, seed=21)).to(dev)
    dec0, sc0 = m.make_decision(x)
    e = torch.from_numpy(xv_weights["enroll"][2:5].copy()).to(dev)       # three of the ten speakers, re-ordered set
    sc_o = m.score(x, enroll_embs=e)
    assert sc_o.shape == (3, 3)
    np.testing.assert_array_equal(sc_o.cpu().numpy(), sc0[:, 2:5].cpu().numpy())   # same rows -> same scores, bit for bit
    dec_o, _ = m.make_decision(x, enroll_embs=e)
    assert dec_o.cpu().tolist() == sc0[:, 2:5].argmax(1).cpu().tolist()
    with torch.no_grad():
        o_sc = oracle_model.score(x.cpu(), enroll_embs=e.cpu())
    np.testing.assert_allclose(sc_o.cpu().numpy(), o_sc.numpy(), rtol=2e-3, atol=0.2)
    # nothing stuck
    assert m.num_spks == 10 and m.enroll_embs.shape == (10, m.dim)
    dec1, sc1 = m.make_decision(x)
    assert dec1.cpu().tolist() == dec0.cpu().tolist()
    np.testing.assert_array_equal(sc1.cpu().numpy(), sc0.cpu().numpy())
    # set_enroll (the persistent form) re-uses / re-sizes the device table without leaking
    for _ in range(3):
        m.set_enroll(xv_weights["enroll"][:4])
        assert m.make_decision(x)[1].shape == (3, 4)
        m.set_enroll(xv_weights["enroll"])
    np.testing.assert_array_equal(m.make_decision(x)[1].cpu().numpy(), sc0.cpu().numpy())


@pytest.mark.parametrize("variant", ["osi_untargeted", "osi_targeted", "csi_targeted_margin", "sv_untargeted", "ce_targeted"])
def test_loss_gradient_variants_match_oracle_autograd(xv_weights, dev, variant):
    """d loss / d features for every loss branch the tail kernel hand-codes (attack/utils.py:41-102)."""
    from oracle import attacks as oatk
    from oracle.xv_plda import XvPlda
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    from speakerguard_amd.model.xv_plda import xv_plda
    g = load_golden("xv_thresh.npz")
    thr = g["meta"]["threshold"]
    feats = torch.from_numpy(g["feats"])
    y = torch.from_numpy(g["y"])
    w = dict(xv_weights)
    if variant.startswith("sv"):
        w["enroll"] = xv_weights["enroll"][3:4]
        y = torch.from_numpy(g["ysv"])
    spec = {"osi_untargeted": SEC4SR_MarginLoss(False, 0.5, "OSI", thr, False),
            "osi_targeted": SEC4SR_MarginLoss(True, 0.5, "OSI", thr, False),
            "csi_targeted_margin": SEC4SR_MarginLoss(True, 0.2, "CSI", None, True),
            "sv_untargeted": SEC4SR_MarginLoss(False, 0.5, "SV", thr, False),
            "ce_targeted": SEC4SR_CrossEntropy()}[variant]
    if variant == "ce_targeted":
        y = torch.tensor([1, 4, 6])
    om = XvPlda(w, threshold=thr)
    hm = xv_plda.from_weights(w, threshold=thr, device=dev, dither=0.0)
    xin = feats.clone().requires_grad_(True)
    _, sc = om.make_decision(xin, flag=1)
    if isinstance(spec, SEC4SR_CrossEntropy):
        lo = oatk.cross_entropy_loss(sc, y)
    else:
        lo = oatk.margin_loss(sc, y, spec.targeted, spec.confidence, spec.task, spec.threshold, spec.clip_max)
    lo.backward(torch.ones_like(lo))
    dec, scores, loss, grad = hm.loss_grad(feats.to(dev), y.to(dev), spec, flag=1)
    np.testing.assert_allclose(loss.cpu().numpy(), lo.detach().numpy(), rtol=1e-3, atol=5e-2)
    gs = xin.grad.abs().max().item() + 1e-30
    np.testing.assert_allclose(grad.cpu().numpy(), xin.grad.numpy(), rtol=0, atol=3e-3 * gs)


# ------------------------------------------------------------------------------ from waveforms (front-end unpinned)
def test_forward_from_waveform_matches_oracle(hip_model, oracle_model, dev):
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(4, 48000, seed=21))
    dec, scores = hip_model.make_decision(x.to(dev))
    with torch.no_grad():
        odec, oscores = oracle_model.make_decision(x)
    log("wav forward: scores max abs err %.3e" % (scores.cpu() - oscores).abs().max().item())
    np.testing.assert_allclose(scores.cpu().numpy(), oscores.numpy(), rtol=2e-3, atol=0.15)
    assert dec.cpu().tolist() == odec.tolist()


def test_waveform_gradient_matches_oracle_autograd(hip_model, oracle_model, dev):
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    x = torch.from_numpy(synth.make_waveforms(3, 48000, seed=22))
    with torch.no_grad():
        y = oracle_model.make_decision(x)[0]
    xin = x.clone().requires_grad_(True)
    _, sc = oracle_model.make_decision(xin)
    oatk.cross_entropy_loss(sc, y).backward(torch.ones(3))
    dec, scores, loss, grad = hip_model.loss_grad(x.to(dev), y.to(dev), SEC4SR_CrossEntropy())
    want = xin.grad.numpy()
    got = grad.cpu().numpy()
    gs = np.abs(want).max()
    err = np.abs(got - want).max() / gs
    sign_mismatch = float((np.sign(got) != np.sign(want)).mean())
    log("wav grad: max err / max|grad| = %.3e, sign mismatch fraction %.3e" % (err, sign_mismatch))
    # both fp32 paths against the same model evaluated in fp64: is the HIP path at least as close
    # to the exact gradient as the fp32 oracle is?
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth as _s
    m64 = XvPlda(_s.make_xv_weights()).double()
    x64 = x.double().requires_grad_(True)
    _, sc64 = m64.make_decision(x64)
    torch.nn.functional.cross_entropy(sc64, y, reduction="none").backward(torch.ones(3, dtype=torch.float64))
    g64 = x64.grad.numpy()
    for nm, arr in (("hip", got), ("oracle-fp32", want)):
        log("   %s vs fp64 truth: max err/max %.3e, rms err/rms %.3e, sign mismatch %.3e" % (
            nm, np.abs(arr - g64).max() / np.abs(g64).max(), np.sqrt(((arr - g64) ** 2).mean() / (g64 ** 2).mean()),
            float((np.sign(arr) != np.sign(g64)).mean())))
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-3 * gs)
    assert sign_mismatch < 1.5e-3  # 10x the measured 1.5e-4 (was 5e-3); the fp64 judgement: tests/test_gpu_truth.py


def test_short_and_ragged_lengths(hip_model, oracle_model, dev):
    """Shortest utterance the TDNN context allows, and a length that is not a multiple of the hop."""
    from speakerguard_amd import synth
    for T in (5200, 16123):
        x = torch.from_numpy(synth.make_waveforms(2, T, seed=23))
        dec, scores = hip_model.make_decision(x.to(dev))
        with torch.no_grad():
            odec, oscores = oracle_model.make_decision(x)
        np.testing.assert_allclose(scores.cpu().numpy(), oscores.numpy(), rtol=2e-3, atol=0.2)
        assert dec.cpu().tolist() == odec.tolist()
    from speakerguard_amd._native import NativeError
    with pytest.raises(NativeError):
        hip_model.make_decision(torch.zeros(1, 1, 2000, device=dev))  # too few frames for the 30-frame context


def test_long_utterance_sliding_cmvn_and_gradient(hip_model, oracle_model, dev):
    """12 s utterances (1200 frames): the 300-frame sliding CMVN window (iv_plda.py:296-377) is no longer the global
    mean, a tile of the contractions no longer spans a whole utterance; forward and d loss/d waveform vs the oracle."""
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    T = 192000
    x = torch.from_numpy(synth.make_waveforms(2, T, seed=29))
    xin = x.clone().requires_grad_(True)
    odec, osc = oracle_model.make_decision(xin)
    y = (odec + 1) % 10
    lo = oatk.cross_entropy_loss(osc, y)
    lo.backward(torch.ones_like(lo))
    dec, scores, loss, grad = hip_model.loss_grad(x.to(dev), y.to(dev), SEC4SR_CrossEntropy())
    assert dec.cpu().tolist() == odec.tolist()
    np.testing.assert_allclose(scores.cpu().numpy(), osc.detach().numpy(), rtol=2e-3, atol=0.2)
    np.testing.assert_allclose(loss.cpu().numpy(), lo.detach().numpy(), rtol=2e-3, atol=2e-2)
    want, got = xin.grad.numpy(), grad.cpu().numpy()
    gs = np.abs(want).max()
    err, sm = np.abs(got - want).max() / gs, float((np.sign(got) != np.sign(want)).mean())
    log("12 s utterances: score err %.3e, d loss/d wav err/max %.3e, sign mismatch %.3e" % (
        (scores.cpu() - osc.detach()).abs().max().item(), err, sm))
    # four times the frames of the 3 s case: a ReLU whose pre-activation is within round-off of 0 flips between the two
    # fp32 implementations somewhere and moves the gradient of its receptive field (same effect and policy as in
    # tests/test_gpu_feco.py): bulk tolerance + a bound on the outliers
    bad = float((np.abs(got - want) > 3e-3 * gs).mean())
    assert bad < 5e-3 and err < 2e-2 and sm < 1.6e-3, (bad, err, sm)  # sm: 10x the measured 1.6e-4 (was 5e-3)


# ------------------------------------------------------------------------------ PGD update + loops
def test_pgd_update_kernel_is_bit_exact(hip_model, dev):
    g = torch.Generator().manual_seed(0)
    n = 3 * 48000 + 5
    x = (torch.rand(n, generator=g) * 2 - 1).to(dev)
    grad = torch.randn(n, generator=g).to(dev)
    grad[::7] = 0.0
    lower = torch.clamp(x - 0.002, min=-1)
    upper = torch.clamp(x + 0.002, max=1)
    for gsn in (1, -1):
        want = torch.min(torch.max(x + 0.0004 * torch.sign(grad) * gsn, lower), upper)
        got = hip_model.pgd_update(x.clone(), grad, lower, upper, 0.0004, gsn)
        assert torch.equal(got, want)


def _stepwise_pgd(model, x, y, lower, upper, spec, step, iters, grad_sign):
    x = x.clone()
    for _ in range(iters):
        _, _, _, grad = model.loss_grad(x, y, spec)
        model.pgd_update(x, grad, lower, upper, step, grad_sign)
    dec, scores, loss, _ = model.loss_grad(x, y, spec, want_grad=False)
    return x, dec, scores, loss


def test_fused_loop_equals_stepwise_calls(hip_model, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    x = torch.from_numpy(synth.make_waveforms(4, 32000, seed=24)).to(dev)
    y = hip_model.make_decision(x)[0]
    lower, upper = torch.clamp(x - 0.002, min=-1), torch.clamp(x + 0.002, max=1)
    spec = SEC4SR_CrossEntropy()
    xa, success, dec, scores, loss, ltr, dtr = hip_model.pgd_run(x, y, lower, upper, spec, 0.0004, 4, 1, trace=True)
    xb, decb, scoresb, lossb = _stepwise_pgd(hip_model, x, y, lower, upper, spec, 0.0004, 4, 1)
    assert torch.equal(xa, xb) and torch.equal(dec, decb) and torch.equal(scores, scoresb)
    assert torch.equal(ltr[-1], loss) and torch.equal(dtr[-1], dec)
    assert success.bool().tolist() == (dec != y).tolist()


def test_fused_eot_over_dither_equals_stepwise_replay(xv_weights, dev, monkeypatch):
    """The reference's default front-end is random (dither = 1.0, xv_plda.py:119) and EOT averages its gradient over
    fresh draws (EOT.py:16-54).  The fused loop runs those repeats on the device; replaying its per-pass generator
    keys through the per-step API (loss_grad with an explicit key, gradients summed in pass order by torch, then
    sg_pgd_update) must give the same audio bit for bit, and the final single-pass decisions."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.model.xv_plda import xv_plda
    m = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=11)
    x = torch.from_numpy(synth.make_waveforms(3, 24000, seed=26)).to(dev)
    y = m.make_decision(x)[0]
    lower, upper = torch.clamp(x - 0.002, min=-1), torch.clamp(x + 0.002, max=1)
    spec = SEC4SR_CrossEntropy()
    iters, reps = 3, 4
    xa, success, dec, scores, loss, _, _ = m.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=reps, eot_batch_size=2)
    base = m.last_fused_seed
    xb = x.clone()
    grads, step_loss, step_dec = [], [], []
    for it in range(iters):
        acc, lsum, decs = None, None, []
        for r in range(reps):
            d_r, _, l_r, g = m.loss_grad(xb, y, spec, dither_seed=m.fused_pass_seed(base, it, r))
            grads.append(g)
            acc = g if acc is None else acc + g
            lsum = l_r if lsum is None else lsum + l_r
            decs.append(d_r.cpu().tolist())
        step_loss.append(torch.from_numpy(lsum.cpu().numpy() / np.float32(reps)).to(dev))  # true division, like the kernel
        step_dec.append([_vote([decs[r][b] for r in range(reps)]) for b in range(x.shape[0])])
        m.pgd_update(xb, acc.contiguous(), lower, upper, 0.0004, 1)
    d2, s2, l2, _ = m.loss_grad(xb, y, spec, want_grad=False, dither_seed=m.fused_pass_seed(base, iters, 0))
    assert torch.equal(xa, xb)
    assert torch.equal(dec, d2) and torch.equal(scores, s2) and torch.equal(loss, l2)
    assert success.bool().tolist() == (dec != y).tolist()
    # the device loop runs the 4 repeats as one batch of 12 rows; when a pass cannot hold them all they go in groups with
    # the sum handed on (here forced: 2 + 2 repeats, then 1 + 1 + 1 + 1) -- same bits.  The per-step records are what the
    # reference prints (attack/FGSM.py:50-58): the loss averaged over the step's repeats, the decision voted over them
    # (round 3; round 2 recorded the first repeat) -- with forced groups too (round 4: the passes of a step collect their
    # rows and the reduction runs over all repeats; round 3 covered the repeats of the step's first pass only).
    m._draw = 100  # same generator key for the three runs
    ref_tr = m.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=reps, eot_batch_size=2, trace=True)
    for cap in (6, 3):
        monkeypatch.setenv("SG_EOT_MAX_ROWS", str(cap))
        m._draw = 100
        got = m.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=reps, eot_batch_size=2, trace=True)
        for a, b in zip(got, ref_tr):  # adversarial audio, flags, decisions, scores, loss AND the per-step records
            assert torch.equal(a, b), cap
    monkeypatch.delenv("SG_EOT_MAX_ROWS")
    # the records of the un-grouped run against the replayed repeats (a fresh run with the first run's key)
    m2 = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=11)
    m2.make_decision(x)  # the one pass `m` had made before its fused run: same generator key
    tr = m2.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=reps, eot_batch_size=2, trace=True)
    assert m2.last_fused_seed == base and torch.equal(tr[0], xa)
    for it in range(iters):
        assert torch.equal(tr[5][it], step_loss[it]), it
        assert tr[6][it].cpu().tolist() == step_dec[it], it
    assert torch.equal(tr[5][iters], loss) and torch.equal(tr[6][iters], dec)
    # the repeats really are different draws, and EOT changes the trajectory
    assert not torch.equal(grads[0], grads[1])
    x1 = m.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=1)[0]
    assert not torch.equal(x1, xa)
    # host class: PGD(EOT_size=4) on a dithered model takes the fused path and respects the epsilon ball
    from speakerguard_amd.attack.PGD import PGD
    atk = PGD(m, epsilon=0.002, step_size=0.0004, max_iter=iters, batch_size=3, EOT_size=reps, EOT_batch_size=2, verbose=0)
    assert atk._device_route(3) == ('pgd_run', ())
    adv, succ = atk.attack(x, y)
    assert (adv - x).abs().max().item() <= 0.002 + 1e-7 and len(succ) == 3
    frac = float(((xa - x).abs() > 0).float().mean())
    log("fused EOT(%d) over dither: equals the stepwise replay bit for bit; %.1f%% of samples moved" % (reps, 100 * frac))


@pytest.mark.parametrize("loss_name,targeted", [("Entropy", False), ("Margin", False), ("Entropy", True)])
def test_pgd_attack_matches_oracle(hip_model, oracle_model, dev, loss_name, targeted):
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    B, eps, step, iters = 4, 0.002, 0.0004, 5
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=25))
    with torch.no_grad():
        y = oracle_model.make_decision(x)[0]
    if targeted:
        y = (y + 3) % 10
    oadv, osucc = oatk.PGD(oracle_model, task="CSI", epsilon=eps, step_size=step, max_iter=iters, loss=loss_name,
                           targeted=targeted, batch_size=B).attack(x.clone(), y)
    adv, succ = PGD(hip_model, task="CSI", epsilon=eps, step_size=step, max_iter=iters, loss=loss_name,
                    targeted=targeted, batch_size=B, verbose=0).attack(x.to(dev), y.to(dev))
    diff = (adv.cpu() - oadv).abs()
    frac = float((diff > 1e-7).float().mean())
    log("PGD-%d %s targeted=%s: samples differing %.4f%%, max|diff| %.2e, success hip=%s oracle=%s"
        % (iters, loss_name, targeted, 100 * frac, diff.max().item(), succ, osucc))
    # two fp32 implementations of the same PGD drift apart through sign(): the reference-vs-oracle
    # pair (both PyTorch-CPU, tests/test_oracle_golden.py) already differs in 2.3 % of the samples
    # after 5 steps; the stated tolerance is 2 % per step.
    assert frac < 0.02 * iters, "too many perturbation samples differ from the oracle"
    assert diff.max().item() <= 2 * eps + 1e-6
    assert (adv.cpu() - x).abs().max().item() <= eps + 1e-6
    assert succ == osucc
    with torch.no_grad():
        odec = oracle_model.make_decision(oadv)[0]
    assert hip_model.make_decision(adv)[0].cpu().tolist() == odec.tolist()


class _FeatAdapter:
    """(n,1,F*30) in [-1,1) -> MFCC features; same adapter that produced the fixture."""

    def __init__(self, model, F, scale):
        self.model, self.F, self.scale, self.threshold = model, F, scale, model.threshold

    def loss_grad(self, x, y, spec, flag=0, want_grad=True):
        feats = (x.view(x.shape[0], self.F, 30) * self.scale).contiguous()
        dec, sc, loss, g = self.model.loss_grad(feats, y, spec, flag=1, want_grad=want_grad)
        if g is not None:
            g = (g * self.scale).view(x.shape)
        return dec, sc, loss, g

    def make_decision(self, x):
        return self.model.make_decision((x.view(x.shape[0], self.F, 30) * self.scale).contiguous(), flag=1)

    def pgd_update(self, *a):
        return self.model.pgd_update(*a)


def test_pgd_feature_level_matches_reference_fixture(hip_model, dev):
    """Trajectories the REFERENCE PGD/CWinf produced with the reference xv_plda from flag=1."""
    from speakerguard_amd.attack.CWinf import CWinf
    from speakerguard_amd.attack.PGD import PGD
    g = load_golden("xv_pgd_featlevel.npz")
    x0 = torch.from_numpy(g["x0"]).to(dev)
    adapter = _FeatAdapter(hip_model, 300, g["meta"]["scale"])
    assert adapter.make_decision(x0)[0].cpu().tolist() == g["clean_decisions"].tolist()
    for name, cls, kw in (("pgd_ce", PGD, dict(loss="Entropy")), ("pgd_ce_t", PGD, dict(loss="Entropy", targeted=True)),
                          ("cwinf", CWinf, dict())):
        atk = cls(adapter, task="CSI", epsilon=g["meta"]["eps"], step_size=g["meta"]["step"],
                  max_iter=g["meta"]["max_iter"], batch_size=3, verbose=0, **kw)
        adv, success = atk.attack(x0.clone(), torch.from_numpy(g[name + "_y"]).to(dev))
        diff = np.abs(adv.cpu().numpy() - g[name + "_adv"])
        log("feature-level %s vs reference: samples differing %.3f%%" % (name, 100 * (diff > 1e-6).mean()))
        assert (diff > 1e-6).mean() < 0.10 and diff.max() <= 2 * g["meta"]["eps"] + 1e-6
        assert list(success) == g[name + "_success"].tolist()
        assert adapter.make_decision(adv)[0].cpu().tolist() == g[name + "_decisions"].tolist()


# ------------------------------------------------------------------------------ full-size properties (BASELINE config 2)
def test_full_size_pgd_properties(hip_model, dev):
    """B=64 x 3 s: epsilon ball, [-1,1] box, run-to-run determinism, shard invariance (a batch gives
    bit-identical per-utterance results to its halves -- what the multi-GPU batch shard relies on)."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    B, T, eps = 64, 48000, 0.002
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=1234)).to(dev)
    y = hip_model.make_decision(x)[0]
    lower, upper = torch.clamp(x - eps, min=-1), torch.clamp(x + eps, max=1)
    spec = SEC4SR_CrossEntropy()
    run = lambda sl: hip_model.pgd_run(x[sl], y[sl], lower[sl], upper[sl], spec, 0.0004, 3, 1)
    a = run(slice(0, B))
    b = run(slice(0, B))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "not deterministic"
    lo, hi = run(slice(0, B // 2)), run(slice(B // 2, B))
    assert torch.equal(a[0], torch.cat((lo[0], hi[0]))), "result depends on how the batch is sharded"
    assert torch.equal(a[3], torch.cat((lo[3], hi[3])))
    assert (a[0] - x).abs().max().item() <= eps + 1e-7
    assert a[0].abs().max().item() <= 1.0
    assert torch.isfinite(a[3]).all()
    moved = ((a[0] - x).abs() > 0).float().mean().item()
    log("full-size PGD-3: fraction of samples moved %.4f, successes %d/64" % (moved, int(a[1].sum())))
    assert moved > 0.99


def test_full_size_shard_invariance_down_to_eight(hip_model, dev):
    """BASELINE metric shape (64 x 3 s) cut the way 2, 4 and 8 GPUs would cut it: the shards of 32 / 16 / 8 utterances run
    different contraction kernels (round-2 stream-K variants, 32-row tiles) and must still reproduce the full batch
    bit for bit -- audio, scores and success flags."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    B, eps = 64, 0.002
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=4321)).to(dev)
    y = hip_model.make_decision(x)[0]
    lower, upper = torch.clamp(x - eps, min=-1), torch.clamp(x + eps, max=1)
    spec = SEC4SR_CrossEntropy()
    run = lambda sl: hip_model.pgd_run(x[sl], y[sl], lower[sl], upper[sl], spec, 0.0004, 2, 1)
    full = run(slice(0, B))
    for world in (2, 4, 8):
        n = B // world
        parts = [run(slice(r * n, (r + 1) * n)) for r in range(world)]
        assert torch.equal(full[0], torch.cat([p[0] for p in parts])), "audio differs when cut into %d shards" % world
        assert torch.equal(full[3], torch.cat([p[3] for p in parts])) and torch.equal(full[1], torch.cat([p[1] for p in parts]))
    # one utterance alone (the reference's default batch_size = 1) too
    one = run(slice(5, 6))
    assert torch.equal(one[0], full[0][5:6]) and torch.equal(one[3], full[3][5:6])
    log("full-size shard invariance: 64 == 2x32 == 4x16 == 8x8 == single utterances, bit for bit")


def test_size_independent_attack_identities(hip_model, dev):
    """Properties that hold at any size, checked at 64 x 3 s: a zero step leaves the audio untouched; FGSM is PGD with one
    step of size epsilon (FGSM.py:35-36); an int16-scaled copy of the batch is attacked identically up to the scale
    (check_input_range, model/utils.py:7-19, decides once per batch)."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FGSM import FGSM
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    B, eps = 64, 0.002
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=777)).to(dev)
    y = hip_model.make_decision(x)[0]
    lower, upper = torch.clamp(x - eps, min=-1), torch.clamp(x + eps, max=1)
    spec = SEC4SR_CrossEntropy()
    still = hip_model.pgd_run(x, y, lower, upper, spec, 0.0, 2, 1)
    assert torch.equal(still[0], x)
    a1, s1 = FGSM(hip_model, epsilon=eps, batch_size=B, verbose=0).attack(x, y)
    a2, s2 = PGD(hip_model, epsilon=eps, step_size=eps, max_iter=1, batch_size=B, verbose=0).attack(x, y)
    assert torch.equal(a1, a2) and s1 == s2
    # the gradient of the int16-scaled waveform is the [-1,1] gradient divided by 2^15 (the model sees the same samples)
    _, sc_a, _, g_a = hip_model.loss_grad(x, y, spec)
    _, sc_b, _, g_b = hip_model.loss_grad(x * 32768.0, y, spec)
    assert torch.equal(sc_a, sc_b)
    np.testing.assert_allclose((g_b * 32768.0).cpu().numpy(), g_a.cpu().numpy(), rtol=1e-6, atol=0)
    log("size-independent identities at 64 x 3 s: zero step, FGSM == PGD-1(eps), int16-scale covariance")


def test_gradient_is_a_descent_direction_at_full_size(hip_model, dev):
    """Size-independent sanity of the hand-coded backward at B=64 x 3 s: moving a small distance along
    +grad changes the loss by h * |grad| (first-order Taylor).  Margin loss: the cross-entropy saturates
    to exactly 0 in fp32 for confidently classified utterances, which makes the ratio 0/0."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_MarginLoss
    x = torch.from_numpy(synth.make_waveforms(64, 48000, seed=99)).to(dev)
    y = hip_model.make_decision(x)[0]
    spec = SEC4SR_MarginLoss(False, 0., "CSI", None, False)
    _, _, l0, g = hip_model.loss_grad(x, y, spec)
    gnorm = g.flatten(1).norm(dim=1)
    assert torch.all(gnorm > 0)
    gn = g / gnorm.view(-1, 1, 1)
    h = 2e-4
    _, _, l1, _ = hip_model.loss_grad(x + h * gn, y, spec, want_grad=False)
    ratio = ((l1 - l0) / (h * gnorm)).cpu().numpy()
    log("directional derivative / predicted over 64 utterances: min %.3f median %.3f max %.3f"
        % (ratio.min(), np.median(ratio), ratio.max()))
    assert np.all(ratio > 0.7) and np.all(ratio < 1.3)


# ------------------------------------------------------------------------------ CW2 / FAKEBOB on the engine
def test_cw2_matches_oracle(hip_model, oracle_model, dev, capsys):
    """attack/CW2.py loop (tanh box, margin loss with clip, Adam, binary search) driven by the engine
    vs the same loop driven by the oracle's autograd.  Adam divides by sqrt(v): a gradient entry that
    differs in the last bits moves the modifier by the same relative amount only, so the tolerance is a
    plain allclose on the adversarial audio."""
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.CW2 import CW2
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=31))
    with torch.no_grad():
        y = oracle_model.make_decision(x)[0]
    kw = dict(task="CSI", initial_const=1e-2, binary_search_steps=2, max_iter=6, stop_early=True, stop_early_iter=3,
              lr=2e-3, batch_size=2)
    oadv, osucc = oatk.CW2(oracle_model, **kw).attack(x.clone(), y)
    adv, succ = CW2(hip_model, verbose=0, **kw).attack(x.to(dev), y.to(dev))
    diff = (adv.cpu() - oadv).abs().max().item()
    log("CW2 (2 search steps x 6 iters): max |x_adv - oracle| = %.3e, success hip=%s oracle=%s" % (diff, succ, osucc))
    assert succ == osucc
    # Adam's first update is lr * g / (|g| + eps) ~ lr * sign(g): an entry whose gradient is round-off
    # noise moves by +-lr on either side, so a handful of samples may differ by up to 2 * lr per step.
    d = (adv.cpu() - oadv).abs().numpy()
    assert (d > 2e-4).mean() < 1e-3 and d.max() <= 2 * 2e-3 * 6 + 1e-6


def test_cw2_targeted_sv_batch32(xv_weights, dev):
    """BASELINE.json configs[2]: CW2 (L2, Adam inner optimiser) targeted on the SV task, batch 32.  Imposter
    utterances are pushed to be accepted as the single enrolled speaker.  1 s audio vs the oracle loop; then the
    3 s batch on the device alone for the properties that do not need the oracle."""
    from oracle import attacks as oatk
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.attack.CW2 import CW2
    from speakerguard_amd.model.xv_plda import xv_plda
    w = dict(xv_weights)
    w["enroll"] = xv_weights["enroll"][:1].copy()  # SV: one enrolled speaker
    x = torch.from_numpy(synth.make_waveforms(32, 16000, seed=34))
    probe = XvPlda(w, threshold=None)
    with torch.no_grad():
        clean = probe.make_decision(x)[1][:, 0]
    thr = float(clean.max()) + 2.0  # every utterance starts rejected
    om, hm = XvPlda(w, threshold=thr), xv_plda.from_weights(w, threshold=thr, device=dev, dither=0.0)
    y = torch.zeros(32, dtype=torch.long)
    assert hm.make_decision(x.to(dev))[0].cpu().tolist() == [-1] * 32
    kw = dict(task="SV", targeted=True, confidence=0.0, initial_const=1e-2, binary_search_steps=2, max_iter=5,
              stop_early=True, stop_early_iter=5, lr=2e-3, batch_size=32)
    oadv, osucc = oatk.CW2(om, **kw).attack(x.clone(), y)
    adv, succ = CW2(hm, verbose=0, **kw).attack(x.to(dev), y.to(dev))
    d = (adv.cpu() - oadv).abs().numpy()
    log("CW2 targeted SV, batch 32 x 1 s: max |x_adv - oracle| %.3e, differing(>2e-4) %.4f%%, success %d/32 (oracle %d/32)" % (
        d.max(), 100 * (d > 2e-4).mean(), sum(succ), sum(osucc)))
    assert succ == osucc
    assert (d > 2e-4).mean() < 1e-3 and d.max() <= 2 * 2e-3 * 5 + 1e-6
    # full 3 s batch: success flags agree with the model's own decision on the returned audio
    x3 = torch.from_numpy(synth.make_waveforms(32, 48000, seed=35)).to(dev)
    thr3 = float(hm.make_decision(x3)[1][:, 0].max()) + 2.0
    hm.set_enroll(threshold=thr3)
    adv3, succ3 = CW2(hm, verbose=0, **dict(kw, max_iter=8)).attack(x3, y.to(dev))
    dec3 = hm.make_decision(adv3)[0].cpu().tolist()
    assert all((dd == 0) == ss for dd, ss in zip(dec3, succ3))
    assert adv3.abs().max().item() <= 1.0 and torch.isfinite(adv3).all()
    l2 = (adv3 - x3).flatten(1).norm(dim=1)
    log("CW2 targeted SV, batch 32 x 3 s (device only): success %d/32, mean L2 of successes %.4f" % (
        sum(succ3), float(l2[torch.tensor(succ3)].mean()) if any(succ3) else float("nan")))


def test_fakebob_matches_oracle_with_shared_noise(hip_model, oracle_model, dev):
    """FAKEBOB / NES (forward-only queries): both sides draw the NES noise from the same seeded CPU
    generator so the trajectories are comparable."""
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=32))
    with torch.no_grad():
        y = oracle_model.make_decision(x)[0]
    kw = dict(task="CSI", epsilon=0.002, max_iter=4, max_lr=0.0005, min_lr=1e-6, samples_per_draw=8,
              samples_per_draw_batch_size=4, sigma=0.001, stop_early=True, stop_early_iter=2, batch_size=1)
    g = torch.Generator().manual_seed(5)
    oadv, osucc = oatk.FAKEBOB(oracle_model, noise_fn=lambda shape: torch.randn(shape, generator=g), **kw).attack(x.clone(), y)
    g2 = torch.Generator().manual_seed(5)
    adv, succ = FAKEBOB(hip_model, verbose=0, noise_fn=lambda shape: torch.randn(shape, generator=g2), **kw).attack(
        x.to(dev), y.to(dev))
    diff = (adv.cpu() - oadv).abs()
    frac = float((diff > 1e-7).float().mean())
    log("FAKEBOB-4: samples differing %.3f%%, success hip=%s oracle=%s" % (100 * frac, succ, osucc))
    assert succ == osucc
    assert frac < 0.05 and diff.max().item() <= 2 * 0.002 + 1e-6


@pytest.mark.timeout(300)  # the reference loop has no iteration bound (FAKEBOB.py:236-278)
def test_estimate_threshold_matches_oracle_with_shared_noise(xv_weights, dev):
    """SURVEY 8(f) N2 on the native engine: a rejected voice is pushed up the threshold ladder with NES
    queries until the (hidden) OSI threshold accepts it; same noise stream on both sides."""
    from oracle import attacks as oatk
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(1, 16000, seed=41))
    probe = XvPlda(xv_weights, threshold=None)
    with torch.no_grad():
        top = float(probe.make_decision(x)[1].max())
    hidden = top + 0.25 * abs(top)  # the voice starts below the threshold: rejected
    om = XvPlda(xv_weights, threshold=hidden)
    hm = xv_plda.from_weights(xv_weights, threshold=hidden, device=dev, dither=0.0)
    assert int(hm.make_decision(x.to(dev))[0][0]) == -1
    kw = dict(task="OSI", epsilon=0.004, max_lr=0.001, min_lr=1e-6, samples_per_draw=8, samples_per_draw_batch_size=4,
              sigma=0.001, plateau_length=3)
    g = torch.Generator().manual_seed(9)
    want = oatk.FAKEBOB(om, noise_fn=lambda shape: torch.randn(shape, generator=g), **kw).estimate_threshold(x.clone(), step=0.1)
    g2 = torch.Generator().manual_seed(9)
    atk = FAKEBOB(hm, verbose=0, noise_fn=lambda shape: torch.randn(shape, generator=g2), **kw)
    got = atk.estimate_threshold(x.to(dev), step=0.1)
    log("estimate_threshold: hidden %.4f, oracle %.4f, hip %.4f" % (hidden, want, got))
    assert got is not None and atk.threshold == got
    assert got > hidden                                  # first accepted top score
    assert abs(got - want) <= 0.02 * abs(hidden) + 1e-3  # sign-step trajectories drift (H3); same rung of the ladder


def test_defended_model_passthrough_and_sharded_wrapper(hip_model, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.shard import ShardedAttack
    x = torch.from_numpy(synth.make_waveforms(3, 16000, seed=33)).to(dev)
    dm = defended_model(hip_model)
    d0, s0 = hip_model.make_decision(x)
    d1, s1 = dm.make_decision(x)
    assert torch.equal(d0, d1) and torch.equal(s0, s1)
    a = PGD(hip_model, max_iter=3, batch_size=3, verbose=0).attack(x, d0)
    b = PGD(dm, max_iter=3, batch_size=3, verbose=0).attack(x, d0)
    c = ShardedAttack(PGD(hip_model, max_iter=3, batch_size=3, verbose=0)).attack(x, d0)  # world size 1
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert torch.equal(a[0], c[0]) and a[1] == c[1]
    lam = lambda t: t * 1.0
    with pytest.raises(NotImplementedError):
        PGD(defended_model(hip_model, defense=[(0, lam)]), max_iter=1, verbose=0).attack(x, d0)


# ------------------------------------------------------------------------------ native attack-state kernels
def test_device_noise_is_shard_invariant(xv_weights, dev):
    """SURVEY 8(e) / ADVICE r1: device-generated noise (MFCC dither, NES queries) is keyed by the chunk's GLOBAL
    position, so attacking the two halves of a batch as two ranks would (attacker.index_offset = shard start, same
    attack-call count) reproduces the unsharded run bit for bit."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(4, 16000, seed=31)).to(dev)

    def halves(make, model):
        model._noise_epoch = 0
        full = make().attack(x, y)
        parts = []
        for lo, hi in ((0, 2), (2, 4)):
            model._noise_epoch = 0
            atk = make()
            atk.index_offset = lo
            parts.append(atk.attack(x[lo:hi], y[lo:hi]))
        return full, (torch.cat([p[0] for p in parts], 0), sum((list(p[1]) for p in parts), []))

    # (1) PGD + EOT over random dither (the reference's default front-end, xv_plda.py:119)
    md = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=5)
    y = md.make_decision(x)[0]
    full, sharded = halves(lambda: PGD(md, epsilon=0.002, step_size=0.0005, max_iter=2, batch_size=2, EOT_size=2,
                                       EOT_batch_size=2, verbose=0), md)
    assert torch.equal(full[0], sharded[0]) and list(full[1]) == sharded[1]
    # different chunks really see different noise: utterance 0 attacked as "global utterance 2" moves differently
    md._noise_epoch = 0
    shifted = PGD(md, epsilon=0.002, step_size=0.0005, max_iter=2, batch_size=2, EOT_size=2, EOT_batch_size=2, verbose=0)
    shifted.index_offset = 2
    assert not torch.equal(shifted.attack(x[0:2], y[0:2])[0], full[0][0:2])
    # (2) FAKEBOB with the engine's own NES noise (counter-based generator), deterministic front-end
    m0 = xv_plda.from_weights(xv_weights, device=dev, dither=0.0)
    full, sharded = halves(lambda: FAKEBOB(m0, task="CSI", epsilon=0.002, max_iter=2, samples_per_draw=4,
                                           samples_per_draw_batch_size=4, batch_size=2, verbose=0), m0)
    assert torch.equal(full[0], sharded[0]) and list(full[1]) == sharded[1]
    log("device noise (dither + NES) shard-invariant: halves == full batch bit for bit")


def test_noise_does_not_depend_on_where_the_batch_is_cut(xv_weights, dev):
    """Round 4: shards are cut with granule 1 (shard.py), so the noise an utterance sees must be a function of its GLOBAL
    index and the EOT repeat only -- not of the chunk it happens to be attacked in.  One chunk of 5 against the cuts
    (0,2) + (2,5) and 5 x 1, with the random dither of the reference's default front-end: the device loop
    (sg_xv_pgd_run, repeats batched inside), the host-chained EOT loop (EOT.py:29 materialises the repeats: rows =
    repeat * B + utterance, named to the kernel through sg_dither.rep_rows) and CW2 (one pass per iteration)."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.CW2 import CW2
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(5, 16000, seed=33)).to(dev)
    md = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=9)
    y = md.make_decision(x)[0]

    class HostLoop(PGD):  # the step-by-step loop over EOT.forward instead of the device loop
        def _device_route(self, n_audios):
            return None

    makers = {
        "device loop": lambda bs: PGD(md, epsilon=0.002, step_size=0.0005, max_iter=2, batch_size=bs, EOT_size=4, EOT_batch_size=2, verbose=0),
        "host-chained EOT": lambda bs: HostLoop(md, epsilon=0.002, step_size=0.0005, max_iter=2, batch_size=bs, EOT_size=4, EOT_batch_size=2, verbose=0),
        "CW2": lambda bs: CW2(md, initial_const=0.1, binary_search_steps=1, max_iter=3, stop_early=False, lr=2e-3, batch_size=bs, verbose=0),
    }
    for name, make in makers.items():
        md._noise_epoch = 0
        full = make(5).attack(x, y)
        for cuts in (((0, 2), (2, 5)), tuple((i, i + 1) for i in range(5))):
            parts = []
            for lo, hi in cuts:
                md._noise_epoch = 0
                atk = make(5)
                atk.index_offset = lo
                parts.append(atk.attack(x[lo:hi], y[lo:hi]))
            assert torch.equal(full[0], torch.cat([p[0] for p in parts], 0)), (name, cuts)
            assert list(full[1]) == sum((list(p[1]) for p in parts), []), (name, cuts)
        md._noise_epoch = 0
        chunked = make(2).attack(x, y)  # the same attack in chunks of 2, 2, 1
        assert torch.equal(full[0], chunked[0]) and list(full[1]) == list(chunked[1]), name
        md._noise_epoch = 0
        moved = make(5)
        moved.index_offset = 1  # ... and the index matters: the same audio attacked as utterances 1.. moves differently
        assert not torch.equal(moved.attack(x[:2], y[:2])[0], full[0][:2]), name
    log("device noise: one chunk of 5 == cuts (0,2)+(2,5) == 5 x 1 == chunks of 2 bit for bit (device loop, host-chained EOT, CW2)")


class _OneRankOf(object):
    """speakerguard_amd.shard.ShardedAttack as rank `rank` of `world` sees it, without a process group: the exchange is
    replaced by writing this rank's rows into the full-size result (the gloo tests cover the exchange itself)."""

    def __new__(cls, attacker, world, rank):
        from speakerguard_amd.shard import ShardedAttack

        class One(ShardedAttack):
            def _world(self):
                return world, rank

            def _gather_rows(self, local, bounds, n):
                out = torch.zeros((n,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
                s, e = bounds[rank]
                out[s:e] = local[: e - s]
                return out
        return One(attacker, gather_audio=True)


def test_sharded_attack_cuts_the_metrics_batch_over_eight_ranks(xv_weights, dev):
    """`ShardedAttack(PGD(batch_size=64)).attack(x64, y64)` on 8 (and 3) ranks -- every rank gets
    64 / world utterances, runs them as ONE device loop, and the ranks' results put together are the single-GPU
    result bit for bit (flags, audio), with the reference's default dither on and EOT 2."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.xv_plda import xv_plda
    from speakerguard_amd.shard import shard_bounds
    x = torch.from_numpy(synth.make_waveforms(64, 48000, seed=1234)).to(dev)
    for dither in (0.0, 1.0):
        md = xv_plda.from_weights(xv_weights, device=dev, dither=dither, dither_seed=4)
        y = md.make_decision(x)[0]
        make = lambda: PGD(md, epsilon=0.0005, step_size=0.0002, max_iter=3, batch_size=64, EOT_size=2 if dither else 1,
                           EOT_batch_size=2 if dither else 1, verbose=0)
        md._noise_epoch = 0
        ref_adv, ref_succ = make().attack(x, y)
        for world in (8, 3):
            adv, flags, seen = torch.zeros_like(ref_adv), np.zeros(64, bool), []
            for rank in range(world):
                md._noise_epoch = 0
                atk = make()
                sizes = []
                inner = atk.attack_batch
                atk.attack_batch = lambda xb, *a, inner=inner, sizes=sizes: (sizes.append(int(xb.shape[0])), inner(xb, *a))[1]
                a, f = _OneRankOf(atk, world, rank).attack(x, y)
                adv += a
                flags |= np.asarray(f)
                seen.append(sizes)
            assert [sum(c) for c in seen] == [e - s for s, e in shard_bounds(64, world)] and all(len(c) == 1 for c in seen), seen
            assert torch.equal(adv, ref_adv) and flags.tolist() == [bool(v) for v in ref_succ], (dither, world)
        assert 0 < sum(ref_succ) < 64, "both outcomes: %d of 64" % sum(ref_succ)
    log("ShardedAttack(PGD(batch_size=64)) on 8 / 3 emulated ranks: 8 (22/21/21) utterances per rank, one chunk each, "
        "== the single-GPU attack bit for bit, dither 0 and dither 1 + EOT 2 (%d of 64 fooled)" % sum(ref_succ))


def test_query_sharded_model_call_is_the_unsharded_call(xv_weights, dev):
    """BASELINE.json configs[4] (query batch sharded over the GPUs): speakerguard_amd.shard.QueryShardedModel splits
    the ROWS of one model call over the ranks.  The exchange itself is covered on the CPU by a 2-rank gloo test
    (tests/test_shard_gloo.py); here the ranks are emulated one after the other on the one GPU, with the random
    dither of the reference's default front-end on: every row slice (2, 3 and 8 ranks, uneven cuts, more ranks than
    rows) must reproduce its rows of the full call bit for bit, and FAKEBOB on the sliced model must be FAKEBOB on
    the plain one."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.model.xv_plda import xv_plda
    from speakerguard_amd.shard import QueryShardedModel, row_slices

    class SerialRanks(QueryShardedModel):
        """world emulated ranks, one after the other; every rank starts from the same per-call draw counter."""
        world = 2

        def loss_grad(self, x, y, loss_spec, want_grad=True, **kw):
            base = self.base_model
            run, keep = row_slices(x.shape[0], self.world)
            draw0, outs = base._draw, []
            for (lo, hi), (ks, ke) in zip(run, keep):
                base._draw = draw0
                out = self._call_rows(x, y, loss_spec, lo, hi, want_grad, kw)
                outs.append([None if t is None else t[: ke - ks] for t in out])
            return tuple(None if outs[0][i] is None else torch.cat([o[i] for o in outs], 0) for i in range(4))

    md = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=11)
    x = torch.from_numpy(synth.make_waveforms(7, 16000, seed=41)).to(dev)
    y = (torch.arange(7) % 10).to(dev)
    spec = SEC4SR_CrossEntropy()
    md._draw = 0
    full = md.loss_grad(x, y, spec, want_grad=True)
    proxy = SerialRanks(md)
    for world in (2, 3, 8):
        proxy.world = world
        md._draw = 0
        got = proxy.loss_grad(x, y, spec, want_grad=True)
        assert md._draw == 1 and md._row_base == 0
        for a, b in zip(got, full):
            assert torch.equal(a, b), world
    md._draw = 0
    md._row_base = 3  # the row key matters: the same rows scored as "rows 3.." see other noise
    assert not torch.equal(md.loss_grad(x[:2], y[:2], spec, want_grad=False)[1], full[1][:2])
    md._row_base = 0

    kw = dict(task="CSI", epsilon=0.002, max_iter=3, samples_per_draw=6, samples_per_draw_batch_size=6, batch_size=2,
              EOT_size=2, EOT_batch_size=2, verbose=0)
    md._noise_epoch = 0
    ref_adv, ref_succ = FAKEBOB(md, **kw).attack(x[:2], y[:2])
    for world in (2, 8):
        proxy.world = world
        md._noise_epoch = 0
        adv, succ = FAKEBOB(proxy, **kw).attack(x[:2], y[:2])
        assert torch.equal(adv, ref_adv) and list(succ) == list(ref_succ), world
    log("query-sharded model call (2 / 3 / 8 emulated ranks, dither on, EOT 2): rows and FAKEBOB result bit-identical")


def test_cw2_step_kernel_matches_torch_adam(hip_model, dev):
    """sg_cw2_step vs torch.tanh/atanh + torch.optim.Adam on the same numbers (CW2.py:72-82)."""
    g = torch.Generator().manual_seed(2)
    B, T = 3, 16000
    x = (torch.rand(B, 1, T, generator=g) * 1.9 - 0.95).to(dev)
    const = torch.tensor([1e-3, 0.5, 20.0], device=dev)
    modifier = torch.zeros_like(x)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    ref_mod = torch.zeros_like(x, requires_grad=True)
    opt = torch.optim.Adam([ref_mod], lr=1e-2)
    inp, l2 = hip_model.cw2_step(modifier, None, None, x, None, None, const, 1e-2, 0)
    ref_inp = torch.tanh(ref_mod + torch.atanh(x * 0.999999))
    np.testing.assert_allclose(inp.cpu().numpy(), ref_inp.detach().cpu().numpy(), rtol=0, atol=2e-7)
    for t in range(1, 4):
        g1 = torch.randn(B, 1, T, generator=g).to(dev) * 1e-3
        ref_inp = torch.tanh(ref_mod + torch.atanh(x * 0.999999))
        (const * (ref_inp * g1).sum((1, 2)) + ((ref_inp - x) ** 2).sum((1, 2))).sum().backward()
        opt.step()
        opt.zero_grad()
        inp, l2 = hip_model.cw2_step(modifier, m, v, x, inp, g1, const, 1e-2, t)
        want = torch.tanh(ref_mod + torch.atanh(x * 0.999999)).detach()
        err = (inp - want).abs().max().item()
        assert err < 5e-6, (t, err)
        np.testing.assert_allclose(l2.cpu().numpy(), ((want - x) ** 2).sum((1, 2)).cpu().numpy(), rtol=2e-5)
    log("cw2_step vs torch Adam after 3 steps: max |input diff| %.2e" % err)


def test_nes_and_fakebob_kernels(hip_model, dev):
    g = torch.Generator().manual_seed(3)
    n, T, half, sigma = 2, 16000, 4, 0.001
    x = (torch.rand(n, 1, T, generator=g) * 1.8 - 0.9).to(dev)
    noise = torch.randn(n, half, 1, T, generator=g).to(dev)
    for with_clean in (True, False):
        q, _ = hip_model.nes_queries(x, half, with_clean, sigma, 7, 0, noise)
        full = torch.cat((noise, -noise), 1)
        if with_clean:
            full = torch.cat((torch.zeros_like(x).unsqueeze(1), full), 1)
        want = (full * sigma + x.unsqueeze(1)).view(-1, 1, T)
        assert torch.equal(q, want)
        Q = 2 * half + int(with_clean)
        loss = torch.randn(n, Q, generator=g).to(dev)
        grad = torch.zeros_like(x)
        hip_model.nes_grad(loss, grad, n, T, half, with_clean, 7, 0, noise, False, sigma, 2)
        l = loss[:, 1:] if with_clean else loss
        ref = torch.mean(l.unsqueeze(2).unsqueeze(3) * torch.cat((noise, -noise), 1), 1) / sigma / 2
        np.testing.assert_allclose(grad.cpu().numpy(), ref.cpu().numpy(), rtol=2e-6, atol=3e-4)  # |grad| ~ 300; sum order differs
    # internal generator: reproducible, N(0,1), and nes_grad regenerates exactly what nes_queries used
    q1, z1 = hip_model.nes_queries(x, half, True, sigma, 11, 4, None, want_noise=True)
    q2, z2 = hip_model.nes_queries(x, half, True, sigma, 11, 4, None, want_noise=True)
    assert torch.equal(q1, q2) and torch.equal(z1, z2)
    assert not torch.equal(z1, hip_model.nes_queries(x, half, True, sigma, 12, 4, None, want_noise=True)[1])
    assert abs(z1.mean().item()) < 0.01 and abs(z1.std().item() - 1.0) < 0.01
    loss = torch.randn(n, 2 * half + 1, generator=g).to(dev)
    ga, gb = torch.zeros_like(x), torch.zeros_like(x)
    hip_model.nes_grad(loss, ga, n, T, half, True, 11, 4, None, False, 0.0, 1)
    hip_model.nes_grad(loss, gb, n, T, half, True, 11, 4, z1.contiguous(), False, 0.0, 1)
    assert torch.equal(ga, gb)
    # FAKEBOB.py:93-104
    prev = torch.randn(n, 1, T, generator=g).to(dev)
    grad = torch.randn(n, 1, T, generator=g).to(dev)
    grad[:, :, ::5] = 0.0
    prev[:, :, ::5] = 0.0
    lr = torch.tensor([1e-3, 2.5e-4], device=dev)
    lower, upper = torch.clamp(x - 0.002, min=-1), torch.clamp(x + 0.002, max=1)
    mg = 0.9 * prev + (1.0 - 0.9) * grad
    want_x = torch.min(torch.max(x + (-1) * lr.view(-1, 1, 1) * torch.sign(mg), lower), upper)
    xx, gg = x.clone(), grad.clone()
    hip_model.fakebob_step(xx, gg, prev, lr, lower, upper, 0.9, -1)
    assert torch.equal(xx, want_x) and torch.equal(gg, mg)


@pytest.mark.parametrize("D,n_spk", [(150, 7), (37, 3), (512, 10)])
def test_backend_dimensions_not_multiples_of_four(dev, D, n_spk):
    """LDA / PLDA dimension read from the model files (iv_plda.py:424): the tail kernel's device copies pad the matrix rows
    to 16-byte multiples (its products use 16-byte column loads).  Scores and decisions from the waveform, and d loss / d raw
    MFCC features of the SAME feature tensor, against the oracle, for dimensions that need the padding (150, 37) and for the
    largest one the kernel admits (512).  (The gradient is compared at feature level on purpose: with these uncalibrated random
    weights a 6e-5 difference between the two MFCC implementations flips a few ReLU units of some utterances and moves
    d loss / d waveform by up to 3 % -- tests/tools/grad_sensitivity.py shows that the HIP chain fed the oracle's features, and
    the HIP MFCC backward fed the oracle's feature gradient, each agree with the oracle to 1e-5.)"""
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.model.xv_plda import xv_plda
    w = synth.make_xv_weights(seed=3, D=D, n_spk=n_spk, calibrated=False)
    hip = xv_plda.from_weights(w, device=dev, dither=0.0)
    om = XvPlda(w, faithful=False)
    x = torch.from_numpy(synth.make_waveforms(3, 16000, seed=77))
    y = torch.arange(3) % n_spk
    dec, scores = hip.make_decision(x.to(dev))
    with torch.no_grad():
        odec, oscores = om.make_decision(x)
        feats = om.compute_feat(x, 1)
    sc = np.abs(oscores.numpy()).max()
    np.testing.assert_allclose(scores.cpu().numpy(), oscores.numpy(), rtol=0, atol=2e-4 * sc + 1e-3)
    assert dec.cpu().tolist() == odec.tolist()
    fin = feats.clone().requires_grad_(True)
    _, fsc = om.make_decision(fin, flag=1)
    torch.nn.functional.cross_entropy(fsc, y, reduction="none").backward(torch.ones(3))
    want = fin.grad.numpy()
    _, hsc, _, grad = hip.loss_grad(feats.to(dev), y.to(dev), SEC4SR_CrossEntropy(), flag=1)
    got = grad.cpu().numpy()
    gs = np.abs(want).max()
    assert gs > 0
    np.testing.assert_allclose(hsc.cpu().numpy(), fsc.detach().numpy(), rtol=0, atol=2e-4 * sc + 1e-3)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-4 * gs)
    log("back-end D=%d, %d speakers: scores max err %.2e of %.1f; d loss / d raw feats max err / max %.2e" % (
        D, n_spk, np.abs(scores.cpu().numpy() - oscores.numpy()).max(), sc, np.abs(got - want).max() / gs))


# ---- the PLDA back end at its corner shapes (tests/plda_cases.py): D = 150, S = 1, 27 / 28 (table in LDS or not), 64 / 65 (wave /
# block form of the loss); one model of 65 speakers, a case enrols the first S
@pytest.fixture(scope="module")
def backend_case(dev):
    import plda_cases as P
    from speakerguard_amd.model.xv_plda import xv_plda
    w = P.xv_weights()
    return w, xv_plda.from_weights(w, device=dev, dither=0.0), torch.from_numpy(P.waveforms()).to(dev)


@pytest.mark.parametrize("S", [1, 27, 28, 64, 65])
def test_backend_corner_shapes_against_float64_scores(backend_case, S):
    """scores against the float64 log-likelihood ratio of the model's OWN returned embedding under the score rule of
    tests/truth.py (the yard: the same recomputation in float32), decisions = the float64 arg-max outside the tie margin"""
    import plda_cases as P
    w, m, x = backend_case
    m.set_enroll(w["enroll"][:S])
    dec, scores, emb, _ = m._forward(x, 0, want_emb=True)
    emb = emb.cpu().numpy()
    truth = P.llr(emb, w["enroll"][:S], w["plda_psi"])
    yard = P.llr(emb, w["enroll"][:S], w["plda_psi"], np.float32).astype(np.float64)
    err, bound = np.abs(scores.cpu().numpy().astype(np.float64) - truth).max(1), P.xv_score_bound(truth, yard)
    log("back-end corner D=%d S=%d: score err %s, bound %s, margin %s" % (P.D, S, err, bound, P.top_two_margin(truth)))
    assert scores.shape == (P.B, S) and np.isfinite(emb).all() and (err <= bound).all(), (err, bound)
    clear = P.top_two_margin(truth) > bound
    assert clear.mean() >= 0.9 and (dec.cpu().numpy()[clear] == truth.argmax(1)[clear]).all()


@pytest.mark.parametrize("S", [1, 27, 28, 64, 65])
def test_backend_corner_shapes_override_and_reenrol_bit_for_bit(backend_case, S):
    """test_enroll_embs_argument_is_a_per_call_override at every corner count: a permuted subset through ``enroll_embs=`` gives
    the matching columns of the full-table scores, and a smaller table enrolled and the full one enrolled again the first ones"""
    import plda_cases as P
    w, m, x = backend_case
    full = w["enroll"][:S]
    m.set_enroll(full)
    sc0 = m.score(x)
    idx = P.subset(S)
    sub = m.score(x, enroll_embs=torch.from_numpy(full[idx].copy()).to(x.device))
    assert sub.shape == (P.B, len(idx)) and torch.equal(sub, sc0[:, torch.from_numpy(idx).to(x.device)])
    assert m.num_spks == S and torch.equal(m.score(x), sc0)
    m.set_enroll(full[:max(1, S // 2)])
    assert m.score(x).shape == (P.B, max(1, S // 2))
    m.set_enroll(full)
    assert torch.equal(m.score(x), sc0)


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("loss_name", ["Entropy", "Margin"])
def test_backend_corner_shapes_gradient_is_row_invariant(backend_case, loss_name, S):
    """loss_grad from the waveform: finite, and three rows in one call bit-equal to the same rows one at a time"""
    import plda_cases as P
    from speakerguard_amd.attack.utils import resolve_loss
    w, m, x = backend_case
    m.set_enroll(w["enroll"][:S])
    spec, _ = resolve_loss(loss_name, targeted=False, task='CSI', threshold=None, clip_max=False)
    y = (torch.arange(P.B) % S).to(x.device)
    dec, sc, loss, grad = m.loss_grad(x, y, spec, flag=0)
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all() and grad.shape == x.shape
    for i in range(P.B):
        d1, s1, l1, g1 = m.loss_grad(x[i:i + 1], y[i:i + 1], spec, flag=0)
        assert torch.equal(g1, grad[i:i + 1]) and torch.equal(s1, sc[i:i + 1]) and torch.equal(l1, loss[i:i + 1]) and torch.equal(d1, dec[i:i + 1])
