"""The power of the fp64 gradient policy (tests/truth.py), proved on the CPU before anything is judged by it.

Accept: an independent fp32 evaluation of the oracle passes ``truth.check``.  Reject: each planted defect -- the fp64
oracle with one function monkeypatched, rounded to fp32 like a kernel's output -- fails it, on the metric that should catch
it.  Batch 8 x 3 s, labels shifted off the model's own decisions (a confidently classified utterance has a round-off-only
cross-entropy gradient in fp32).
"""
import copy

import numpy as np
import pytest
import torch

import truth
from oracle import audionet as oan
from oracle import kaldi_mfcc
from oracle import xv_plda as oxv

B, T = 8, 48000


def _grad_scaled(t, factor):
    """Identity forward; the gradient arriving at `t` is multiplied by `factor` (a broadcastable tensor)."""
    t = t.clone()
    t.register_hook(lambda g: g * factor.to(g.dtype))
    return t


def _as_fp32(side):
    """A kernel's output: the defective fp64 answer rounded to float32."""
    r = lambda a: a.astype(np.float32).astype(np.float64)
    return truth.Side(r(side.scores), r(side.loss), r(side.grad))


@pytest.fixture(scope="module")
def xv():
    from speakerguard_amd import synth
    w = synth.make_xv_weights(seed=0, D=200, n_spk=10)
    om = oxv.XvPlda(w)
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=5))
    with torch.no_grad():
        y = (om.make_decision(x)[0] + 1) % 10
    loss = truth.Loss("ce")
    f32, f64 = truth.evaluate(om, x, y, loss)
    return dict(w=w, om=om, m64=copy.deepcopy(om).double(), x=x, y=y, loss=loss, f32=f32, f64=f64)


@pytest.fixture(scope="module")
def an():
    from speakerguard_amd import synth
    om = oan.AudioNet(synth.make_audionet_state_dict(seed=0, num_class=251))
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=5))
    with torch.no_grad():
        y = (om.make_decision(x)[0] + 1) % 251
    loss = truth.Loss("ce")
    f32, f64 = truth.evaluate(om, x, y, loss)
    return dict(om=om, m64=copy.deepcopy(om).double(), x=x, y=y, loss=loss, f32=f32, f64=f64)


def test_losses_match_the_oracle_attack_losses():
    """truth.Loss (dtype-preserving) is the loss of oracle/attacks.py, branch by branch."""
    from oracle import attacks as oatk
    g = torch.Generator().manual_seed(3)
    s = torch.randn(6, 5, generator=g) * 3
    y = torch.tensor([0, 1, 2, 3, -1, 4])
    np.testing.assert_allclose(truth.Loss("ce")(s, y.clamp(min=0)).numpy(),
                               oatk.cross_entropy_loss(s, y.clamp(min=0)).numpy(), rtol=1e-6, atol=1e-6)
    for task in ("CSI", "OSI"):
        for targeted in (False, True):
            for clip in (False, True):
                lo = truth.Loss("margin", targeted, 0.3, task, 0.5, clip)
                want = oatk.margin_loss(s, y, targeted, 0.3, task, 0.5, clip)
                np.testing.assert_allclose(lo(s, y).numpy(), want.numpy(), rtol=1e-6, atol=1e-6, err_msg=repr(lo))
    ysv = torch.tensor([0, -1, 0, -1, 0, 0])
    for targeted in (False, True):
        lo = truth.Loss("margin", targeted, 0.0, "SV", 0.5, True)
        np.testing.assert_allclose(lo(s[:, :1], ysv).numpy(), oatk.margin_loss(s[:, :1], ysv, targeted, 0.0, "SV", 0.5, True).numpy(),
                                   rtol=1e-6, atol=1e-6)
    assert truth.Loss("ce")(s.double(), y.clamp(min=0)).dtype == torch.float64


def test_metrics_on_a_hand_made_gradient():
    g64 = np.zeros((2, 400))
    g64[:, :] = 1.0
    g = g64.copy()
    g[0, 320:400] = 0.0      # the last half hop of utterance 0 dropped
    g[1, 5] = -1.0           # one decided sign flipped in utterance 1
    np.testing.assert_allclose(truth.utt_error(g, g64), [np.sqrt(80 / 400), np.sqrt(4 / 400)])
    np.testing.assert_allclose(truth.block_error(g, g64), [1.0, np.sqrt(4 / 160)])  # the partial hop counts over its 80
    assert truth.decided_sign(g, g64).tolist() == [80, 1]  # a zeroed decided entry disagrees too
    assert truth.decided_sign(g, g64, tau=1.5).tolist() == [0, 0]


def test_fp32_oracle_accepted_xvector(xv):
    """The reference structure of the oracle (per-utterance loops, the running-sum CMVN) in fp32, judged with the batched
    fp32 oracle as yardstick: accepted.  So is the batched oracle itself (decided signs 0)."""
    faithful, _ = truth.evaluate(oxv.XvPlda(xv["w"], faithful=True), xv["x"], xv["y"], xv["loss"], truth_model=xv["m64"])
    rep = truth.check(faithful, xv["f32"], xv["f64"], "xv faithful fp32 oracle")
    print(rep.line())
    rep.assert_ok()
    truth.check(xv["f32"], xv["f32"], xv["f64"], "xv fp32 oracle").assert_ok()
    assert xv["f32"].loss.min() > 0.5  # shifted labels: off saturation


def test_fp32_oracle_accepted_audionet(an):
    """AudioNet in fp32 one utterance at a time against the batched fp32 oracle: accepted."""
    rows = [truth.evaluate(an["om"], an["x"][b:b + 1], an["y"][b:b + 1], an["loss"], truth_model=an["m64"])[0]
            for b in range(B)]
    per = truth.Side(*(np.concatenate([getattr(r, k) for r in rows]) for k in ("scores", "loss", "grad")))
    rep = truth.check(per, an["f32"], an["f64"], "AudioNet per-utterance fp32 oracle")
    print(rep.line())
    rep.assert_ok()


def _patched_truth(monkeypatch, d, module, name, fn, forward=truth.default_forward):
    monkeypatch.setattr(module, name, fn)
    return _as_fp32(truth.evaluate_truth(d["m64"], d["x"], d["y"], d["loss"], forward))


def _rejected(d, judged, metric, what):
    rep = truth.check(judged, d["f32"], d["f64"], what)
    print(rep.line())
    assert metric in rep.failed, rep.line()
    return rep


def test_rejects_cmvn_window_over_n_plus_one(xv, monkeypatch):
    def cmvn(feats):
        nf = feats.shape[1]
        se = np.array([oxv.cmvn_window(t, nf) for t in range(nf)])
        start, end = torch.from_numpy(se[:, 0]), torch.from_numpy(se[:, 1])
        csum = torch.cat((torch.zeros(feats.shape[0], 1, feats.shape[2], dtype=feats.dtype), feats.cumsum(1)), 1)
        return feats - (csum[:, end, :] - csum[:, start, :]) / (end - start + 1).to(feats.dtype).view(1, nf, 1)
    _rejected(xv, _patched_truth(monkeypatch, xv, oxv, "cmvn_closed_form", cmvn), "utt", "xv CMVN n + 1")


@pytest.mark.parametrize("edge", ["last400", "first240"])
def test_rejects_dropped_edge_gradient(xv, monkeypatch, edge):
    """The gradient of the last frame's 400 samples (a partial tile, the reflected tail) or of the first 240 (the reflect
    padding and the pre-emphasis replicate pad) lost in the backward."""
    orig = kaldi_mfcc.get_strided

    def get_strided(wav):
        m = torch.ones_like(wav)
        if edge == "last400":
            m[-400:] = 0
        else:
            m[:240] = 0
        return orig(_grad_scaled(wav, m))
    rep = _rejected(xv, _patched_truth(monkeypatch, xv, kaldi_mfcc, "get_strided", get_strided), "block", "xv " + edge)
    assert "decided_sign" in rep.failed


def test_rejects_tdnn1_edge_frames_dropped(xv, monkeypatch):
    """tdnn1's data gradient without its first and last input frames (the edge taps of the transposed contraction)."""
    def forward(m, x):
        feats = m.compute_feat(x, flag=2)
        mask = torch.ones(1, feats.shape[1], 1, dtype=feats.dtype)
        mask[:, 0] = mask[:, -1] = 0
        return m.scoring_trials(m.enroll_embs, m.extract_emb(_grad_scaled(feats, mask)))
    judged = _as_fp32(truth.evaluate_truth(xv["m64"], xv["x"], xv["y"], xv["loss"], forward))
    _rejected(xv, judged, "block", "xv tdnn1 edge frames")


def test_rejects_one_utterance_scaled(xv):
    """The smallest relative scale error of one utterance's gradient the bound still catches, planted on the utterance where
    the yardstick's own error is largest (the loosest bound of the batch): 1.5 %."""
    u = int(np.argmax(truth.utt_error(xv["f32"].grad, xv["f64"].grad)))
    f = torch.ones(B, 1, 1, dtype=torch.float64)
    f[u] = 1.015
    judged = _as_fp32(truth.evaluate_truth(xv["m64"], xv["x"], xv["y"], xv["loss"],
                                           lambda m, x: m(_grad_scaled(x, f))))
    rep = _rejected(xv, judged, "utt", "xv utterance %d gradient x 1.015" % u)
    assert {f[1] for f in rep.failures if f[0] == "utt"} == {u}


def test_rejects_audionet_reflect_pad_as_zero_pad_in_the_adjoint(an, monkeypatch):
    def preprocess(wav):
        wav = wav[:, 1:] - oan.PREEMPH * wav[:, :-1]
        p = oan.N_FFT // 2
        left, right = wav[:, 1:p + 1].flip(1).detach(), wav[:, -p - 1:-1].flip(1).detach()  # no gradient through the pad
        spec = torch.stft(torch.cat((left, wav, right), 1), n_fft=oan.N_FFT, hop_length=oan.HOP, win_length=oan.WIN,
                          window=torch.hann_window(oan.WIN, dtype=wav.dtype), center=False, return_complex=True)
        mel = torch.matmul((spec.real.pow(2) + spec.imag.pow(2)).transpose(2, 1), oan._MEL.t().to(wav.dtype)).transpose(2, 1)
        return 10 * torch.clamp(mel, oan.EPSILON).log10()
    judged = _patched_truth(monkeypatch, an, oan, "preprocess", preprocess)
    np.testing.assert_allclose(judged.scores, an["f64"].scores, rtol=1e-6)  # the forward is untouched
    _rejected(an, judged, "block", "AudioNet reflect pad as zero pad in the adjoint")


def test_rejects_audionet_mel_band_missing_in_the_backward(an, monkeypatch):
    orig = oan.preprocess

    def preprocess(wav):
        band = torch.ones(oan.N_MELS, 1, dtype=torch.float64)
        band[10] = 0
        real = oan._MEL
        try:  # band 10 of the mel product carries no gradient: M = M * mask + (M * (1 - mask)) seen through a detached input
            oan._MEL = real * band.float()
            with_grad = orig(wav)
            oan._MEL = real
            wav_d = wav.detach()
            full = orig(wav_d)
        finally:
            oan._MEL = real
        keep = band.to(wav.dtype).view(1, oan.N_MELS, 1)
        return with_grad * keep + full * (1 - keep)
    judged = _patched_truth(monkeypatch, an, oan, "preprocess", preprocess)
    np.testing.assert_allclose(judged.scores, an["f64"].scores, rtol=1e-6)
    _rejected(an, judged, "utt", "AudioNet mel band 10 missing in the backward")


def test_clipped_loss_needs_an_exactly_zero_gradient(xv):
    """Untargeted margin loss, clipped at 0 where the label is not the decision (odd rows): the truth's gradient is exactly
    zero there, so is the yardstick's; a judged gradient with round-off in it is rejected."""
    x, y0 = xv["x"], xv["y"].clone()
    y0[::2] = (y0[::2] - 1) % 10  # even rows: the model's own decision
    lo = truth.Loss("margin", False, 0.0, "CSI", None, True)
    f32, f64 = truth.evaluate(xv["om"], x, y0, lo, truth_model=xv["m64"])
    clipped = f64.loss == 0
    assert clipped.any() and np.all(f32.grad[clipped] == 0)
    truth.check(f32, f32, f64, "clipped margin", clipped=clipped).assert_ok()
    bad = truth.Side(f32.scores, f32.loss, f32.grad.copy())
    bad.grad[np.nonzero(clipped)[0][0], 0, 100] = 1e-12
    assert "clipped_zero" in truth.check(bad, f32, f64, "clipped margin, one stray entry", clipped=clipped).failed
