"""The engine's scores, loss and d loss / d input against the float64 truth, at the benchmark's and the BASELINE configs'
shapes, utterance by utterance (tests/truth.py holds the policy; tests/test_truth_power.py proves it rejects planted
defects).  The fp32 oracle on the same input is the yardstick: the engine must be at least about as close to the fp64
model as the oracle is.  Dither 0, synthetic waveforms, labels shifted off the model's own decisions where the loss would
otherwise saturate (a confidently classified utterance has a cross-entropy gradient that is fp32 round-off on both sides).

Every case appends its measured metrics, engine and yardstick side by side, to the parity log.
"""
import numpy as np
import pytest
import torch

import truth
from conftest import log

pytestmark = pytest.mark.gpu

T3 = 48000
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def xv_hip(xv_weights, dev):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=dev, dither=0.0)


@pytest.fixture(scope="module")
def xv_ora(xv_weights):
    from oracle.xv_plda import XvPlda
    return XvPlda(xv_weights)


@pytest.fixture(scope="module")
def an_sd():
    from speakerguard_amd import synth
    return synth.make_audionet_state_dict(seed=0, num_class=251)


@pytest.fixture(scope="module")
def an_hip(an_sd, dev):
    from speakerguard_amd.model.audionet_csine import audionet_csine
    return audionet_csine.from_weights(an_sd, device=dev)


@pytest.fixture(scope="module")
def an_ora(an_sd):
    from oracle.audionet import AudioNet
    return AudioNet(an_sd)


_CACHE = {}


def _oracle(key, model, x, y, loss, forward=truth.default_forward):
    """(fp32, fp64) of the oracle, shared by the cases that differ only on the engine's side (front-end precision)."""
    if key not in _CACHE:
        _CACHE[key] = truth.evaluate(model, x, y, loss, forward)
    return _CACHE[key]


def _wav(B, T, seed):
    from speakerguard_amd import synth
    return torch.from_numpy(synth.make_waveforms(B, T, seed=seed))


def _shifted(model, x, n):
    with torch.no_grad():
        return (model.make_decision(x)[0] + 1) % n


def _judge(name, hip, ora, x, y, loss, fp, flag=0, hop=truth.HOP, forward=truth.default_forward, hip_call=None,
           layers=5, pattern_pass=None):
    """The engine's loss_grad on (x, y) judged against the truth; an utterance over a bound is re-judged against the fp64
    model run with the engine's own ReLU / max-pool pattern (read back right after the call, or after `pattern_pass`: the
    engine's pass of the model on the FeCo-compressed features, which the defended call does not leave behind)."""
    f32, f64 = fp
    if hip_call is None:
        dec, scores, lo, grad = hip.loss_grad(x.to(DEV), y.to(DEV), loss.spec(), flag=flag)
    else:
        dec, scores, lo, grad = hip_call()
    judged = truth.Side.of(scores, lo, grad)
    clipped = (f64.loss == 0) if loss.clip_max else None
    base = getattr(hip, "base_model", hip)

    def pattern_truth():  # (check calls it before anything else runs on the engine)
        if pattern_pass is not None:
            pattern_pass()
        acts = [base.read_activation(l, x.shape[0]).cpu().numpy() for l in range(1, layers + 1)]
        return truth.pattern_truths(_m64(ora), acts, x, y, loss, forward)
    rep = truth.check(judged, f32, f64, name, hop=hop, clipped=clipped, pattern_truth=pattern_truth)
    log("truth " + rep.line())
    rep.assert_ok()
    return rep, judged


_M64 = {}


def _m64(ora):
    import copy
    if id(ora) not in _M64:  # (the oracle is kept alive with its copy: its id cannot be reused)
        _M64[id(ora)] = (ora, copy.deepcopy(ora).double())
    return _M64[id(ora)][1]


# ------------------------------------------------------------------------------------------------------------ x-vector
@pytest.mark.parametrize("bits", [32, 64])
def test_xv_ce_benchmark_shape(xv_hip, xv_ora, bits):
    """64 x 3 s, cross-entropy: the benchmark's shape, both transform precisions of the MFCC."""
    x = _wav(64, T3, 101)
    y = _shifted(xv_ora, x, 10)
    lo = truth.Loss("ce")
    xv_hip.configure_frontend(bits)
    try:
        _judge("xv CE 64x3s float%d transforms" % bits, xv_hip, xv_ora, x, y, lo, _oracle("xv_ce_64", xv_ora, x, y, lo))
    finally:
        xv_hip.configure_frontend(32)


def test_xv_margin_csi_untargeted(xv_hip, xv_ora):
    """64 x 3 s, Margin CSI untargeted (clipped at 0): odd rows labelled off the decision clip to exactly 0."""
    x = _wav(64, T3, 102)
    with torch.no_grad():
        y = xv_ora.make_decision(x)[0]
    y[1::2] = (y[1::2] + 1) % 10
    lo = truth.Loss("margin", False, 0.0, "CSI", None, True)
    rep, _ = _judge("xv Margin CSI 64x3s", xv_hip, xv_ora, x, y, lo, _oracle("xv_mcsi", xv_ora, x, y, lo))
    assert rep.zero_loss >= 16


def _between(scores):
    """A threshold in the widest gap of the middle half of `scores`: no utterance within round-off of it."""
    s = np.sort(np.asarray(scores, np.float64))
    n = len(s)
    lo, hi = n // 4, 3 * n // 4
    i = lo + int(np.argmax(np.diff(s[lo:hi + 1])))
    return float((s[i] + s[i + 1]) / 2)


def test_xv_margin_sv_targeted_cw2_shape(xv_weights, dev):
    """32 x 3 s, Margin SV targeted with clip and threshold: the loss configs[2] (CW2) differentiates."""
    from oracle.xv_plda import XvPlda
    from speakerguard_amd.model.xv_plda import xv_plda
    w = dict(xv_weights)
    w["enroll"] = xv_weights["enroll"][3:4]
    ora = XvPlda(w)
    x = _wav(32, T3, 103)
    with torch.no_grad():
        s0 = ora.score(x)[:, 0]
    thr = _between(s0.numpy())
    ora.threshold = thr
    hip = xv_plda.from_weights(w, threshold=thr, device=dev, dither=0.0)
    y = torch.zeros(32, dtype=torch.int64)
    lo = truth.Loss("margin", True, 0.0, "SV", thr, True)
    rep, _ = _judge("xv Margin SV targeted 32x3s", hip, ora, x, y, lo, _oracle("xv_sv", ora, x, y, lo))
    assert 0 < rep.zero_loss < 32


def test_xv_margin_osi(xv_weights, xv_ora, dev):
    """16 x 3 s, Margin OSI untargeted with a threshold between the utterances' best scores."""
    from speakerguard_amd.model.xv_plda import xv_plda
    x = _wav(16, T3, 104)
    with torch.no_grad():
        sc = xv_ora.score(x)
    thr = _between(sc.max(1)[0].numpy())
    hip = xv_plda.from_weights(xv_weights, threshold=thr, device=dev, dither=0.0)
    y = sc.argmax(1)
    lo = truth.Loss("margin", False, 0.0, "OSI", thr, True)
    _judge("xv Margin OSI 16x3s", hip, xv_ora, x, y, lo, _oracle("xv_osi", xv_ora, x, y, lo))


@pytest.mark.parametrize("B,T", [(9, 52960), (5, 16123), (2, 192000)])
def test_xv_ragged_and_long(xv_hip, xv_ora, B, T):
    """Lengths that are not a multiple of the hop, and 12 s utterances where the 300-frame sliding CMVN is not the global
    mean."""
    x = _wav(B, T, 105 + B)
    y = _shifted(xv_ora, x, 10)
    lo = truth.Loss("ce")
    _judge("xv CE %dx%d" % (B, T), xv_hip, xv_ora, x, y, lo, _oracle(("xv_rag", B, T), xv_ora, x, y, lo))


@pytest.mark.parametrize("flag", [1, 2])
def test_xv_feature_level_inputs(xv_hip, xv_ora, flag):
    """64 utterances of features (flag 1: raw MFCC, flag 2: after CMVN), d loss / d features judged per frame."""
    x = _wav(64, T3, 110)
    with torch.no_grad():
        feats = xv_ora.compute_feat(x, flag=flag)
    y = _shifted(xv_ora, x, 10)
    lo = truth.Loss("ce")
    fwd = lambda m, f: m(f, flag=flag)
    _judge("xv CE 64 features flag %d" % flag, xv_hip, xv_ora, feats, y, lo,
           _oracle(("xv_flag", flag), xv_ora, feats, y, lo, fwd), flag=flag, hop=feats.shape[2], forward=fwd)


def test_xv_feco_flag1(xv_hip, xv_ora, dev):
    """FeCo at flag 1 (raw MFCC), 16 x 3 s: the oracle compresses with the device's cluster ids."""
    from oracle import feco
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    x = _wav(16, T3, 111)
    d = FeCoDefense(0.5)
    dm = defended_model(xv_hip, defense=[(1, d)])
    ids = d.fwd(xv_hip.compute_feat(x.to(dev), flag=1))[1][0].cpu().numpy()
    k = ids.shape[1] // 2

    def fwd(m, xin):
        f = m.compute_feat(xin, flag=1)
        return m(torch.stack([feco.compress_from_ids(f[b], ids[b], k, force=True) for b in range(f.shape[0])]), flag=1)
    with torch.no_grad():
        y = (fwd(xv_ora, x).argmax(1) + 1) % 10
    lo = truth.Loss("ce")
    _judge("xv + FeCo@1 CE 16x3s", dm, xv_ora, x, y, lo, _oracle("xv_feco", xv_ora, x, y, lo, fwd), forward=fwd,
           hip_call=lambda: dm.loss_grad(x.to(dev), y.to(dev), lo.spec()),
           pattern_pass=lambda: xv_hip.loss_grad(d.fwd(xv_hip.compute_feat(x.to(dev), flag=1))[0], y.to(dev), lo.spec(), flag=1))


# ------------------------------------------------------------------------------------------------------------ AudioNet
@pytest.mark.parametrize("bits", [32, 64])
def test_audionet_ce_64(an_hip, an_ora, bits):
    x = _wav(64, T3, 121)
    y = _shifted(an_ora, x, 251)
    lo = truth.Loss("ce")
    an_hip.configure_frontend(bits)
    try:
        _judge("AudioNet CE 64x3s float%d transforms" % bits, an_hip, an_ora, x, y, lo,
               _oracle("an_ce_64", an_ora, x, y, lo), layers=8)
    finally:
        an_hip.configure_frontend()


def test_audionet_margin_64(an_hip, an_ora):
    x = _wav(64, T3, 122)
    with torch.no_grad():
        y = an_ora.make_decision(x)[0]
    y[1::2] = (y[1::2] + 1) % 251
    lo = truth.Loss("margin", False, 0.0, "CSI", None, True)
    rep, _ = _judge("AudioNet Margin CSI 64x3s", an_hip, an_ora, x, y, lo, _oracle("an_m_64", an_ora, x, y, lo), layers=8)
    assert rep.zero_loss >= 16


def test_audionet_ce_256_large_batch_plan(an_hip, an_ora, dev):
    """256 x 3 s: the planner's large-batch plan (overlap-add inside the log-mel adjoint), asserted from the stage trace."""
    x = _wav(256, T3, 123)
    y = _shifted(an_ora, x, 251)
    lo = truth.Loss("ce")
    an_hip.configure_frontend()
    out = {}
    tags = [t for t, _ in an_hip.trace_stages(
        lambda: out.__setitem__("r", an_hip.loss_grad(x.to(dev), y.to(dev), lo.spec())), max_records=128)]
    assert "an_logmel_bwd" in tags and "an_overlap_add" not in tags, tags
    _judge("AudioNet CE 256x3s (fused overlap-add plan)", an_hip, an_ora, x, y, lo, _oracle("an_256", an_ora, x, y, lo),
           hip_call=lambda: out["r"], layers=8)


def test_audionet_ragged(an_hip, an_ora):
    x = _wav(5, 20011, 124)
    y = _shifted(an_ora, x, 251)
    lo = truth.Loss("ce")
    _judge("AudioNet CE 5x20011", an_hip, an_ora, x, y, lo, _oracle("an_rag", an_ora, x, y, lo), layers=8)


def _an_feco_setup(an_hip, dev, seed):
    from oracle import feco
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    x = _wav(64, T3, seed)
    d = FeCoDefense(0.5)
    dm = defended_model(an_hip, defense=[(1, d)])
    ids = d.fwd(an_hip.compute_feat(x.to(dev), flag=1))[1][0].cpu().numpy()
    k = ids.shape[1] // 2

    def fwd(m, xin):
        f = m.compute_feat(xin, flag=1)
        return m(torch.stack([feco.compress_from_ids(f[b], ids[b], k, force=True) for b in range(f.shape[0])]), flag=1)
    return x, d, dm, fwd


def test_audionet_feco_64(an_hip, an_ora, dev):
    """FeCo-defended AudioNet (configs[3]'s model), 64 x 3 s, deterministic initialisation, the oracle compressing with the
    device's cluster ids."""
    x, d, dm, fwd = _an_feco_setup(an_hip, dev, 125)
    with torch.no_grad():
        y = (fwd(an_ora, x).argmax(1) + 1) % 251
    lo = truth.Loss("ce")
    _judge("AudioNet + FeCo@1 CE 64x3s", dm, an_ora, x, y, lo, _oracle("an_feco", an_ora, x, y, lo, fwd), forward=fwd,
           hip_call=lambda: dm.loss_grad(x.to(dev), y.to(dev), lo.spec()), layers=8,
           pattern_pass=lambda: an_hip.loss_grad(d.fwd(an_hip.compute_feat(x.to(dev), flag=1))[0], y.to(dev), lo.spec(), flag=1))


# ------------------------------------------------------------------------------------------------------------ one step
def _one_step(name, x, x_adv, step, f32, f64):
    got = truth.one_step_signs(x_adv.cpu().numpy(), x.numpy(), step)
    yard = np.sign(f32.grad).reshape(got.shape)
    frac, dec_bad, yfrac, ydec_bad = truth.one_step(got, yard, f64.grad)
    log("truth one-step %s: sign step vs fp64 -- differing fraction %.3e (fp32 oracle %.3e), on decided entries %d (%d)"
        % (name, frac, yfrac, dec_bad, ydec_bad))
    assert dec_bad == 0 and frac <= 2 * yfrac, (frac, yfrac, dec_bad)


def test_one_step_xv_configs1_shape(xv_hip, xv_ora, dev):
    """One step of the fused device loop bench.py times (configs[1]: 64 x 3 s, eps 0.002, step 0.0004): the step taken
    is step * sign(g64) on every decided entry, and differs overall at most twice as often as the fp32 oracle's own step."""
    x = _wav(64, T3, 101)
    y = _shifted(xv_ora, x, 10)
    lo = truth.Loss("ce")
    f32, f64 = _oracle("xv_ce_64", xv_ora, x, y, lo)
    xd = x.to(dev)
    lower, upper = torch.clamp(xd - 0.002, min=-1), torch.clamp(xd + 0.002, max=1)
    x_adv = xv_hip.pgd_run(xd, y.to(dev), lower, upper, lo.spec(), 0.0004, 1, 1)[0]
    _one_step("xv PGD configs[1] 64x3s", x, x_adv, 0.0004, f32, f64)


def test_one_step_audionet_feco(an_hip, an_ora, dev):
    x, d, dm, fwd = _an_feco_setup(an_hip, dev, 125)
    with torch.no_grad():
        y = (fwd(an_ora, x).argmax(1) + 1) % 251
    lo = truth.Loss("ce")
    f32, f64 = _oracle("an_feco", an_ora, x, y, lo, fwd)
    xd = x.to(dev)
    lower, upper = torch.clamp(xd - 0.002, min=-1), torch.clamp(xd + 0.002, max=1)
    x_adv = an_hip.pgd_run_feco(xd, y.to(dev), lower, upper, lo.spec(), 0.0004, 1, 1, d)[0]
    _one_step("AudioNet + FeCo@1 PGD 64x3s", x, x_adv, 0.0004, f32, f64)
