"""The loss stage on the device (loss_device.h) against the reference, at ties and at every class count.

1. The serial form (sg_loss_eval through attack.utils.loss_dscores) on the fixture tests/golden/loss_ref.npz -- the
   reference's own SEC4SR_CrossEntropy / SEC4SR_MarginLoss on designed score tables: the margin loss bit for bit, the
   cross entropy within the reference's own float32 error against float64.
2. Every other device form -- the x-vector tail's one-wave (S <= 64) and 1024-thread block (S > 64) forms, the AudioNet
   head's block form in the separate launch, inside the fused backward and in the one-launch form -- equals the serial form
   inside real passes, with enrolled speakers / classes duplicated so that the scores tie exactly.  d loss / d scores of a
   form is compared through its gradient: loss_grad(x, y, ScoreVJP(dsc_serial)) runs the same backward on the serial
   form's d loss / d scores.
3. Whole-model truth (tests/truth.py) at class counts other than the default.
4. Labels the loss stage cannot take are refused on the host before any launch.
"""
import types

import numpy as np
import pytest
import torch

import truth
from conftest import load_golden, log

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def ref():
    return load_golden("loss_ref.npz")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from speakerguard_amd import _native as N
    return N.Context(0)


def _spec(cfg, thr, conf):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    kind, task, targeted, clip = cfg
    return SEC4SR_CrossEntropy() if kind == "ce" else SEC4SR_MarginLoss(targeted, conf, task, thr, clip)


def _tables(g):
    for S in g["meta"]["sizes"]:
        for v, (thr, conf) in enumerate(g["meta"]["variants"]):
            yield "S%d_v%d" % (S, v), S, thr, conf


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rows(g, tag, rows):
    return ", ".join("%d:%s" % (r, g["meta"]["rows"][tag][r]) for r in rows[:6])


# ------------------------------------------------------------------------------------------------ 1. serial form vs reference
def test_serial_form_margin_equals_the_reference_bit_for_bit(ref, ctx):
    """Decisions, loss and d loss / d scores of every margin configuration equal the reference's bits, except for the sign
    of a zero, which is recorded (parity log) rather than asserted: the reference's CSI imposter rows get ONE
    0 * sum(scores of all imposter rows) (attack/utils.py:97), so their zero loss takes the sign of the batch's sum while
    the device writes +0 per row; and a gradient entry that is zero in both may carry either sign (the clip multiplies by
    k = 0, autograd accumulates +0 and -0 terms)."""
    from speakerguard_amd.attack.utils import loss_dscores
    n_cases, signed_zero, zero_sign = 0, 0, {}
    for tag, S, thr, conf in _tables(ref):
        holder = types.SimpleNamespace(ctx=ctx, threshold=thr)
        sc = torch.from_numpy(ref[tag + "_scores"]).to(DEV)
        lab = ref[tag + "_labels"]
        y = torch.from_numpy(lab).to(DEV)
        for name, cfg in ref["meta"]["configs"].items():
            if cfg[0] != "margin" or (cfg[1] == "SV" and S != 1):
                continue
            dec, loss, dsc = (t.cpu().numpy() for t in loss_dscores(holder, sc, y, _spec(cfg, thr, conf)))
            want_l, want_g = ref["%s_%s_loss" % (tag, name)], ref["%s_%s_grad" % (tag, name)]
            where = "%s %s" % (tag, name)
            assert np.array_equal(dec, ref[tag + "_dec"]), (where, _rows(ref, tag, np.nonzero(dec != ref[tag + "_dec"])[0]))
            diff = _bits(dsc) != _bits(want_g)
            bad = np.nonzero((diff & ~((dsc == 0) & (want_g == 0))).any(1))[0]
            assert len(bad) == 0, "%s d loss / d scores differs on rows %s" % (where, _rows(ref, tag, bad))
            if diff.any():
                zero_sign[name] = zero_sign.get(name, 0) + int(diff.sum())
            imp_csi = (lab == -1) & (cfg[1] == "CSI")
            diff = _bits(loss) != _bits(want_l)
            bad = np.nonzero(diff & ~imp_csi & ~((loss == 0) & (want_l == 0)))[0]
            assert len(bad) == 0, "%s loss differs on rows %s: %s vs %s" % (where, _rows(ref, tag, bad), loss[bad], want_l[bad])
            if (diff & ~imp_csi).any():
                zero_sign[name + " loss"] = zero_sign.get(name + " loss", 0) + int((diff & ~imp_csi).sum())
            assert (_bits(loss[imp_csi]) == 0).all() and (want_l[imp_csi] == 0).all(), where
            signed_zero += int((_bits(want_l[imp_csi]) != 0).sum())
            n_cases += 1
    log("loss stage, serial form: %d margin tables equal the reference bit for bit up to the sign of zero (%d CSI imposter "
        "losses are -0 in the reference, +0 on the device; other zeros of opposite sign, by configuration: %s)"
        % (n_cases, signed_zero, zero_sign))


def _in_order_sum_bound(s32):
    """Per row, a bound on what the device's in-order float32 sum so = sum_{s != argmax} exp(s - max) (loss_device.h
    sum_in_order_except) adds to the error of lse = log(1 + so): recursive summation errs by at most u * (sum of the
    partial sums' magnitudes) (Higham, Accuracy and Stability, 4.2), each expf term by about u of itself; u = eps / 2,
    taken as eps.  torch reduces pairwise, so where many comparable terms meet -- 249 equal ones at S = 251 -- the device's
    sum carries more round-off than the reference's (measured 1.6e-6 against 5.8e-8 on the loss); where one or a few
    terms dominate, the usual case, the bound is a few eps."""
    s64 = s32.astype(np.float64)
    ja = s64.argmax(1)
    t = np.exp(s64 - s64.max(1, keepdims=True))
    t[np.arange(len(t)), ja] = 0.0
    part = np.cumsum(t, 1)
    so = part[:, -1]
    return EPS32 * (part.sum(1) + so) / (1.0 + so)


def test_serial_form_cross_entropy_against_the_reference(ref, ctx):
    """Decisions exact; d/ds_y exactly 0 wherever the reference's is; per row, the error of loss and gradient against a
    float64 evaluation at most 2x the reference's float32 error plus a floor: 4 float32 ulps of the row's scale (loss:
    1 + |loss|, gradient: 1) and the bound of the device's in-order sum (_in_order_sum_bound; times max |d/ds| for the
    gradient).  The worst ratio of error to allowance is logged per class count.  Imposter rows: a zero loss and an exactly
    zero gradient."""
    import torch.nn.functional as F
    from speakerguard_amd.attack.utils import loss_dscores
    worst, worst_err = {}, {}
    for tag, S, thr, conf in _tables(ref):
        holder = types.SimpleNamespace(ctx=ctx, threshold=thr)
        sc32, lab = ref[tag + "_scores"], ref[tag + "_labels"]
        dec, loss, dsc = (t.cpu().numpy() for t in loss_dscores(holder, torch.from_numpy(sc32).to(DEV),
                                                                torch.from_numpy(lab).to(DEV), _spec(("ce", "CSI", False, False), thr, conf)))
        want_l, want_g = ref[tag + "_ce_loss"], ref[tag + "_ce_grad"]
        assert np.array_equal(dec, ref[tag + "_dec"]), tag
        imp = lab == -1
        assert (loss[imp] == 0).all() and (_bits(dsc[imp]) == 0).all(), tag
        keep = ~imp
        y = lab[keep]
        s64 = torch.from_numpy(sc32[keep]).double().requires_grad_(True)
        l64 = F.cross_entropy(s64, torch.from_numpy(y), reduction="none")
        l64.backward(torch.ones_like(l64))
        l64, g64 = l64.detach().numpy(), s64.grad.numpy()
        sat = want_g[keep, y] == 0
        assert (dsc[keep, y][sat] == 0).all(), (tag, "d/ds_y not exactly 0 where the reference saturates")
        serial = _in_order_sum_bound(sc32[keep])
        for what, got, want, truth64, floor in (("loss", loss[keep], want_l[keep], l64, 4 * EPS32 * (1 + np.abs(l64)) + serial),
                                                ("grad", dsc[keep], want_g[keep], g64, 4 * EPS32 + serial * np.abs(g64).max(1))):
            e_dev = np.abs(got.astype(np.float64) - truth64).reshape(len(truth64), -1).max(1)
            e_ref = np.abs(want.astype(np.float64) - truth64).reshape(len(truth64), -1).max(1)
            allow = 2 * e_ref + floor
            bad = np.nonzero(e_dev > allow)[0]
            assert len(bad) == 0, "%s CE %s rows %s: device error %s, reference %s, allowed %s" % (
                tag, what, bad[:6], e_dev[bad][:6], e_ref[bad][:6], allow[bad][:6])
            k = "S=%d %s" % (S, what)
            worst[k] = max(worst.get(k, 0.0), float((e_dev / allow).max()))
            worst_err[k] = max(worst_err.get(k, 0.0), float(e_dev.max()))
    log("loss stage, serial form: cross entropy within 2x the reference's float32 error against float64 + floor; worst "
        "error / allowance and worst error per class count: %s" % ", ".join(
            "%s %.3f %.1e" % (k, worst[k], worst_err[k]) for k in sorted(worst, key=lambda k: (int(k.split()[0][2:]), k))))


# ------------------------------------------------------------------------------------------------ 2. every form == serial form
def _branches(S, thr):
    """Every loss branch the stage has: CE, Margin CSI / OSI targeted or not, clipped or not (and SV at S = 1)."""
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    out = [("CE", SEC4SR_CrossEntropy())]
    tasks = ("CSI", "OSI", "SV") if S == 1 else ("CSI", "OSI")
    for task in tasks:
        for tg in (False, True):
            for clip in (False, True):
                out.append(("Margin %s t%d c%d" % (task, tg, clip), SEC4SR_MarginLoss(tg, 0.25, task, thr, clip)))
    return out


def _labels(S, B, top, pairs):
    """Rows: the first of the tied pair at the argmax, the second, an imposter, and both members of another duplicated pair
    (ties between `real` and the maximum, between `other` candidates, and below the maximum)."""
    if S == 1:
        return torch.tensor(([0, -1] * B)[:B], device=DEV)
    a, b = top
    c, d = next((p for p in pairs if p != top), ((b + 1) % S, (b + 2) % S))
    return torch.tensor(([a, b, -1, c, d] * B)[:B], device=DEV)


def _form_equals_serial(model, x, S, thr, top, pairs, name, sv_labels=None):
    """Every loss branch: decisions and loss of the form equal the serial form's, and so does the gradient the form's
    d loss / d scores gives.  `top`: the duplicated pair every utterance has as its maximum (the first index must win)."""
    from speakerguard_amd.attack.utils import ScoreVJP, loss_dscores
    dec0, sc0 = model.make_decision(x)
    for a, b in pairs:  # the duplicated speakers / classes really tie
        assert torch.equal(sc0[:, a], sc0[:, b]), (name, a, b)
    if top is not None:
        assert (dec0 == top[0]).all(), (name, "the tied pair is not every utterance's decision", top, dec0)
    n = 0
    for bname, spec in _branches(S, thr):
        y = sv_labels if spec.task == "SV" else _labels(S, x.shape[0], top, pairs)
        dec, scores, loss, grad = model.loss_grad(x, y, spec)
        dec_s, loss_s, dsc_s = loss_dscores(model, scores, y, spec)
        where = "%s %s" % (name, bname)
        assert torch.equal(dec, dec_s), (where, dec, dec_s)
        assert torch.equal(loss.view(torch.int32), loss_s.view(torch.int32)), (where, loss, loss_s)
        g_serial = model.loss_grad(x, y, ScoreVJP(dsc_s))[3]
        assert torch.equal(grad, g_serial), (where, (grad - g_serial).abs().max().item())
        n += 1
    return n, dec0


def _pgd_fused_equals_stepwise(model, x, thr, name):
    """sg_*_pgd_run over 2 steps == loss_grad + pgd_update stepwise; the success flags are dec != y (dec == y targeted)."""
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    dec0 = model.make_decision(x)[0]
    lower, upper = torch.clamp(x - 0.002, min=-1), torch.clamp(x + 0.002, max=1)
    for spec, sign, targeted in ((SEC4SR_CrossEntropy(), 1, False), (SEC4SR_MarginLoss(True, 0.0, "OSI", thr, True), -1, True)):
        y = dec0.clone() if not targeted else (dec0.clamp(min=0) + 1) % model.num_spks
        xa, success, dec, scores, loss, _, _ = model.pgd_run(x, y, lower, upper, spec, 0.0004, 2, sign)
        xs = x.clone()
        for _ in range(2):
            g = model.loss_grad(xs, y, spec)[3]
            model.pgd_update(xs, g, lower, upper, 0.0004, sign)
        d2, s2, l2, _ = model.loss_grad(xs, y, spec, want_grad=False)
        assert torch.equal(xa, xs) and torch.equal(dec, d2) and torch.equal(scores, s2) and torch.equal(loss, l2), name
        want = (dec == y) if targeted else (dec != y)
        assert torch.equal(success.bool(), want), (name, success, dec, y)


XV_GRID = [(1, 200), (32, 200), (33, 200), (64, 200), (65, 200), (251, 200), (1024, 200), (32, 128), (33, 128)]


def _dup_pairs(S):
    """Duplicated speakers / classes: within one wave or thread group (0, 1), (3, 40), (S - 2, S - 1), and far apart
    (5, 900): at 1024 threads 5 and 900 are different waves, at 256 / 512 threads (AudioNet) too (900 is thread 132 / 388)."""
    return [p for p in ((0, 1), (3, 40), (5, 900), (S - 2, S - 1)) if 0 <= p[0] < p[1] < S]


SV_LABELS = [0, -1, 0, -1, 0]


@pytest.mark.parametrize("S,D", XV_GRID)
def test_xv_tail_forms_equal_the_serial_form(S, D):
    """x-vector tail: the one-wave form (S <= 64), the 1024-thread block form (S > 64); D = 128 at S = 32 / 33 crosses the
    enrolled-in-LDS limit (S D <= 4096).  Each duplicated pair in turn is made every utterance's maximum: both members
    enrol k^-1 times the mean of the utterances' own embeddings (k = psi / (psi + 1): the PLDA mean of a speaker with
    that enrolment is the test embedding itself), which out-scores the random speakers by ~200."""
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    w = synth.make_xv_weights(seed=1, D=D, n_spk=S, calibrated=False)
    pairs = _dup_pairs(S)
    e0 = w["enroll"].copy()
    for a, b in pairs:
        e0[b] = e0[a]
    x = torch.from_numpy(synth.make_waveforms(5, 12000, seed=S + D)).to(DEV)
    probe = xv_plda.from_weights(dict(w, enroll=e0), device=DEV, dither=0.0)
    psi = np.asarray(w["plda_psi"], np.float32)
    star = (probe.embedding(x).mean(0).cpu().numpy() / (psi / (psi + 1.0))).astype(np.float32)
    n, m = 0, None
    for top in (pairs or [None]):
        e = e0.copy()
        if top is not None:
            e[top[0]] = e[top[1]] = star
        w1 = dict(w, enroll=e)
        thr = float(xv_plda.from_weights(w1, device=DEV, dither=0.0).make_decision(x)[1][0].median())  # every row accepted
        m = xv_plda.from_weights(w1, threshold=thr, device=DEV, dither=0.0)
        passes, _ = _form_equals_serial(m, x, S, thr, top, pairs, "xv S=%d D=%d top %s" % (S, D, top),
                                        torch.tensor(SV_LABELS, device=DEV))
        n += passes
    if S == 251:
        _pgd_fused_equals_stepwise(m, x, thr, "xv S=%d" % S)
    log("loss stage, x-vector tail S=%d D=%d: each of %s tied at the maximum in turn, %d loss-branch passes equal the serial "
        "form" % (S, D, pairs, n))


# the launch forms of the AudioNet head (SG_TUNE knobs, sg_api_audionet.hip) and the stage tags that show which one ran
AN_MODES = {
    "separate an_tail": ({"SG_AN_HEAD": "0"}, {"an_tail": 1, "an_cnn_bwd": 1, "an_cnn_fwdbwd": 0}),
    "head in the fused backward": ({}, {"an_tail": 0, "an_cnn_fwd": 1, "an_cnn_bwd": 1, "an_cnn_fwdbwd": 0}),
    "one launch": ({"SG_AN_ONE": "1", "SG_AN_SLICES": "1"}, {"an_tail": 0, "an_cnn_fwd": 0, "an_cnn_bwd": 0, "an_cnn_fwdbwd": 1}),
}


@pytest.mark.parametrize("S", [1, 10, 32, 33, 1024])
def test_audionet_head_forms_equal_the_serial_form(S, monkeypatch):
    """AudioNet head: the block form (256 / 512 threads; its serial branch at S <= 32) in the separate an_tail launch,
    inside the fused backward and in the one-launch form -- the stage trace shows which ran.  Each duplicated pair in turn
    is every utterance's maximum (its bias raised by 1000)."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.model.audionet_csine import audionet_csine
    sd = synth.make_audionet_state_dict(seed=1, num_class=S)
    pairs = _dup_pairs(S)
    wt, bs0 = sd["fc.weight"].copy(), sd["fc.bias"].copy()
    for a, b in pairs:
        wt[b], bs0[b] = wt[a], bs0[a]
    x = torch.from_numpy(synth.make_waveforms(5, 16000, seed=70 + S)).to(DEV)
    for k in ("SG_AN_HEAD", "SG_AN_ONE", "SG_AN_SLICES"):
        monkeypatch.delenv(k, raising=False)
    n = 0
    for top in (pairs or [None]):
        bs = bs0.copy()
        if top is not None:
            bs[top[0]] += 1000.0
            bs[top[1]] = bs[top[0]]
        m = audionet_csine.from_weights(dict(sd, **{"fc.weight": wt, "fc.bias": bs}), device=DEV)
        thr = float(m.make_decision(x)[1][1].median())  # (the loss's threshold; the model itself never rejects: CSI-NE)
        y_any = torch.zeros(5, dtype=torch.int64, device=DEV)
        for mode, (env, want_tags) in AN_MODES.items():
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            tags = [t for t, _ in m.trace_stages(lambda: m.loss_grad(x, y_any, SEC4SR_CrossEntropy()), max_records=256)]
            for t, c in want_tags.items():
                assert tags.count(t) == c, (S, mode, t, tags)
            passes, _ = _form_equals_serial(m, x, S, thr, top, pairs, "audionet S=%d %s top %s" % (S, mode, top),
                                            torch.tensor(SV_LABELS, device=DEV))
            n += passes
            if S == 1024 and top == pairs[-1]:
                _pgd_fused_equals_stepwise(m, x, thr, "audionet S=%d %s" % (S, mode))
            for k in env:
                monkeypatch.delenv(k)
    log("loss stage, AudioNet head S=%d: each of %s tied at the maximum in turn, %d loss-branch passes over %d launch "
        "forms (stage trace checked) equal the serial form" % (S, pairs, n, len(AN_MODES)))


# ------------------------------------------------------------------------------------------------ 3. whole-model truth
def _truth_cases(hip, ora, S, name, seed):
    from test_gpu_truth import _judge, _shifted, _wav
    x = _wav(3, 24000, seed)
    y_ce = _shifted(ora, x, S)
    with torch.no_grad():
        y_m = ora.make_decision(x)[0]
    for lo, y in ((truth.Loss("ce"), y_ce), (truth.Loss("margin", False, 0.0, "CSI", None, True), y_m)):
        _judge("%s %r S=%d 3x1.5s" % (name, lo, S), hip, ora, x, y, lo, truth.evaluate(ora, x, y, lo))


def test_xv_truth_at_251_speakers():
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    w = synth.make_xv_weights(seed=0, D=200, n_spk=251, calibrated=False)
    _truth_cases(xv_plda.from_weights(w, device=DEV, dither=0.0), XvPlda(w), 251, "xv", 181)


@pytest.mark.parametrize("S", [10, 1024])
def test_audionet_truth_at_other_class_counts(S):
    from oracle.audionet import AudioNet
    from speakerguard_amd import synth
    from speakerguard_amd.model.audionet_csine import audionet_csine
    sd = synth.make_audionet_state_dict(seed=0, num_class=S)
    _truth_cases(audionet_csine.from_weights(sd, device=DEV), AudioNet(sd), S, "audionet", 190 + S)


# ------------------------------------------------------------------------------------------------ 4. labels refused
class _NoLaunch:
    """Stands in for a model's native context: any call is a launch that must not happen."""

    def call(self, *a, **kw):
        raise AssertionError("a native call was made with labels that should have been refused: %s" % (a[:1],))


def _refused(fn, row):
    with pytest.raises(ValueError, match="of row %d " % row):
        fn()


def test_out_of_range_labels_are_refused_before_any_launch(monkeypatch):
    """Every entry point that takes labels refuses CSI / OSI labels outside [-1, S), SV labels other than 0 / -1, and SV
    with more than one enrolled speaker -- on the host, before any native call (the context is replaced by one that fails
    the test if it is called)."""
    from speakerguard_amd import synth
    from speakerguard_amd.adaptive_attack.EOT import EOT
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss, loss_dscores
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.xv_plda import xv_plda
    xv = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=10), device=DEV, dither=0.0)
    an = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=10), device=DEV)
    x = torch.from_numpy(synth.make_waveforms(4, 16000, seed=9)).to(DEV)
    lower, upper = x - 0.002, x + 0.002
    ce, osi = SEC4SR_CrossEntropy(), SEC4SR_MarginLoss(False, 0.0, "OSI", 0.0, True)
    good = torch.tensor([0, 9, -1, 3], device=DEV)
    xv.loss_grad(x, good, ce)  # (accepted: the memo holds these labels now)
    for m in (xv, an):
        monkeypatch.setattr(m, "ctx", _NoLaunch())
        for bad, row in (([0, 10, -1, 3], 1), ([0, 1, 2, -2], 3), ([10, 0, 0, 0], 0)):
            y = torch.tensor(bad, device=DEV)
            for spec in (ce, osi):
                _refused(lambda: m.loss_grad(x, y, spec), row)
                _refused(lambda: m.pgd_run(x, y, lower, upper, spec, 0.0004, 3, 1), row)
                _refused(lambda: loss_dscores(m, torch.zeros(4, 10, device=DEV), y, spec), row)
                _refused(lambda: EOT(m, spec, 2, 2)(x, y), row)
                _refused(lambda: PGD(m, epsilon=0.002, max_iter=2, batch_size=4, verbose=0).attack(x, y), row)
        # SV: labels other than 0 / -1, and more than one enrolled speaker
        sv = SEC4SR_MarginLoss(True, 0.0, "SV", 0.0, True)
        with pytest.raises(ValueError, match="exactly one enrolled speaker"):
            m.loss_grad(x, torch.tensor([0, -1, 0, 0], device=DEV), sv)
    _refused(lambda: an.pgd_run_feco(x, torch.tensor([0, 0, 11, 0], device=DEV), lower, upper, ce, 0.0004, 2, 1,
                                     FeCoDefense(0.5)), 2)
    # labels changed in place after they were accepted are checked again
    good[2] = 10
    _refused(lambda: xv.loss_grad(x, good, ce), 2)
    xv1 = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=1, calibrated=False), device=DEV, dither=0.0)
    monkeypatch.setattr(xv1, "ctx", _NoLaunch())
    _refused(lambda: xv1.loss_grad(x, torch.tensor([0, -1, 1, 0], device=DEV), SEC4SR_MarginLoss(True, 0.0, "SV", 0.0, True)), 2)
    _refused(lambda: xv1.loss_grad(x, torch.tensor([0, -1, 0, 1], device=DEV), ce), 3)
