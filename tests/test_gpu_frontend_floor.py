"""Both front ends at their log floors on digital silence, forward and backward: ``logf(fmaxf(., kEps))`` on the mel energies
and on the frame energy of k_mfcc.hip with the ``> kEps`` gates of k_mfcc_bodies.h, ``10 log10f(fmaxf(., 1e-16f))`` of
an_logmel_fwd_kernel with the ``> 1e-16f`` gate of an_frame_backward -- branches no speech-like waveform of the suite reaches,
and the ones every frame of a zero-padded utterance takes.

Inputs: ``frontend_adjoint.FLOOR_CASES`` -- spans of exact zeros written over a synthetic utterance (``gap``, ``lead``, ``trail``,
``edges``, ``all``), a hard clip at +1.0 that DC removal turns into exact zeros (``plateau``, x-vector) and speech that stops on
the one tap where the periodic Hann window is 0 (``window0``, AudioNet); row r of a batch moves every boundary by 53 r samples.
tests/test_frontend_floor_power.py proves on the CPU the condition these inputs meet (every pre-log value of the oracle is
exactly 0, in float32 and float64 alike, or at least 2**10 x the floor: the float64 VJP through ``torch.clamp`` is an exact
truth), that the judgements below reject an ungated backward, a wrong floor constant and a missing floor, and what exact
silence cannot tell apart.  Tonal, band-limited and constant-but-nonzero audio is out of scope: there the side of the floor a
bin falls on is decided by float32 round-off in the reference itself, and no kernel can be right or wrong about it.

Forward: ``compute_feat`` of every case against the float32 oracle under the suite's own bounds, unchanged (rtol 1e-4, atol 5e-3
of test_mfcc_matches_oracle; atol 8e-4 of test_logmel_matches_oracle), every value finite; exactly, within a configuration
(front end x fft_bits), every silent frame of every row and layout carries the same feature bits.  Logged, not asserted: the
distance of a silent frame's c0 from log(eps32) and of its log-mel from -160 dB in float32 spacings, and the distance of the
float32 oracle itself from the float64 one.
Adjoint, stand-alone: the entries and modes of tests/test_gpu_frontend_adjoint.py on the floor cases, judged by
``frontend_adjoint.judge`` against ``frontend_adjoint.truths``, nothing altered; the all-silent row exactly zero on its own.
In situ: x-vector ``loss_grad`` at flag 0 on (3, 16123) with rows ``edges``, all-silent and plain -- finite scores and loss, the
gradient against the VJP at the call's own dfeats_raw, the silent row exactly 0, each row bit-equal to the row sent alone;
PGD: after one step ``adv == x`` at every sample whose truth gradient is exactly 0 (sign(0) = 0); at max_iter=3 device loop and step
loop bit for bit, and ``adv == x`` at every sample that no step's truth gradient reaches -- a silent sample next to speech moves
at the first step (a frame that holds speech covers it), which ends the silence of the frames that cover IT, so the zero set
of the first gradient shrinks by up to a frame's reach per step (``_never_reached``: the float64 VJP at worst-case iterates).  Ragged x-vector: lengths (16000, 9999, 8000) with a gap inside each
row's own length and 0.9 in the padding -- rows bit-equal to their solo runs, forward (``make_decision``) and backward, exact
zeros behind each length.  (No entry reads the raw MFCC of a ragged pass back, so the ragged forward is pinned through the
scores it feeds, bit for bit.)  AudioNet: flag 0 on (3, 16000) with the same three rows, fused overlap-add forced on and off,
each judged against the VJP at the engine's own flag-1 gradient, the two forms bit for bit; PGD through sg_an_pgd_run.

Measured on an MI355X (profiles/frontend_floor_parity.txt, profiles/frontend_floor_gpu_durations.txt): 181 cases in 3.7 s, the slowest
0.7 s.  Every case holds exact-zero truth samples (400 .. 239 445) and no judged value among them is nonzero; the case nearest its
bound is at 0.62 of it (AudioNet (2, 4096) ``lead``, per row 3.8e-5 where the float32 yard is 3.1e-5), (16, 48000) ``edges`` at 0.30.
A silent frame's c0 is one float32 spacing from log(eps32) and its log-mel exactly -160 dB; all silent frames of a
configuration carry the same bits.  No kernel had to change.
"""
import numpy as np
import pytest
import torch

import frontend_adjoint as fa
import truth
from conftest import log

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CE = truth.Loss("ce")


@pytest.fixture(scope="module")
def xv(xv_weights):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=DEV, dither=0.0)


@pytest.fixture(scope="module")
def iv():
    from speakerguard_amd import synth
    from speakerguard_amd.model.iv_plda import iv_plda
    return iv_plda.from_weights(synth.make_iv_weights(), device=DEV, dither=0.0, white_box=True)


@pytest.fixture(scope="module")
def an():
    from speakerguard_amd import synth
    from speakerguard_amd.model.audionet_csine import audionet_csine
    return audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _judged(what, got, yard, g64, zero_rows=()):
    got = got.detach().cpu().numpy().reshape(g64.shape)
    fails, line, _ = fa.judge(got, yard, g64)
    log("front-end floor, %s: %s%s" % (what, line, "; FAILED %s" % fails[:6] if fails else ""))
    live = [r for r in range(len(g64)) if r not in zero_rows]
    assert np.abs(g64[live]).max() > 0, "an all-zero gradient pins nothing"
    assert (g64 == 0).sum() > 0, "no sample of the truth is exactly zero: the floor is not reached"
    for r in zero_rows:
        assert not g64[r].any() and not got[r].any(), "the silent row %d is not exactly zero" % r
    assert not fails, (fails[:8], line)
    return got


# ------------------------------------------------------------------------------------------------------ forward
_SILENT_BITS = {}  # configuration -> the feature bits of the first silent frame it produced


def _forward_checked(what, config, c, got):
    """the suite's forward bounds against the float32 oracle; finite; every silent frame the same bits within `config`"""
    got = got.detach().cpu().numpy()
    want32, want64 = fa.forward_oracle(c), fa.forward_oracle(c, torch.float64)
    assert got.shape == want32.shape and got.dtype == np.float32
    silent = sorted(fa.floor_report(c)["silent"])
    assert silent
    if fa.inputs(c)["shared"]:
        silent = [(r, f) for r in range(len(got)) for _, f in silent]
    rows = np.stack([got[r, f] for r, f in silent])
    first = _SILENT_BITS.setdefault(config, rows[0].copy())
    differ = int((_bits(rows) != _bits(first)[None]).any(1).sum())
    ulp = lambda v, ref: float(np.abs(v.astype(np.float64) - float(ref)).max() / np.spacing(np.float32(abs(ref))))
    if c.model == "an":
        off = "log-mel of a silent frame %.9g, %.2f float32 spacings from -160 dB" % (rows[0, 0], ulp(rows, -160.0))
    else:
        ref = np.log(np.float32(fa.XV_FLOOR))
        off = "c0 of a silent frame %.9g, %.2f float32 spacings from log(eps32) = %.9g" % (rows[0, 0], ulp(rows[:, 0], ref), ref)
    log("front-end floor, %s %s: max abs err %.3e against the float32 oracle, %.3e against the float64 one (the float32 oracle from the float64 "
        "one: %.3e); %d silent frames, %d of them with other bits than the first of %s; %s" % (
            what, fa.case_id(c), np.abs(got - want32).max(), np.abs(got - want64).max(), np.abs(want32 - want64).max(), len(silent), differ,
            config, off))
    assert np.isfinite(got).all(), "%d non-finite features" % (~np.isfinite(got)).sum()
    assert differ == 0, "%d silent frames carry other bits than the first silent frame of %s" % (differ, config)
    if c.model == "an":
        np.testing.assert_allclose(got, want32, rtol=0, atol=8e-4)   # the bound of test_logmel_matches_oracle
    else:
        np.testing.assert_allclose(got, want32, rtol=1e-4, atol=5e-3)  # the bound of test_mfcc_matches_oracle


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.XV_FLOOR_CASES, ids=fa.case_id)
def test_mfcc_forward_at_the_floor(xv, c, bits):
    xv.configure_frontend(bits)
    try:
        got = xv.compute_feat(_dev(fa.inputs(c)["x"]), flag=1)
    finally:
        xv.configure_frontend(32)
    _forward_checked("sg_xv_mfcc fft_bits=%d" % bits, ("mfcc", bits), c, got)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.IV_FLOOR_CASES, ids=fa.case_id)
def test_mfcc_forward_at_the_floor_through_the_i_vector_route(iv, c, bits):
    iv.ctx.call("sg_xv_configure", bits)
    try:
        got, _ = iv.frontend_forward(_dev(fa.inputs(c)["x"]))
    finally:
        iv.ctx.call("sg_xv_configure", 32)
    _forward_checked("iv_plda.frontend_forward fft_bits=%d" % bits, ("iv mfcc", bits), c, got)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.AN_FLOOR_CASES, ids=fa.case_id)
def test_logmel_forward_at_the_floor(an, c, bits):
    an.configure_frontend(bits, None, None)
    try:
        got = an.compute_feat(_dev(fa.inputs(c)["x"]))
    finally:
        an.configure_frontend(32, None, None)
    _forward_checked("sg_an_logmel fft_bits=%d" % bits, ("logmel", bits), c, got)


# ------------------------------------------------------------------------------------------------------ adjoint, stand-alone
def _zero_rows(c):
    return (0,) if c.variant == "all" else ()


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.XV_FLOOR_CASES, ids=fa.case_id)
def test_mfcc_adjoint_at_the_floor_against_float64(xv, c, bits):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    xv.configure_frontend(bits)
    try:
        _, saved = xv._mfcc(_dev(i["x"]))
        got = xv.frontend_backward(saved, _dev(i["cot"]))
    finally:
        xv.configure_frontend(32)
    V = 4 if c.T % 4 == 0 and i["x"].shape[0] * c.T >= fa.QUAD_MIN else 1
    _judged("sg_xv_mfcc_backward %s fft_bits=%d (rows %d, %d per thread)" % (fa.case_id(c), bits, i["x"].shape[0], V), got, yard, g64, _zero_rows(c))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.IV_FLOOR_CASES, ids=fa.case_id)
def test_mfcc_adjoint_at_the_floor_through_the_i_vector_route(iv, c, bits):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    iv.ctx.call("sg_xv_configure", bits)
    try:
        feats, saved = iv.frontend_forward(_dev(i["x"]))
        assert feats.shape == i["cot"].shape
        got = iv.frontend_backward(saved, _dev(i["cot"]))
    finally:
        iv.ctx.call("sg_xv_configure", 32)
    _judged("iv_plda.frontend_backward %s fft_bits=%d" % (fa.case_id(c), bits), got, yard, g64)


AN_MODES = ("recompute", "reuse", "reuse_fused")


@pytest.mark.parametrize("mode", AN_MODES)
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.AN_FLOOR_CASES, ids=fa.case_id)
def test_logmel_adjoint_at_the_floor_against_float64(an, c, bits, mode):
    from speakerguard_amd import _native as N
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    x, cot = _dev(i["x"]), _dev(i["cot"])
    grad = torch.empty_like(x)
    an.configure_frontend(bits, None, True if mode == "reuse_fused" else None)
    try:
        if mode != "recompute":
            assert an.compute_feat(x).shape == cot.shape  # leaves the mel energies of this x in the workspace
        an.ctx.call("sg_an_logmel_backward", N._ptr(x), x.shape[0], c.T, N._ptr(cot), N._ptr(grad), int(mode != "recompute"), an._stream())
        torch.cuda.synchronize()
    finally:
        an.configure_frontend(32, None, None)
    _judged("sg_an_logmel_backward %s fft_bits=%d %s" % (fa.case_id(c), bits, mode), grad, yard, g64, _zero_rows(c))


# ------------------------------------------------------------------------------------------------------ in situ
def _three_rows(T, seed):
    """(3, 1, T): row 0 ``edges`` (the zero-padded utterance), row 1 all silent, row 2 plain speech"""
    from speakerguard_amd import synth
    x = synth.make_waveforms(3, T, seed=seed)
    fa.apply_layout(x[:1], "edges")
    x[1] = 0.0
    return x


def _never_reached(vjp, x, cot, steps, step=0.0004):
    """the samples whose float64 truth gradient is exactly 0 at EVERY one of `steps` sign steps.  A silent sample next to speech
    has a nonzero gradient (a frame that holds speech covers it) and moves at the first step; the silent frames that cover it
    are silent no longer, so each step the silence loses up to a frame's reach at each of its ends.  Worst case, by the
    truth: every sample reached so far counts as nonzero from then on (an iterate with more zeros has no fewer silent
    frames).  Which samples the float64 VJP leaves exactly 0 does not depend on the cotangent as long as it is dense."""
    xk = np.array(x, np.float32)
    still = np.ones(xk.shape, bool)
    for _ in range(steps):
        reached = vjp(xk, cot).reshape(xk.shape) != 0
        still &= ~reached
        xk = np.where(reached & (xk == 0), np.float32(step), xk)
    return still.reshape(len(x), -1)


def _pgd_both_loops(model, vjp, x, y, cot, g64, monkeypatch, what):
    from speakerguard_amd.attack.PGD import PGD
    kw = dict(epsilon=0.002, step_size=0.0004, batch_size=3, verbose=0)
    x0 = x.cpu().numpy().reshape(g64.shape)
    # one step: no sample moves whose truth gradient is exactly 0 (sign(0) = 0), every silent frame stays silent
    one, _ = PGD(model, max_iter=1, **kw).attack(x, y)
    one = one.cpu().numpy().reshape(g64.shape)
    zero = g64 == 0
    assert zero[1].all() and zero.sum() > zero.shape[1] and (one[zero] == x0[zero]).all(), "%d samples with an exactly zero gradient moved in one step" % (
        one[zero] != x0[zero]).sum()
    atk = PGD(model, max_iter=3, **kw)
    assert atk._device_route(3) == ("pgd_run", ())
    adv_dev, succ_dev = atk.attack(x, y)
    stepper = PGD(model, max_iter=3, **kw)
    monkeypatch.setattr(stepper, "_device_route", lambda n: None)
    adv_step, succ_step = stepper.attack(x, y)
    assert torch.equal(adv_dev, adv_step) and succ_dev == succ_step, "device loop and step loop differ"
    adv = adv_dev.cpu().numpy().reshape(g64.shape)
    still = _never_reached(vjp, x0.reshape(len(x0), 1, -1), cot, 3)
    assert not (still & ~zero).any()
    moved = int((adv[still] != x0[still]).sum())
    log("front-end floor, %s PGD: after 1 step 0 of the %d samples with an exactly zero truth gradient moved (%d of the other %d did); after 3 steps "
        "%d of the %d samples no step's truth gradient reaches moved (%d of the other %d did)" % (
            what, zero.sum(), (one[~zero] != x0[~zero]).sum(), (~zero).sum(), moved, still.sum(), (adv[~still] != x0[~still]).sum(), (~still).sum()))
    assert np.isfinite(adv).all() and still[1].all()  # (AudioNet's 800-sample frames reach across row 0's silence in three steps)
    assert moved == 0, "%d samples with an exactly zero gradient at every step moved" % moved
    assert (adv[0] != x0[0]).any() and (adv[2] != x0[2]).any()


@pytest.fixture(scope="module")
def xv_in_situ(xv):
    B, T = 3, 16123
    x = _three_rows(T, 2300)
    xd, y = _dev(x), torch.arange(B) % 10
    out = [t.clone() for t in xv.loss_grad(xd, y, CE.spec(), flag=0)]
    cot = xv.read_gradient("dfeats_raw").cpu().numpy()
    assert cot.shape == (B, fa.xv_num_frames(T), 30) and np.abs(cot).max() > 0
    yard, g64 = (fa.xv_vjp(x, cot, d) for d in (torch.float32, torch.float64))
    return x, xd, y, out, yard, g64, cot


def test_mfcc_adjoint_in_situ_on_padded_silent_and_plain_rows(xv, xv_in_situ):
    x, xd, y, (dec, scores, loss, grad), yard, g64, _ = xv_in_situ
    assert torch.isfinite(scores).all() and torch.isfinite(loss).all()
    _judged("sg_xv_loss_grad flag 0 in situ (3, 16123) rows edges / silent / plain at its own dfeats_raw", grad, yard, g64, zero_rows=(1,))
    for b in range(3):
        d1, s1, l1, g1 = xv.loss_grad(xd[b:b + 1].contiguous(), y[b:b + 1], CE.spec(), flag=0)
        assert torch.equal(dec[b:b + 1], d1) and torch.equal(scores[b:b + 1], s1) and torch.equal(loss[b:b + 1], l1), b
        assert torch.equal(grad[b:b + 1], g1), (b, float((grad[b:b + 1] - g1).abs().max()))


def test_pgd_on_the_x_vector_keeps_silence_silent(xv, xv_in_situ, monkeypatch):
    x, xd, y, _, _, g64, cot = xv_in_situ
    _pgd_both_loops(xv, fa.xv_vjp, xd, y.to(DEV), cot, g64, monkeypatch, "x-vector")


def test_ragged_x_vector_batch_with_a_gap_in_every_row(xv):
    from test_gpu_xv_ragged import assert_rows_equal_solo, make_batch, solo, spec_of
    lengths = (16000, 9999, 8000)
    x, lens, y = make_batch(lengths, 2400, DEV, fill=0.9)
    for b, t_b in enumerate(lengths):
        a = t_b // 3 + fa.ROW_SHIFT * b
        assert a + 2000 < t_b - 400
        x[b, 0, a:a + 2000] = 0.0
    assert float(x[1, 0, -1]) == pytest.approx(0.9)
    out = [t.clone() for t in xv.loss_grad(x, y, spec_of("Entropy"), lengths=lens)]
    assert torch.isfinite(out[1]).all() and torch.isfinite(out[2]).all() and torch.isfinite(out[3]).all()
    assert_rows_equal_solo(out, solo(xv, x, lens, y, "Entropy", "floor gap"), lens)
    dec, scores = xv.make_decision(x, lengths=lens)  # the ragged forward
    for b, t_b in enumerate(lengths):
        d1, s1 = xv.make_decision(x[b:b + 1, :, :t_b].contiguous())
        assert torch.equal(dec[b:b + 1], d1) and torch.equal(scores[b:b + 1], s1), b
        a = t_b // 3 + fa.ROW_SHIFT * b
        inside = out[3][b, 0, a + 400:a + 1600]  # samples only silent frames cover
        assert not inside.any(), (b, "gradient inside the gap")


@pytest.fixture(scope="module")
def an_in_situ(an):
    B, T = 3, 16000
    assert fa.an_ola_slices(B, fa.an_num_frames(T)) == 12
    x = _three_rows(T, 2500)
    xd, y = _dev(x), torch.arange(B) % 10
    got = {}
    try:
        for ola in (True, False):
            an.configure_frontend(32, None, ola)
            _, _, _, cot = an.loss_grad(an.compute_feat(xd), y, CE.spec(), flag=1)
            _, scores, loss, g = an.loss_grad(xd, y, CE.spec(), flag=0)
            assert torch.isfinite(scores).all() and torch.isfinite(loss).all()
            got[ola] = (g.cpu().numpy(), cot.cpu().numpy())
    finally:
        an.configure_frontend(32, None, None)
    cot = got[True][1]
    yard, g64 = (fa.an_vjp(x, cot, d) for d in (torch.float32, torch.float64))
    return x, xd, y, got, yard, g64, cot


def test_logmel_adjoint_in_situ_on_padded_silent_and_plain_rows(an_in_situ):
    x, xd, y, got, yard, g64, _ = an_in_situ
    assert np.array_equal(_bits(got[True][1]), _bits(got[False][1])) and np.abs(got[True][1]).max() > 0
    for ola in (True, False):
        _judged("sg_an_loss_grad flag 0 in situ (3, 16000) rows edges / silent / plain, overlap-add %s" % (
            "inside the adjoint, 12 runs" if ola else "as the separate pair"), torch.from_numpy(got[ola][0]), yard, g64, zero_rows=(1,))
    assert np.array_equal(_bits(got[True][0]), _bits(got[False][0])), "the two overlap-add forms differ"


def test_pgd_on_audionet_keeps_silence_silent(an, an_in_situ, monkeypatch):
    x, xd, y, _, _, g64, cot = an_in_situ
    _pgd_both_loops(an, fa.an_vjp, xd, y.to(DEV), cot, g64, monkeypatch, "AudioNet")
