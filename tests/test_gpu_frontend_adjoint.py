"""Both front-end adjoints against float64, edge samples included: d loss / d raw MFCC -> d loss / d wav (mfcc_bwd_kernel,
frames_to_wave_kernel<1|4>) and d loss / d log-mel -> d loss / d wav (an_logmel_bwd_kernel, an_frames_to_wave_kernel,
an_frames_to_wave4_kernel, an_logmel_bwd_ola_kernel + an_edge_to_wave_kernel) -- the stage tests/test_gpu_backward_stages.py
stops short of, and its AudioNet counterpart.

Both stages are linear in the cotangent: the float64 vector-Jacobian product of the oracle's front end is an exact truth for
any cotangent (tests/frontend_adjoint.py; tests/test_frontend_adjoint_power.py proves the truths, the restated index
arithmetic and the power of the judgement on the CPU).  Every case is judged by ``frontend_adjoint.judge``, over every sample
of every row: per row utt_error <= C max(yard, FLOOR_UTT), block_error over 160 samples <= C max(yard, FLOOR_BLOCK), no decided
sign wrong, exactly 0 wherever the truth is exactly 0 -- ``truth.POLICY``'s constants, the yard the same VJP in float32 torch.

x-vector, stand-alone ``sg_xv_mfcc_backward`` (recomputed forward), fft_bits 32 and 64: T in {5040, 5041, 5119, 5199, 5200, 16123}
at B = 2; (16 | 15, 48000), the two sides of the switch to four samples per thread; (152, 5056) and (150, 5121), as large with both
edges inside a 32-frame utterance and 4864 frames > 512 blocks x 8 waves (the grid-stride loop and its prefetch iterate), the
second with T % 4 != 0; each with a dense cotangent and with the one-hot family (frames 0, 1, F / 2, F - 2, F - 1 x columns 0, 1,
29, one row each on one shared waveform); int16-scale input; explicit dither at a quarter of the signal's RMS.
Short lengths, T in {400, 401, 479, 480, 559, 560, 719, 720}: the forward in the x-vector context under test_mfcc_matches_oracle's
bound, the adjoint through ``iv_plda(white_box=True).frontend_backward`` (a context holding only the i-vector model accepts
T >= 400; 24 columns).  Refusals just below each accepted length (399, 5039, 1023, 3680): an argument error, output untouched.
x-vector in situ: ``loss_grad`` on waveforms at (2, 5040), (5, 16123), (16, 48000); the call's gradient against the VJP at its own
dfeats_raw readback (the cached-spectrum kernel the pass runs).
AudioNet, stand-alone ``sg_an_logmel_backward``, fft_bits 32 and 64, forward recomputed / reused / reused with the fused
overlap-add forced on: T in {3681, 3684, 3840, 3841, 4096, 16000, 16001} at B = 2 and (5, 4096); dense and one-hot (frames 0, 5, 6,
F - 6, F - 5, F - 1 x bins 0, 31).  In situ: ``loss_grad`` at flag 0 on (3, 16000) with the fused overlap-add forced on (12 runs:
the halo is exercised) and off, against the VJP whose cotangent is the engine's flag-1 gradient on its own compute_feat(x)
-- the same numbers: one forward kernel serves both entries (the spectrum cache only adds stores) and both flags hand the
same features to the same ``an_net_step`` plan --, and the two forms bit for bit.

Measured on an MI355X (profiles/frontend_adjoint_parity.txt, profiles/frontend_adjoint_gpu_durations.txt): 185 cases in 4.1 s, the
slowest 0.8 s (the first case, which loads the model), every other under 0.4 s.  Error per row / worst 160-sample block against
the float64 truth, bounds 6.1e-5 / 4.9e-4 throughout (the float32 yard is under the policy's floors in every case: at most
1.3e-5 / 1.0e-4): sg_xv_mfcc_backward at fft_bits 32 at most 6.0e-6 / 6.6e-5 (yard 1.1e-5 / 6.6e-5), at 64: 5.1e-6 / 4.0e-5; through the
i-vector route at the short lengths 5.3e-6 / 8.7e-6 and 4.8e-6 / 8.1e-6; in situ 6.4e-6 / 6.5e-5 (yard 1.0e-5 / 1.0e-4);
sg_an_logmel_backward at 32: 4.7e-6 / 2.7e-5 (yard 4.8e-6 / 3.4e-5), at 64: 2.6e-6 / 4.4e-5; in situ 1.1e-6 / 3.3e-6 (yard 1.3e-6 / 4.0e-6),
the two overlap-add forms the same bits.  The case nearest its bound is at 0.13 of it ((15, 48000) one-hot, and (16, 48000) in
situ); no decided sign differs and no sample is nonzero where the truth is exactly zero (up to 762 440 such samples in a
case).  The short-length forward is within 6.6e-5 of the oracle (bound 5e-3 + 1e-4 |value|).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_adjoint as fa
import truth
from conftest import log

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CE = truth.Loss("ce")
SENTINEL = -7.25


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _judged(what, got, yard, g64):
    got = got.detach().cpu().numpy().reshape(g64.shape)
    fails, line, _ = fa.judge(got, yard, g64)
    log("front-end adjoint, %s: %s%s" % (what, line, "; FAILED %s" % fails[:6] if fails else ""))
    assert np.abs(g64).max() > 0, "an all-zero gradient pins nothing"
    assert not fails, (fails[:8], line)


# ------------------------------------------------------------------------------------------------------ x-vector, stand-alone
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.XV_CASES, ids=fa.case_id)
def test_mfcc_adjoint_stand_alone_against_float64(xv, c, bits):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    xv.configure_frontend(bits)
    try:
        noise = _dev(i["noise"])
        _, saved = xv._mfcc(_dev(i["x"]), dither_noise=noise)
        got = xv.frontend_backward(saved, _dev(i["cot"]))
    finally:
        xv.configure_frontend(32)
    V = 4 if c.T % 4 == 0 and i["x"].shape[0] * c.T >= fa.QUAD_MIN else 1
    _judged("sg_xv_mfcc_backward %s fft_bits=%d (rows %d, %d per thread)" % (fa.case_id(c), bits, i["x"].shape[0], V), got, yard, g64)


# ------------------------------------------------------------------------------------------------------ short lengths
@pytest.mark.parametrize("T", fa.XV_SHORT)
def test_mfcc_forward_at_the_short_lengths(xv, T):
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(3, T, seed=5))
    got = xv.compute_feat(x.to(DEV), flag=1).cpu()
    want = kaldi_mfcc.mfcc_batch(x * 32768.0)
    assert got.shape == want.shape == (3, fa.xv_num_frames(T), 30)
    log("front-end adjoint, sg_xv_mfcc forward T=%d: max abs err %.3e (values up to %.1f)" % (T, (got - want).abs().max().item(), want.abs().max().item()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, atol=5e-3)  # the bound of test_mfcc_matches_oracle


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.IV_CASES, ids=fa.case_id)
def test_mfcc_adjoint_at_the_short_lengths_through_the_i_vector_route(iv, c, bits):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    iv.ctx.call("sg_xv_configure", bits)
    try:
        feats, saved = iv.frontend_forward(_dev(i["x"]))
        assert feats.shape == i["cot"].shape
        got = iv.frontend_backward(saved, _dev(i["cot"]))
    finally:
        iv.ctx.call("sg_xv_configure", 32)
    _judged("iv_plda.frontend_backward %s fft_bits=%d (rows %d)" % (fa.case_id(c), bits, i["x"].shape[0]), got, yard, g64)


def _refused(ctx, name, out, *args):
    from speakerguard_amd import _native as N
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    with pytest.raises(N.NativeError, match=r"\(code 1\)"):  # SG_ERR_ARG
        ctx.call(name, *args)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "%s wrote to its output before refusing" % name


def test_refusals_just_below_each_accepted_length(xv, an):
    from speakerguard_amd import _native as N
    p = N._ptr
    scale = torch.ones(1, device=DEV)
    dz = xv._dither(None, 0)
    x = torch.full((2, 1, 5039), 0.1, device=DEV)
    feats = torch.empty(2, fa.xv_num_frames(399), 30, device=DEV)
    _refused(xv.ctx, "sg_xv_mfcc", feats, p(x), 2, 399, p(scale), C.byref(dz), p(feats), xv._stream())
    grad, cot = torch.empty(2, 1, 5039, device=DEV), torch.ones(2, fa.xv_num_frames(5039), 30, device=DEV)
    _refused(xv.ctx, "sg_xv_mfcc_backward", grad, p(x), 2, 5039, p(scale), C.byref(dz), p(cot), p(grad), xv._stream())
    grad, cot = torch.empty(2, 1, 3680, device=DEV), torch.ones(2, fa.an_num_frames(3680), 32, device=DEV)
    for reuse in (0, 1):
        _refused(an.ctx, "sg_an_logmel_backward", grad, p(x), 2, 3680, p(cot), p(grad), reuse, an._stream())
    # sg_an_logmel: 1024 samples are one STFT frame; a context with a model loaded also asks for the model's 24 frames, so
    # the first accepted length is pinned on a bare context, against the oracle under test_logmel_matches_oracle's bound
    from oracle import audionet as oan
    from speakerguard_amd import synth
    bare = N.Context(DEV.index or 0)
    try:
        feats = torch.empty(2, fa.an_num_frames(1024), 32, device=DEV)
        _refused(bare, "sg_an_logmel", feats, p(x), 2, 1023, p(feats), an._stream())
        _refused(an.ctx, "sg_an_logmel", feats, p(x), 2, 1023, p(feats), an._stream())
        w = torch.from_numpy(synth.make_waveforms(2, 1024, seed=6))
        wd = w.to(DEV)
        bare.call("sg_an_logmel", p(wd), 2, 1024, p(feats), an._stream())
        torch.cuda.synchronize()
        want = oan.preprocess(w.squeeze(1)).transpose(1, 2)
        np.testing.assert_allclose(feats.cpu().numpy(), want.numpy(), rtol=0, atol=8e-4)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------------ x-vector, in situ
@pytest.mark.parametrize("B,T", [(2, 5040), (5, 16123), (16, 48000)], ids=lambda v: str(v))
def test_mfcc_adjoint_in_situ_against_float64_at_its_own_dfeats_raw(xv, B, T):
    from speakerguard_amd import synth
    x = synth.make_waveforms(B, T, seed=2000 + B + T)
    _, _, _, grad = xv.loss_grad(_dev(x), torch.arange(B) % 10, CE.spec(), flag=0)
    cot = xv.read_gradient("dfeats_raw").cpu().numpy()
    assert cot.shape == (B, fa.xv_num_frames(T), 30) and np.abs(cot).max() > 0
    yard, g64 = (fa.xv_vjp(x, cot, d) for d in (torch.float32, torch.float64))
    _judged("sg_xv_loss_grad flag 0 in situ B=%d T=%d (cached spectrum) at its own dfeats_raw" % (B, T), grad, yard, g64)


# ------------------------------------------------------------------------------------------------------ AudioNet
AN_MODES = ("recompute", "reuse", "reuse_fused")


@pytest.mark.parametrize("mode", AN_MODES)
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c", fa.AN_CASES, ids=fa.case_id)
def test_logmel_adjoint_stand_alone_against_float64(an, c, bits, mode):
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
    _judged("sg_an_logmel_backward %s fft_bits=%d %s (rows %d)" % (fa.case_id(c), bits, mode, x.shape[0]), grad, yard, g64)


def test_logmel_adjoint_in_situ_fused_and_separate_against_float64(an):
    """flag 0 against the VJP at the engine's own flag-1 gradient on its own features (the same numbers, see the module
    docstring), once with the overlap-add inside the adjoint (3 x 12 runs) and once with the separate pair; then bit for bit"""
    from speakerguard_amd import synth
    B, T = 3, 16000
    assert fa.an_ola_slices(B, fa.an_num_frames(T)) == 12
    x = synth.make_waveforms(B, T, seed=2000 + B + T)
    xd, y = _dev(x), torch.arange(B) % 10
    got = {}
    try:
        for ola in (True, False):
            an.configure_frontend(32, None, ola)
            _, _, _, cot = an.loss_grad(an.compute_feat(xd), y, CE.spec(), flag=1)
            _, _, _, g = an.loss_grad(xd, y, CE.spec(), flag=0)
            got[ola] = (g.cpu().numpy(), cot.cpu().numpy())
    finally:
        an.configure_frontend(32, None, None)
    assert np.array_equal(got[True][1].view(np.uint32), got[False][1].view(np.uint32)) and np.abs(got[True][1]).max() > 0
    cot = got[True][1]
    yard, g64 = (fa.an_vjp(x, cot, d) for d in (torch.float32, torch.float64))
    for ola in (True, False):
        _judged("sg_an_loss_grad flag 0 in situ B=%d T=%d, overlap-add %s" % (B, T, "inside the adjoint, 12 runs" if ola else "as the separate pair"),
                torch.from_numpy(got[ola][0]), yard, g64)
    assert np.array_equal(got[True][0].view(np.uint32), got[False][0].view(np.uint32)), "the two overlap-add forms differ"
