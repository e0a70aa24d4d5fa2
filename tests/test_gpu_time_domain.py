"""The time-domain defenses on the device (csrc/k_time_domain.hip, defense.time_domain): every case of the reference fixture
through the C-ABI against the fixture and the restatement (tests/time_domain_restate.py), adjoint identities, batch
independence, the keyed noise of AT, refusals, and the defenses inside defended_model under PGD."""
import ctypes as C

import numpy as np
import pytest
import torch

import time_domain_restate as R
from conftest import load_golden, log
from test_time_domain_restate import ULP, as_bound, as_f64, at_f64, bits, case_cot, case_x, cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
XV_T, AN_T = 5040, 3681  # the shortest waveforms the two models accept (32 MFCC frames / 24 log-mel frames)


@pytest.fixture(scope="module")
def ref():
    return load_golden("time_domain_ref.npz")


def _ctx():
    from speakerguard_amd.metric.metric import _context
    return _context(DEV)


def _spec(kind, param, seed=0, row_keys=(0, 0, 0), noise=None):
    from speakerguard_amd import _native as N
    d = N.WavDefense()
    d.kind, d.param, d.seed = N.SG_TD[kind], float(param), seed & R.MASK64
    d.index_base, d.row_base, d.rep_rows = row_keys
    d.noise_dev = None if noise is None else noise.data_ptr()
    return d


def _saved(kind, B, T):
    if kind == "MS":
        return torch.zeros(B, T, dtype=torch.int8, device=DEV)
    return torch.zeros(3, B, device=DEV) if kind == "AT" else None


def fwd(kind, param, x, raw=False, **kw):
    """x numpy (B,T) -> (out numpy, saved tensor) through sg_wav_defense_forward (QT: after sg_input_scale)"""
    from speakerguard_amd import _native as N
    ctx, s = _ctx(), N.current_stream_ptr(DEV)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    B, T = xd.shape
    noise = kw.pop("noise", None)
    nd = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(DEV)
    saved = _saved(kind, B, T)
    if kind == "QT":
        saved = torch.empty(1, device=DEV)
        ctx.call("sg_input_scale", N._ptr(xd), xd.numel(), N._ptr(saved), s)
    out = torch.full_like(xd, 7.0)
    spec = _spec(kind, param, noise=nd, **kw)
    rc = ctx.lib.sg_wav_defense_forward(ctx.handle, C.byref(spec), N._ptr(xd), B, T, N._ptr(out), N._ptr(saved), s)
    torch.cuda.synchronize()
    if raw:
        return rc
    ctx.check(rc, "sg_wav_defense_forward")
    return out.cpu().numpy(), (spec, xd, saved, nd)


def bwd(state, g):
    from speakerguard_amd import _native as N
    spec, xd, saved, nd = state
    gd = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(DEV)
    gx = torch.full_like(gd, 7.0)
    _ctx().call("sg_wav_defense_backward", C.byref(spec), N._ptr(xd), N._ptr(gd), N._ptr(saved), gd.shape[0], gd.shape[1],
                N._ptr(gx), N.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return gx.cpu().numpy()


# ---------------------------------------------------------------- the fixture through the C-ABI
def test_qt_and_bdr_bit_equal_to_the_reference(ref):
    for c in cases(ref, "QT", "BDR"):
        q = c["param"] if c["kind"] == "QT" else 2 ** (16 - c["param"])
        out, _ = fwd("QT", q, case_x(ref, c))
        assert np.array_equal(bits(out), bits(ref[c["tag"] + "_out"])), c["tag"]
    from speakerguard_amd.defense import BDR, QT
    x = torch.from_numpy(ref["x_T257"]).to(DEV)
    for shape in ((257,), (3, 257), (3, 1, 257)):
        xi = x[0] if len(shape) == 1 else x.view(shape)
        o, sv = QT(3).fwd(xi)
        want = ref["qt_q3_B3_T257_out"] if len(shape) > 1 else R.qt(ref["x_T257"][:1], 3)[0]
        assert o.shape == shape and np.array_equal(o.cpu().numpy().reshape(want.shape), want)
        g = torch.randn(shape, device=DEV)
        assert QT(3).bwd(sv, g) is g  # BPDA's identity: the cotangent itself, nothing launched
    x256 = torch.from_numpy(ref["x_T256"]).to(DEV)
    assert np.array_equal(BDR(8)(x256[:, None, :]).cpu().numpy()[:, 0], ref["bdr_p8_B3_T256_out"])
    assert np.array_equal(BDR(12)(x[:1]).cpu().numpy(), ref["bdr_p12_B1_T257_out"])


def test_ms_forward_bit_equal_and_gradient_equal_to_the_restatement(ref):
    for c in cases(ref, "MS"):
        k, x, g = c["param"], case_x(ref, c), case_cot(ref, c)
        out, st = fwd("MS", k, x)
        assert np.array_equal(bits(out), bits(ref[c["tag"] + "_out"])), c["tag"]
        r_out, r_sel = R.median_smooth(x, k)
        assert np.array_equal(st[2].cpu().numpy(), r_sel), c["tag"]
        gx = bwd(st, g)
        assert np.array_equal(bits(gx), bits(R.median_smooth_bwd(r_sel, g, k))), c["tag"]  # tie cases included
        if not c["ties"]:
            assert np.abs(gx.astype(np.float64) - ref[c["tag"] + "_grad"]).max() <= 2 * 2.0 ** -23 * float(np.abs(g).max()), c["tag"]


def test_as_bit_equal_to_the_fmaf_chain(ref):
    for c in cases(ref, "AS"):
        k, x, g = c["param"], case_x(ref, c), case_cot(ref, c)
        out, st = fwd("AS", k, x)
        assert np.array_equal(bits(out), bits(R.avg_smooth(x, k))), c["tag"]
        gx = bwd(st, g)
        assert np.array_equal(bits(gx), bits(R.avg_smooth(g, k))), c["tag"]
        assert np.abs(out - as_f64(x, k)).max() <= as_bound(k, x) and np.abs(gx - as_f64(g, k)).max() <= as_bound(k, g)


def test_at_with_given_noise_against_float64_and_restatement(ref):
    for c in cases(ref, "AT"):
        tag, x, g, noise, snr = c["tag"], case_x(ref, c), case_cot(ref, c), ref[c["tag"] + "_noise"], c["param"]
        out, st = fwd("AT", snr, x, noise=noise)
        gx = bwd(st, g)
        r_out, sigma, P = R.at_forward(x, noise, snr)
        assert np.array_equal(bits(out), bits(r_out)), tag
        assert np.array_equal(bits(st[2][0].cpu().numpy()), bits(sigma)) and np.array_equal(bits(st[2][1].cpu().numpy()), bits(P))
        assert np.array_equal(bits(gx), bits(R.at_backward(x, noise, g, sigma, P, snr))), tag
        out64, grad64 = at_f64(x, noise, snr, g)
        live = P != 0
        e_out, e_grad = np.abs(out - out64).max(), np.abs(gx[live] - grad64[live]).max()
        tol_out = 2 * np.abs(ref[tag + "_out"] - out64).max()
        tol_grad = 2 * np.abs(ref[tag + "_grad"][live] - grad64[live]).max()
        log("AT %s: out err %.3g (tol %.3g), grad err %.3g (tol %.3g)" % (tag, e_out, tol_out, e_grad, tol_grad))
        assert e_out <= tol_out and e_grad <= tol_grad, tag
        if not live.all():
            assert np.isfinite(gx).all() and np.array_equal(gx[~live], g[~live])


# ---------------------------------------------------------------- adjoint identities (float64 on the host, kernel outputs)
def test_adjoint_identities(ref):
    rs = np.random.RandomState(11)
    B, T = 3, 1031
    u, v = rs.randn(B, T).astype(np.float32), rs.randn(B, T).astype(np.float32)
    uv = float((np.abs(u).astype(np.float64) * np.abs(v)).sum())
    dot = lambda a, b: float((a.astype(np.float64) * b.astype(np.float64)).sum())  # noqa: E731
    for k in (3, 17):
        au, st = fwd("AS", k, u)
        av = bwd(st, v)
        assert abs(dot(au, v) - dot(u, av)) <= (k + 2) * ULP * uv, k
    x = ref["x_T4099"][:1, :T].repeat(3, 0) * np.float32([[1], [0.5], [0.25]])
    for k in (3, 5):
        out, st = fwd("MS", k, x)
        sel = st[2].cpu().numpy().astype(np.int64)
        src = np.arange(T)[None] + sel
        ok = (src >= 0) & (src < T)
        ju = np.where(ok, np.take_along_axis(u, np.clip(src, 0, T - 1), 1), 0)  # J_MS u: a selection (pad: zero)
        jtv = bwd(st, v)
        assert abs(dot(ju, v) - dot(u, jtv)) <= k * ULP * uv, k
    # AT with fixed noise: J u = u + n (x . u) / (T snr sigma), from the kernel's own sigma
    n = rs.randn(B, T).astype(np.float32)
    out, st = fwd("AT", 25, x, noise=n)
    sigma = st[2][0].cpu().numpy().astype(np.float64)
    ju = u + n * ((x.astype(np.float64) * u).sum(1) / (T * 10 ** 2.5 * sigma))[:, None]
    jtv = bwd(st, v)
    # a handful of roundings per value (the fmaf, the tree's ~12 levels count once per term, coef's three) on a Jacobian
    # whose second term is at most max|n| max|x| / (snr sigma) times the identity's weight
    bound = 8 * ULP * uv * (1 + float(np.abs(n).max() * np.abs(x).max()) / (10 ** 2.5 * sigma.min()))
    assert abs(dot(ju, v) - dot(u, jtv)) <= bound


# ---------------------------------------------------------------- batch independence, keyed noise
def test_rows_do_not_depend_on_the_batch(ref):
    x, g = ref["x_T257"], ref["cot_T257"]
    for kind, param in (("QT", 3), ("AS", 5), ("MS", 5), ("AT", 25)):
        kw = dict(seed=77, row_keys=(40, 0, 0)) if kind == "AT" else {}
        whole, st = fwd(kind, param, x, **kw)
        gw = bwd(st, g)
        for b in range(3):
            kb = dict(seed=77, row_keys=(40 + b, 0, 0)) if kind == "AT" else {}
            one, s1 = fwd(kind, param, x[b:b + 1], **kb)
            assert np.array_equal(bits(one[0]), bits(whole[b])), (kind, b)
            assert np.array_equal(bits(bwd(s1, g[b:b + 1])[0]), bits(gw[b])), (kind, b)
    # AT, generated noise: 2 EOT repeats of 3 rows in one call == the same rows cut at row 4 (row_base / rep_rows)
    x6, g6 = np.concatenate([x, x]), np.concatenate([g, -g])
    whole, st = fwd("AT", 25, x6, seed=77, row_keys=(40, 0, 3))
    gw = bwd(st, g6)
    assert np.array_equal(whole[:3], fwd("AT", 25, x, seed=77, row_keys=(40, 0, 0))[0]) and not np.array_equal(whole[:3], whole[3:])
    for lo, hi in ((0, 4), (4, 6)):
        part, sp = fwd("AT", 25, x6[lo:hi], seed=77, row_keys=(40, lo, 3))
        assert np.array_equal(bits(part), bits(whole[lo:hi])) and np.array_equal(bits(bwd(sp, g6[lo:hi])), bits(gw[lo:hi]))
    rep1, _ = fwd("AT", 25, x, seed=(77 + R.REPEAT_STRIDE) & R.MASK64, row_keys=(40, 0, 0))
    assert np.array_equal(bits(rep1), bits(whole[3:]))


def test_at_generated_noise_is_the_documented_stream(ref):
    """out - x over sigma recovers the draws: Philox words restated exactly, logf / cosf to library accuracy"""
    T = 4099
    x = np.full((2, T), 0.5, np.float32)
    out, st = fwd("AT", 25, x, seed=0xABCDEF0123456789, row_keys=((1 << 32) + 5, 0, 0))
    sigma = st[2][0].cpu().numpy()
    want = R.at_noise(0xABCDEF0123456789, (1 << 32) + 5, 0, 0, 2, T)
    got = (out.astype(np.float64) - 0.5) / sigma[:, None]
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()) + 2 * ULP / sigma.min()
    assert abs(want.mean()) < 0.05 and abs(want.std() - 1) < 0.05
    # the class: fresh draws per call, reproducible per (seed, call), backward regenerates the same noise
    from speakerguard_amd.defense import AT
    xt = torch.from_numpy(x).to(DEV)
    a, b = AT(25, seed=1), AT(25, seed=1)
    o1, s1 = a.fwd(xt)
    o2, _ = a.fwd(xt)
    assert torch.equal(o1, b.fwd(xt)[0]) and not torch.equal(o1, o2) and not torch.equal(o1, AT(25, seed=2)(xt))
    g = torch.randn_like(xt)
    n1 = ((o1 - xt) / s1[2][0][:, None]).double()
    want_g = g.double() + xt.double() / (T * 10 ** 2.5 * s1[2][0].double()[:, None]) * (g.double() * n1).sum(1, keepdim=True)
    assert (a.bwd(s1, g).double() - want_g).abs().max() <= 1e-5


def test_refusals():
    x = np.zeros((2, 300), np.float32)
    for kind, param in (("AS", 4), ("AS", 33), ("AS", 0), ("AS", 3.5), ("MS", 2), ("MS", 33), ("MS", -1), ("QT", 0), ("QT", -2),
                        ("QT", float("inf")), ("AT", float("nan"))):
        assert fwd(kind, param, x, raw=True) == 1, (kind, param)
    from speakerguard_amd import _native as N
    ctx = _ctx()
    bad = _spec("AS", 3)
    bad.kind = 9
    xd = torch.zeros(2, 300, device=DEV)
    s = N.current_stream_ptr(DEV)
    assert ctx.lib.sg_wav_defense_forward(ctx.handle, C.byref(bad), N._ptr(xd), 2, 300, N._ptr(xd), None, s) == 1
    assert b"unknown kind" in ctx.lib.sg_last_error(ctx.handle)
    ms = _spec("MS", 3)
    assert ctx.lib.sg_wav_defense_forward(ctx.handle, C.byref(ms), N._ptr(xd), 2, 300, N._ptr(xd), None, s) == 1  # no saved
    assert ctx.lib.sg_wav_defense_forward(ctx.handle, C.byref(ms), N._ptr(xd), 0, 300, N._ptr(xd), None, s) == 1
    assert ctx.lib.sg_wav_defense_backward(ctx.handle, C.byref(_spec("AT", 25)), None, N._ptr(xd), N._ptr(xd), 2, 300, N._ptr(xd), s) == 1
    from speakerguard_amd.defense import AS, MS
    for cls in (AS, MS):
        with pytest.raises(ValueError):
            cls(4)(xd)
    with pytest.raises(NotImplementedError):
        AS(3)(torch.zeros(2, 2, 300, device=DEV))
    with pytest.raises(N.NativeError):
        AS(3)(torch.zeros(2, 300))


# ---------------------------------------------------------------- through the product
def _qt_torch(audio, param=128, bits=16, same_size=True):
    """time_domain.py:10-42 restated with torch (what a user of the parent commit wraps in BPDA)"""
    scale = bool(0.9 * audio.max() <= 1 and 0.9 * audio.min() >= -1)
    a = audio * 32768.0 if scale else audio
    a = torch.round(a / param) * param
    return a / 32768.0 if scale else a


def _ms_torch(audio, param=3, same_size=True):
    pad = (param - 1) // 2
    roll = torch.nn.functional.pad(audio.squeeze(1), (pad, pad), mode="constant", value=0.).unfold(-1, param, 1)
    return torch.median(roll, -1)[0].view(audio.shape)


def _models():
    from speakerguard_amd import synth
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.xv_plda import xv_plda
    return (("xv_plda", lambda: xv_plda.from_weights(synth.make_xv_weights(), device=DEV, dither=0.0), XV_T),
            ("audionet", lambda: audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV), AN_T))


@pytest.mark.parametrize("which", [0, 1], ids=["xv_plda", "audionet"])
def test_qt_and_ms_inside_defended_model(which):
    from speakerguard_amd import synth
    from speakerguard_amd.adaptive_attack.BPDA import BPDA
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense import MS, QT
    from speakerguard_amd.model.defended_model import defended_model
    name, make, T = _models()[which]
    base = make()
    x = torch.from_numpy(synth.make_waveforms(2, T, seed=3)).to(DEV)
    y = torch.tensor([1, 2], device=DEV)
    ce = SEC4SR_CrossEntropy(reduction='none', task='CSI')
    got = defended_model(base, [(0, QT())]).loss_grad(x, y, ce)
    want = defended_model(base, [(0, BPDA(_qt_torch))]).loss_grad(x, y, ce)
    for a, b in zip(got, want):
        assert torch.equal(a, b), name
    # MS: exact forward; the gradient through the defense alone, on the cotangent the model returned
    d = MS()
    nat, tor = defended_model(base, [(0, d)]), defended_model(base, [(0, BPDA(_ms_torch, _ms_torch))])
    (dn, sn), (dt, st) = nat.make_decision(x), tor.make_decision(x)
    assert torch.equal(dn, dt) and torch.equal(sn, st), name
    out, saved = d.fwd(x)
    g0 = base.loss_grad(out, y, ce)[3]
    xin = x.clone().requires_grad_(True)
    gt = torch.autograd.grad(_ms_torch(xin), xin, g0)[0]
    gn = d.bwd(saved, g0)
    assert gn.shape == x.shape and float((gn - gt).abs().max()) <= 2 * 2.0 ** -23 * float(g0.abs().max()), name
    assert torch.equal(nat.loss_grad(x, y, ce)[3], gn)


@pytest.mark.parametrize("which", [0, 1], ids=["xv_plda", "audionet"])
def test_pgd_eot_against_at(which):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AT
    from speakerguard_amd.model.defended_model import defended_model
    name, make, T = _models()[which]
    x = torch.from_numpy(synth.make_waveforms(2, T, seed=3)).to(DEV)
    kw = dict(task="CSI", epsilon=0.002, step_size=0.0004, max_iter=3, batch_size=2, EOT_size=2, EOT_batch_size=2, verbose=0)

    base = make()
    y = base.make_decision(x)[0]

    def run(seed):
        base._noise_epoch = 0  # a fresh model's bookkeeping: attack() calls so far (the keys depend on it by design)
        return PGD(defended_model(base, [(0, AT(25, seed=seed))]), **kw).attack(x, y)[0]

    a1, a2, a3 = run(1), run(1), run(2)
    assert torch.equal(a1, a2) and not torch.equal(a1, a3), name
    assert float((a1 - x).abs().max()) <= 0.002 + 1e-7 and not torch.equal(a1, x)
    # the same attack as a hand-written step loop over loss_grad / pgd_update
    dm = defended_model(base, [(0, AT(25, seed=1))])
    atk = PGD(dm, **kw)
    base._noise_epoch = 0
    base.begin_attack()
    base.begin_batch(0, 1)  # chunk at utterance 0; PGD tags its batches with the restart number (0) + 1
    xa = x.clone()
    lower, upper = torch.clamp(x - 0.002, min=-1).contiguous(), torch.clamp(x + 0.002, max=1).contiguous()
    for _ in range(3):
        base._rep_rows = 2
        try:
            g = dm.loss_grad(xa.repeat(2, 1, 1), y.repeat(2), atk.loss, want_grad=True)[3]
        finally:
            base._rep_rows = 0
        base.pgd_update(xa, g.view(2, 2, 1, T).mean(0).contiguous(), lower, upper, 0.0004, atk.grad_sign)
    assert torch.equal(xa, a1), name


def test_as_then_feco_on_audionet():
    """sequential [(0, AS(3)), (1, FeCoDefense)]: a native gradient through both levels (it used to raise)"""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense import AS
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.defended_model import defended_model
    base = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV)
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=3)).to(DEV)
    y = torch.tensor([1, 2], device=DEV)
    ce = SEC4SR_CrossEntropy(reduction='none', task='CSI')
    d0, d1 = AS(3), FeCoDefense(0.5)
    dec, sc, loss, g = defended_model(base, [(0, d0), (1, d1)]).loss_grad(x, y, ce)
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # the chain by hand: d AS^T (front-end^T (FeCo^T (network gradient)))
    sm, sv0 = d0.fwd(x)
    feats, front = base.frontend_forward(sm)
    comp, sv1 = d1.fwd(feats)
    gf = base.loss_grad(comp, y, ce, flag=1)[3]
    assert torch.equal(g, d0.bwd(sv0, base.frontend_backward(front, d1.bwd(sv1, gf))))
