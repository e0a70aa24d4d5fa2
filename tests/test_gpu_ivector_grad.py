"""The i-vector gradient on the GPU (iv_plda(white_box=True), csrc/k_ivector_bwd.hip): the backward's stage entries and the
whole chain against float64 truth (tests/iv_restate_grad.py) under the reference's own error, the saturated rows, the wav flag,
invariance under batching and chunking, the forward outputs, and the white-box attacks.  Shapes: the fixtures'
(tests/golden/make_golden_ivector.py, make_golden_ivector_grad.py) -- models A = (C 16, R 24) and B = (C 80, R 100: tile
remainders), F in {2, 13, 100, 331} frames, 5 / 5 / 3 / 1 utterances; model C = (C 272, R 262), F 13 and 100 with 3 and 2
utterances: a second 256-component span in iv_dgamma / iv_dll / iv_dx_post and a second float64 flush in iv_dx_quad, a second
stride in iv_solve_bwd and the tail's adjoint, five d n slices (the last one partial) for iv_slice_sum, and calls of 19 and 33
rows for the second and third group of 16 utterances of iv_rowdot."""
import functools

import numpy as np
import pytest
import torch

import iv_restate_grad as G
from conftest import load_golden, log
from test_ivector_cpu import FILES, GRAD_FILES, MODEL_CASE_IDS, MODEL_CASES, MODELS, checksum

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Sys:
    def __init__(self, tag, dev):
        from speakerguard_amd import synth
        from speakerguard_amd.model.iv_plda import iv_plda
        self.tag = tag
        self.g = load_golden(FILES[tag])
        self.gf = load_golden(GRAD_FILES[tag])
        self.w = synth.make_iv_weights(**MODELS[tag])
        assert checksum(self.w) == self.g["meta"][tag]["weights_sha256"] == self.gf["meta"]["weights_sha256"]
        self.truth = G.IvGrad(self.w)
        self.adj, self.adj32 = G.IvAdjoint(self.w), G.IvAdjoint(self.w, np.float32)
        self.m = iv_plda.from_weights(self.w, device=dev, dither=0.0, white_box=True)
        self.raws = load_golden("iv_ref.npz")

    @functools.lru_cache(maxsize=None)
    def truth_grad(self, F, flag, loss):
        """float64 (loss, grad) of the fixture's case, computed once"""
        ls, g, _ = self.truth.loss_and_grad(self.x(F, flag), self.gf["y_%s_f%d_%d" % (loss, flag, F)],
                                            "margin" if loss == "margin" else "ce", flag)
        return ls, g

    def x(self, F, flag):
        """the fixture's input of `flag`: its own frames, or the first rows of the shared raw inputs"""
        return self.g["x_%d" % F] if flag == 3 else self.raws["raw_%d" % F][:len(self.g["x_%d" % F])]

    @functools.lru_cache(maxsize=None)
    def solve_case(self, F):
        """the solve entry's case, computed once: float32-rounded true statistics, a random d w, the float64 and the float32
        adjoint -> (n32, f32, dw, want, ref); want and ref: lists of (d n, d f) per utterance"""
        t = self.truth.np.chain(self.g["x_%d" % F])
        n32, f32 = t["zeroth"].astype(np.float32), t["first"].astype(np.float32)
        B = n32.shape[0]
        dw = np.random.RandomState(100 + F).randn(B, MODELS[self.tag]["R"]).astype(np.float32)
        want = [self.adj.solve(n32[b], f32[b], dw[b]) for b in range(B)]
        ref = [self.adj32.solve(n32[b], f32[b], dw[b]) for b in range(B)]
        return n32, f32, dw, want, ref


@pytest.fixture(scope="module")
def sys_(dev):
    return {tag: Sys(tag, dev) for tag in ("a", "b", "c")}


def spec_of(loss):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    if loss == "margin":
        return SEC4SR_MarginLoss(targeted=False, confidence=0.0, task="CSI", threshold=None, clip_max=True)
    return SEC4SR_CrossEntropy()


def judge(what, got, ref, truth):
    """tests/test_gpu_ivector.py's rule, per utterance: err_gpu <= max(4 err_ref, 2^-20 max|truth|); the worst ratio is logged"""
    got, ref, truth = (np.asarray(a, np.float64) for a in (got, ref, truth))
    assert np.all(np.isfinite(got)), what
    worst = 0.0
    for b in range(truth.shape[0]):
        e_gpu, e_ref, top = np.abs(got[b] - truth[b]).max(), np.abs(ref[b] - truth[b]).max(), np.abs(truth[b]).max()
        bound = max(4.0 * e_ref, FLOOR * top)
        worst = max(worst, e_gpu / bound)
        log("iv_grad_parity %-40s utt %d  err_gpu %.3e  err_ref %.3e  max|q| %.3e  err_gpu/bound %.3f"
            % (what, b, e_gpu, e_ref, top, e_gpu / bound))
    assert worst <= 1.0, (what, worst)


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@pytest.mark.parametrize("F,B,tag", MODEL_CASES, ids=MODEL_CASE_IDS)
def test_stage_entries_against_truth(sys_, dev, tag, F, B):
    """each backward stage fed float32-rounded truth inputs and a random float32 output gradient; err_ref is the float32 run of
    the hand-written numpy adjoint (the fixture holds the reference's gradient at the chain's ends only)"""
    from speakerguard_amd import _native as N
    s = sys_[tag]
    m, C, Rk = s.m, MODELS[tag]["C"], MODELS[tag]["R"]
    rs = np.random.RandomState(100 + F)
    x = s.g["x_%d" % F]
    # the solve and the assembly
    n32, f32, dw, want, ref = s.solve_case(F)
    assert np.array_equal(dw, rs.randn(B, Rk).astype(np.float32))  # (the generator moves on: the draws below stay where they were)
    dn, df = torch.empty(B, C, device=dev), torch.empty(B, C, 72, device=dev)
    n_d, f_d, dw_d = dv(n32, dev), dv(f32, dev), dv(dw, dev)  # (named: a temporary's memory is reused by the next one)
    m.ctx.call("sg_iv_extract_backward", N._ptr(n_d), N._ptr(f_d), N._ptr(dw_d), B, N._ptr(dn), N._ptr(df), m._stream())
    judge("%s extract_bwd d_zeroth F=%d" % (tag, F), dn.cpu().numpy(), np.stack([r[0] for r in ref]), np.stack([r[0] for r in want]))
    judge("%s extract_bwd d_first F=%d" % (tag, F), df.cpu().numpy(), np.stack([r[1] for r in ref]), np.stack([r[1] for r in want]))
    # statistics, softmax, log-likelihoods
    dn_in, df_in = rs.randn(B, C).astype(np.float32), rs.randn(B, C, 72).astype(np.float32)
    want = np.stack([s.adj.stats(x[b], dn_in[b], df_in[b]) for b in range(B)])
    ref = np.stack([s.adj32.stats(x[b], dn_in[b], df_in[b]) for b in range(B)])
    dx = torch.empty(B, F, 72, device=dev)
    x_d, dn_d, df_d = dv(x, dev), dv(dn_in, dev), dv(df_in, dev)
    m.ctx.call("sg_iv_stats_backward", N._ptr(x_d), B, F, N._ptr(dn_d), N._ptr(df_d), N._ptr(dx), m._stream())
    judge("%s stats_bwd F=%d" % (tag, F), dx.cpu().numpy(), ref, want)
    if tag != "a":
        return  # the front-end is model-independent
    dcm = rs.randn(B, F, 72).astype(np.float32)
    want_d = np.stack([s.adj.cmvn(dcm[b]) for b in range(B)])
    ref_d = np.stack([s.adj32.cmvn(dcm[b]) for b in range(B)])
    want_r = np.stack([s.adj.delta(want_d[b]) for b in range(B)])
    ref_r = np.stack([s.adj32.delta(ref_d[b]) for b in range(B)])
    dd, dr, dcm_d = torch.empty(B, F, 72, device=dev), torch.empty(B, F, 24, device=dev), dv(dcm, dev)
    m.ctx.call("sg_iv_delta_cmvn_backward", N._ptr(dcm_d), 3, B, F, N._ptr(dd), N._ptr(dr), m._stream())
    judge("cmvn_bwd F=%d" % F, dd.cpu().numpy(), ref_d, want_d)
    judge("delta_cmvn_bwd F=%d" % F, dr.cpu().numpy(), ref_r, want_r)
    dr2 = torch.empty(B, F, 24, device=dev)
    m.ctx.call("sg_iv_delta_cmvn_backward", N._ptr(dd), 2, B, F, None, N._ptr(dr2), m._stream())
    assert torch.equal(dr, dr2)  # d delta -> d raw alone: the same second half
    dr3 = torch.empty(B, F, 24, device=dev)
    m.ctx.call("sg_iv_delta_cmvn_backward", N._ptr(dcm_d), 3, B, F, None, N._ptr(dr3), m._stream())
    assert torch.equal(dr, dr3)


@pytest.mark.parametrize("F,B,tag", MODEL_CASES, ids=MODEL_CASE_IDS)
def test_chain_gradient_against_truth(sys_, dev, tag, F, B):
    """flags 3 and 1, both judged losses, err_ref the reference's recorded gradient; flag 2 against the flag-1 truth pushed
    through the delta adjoint; then the saturated rows: finite, and the loss of want_grad=False bit for bit"""
    s = sys_[tag]
    m = s.m
    assert s.gf["meta"]["judged_losses"] == ["ce", "margin"]
    for flag in (3, 1):
        x = dv(s.x(F, flag), dev)
        for loss in ("ce", "margin"):
            key = "%s_f%d_%d" % (loss, flag, F)
            y = torch.from_numpy(s.gf["y_" + key]).to(dev)
            ls_t, g_t = s.truth_grad(F, flag, loss)
            dec, sc, ls, grad = m.loss_grad(x, y, spec_of(loss), flag=flag, want_grad=True)
            assert grad.shape == x.shape
            judge("%s chain flag %d %s F=%d" % (tag, flag, loss, F), grad.cpu().numpy(), s.gf["grad_" + key], g_t)
            np.testing.assert_allclose(ls.cpu().numpy(), ls_t, rtol=1e-4, atol=1e-5)
            if flag == 1:
                delta = m.comput_feat_from_feat(x, 1, 2)
                g2 = m.loss_grad(delta, y, spec_of(loss), flag=2, want_grad=True)[3]
                assert g2.shape == delta.shape
                pushed = np.stack([s.adj.delta(u) for u in g2.cpu().numpy().astype(np.float64)])
                judge("%s chain flag 2 %s F=%d" % (tag, loss, F), pushed, s.gf["grad_" + key], g_t)
        y = torch.from_numpy(s.gf["y_sat_f%d_%d" % (flag, F)]).to(dev)
        _, _, ls, grad = m.loss_grad(x, y, spec_of("ce"), flag=flag, want_grad=True)
        assert torch.isfinite(grad).all()
        assert torch.equal(ls, m.loss_grad(x, y, spec_of("ce"), flag=flag, want_grad=False)[2])


def test_wav_gradient_against_autograd(sys_, dev):
    """flag 0, 2 x 16000 samples, dither off, against float64 autograd through oracle.kaldi_mfcc and the restatement.  The bound
    is 10 x the value measured on the first GPU run (the convention of tests/test_gpu_xv.py's wav-gradient test)."""
    from speakerguard_amd import synth
    s = sys_["a"]
    om = G.IvGradOracleModel(s.w)
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=32))
    xt = x.clone().requires_grad_(True)
    sc_t = om.scores(xt)
    dec = sc_t.argmax(1)
    y = (dec + 1) % sc_t.shape[1]
    ls_t = torch.stack([G.loss_t(a, int(l), "ce") for a, l in zip(sc_t, y)])
    ls_t.sum().backward()
    g_t = xt.grad.numpy().astype(np.float64)
    xd = x.to(dev)
    _, _, ls, grad = s.m.loss_grad(xd, y.to(dev), spec_of("ce"), flag=0, want_grad=True)
    g = grad.cpu().numpy().astype(np.float64)
    assert grad.shape == x.shape and np.isfinite(g).all()
    rel = [float(np.abs(g[b] - g_t[b]).max() / np.abs(g_t[b]).max()) for b in range(2)]
    sign = float((np.sign(g) != np.sign(g_t)).mean())
    log("iv_grad_parity wav flag 0: max err / max|g| %s, sign mismatch fraction %.5f" % (["%.3e" % r for r in rel], sign))
    # measured on the first GPU run: max err / max|g| 7.776e-05 and 2.641e-05, no sign mismatch among the 32000 samples.  The
    # bounds are 10 x the measured values; a measured fraction of 0 means "below one sample", so its bound is 10 samples' worth.
    WAV_REL_MEASURED, WAV_SIGN_MEASURED = 7.776e-05, 1.0 / g.size
    assert max(rel) <= 10 * WAV_REL_MEASURED and sign <= 10 * WAV_SIGN_MEASURED
    # a sg_pgd_update step along it raises the restatement's loss
    adv = xd.clone()
    lo, hi = torch.full_like(adv, -1.0), torch.full_like(adv, 1.0)
    s.m.pgd_update(adv, grad.contiguous(), lo, hi, 0.0004, 1)
    with torch.no_grad():
        sc2 = om.scores(adv.cpu())
        ls2 = torch.stack([G.loss_t(a, int(l), "ce") for a, l in zip(sc2, y)])
    assert (ls2 > ls_t.detach()).all()
    np.testing.assert_allclose(ls.cpu().numpy(), ls_t.detach().numpy(), rtol=1e-3, atol=1e-4)


def test_invariance_under_batching_and_chunking(sys_, dev):
    spec = spec_of("ce")
    for tag in ("a", "b"):
        s = sys_[tag]
        x = dv(s.g["x_13"], dev)
        y = torch.from_numpy(s.gf["y_ce_f3_13"]).to(dev)
        full = s.m.loss_grad(x, y, spec, flag=3, want_grad=True)
        again = s.m.loss_grad(x, y, spec, flag=3, want_grad=True)
        assert all(torch.equal(a, b) for a, b in zip(full, again))
        for i in range(5):
            one = s.m.loss_grad(x[i:i + 1], y[i:i + 1], spec, flag=3, want_grad=True)
            assert all(torch.equal(a[i:i + 1], b) for a, b in zip(full, one)), (tag, i)
    # a call that straddles the 64-row chunk boundary against its slices (flag 1: every backward kernel runs)
    m = sys_["a"].m
    rs = np.random.RandomState(7)
    raw = dv(rs.randn(150, 13, 24), dev)
    y = torch.from_numpy(rs.randint(0, 4, 150)).to(dev)
    full = m.loss_grad(raw, y, spec, flag=1, want_grad=True)
    for lo, hi in ((0, 1), (60, 70), (63, 64), (64, 65), (100, 150), (149, 150)):
        part = m.loss_grad(raw[lo:hi], y[lo:hi], spec, flag=1, want_grad=True)
        assert all(torch.equal(a[lo:hi], b) for a, b in zip(full, part)), (lo, hi)


def group_rows(s, B0=16):
    """tests/test_gpu_ivector.py's call of model C: B0 rows of other frames, then the fixture's three utterances of 13 frames"""
    from speakerguard_amd import synth
    return np.concatenate([synth.make_iv_frames(s.w, B0, 13, seed=77), s.g["x_13"]])


def test_second_utterance_group_against_truth(sys_, dev):
    """19 rows of model C, flag 3: iv_rowdot's (and the forward assembly's) second group of 16 utterances holds the fixture's
    three -- both judged losses against truth under the rule and bit-equal to the 3-row call; then sg_iv_extract_backward alone"""
    from speakerguard_amd import _native as N
    s = sys_["c"]
    m, C, Rk = s.m, MODELS["c"]["C"], MODELS["c"]["R"]
    x19 = dv(group_rows(s), dev)
    rs = np.random.RandomState(19)
    for loss in ("ce", "margin"):
        key = "%s_f3_13" % loss
        y = torch.from_numpy(np.concatenate([rs.randint(0, MODELS["c"]["n_spk"], 16), s.gf["y_" + key]])).to(dev)
        full = m.loss_grad(x19, y, spec_of(loss), flag=3, want_grad=True)
        three = m.loss_grad(x19[16:], y[16:], spec_of(loss), flag=3, want_grad=True)
        assert full[3].shape == x19.shape
        judge("c 19 rows chain flag 3 %s F=13" % loss, full[3][16:].cpu().numpy(), s.gf["grad_" + key], s.truth_grad(13, 3, loss)[1])
        assert all(torch.equal(a[16:], b) for a, b in zip(full, three)), loss
    # the solve's adjoint with B = 19: rows 16 .. 18 are test_stage_entries_against_truth's case
    n32, f32, dw, want, ref = s.solve_case(13)
    n16, f16 = m.stats(x19[:16])
    n_d = torch.cat([n16, dv(n32, dev)]).contiguous()
    f_d = torch.cat([f16, dv(f32, dev)]).contiguous()
    dw_d = dv(np.concatenate([rs.randn(16, Rk), dw]), dev)

    def run(lo, hi):
        nb = hi - lo
        dn, df = torch.empty(nb, C, device=dev), torch.empty(nb, C, 72, device=dev)
        a, b, c = n_d[lo:hi].contiguous(), f_d[lo:hi].contiguous(), dw_d[lo:hi].contiguous()
        m.ctx.call("sg_iv_extract_backward", N._ptr(a), N._ptr(b), N._ptr(c), nb, N._ptr(dn), N._ptr(df), m._stream())
        torch.cuda.synchronize()
        return dn, df

    dn, df = run(0, 19)
    judge("c 19 rows extract_bwd d_zeroth F=13", dn[16:].cpu().numpy(), np.stack([r[0] for r in ref]), np.stack([r[0] for r in want]))
    judge("c 19 rows extract_bwd d_first F=13", df[16:].cpu().numpy(), np.stack([r[1] for r in ref]), np.stack([r[1] for r in want]))
    for lo, hi in ((16, 19), (0, 16)):
        dn1, df1 = run(lo, hi)
        assert torch.equal(dn[lo:hi], dn1) and torch.equal(df[lo:hi], df1), (lo, hi)


def test_a_33_row_gradient_equals_its_rows(sys_, dev):
    """model C, groups of 16, 16 and 1 utterances: the first and last row of every group equal the same row sent alone"""
    s = sys_["c"]
    x = dv(group_rows(s, 30), dev)
    y = torch.from_numpy(np.random.RandomState(33).randint(0, MODELS["c"]["n_spk"], 33)).to(dev)
    for loss in ("ce", "margin"):
        full = s.m.loss_grad(x, y, spec_of(loss), flag=3, want_grad=True)
        for i in (0, 15, 16, 31, 32):
            one = s.m.loss_grad(x[i:i + 1], y[i:i + 1], spec_of(loss), flag=3, want_grad=True)
            assert all(torch.equal(a[i:i + 1], b) for a, b in zip(full, one)), (loss, i)


def test_forward_outputs_are_the_forward_pass(sys_, dev):
    for tag in ("a", "b", "c"):
        s = sys_[tag]
        for flag, x in ((3, s.x(100, 3)), (1, s.x(100, 1))):
            x = dv(x, dev)
            y = torch.from_numpy(s.gf["y_ce_f%d_100" % flag]).to(dev)
            for loss in ("ce", "margin"):
                a = s.m.loss_grad(x, y, spec_of(loss), flag=flag, want_grad=True)
                b = s.m.loss_grad(x, y, spec_of(loss), flag=flag, want_grad=False)
                assert b[3] is None and all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))
            dec, sc = s.m.make_decision(x, flag=flag)
            assert torch.equal(dec, a[0]) and torch.equal(sc, a[1])


@pytest.mark.parametrize("loss_name", ["Entropy", "Margin"])
def test_pgd_attack_matches_oracle(sys_, dev, loss_name):
    """oracle.attacks.PGD on the float64 differentiable model against PGD(iv_plda(white_box=True)): 2 x 1 s, 5 iterations,
    untargeted; the bounds of tests/test_gpu_xv.py::test_pgd_attack_matches_oracle"""
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    s = sys_["a"]
    om = G.IvGradOracleModel(s.w)
    eps, step, iters = 0.002, 0.0004, 5
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=32))
    with torch.no_grad():
        y = om.make_decision(x)[0]
    assert s.m.make_decision(x.to(dev))[0].cpu().tolist() == y.tolist()
    kw = dict(task="CSI", epsilon=eps, step_size=step, max_iter=iters, loss=loss_name, targeted=False, batch_size=2)
    oadv, osucc = oatk.PGD(om, **kw).attack(x.clone(), y)
    atk = PGD(s.m, verbose=0, **kw)
    assert atk._device_route(2) is None  # the step loop over loss_grad / pgd_update
    adv, succ = atk.attack(x.to(dev), y.to(dev))
    diff = (adv.cpu() - oadv).abs()
    frac = float((diff > 1e-7).float().mean())
    log("iv PGD-%d %s: samples differing %.4f%%, max|diff| %.2e, success hip=%s oracle=%s"
        % (iters, loss_name, 100 * frac, diff.max().item(), succ, osucc))
    assert succ == osucc
    assert frac < 0.02 * iters and diff.max().item() <= 2 * eps + 1e-6


def test_fgsm_and_cw2_run(sys_, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.CW2 import CW2
    from speakerguard_amd.attack.FGSM import FGSM
    m = sys_["a"].m
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=33)).to(dev)
    y = m.make_decision(x)[0]
    eps = 0.002
    adv, succ = FGSM(m, task="CSI", epsilon=eps, batch_size=2, verbose=0).attack(x, y)
    assert adv.shape == x.shape and torch.isfinite(adv).all() and len(succ) == 2
    assert (adv - x).abs().max().item() <= eps + 1e-6 and adv.abs().max().item() <= 1.0
    assert (adv != x).any()
    adv, succ = CW2(m, task="CSI", binary_search_steps=1, max_iter=3, batch_size=2, verbose=0).attack(x, y)
    assert adv.shape == x.shape and torch.isfinite(adv).all() and adv.abs().max().item() <= 1.0 and len(succ) == 2


def test_default_model_still_raises(sys_, dev):
    from speakerguard_amd.model.iv_plda import iv_plda
    s = sys_["a"]
    m = iv_plda.from_weights(s.w, device=dev, dither=0.0)
    x = dv(s.g["x_13"], dev)
    y = torch.zeros(5, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match="gradient is not built"):
        m.loss_grad(x, y, spec_of("ce"), flag=3)
    for fn in (m.pgd_run, s.m.pgd_run, s.m.pgd_run_defended, s.m.pgd_run_feco):
        with pytest.raises(NotImplementedError, match="gradient is not built"):
            fn(None)
    assert m.loss_grad(x, y, spec_of("ce"), flag=3, want_grad=False)[3] is None
