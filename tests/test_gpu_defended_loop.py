"""Input-level defenses inside the device-resident x-vector PGD loop (sg_xv_pgd_run_defended) against the step loop it
replaces (FGSM.attack_batch over defended_model._loss_grad_through_defenses), bit for bit.

Shapes: B = 3 utterances of T = 5043 samples -- 3 over the shortest accepted waveform, no multiple of 4, B * T odd (plane 1 of
the repeat sum is misaligned), longer than the filter's 4096-sample pass (state carries across passes)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T = 3, 5043
EPS, STEP, ITERS = 0.002, 0.0004, 3
KW = dict(task="CSI", epsilon=EPS, step_size=STEP, max_iter=ITERS, batch_size=B, verbose=0)


def _base(dither=0.0):
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(synth.make_xv_weights(), device=DEV, dither=dither)


@pytest.fixture(scope="module")
def base():
    return _base()


@pytest.fixture(scope="module")
def xy(base):
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(DEV)
    return x, base.make_decision(x)[0]  # labels = the clean decisions


def _bounds(x):
    return torch.clamp(x - EPS, min=-1).contiguous(), torch.clamp(x + EPS, max=1).contiguous()


def _fresh(base, index_base=0):
    """the noise bookkeeping of the first batch of a fresh model's first attack (the keys depend on it by design)"""
    base._noise_epoch = 0
    base.begin_attack()
    base.begin_batch(index_base, 1)


def _attack(base, chain, x, y, fuse, index_offset=0, **kw):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.defended_model import defended_model
    atk = PGD(defended_model(base, [(0, d) for d in chain]), **dict(KW, **kw))
    atk.fuse_input_defenses = fuse
    atk.fuse_randomised_input_defenses = True  # AT chains on the device route too (off by default: its noise keys differ)
    atk.index_offset = index_offset
    base._noise_epoch = 0
    return atk.attack(x, y)


def _count_calls(base, monkeypatch):
    calls = []
    real = base.ctx.call
    monkeypatch.setattr(base.ctx, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _chains():
    from speakerguard_amd.defense import AS, BDR, BPF, LPF, MS, QT
    return {"QT": lambda: [QT()], "BDR": lambda: [BDR()], "AS3": lambda: [AS(3)], "MS3": lambda: [MS(3)],
            "LPF": lambda: [LPF(5000)], "BPF": lambda: [BPF()], "AS3-QT-LPF": lambda: [AS(3), QT(), LPF(5000)],
            "MS5-AS31-BDR-BPF": lambda: [MS(5), AS(31), BDR(), BPF()]}


# ---------------------------------------------------------------- 1. deterministic chains: fused == step loop
@pytest.mark.parametrize("name", ["QT", "BDR", "AS3", "MS3", "LPF", "BPF", "AS3-QT-LPF", "MS5-AS31-BDR-BPF"])
def test_deterministic_chain_equals_step_loop(base, xy, name, monkeypatch):
    x, y = xy
    chain = _chains()[name]()
    calls = _count_calls(base, monkeypatch)
    adv, succ = _attack(base, chain, x, y, fuse=True)
    assert calls.count("sg_xv_pgd_run_defended") == 1 and "sg_xv_loss_grad" not in calls, calls  # (one batch)
    del calls[:]
    ref, rsucc = _attack(base, chain, x, y, fuse=False)
    assert "sg_xv_pgd_run_defended" not in calls and calls.count("sg_xv_loss_grad") == ITERS + 1
    assert torch.equal(adv, ref) and succ == rsucc, (name, float((adv - ref).abs().max()))
    assert not torch.equal(adv, x) and float((adv - x).abs().max()) <= EPS + 1e-7


# ---------------------------------------------------------------- 2. traces
@pytest.mark.parametrize("name", ["AS3", "LPF"])
def test_traces_equal_step_loop(base, xy, name):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.defended_model import defended_model
    x, y = xy
    chain = _chains()[name]()
    dm = defended_model(base, [(0, d) for d in chain])
    atk = PGD(dm, **KW)
    lower, upper = _bounds(x)
    _fresh(base)
    adv, success, dec, scores, loss, ltr, dtr = base.pgd_run_defended(x, y, lower, upper, atk.loss, STEP, ITERS, atk.grad_sign, chain,
                                                                      trace=True)
    xa = x.clone()
    for it in range(ITERS + 1):
        d_, s_, l_, g = dm.loss_grad(xa, y, atk.loss, want_grad=True)
        assert torch.equal(ltr[it], l_) and torch.equal(dtr[it], d_), (name, it)
        if it < ITERS:
            base.pgd_update(xa, g.contiguous(), lower, upper, STEP, atk.grad_sign)
    assert torch.equal(xa, adv) and torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(loss, l_)
    assert success.bool().tolist() == (d_ != y).tolist()


# ---------------------------------------------------------------- 3. AT with EOT, replayed
def _replay_chain(base, chain, keys, h, it, rep_rows):
    from speakerguard_amd.model.xv_plda import xv_plda
    tape = []
    for d, k in zip(chain, keys):
        if k is not None:
            h, sv = d.fwd(h, seed=xv_plda.fused_pass_seed(k, it, 0), row_keys=(0, 0, rep_rows))
        else:
            h, sv = d.fwd(h)
        tape.append((d, sv))
    return h, tape


@pytest.mark.parametrize("dither", [0.0, 1.0])
@pytest.mark.parametrize("name", ["AT", "AS3-AT", "AT-QT"])
def test_at_with_eot_equals_replay(xy, name, dither):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AS, AT, QT
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.model.xv_plda import xv_plda
    x, y = xy
    base = _base(dither)
    make = {"AT": lambda s: [AT(25, seed=s)], "AS3-AT": lambda s: [AS(3), AT(25, seed=s)], "AT-QT": lambda s: [AT(25, seed=s), QT()]}[name]
    chain = make(1)
    atk = PGD(defended_model(base, [(0, d) for d in chain]), **KW)
    lower, upper = _bounds(x)
    R = 2
    _fresh(base)
    adv, success, dec, scores, loss, _, _ = base.pgd_run_defended(x, y, lower, upper, atk.loss, STEP, ITERS, atk.grad_sign, chain,
                                                                  eot_size=R, eot_batch_size=R)
    keys, dkey = base.last_fused_defense_seeds, base.last_fused_seed
    assert [k is not None for k in keys] == [isinstance(d, AT) for d in chain]
    xa = x.clone()
    for it in range(ITERS):
        h, tape = _replay_chain(base, chain, keys, xa.repeat(R, 1, 1), it, B)
        base._rep_rows = B
        try:
            g = base.loss_grad(h, y.repeat(R), atk.loss, dither_seed=xv_plda.fused_pass_seed(dkey, it, 0))[3]
        finally:
            base._rep_rows = 0
        for d, sv in reversed(tape):
            g = d.bwd(sv, g)
        g = g.view(R, B, 1, T)
        tot = g[0]
        for r in range(1, R):
            tot = tot + g[r]  # the explicit sequential float32 sum over the repeats
        base.pgd_update(xa, tot.contiguous(), lower, upper, STEP, atk.grad_sign)
    assert torch.equal(adv, xa), (name, dither, float((adv - xa).abs().max()))
    assert not torch.equal(adv, x)
    # the final pass: one repeat, forward only, at it = max_iter
    h, _ = _replay_chain(base, chain, keys, xa, ITERS, 0)
    d_, s_, l_, _ = base.loss_grad(h, y, atk.loss, want_grad=False, dither_seed=xv_plda.fused_pass_seed(dkey, ITERS, 0))
    assert torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(loss, l_)
    assert success.bool().tolist() == (d_ != y).tolist()
    # through the attack: the same seed twice gives the same audio, another seed another
    kw = dict(EOT_size=R, EOT_batch_size=R)
    a1, a2, a3 = (_attack(base, make(s), x, y, True, **kw)[0] for s in (1, 1, 2))
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)


def test_at_chain_takes_the_device_loop_only_on_request(base, xy, monkeypatch):
    """by default an attack against AT keeps the step loop and its noise (the two routes key AT differently)"""
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AS, AT
    from speakerguard_amd.model.defended_model import defended_model
    x, y = xy
    calls = _count_calls(base, monkeypatch)
    atk = PGD(defended_model(base, [(0, AS(3)), (0, AT(25, seed=1))]), **dict(KW, EOT_size=2, EOT_batch_size=2))
    atk.attack(x, y)
    assert "sg_xv_pgd_run_defended" not in calls and calls.count("sg_xv_loss_grad") == ITERS + 1
    del calls[:]
    atk.fuse_randomised_input_defenses = True
    atk.attack(x, y)
    assert calls.count("sg_xv_pgd_run_defended") == 1 and "sg_xv_loss_grad" not in calls


# ---------------------------------------------------------------- 4. repeat groups
def test_repeat_groups_equal_ungrouped(base, xy, monkeypatch):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AS, AT
    from speakerguard_amd.model.defended_model import defended_model
    x, y = xy
    chain = [AS(3), AT(25)]
    atk = PGD(defended_model(base, [(0, d) for d in chain]), **KW)
    lower, upper = _bounds(x)

    def run():
        _fresh(base)
        out = base.pgd_run_defended(x, y, lower, upper, atk.loss, STEP, ITERS, atk.grad_sign, chain, eot_size=4, eot_batch_size=4,
                                    trace=True)
        return out[0], out[5], out[6]

    monkeypatch.delenv("SG_EOT_MAX_ROWS", raising=False)
    whole = run()
    for rows, G in ((2 * B, 2), (B, 1)):
        monkeypatch.setenv("SG_EOT_MAX_ROWS", str(rows))
        part = run()
        for a, b in zip(whole, part):
            assert torch.equal(a, b), G
    assert not torch.equal(whole[0], x)


# ---------------------------------------------------------------- 5. cut independence
def test_cut_independence(base, xy):
    from speakerguard_amd.defense import AT, LPF
    x, y = xy
    kw = dict(EOT_size=2, EOT_batch_size=2)
    make = lambda: [AT(25, seed=3), LPF(5000)]  # noqa: E731
    whole = _attack(base, make(), x, y, True, **kw)[0]
    head = _attack(base, make(), x[0:2], y[0:2], True, **kw)[0]
    tail = _attack(base, make(), x[2:3], y[2:3], True, index_offset=2, **kw)[0]
    assert torch.equal(whole, torch.cat((head, tail), 0))
    assert not torch.equal(whole, x)


# ---------------------------------------------------------------- 6. refusals
def _stage(kind=None, param=0.0, sos=None, tag=None, noise=None):
    from speakerguard_amd import _native as N
    st = N.WavStage()
    if sos is not None:
        st.tag = N.SG_WAV_STAGE_FILTER
        st.u.filter.n_sections, st.u.filter.sos = len(sos), sos.ctypes.data_as(C.POINTER(C.c_double))
        st.u.filter.clip_mode, st.u.filter.bits = N.SG_FD_CLIP_RANGE, 16
    else:
        st.tag = N.SG_WAV_STAGE_DEFENSE
        st.u.defense.kind, st.u.defense.param = N.SG_TD[kind], param
        if noise is not None:
            st.u.defense.noise_dev = noise.data_ptr()
    if tag is not None:
        st.tag = tag
    return st


def test_refusals_leave_the_audio_untouched(base, xy):
    from speakerguard_amd import _native as N
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    x, y = xy
    lower, upper = _bounds(x)
    noise = torch.zeros(B, T, device=DEV)
    unstable = np.array([[1.0, 0.0, 0.0, 1.0, -2.5, 1.0]])  # poles at 2 and 0.5
    good = _stage("AS", 3.0)
    cases = {
        "length 0": [],
        "cap + 1": [good] * (N.SG_WAV_CHAIN_MAX + 1),
        "unknown tag": [_stage("AS", 3.0, tag=7)],
        "AS window 4": [_stage("AS", 4.0)],
        "pole outside the unit circle": [_stage(sos=unstable)],
        "noise_dev": [_stage("AT", 25.0, noise=noise)],
    }
    p = N.PgdParams()
    p.loss = SEC4SR_CrossEntropy(reduction='none', task='CSI').native()
    p.step_size, p.max_iter, p.grad_sign, p.eot_size, p.eot_batch_size = STEP, ITERS, 1, 1, 1
    xa = x.clone()
    outs = (torch.empty(B, device=DEV, dtype=torch.uint8), torch.empty(B, device=DEV, dtype=torch.int64),
            torch.empty(B, base.num_spks, device=DEV), torch.empty(B, device=DEV))
    for what, stages in cases.items():
        arr = (N.WavStage * max(1, len(stages)))(*stages)
        rc = base.ctx.lib.sg_xv_pgd_run_defended(base.ctx.handle, N._ptr(xa), N._ptr(y), N._ptr(lower), N._ptr(upper), B, T, C.byref(p),
                                                 arr, len(stages), *[N._ptr(t) for t in outs], None, None, base._stream())
        assert rc == 1, (what, rc, base.ctx.lib.sg_last_error(base.ctx.handle))  # SG_ERR_ARG
    rc = base.ctx.lib.sg_xv_pgd_run_defended(base.ctx.handle, N._ptr(xa), N._ptr(y), N._ptr(lower), N._ptr(upper), B, T, C.byref(p),
                                             None, 1, *[N._ptr(t) for t in outs], None, None, base._stream())
    assert rc == 1  # a missing chain
    torch.cuda.synchronize()
    assert torch.equal(xa, x)


# ---------------------------------------------------------------- 7. the repeat-summing update on its own
@pytest.mark.parametrize("G", [3, 4])
def test_rep_sum_update_kernel(base, G):
    from speakerguard_amd import _native as N
    n = B * T  # 15129: plane r starts r * 15129 floats in -- misaligned by 1, 2, 3 floats
    rng = np.random.default_rng(5)
    planes = rng.standard_normal((G, n)).astype(np.float32)
    planes[:, :64] = 0.0                                  # exactly zero sums: sign 0 leaves x unchanged
    planes[1, 64:128] = -planes[0, 64:128]
    planes[2:, 64:128] = 0.0
    carry = rng.standard_normal(n).astype(np.float32)
    x0 = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    lo, hi = x0 - np.float32(EPS), x0 + np.float32(EPS)
    x0 = np.clip(x0 + rng.uniform(-EPS, EPS, n).astype(np.float32), lo, hi)
    want = planes[0].copy()
    for r in range(1, G):
        want = want + planes[r]                           # ((p0 + p1) + p2) + ..., float32
    want_c = carry + planes[0]
    for r in range(1, G):
        want_c = want_c + planes[r]
    assert want.dtype == np.float32 and (want[:128] == 0).all()
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    pd, cd, lod, hid = dev(planes), dev(carry), dev(lo), dev(hi)
    s = base._stream()
    for carry_d, tot in ((None, want), (cd, want_c)):
        got = torch.empty(n, device=DEV)
        base.ctx.call("sg_wav_rep_sum_update", N._ptr(pd), G, n, N._ptr(carry_d), N._ptr(got), None, None, None, 0.0, 1, s)
        assert np.array_equal(got.cpu().numpy(), tot)
        for sign in (1, -1):
            xa, xb = dev(x0), dev(x0)
            base.ctx.call("sg_wav_rep_sum_update", N._ptr(pd), G, n, N._ptr(carry_d), None, N._ptr(xa), N._ptr(lod), N._ptr(hid),
                          STEP, sign, s)
            base.ctx.call("sg_pgd_update", N._ptr(xb), N._ptr(got), N._ptr(lod), N._ptr(hid), n, STEP, sign, s)
            assert torch.equal(xa, xb)
            if carry_d is None:
                assert np.array_equal(xa[:128].cpu().numpy(), x0[:128])
            assert not torch.equal(xa, dev(x0))
    # in place on the carried plane (how the loop hands the sum from group to group)
    acc = cd.clone()
    base.ctx.call("sg_wav_rep_sum_update", N._ptr(pd), G, n, N._ptr(acc), N._ptr(acc), None, None, None, 0.0, 1, s)
    assert np.array_equal(acc.cpu().numpy(), want_c)
