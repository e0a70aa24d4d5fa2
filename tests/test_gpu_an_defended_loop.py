"""Input-level defenses inside AudioNet's device-resident PGD loops (sg_an_pgd_run_defended) against the step loop they replace
(FGSM.attack_batch over defended_model._loss_grad_through_defenses), bit for bit.

Shapes: B = 3 utterances of T = 5043 samples as in test_gpu_defended_loop.py -- B * T odd (plane 1 of the repeat sum is
misaligned), longer than the filter's 4096-sample pass, 32 log-mel frames, which the AudioNet stack still accepts.  The
tests with FeCoDefense(0.5) behind the chain use T = 10081 (odd, 64 frames): the network then sees k = int(F / 2) cluster
frames and needs k >= 24 of them (3 frames at conv8) -- at 5043, k = 16 is refused by the device loop and by the step loop
alike -- and the single-utterance step loop of the shard test drops empty clusters, so k = 32 leaves it 8 to lose."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, T_FECO = 3, 5043, 10081
EPS, STEP, ITERS = 0.002, 0.0004, 3
KW = dict(task="CSI", epsilon=EPS, step_size=STEP, max_iter=ITERS, batch_size=B, verbose=0)
CALL = "sg_an_pgd_run_defended"


@pytest.fixture(scope="module")
def base():
    from speakerguard_amd import synth
    from speakerguard_amd.model.audionet_csine import audionet_csine
    return audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV)


def _xy(base, t):
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, t, seed=3)).to(DEV)
    return x, base.make_decision(x)[0]  # labels = the clean decisions


@pytest.fixture(scope="module")
def xy(base):
    return _xy(base, T)


@pytest.fixture(scope="module")
def xy_feco(base):
    return _xy(base, T_FECO)


def _bounds(x):
    return torch.clamp(x - EPS, min=-1).contiguous(), torch.clamp(x + EPS, max=1).contiguous()


def _fresh(base, index_base=0):
    """the noise bookkeeping of the first batch of a fresh model's first attack (the keys depend on it by design)"""
    base._noise_epoch = 0
    base.begin_attack()
    base.begin_batch(index_base, 1)


def _attack(base, defense, x, y, index_offset=0, **attrs):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.defended_model import defended_model
    kw = {k: attrs.pop(k) for k in list(attrs) if k in ("EOT_size", "EOT_batch_size", "batch_size")}
    atk = PGD(defended_model(base, defense), **dict(KW, **kw))
    atk.fuse_randomised_input_defenses = True  # AT chains on the device route too (off by default: its noise keys differ)
    for k, v in attrs.items():
        setattr(atk, k, v)
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


# ---------------------------------------------------------------- 1. deterministic chains: device loop == step loop
@pytest.mark.parametrize("name", ["QT", "BDR", "AS3", "MS3", "LPF", "BPF", "AS3-QT-LPF", "MS5-AS31-BDR-BPF"])
def test_deterministic_chain_equals_step_loop(base, xy, name, monkeypatch):
    x, y = xy
    defense = [(0, d) for d in _chains()[name]()]
    calls = _count_calls(base, monkeypatch)
    adv, succ = _attack(base, defense, x, y)
    assert calls.count(CALL) == 1 and "sg_an_loss_grad" not in calls, calls  # (one batch)
    del calls[:]
    ref, rsucc = _attack(base, defense, x, y, fuse_input_defenses=False)
    assert CALL not in calls and calls.count("sg_an_loss_grad") == ITERS + 1
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


# ---------------------------------------------------------------- 3. AT with EOT 2, replayed
def _replay_chain(base, chain, keys, h, it, rep_rows):
    tape = []
    for d, k in zip(chain, keys):
        if k is not None:
            h, sv = d.fwd(h, seed=base.fused_pass_seed(k, it, 0), row_keys=(0, 0, rep_rows))
        else:
            h, sv = d.fwd(h)
        tape.append((d, sv))
    return h, tape


@pytest.mark.parametrize("name", ["AT", "AS3-AT", "AT-QT"])
def test_at_with_eot_equals_replay(base, xy, name, monkeypatch):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AS, AT, QT
    from speakerguard_amd.model.defended_model import defended_model
    x, y = xy
    make = {"AT": lambda s: [AT(25, seed=s)], "AS3-AT": lambda s: [AS(3), AT(25, seed=s)], "AT-QT": lambda s: [AT(25, seed=s), QT()]}[name]
    chain = make(1)
    atk = PGD(defended_model(base, [(0, d) for d in chain]), **KW)
    lower, upper = _bounds(x)
    R = 2

    def run():
        _fresh(base)
        return base.pgd_run_defended(x, y, lower, upper, atk.loss, STEP, ITERS, atk.grad_sign, chain, eot_size=R, eot_batch_size=R,
                                     trace=True)

    monkeypatch.delenv("SG_EOT_MAX_ROWS", raising=False)
    adv, success, dec, scores, loss, ltr, dtr = run()
    keys = base.last_fused_defense_seeds
    assert [k is not None for k in keys] == [isinstance(d, AT) for d in chain]
    xa = x.clone()
    for it in range(ITERS):
        h, tape = _replay_chain(base, chain, keys, xa.repeat(R, 1, 1), it, B)
        d_, _, l_, g = base.loss_grad(h, y.repeat(R), atk.loss)
        # the step's records: loss averaged, decision voted over the repeats (numpy's true division, as the kernel divides)
        l_ = l_.view(R, B).cpu().numpy()
        assert np.array_equal((l_[0] + l_[1]) / np.float32(R), ltr[it].cpu().numpy()), (name, it)
        d_ = d_.view(R, B).cpu().tolist()
        assert dtr[it].cpu().tolist() == [Counter(d_[r][b] for r in range(R)).most_common(1)[0][0] for b in range(B)]
        for d, sv in reversed(tape):
            g = d.bwd(sv, g)
        g = g.view(R, B * T).contiguous()
        # the repeat sum and the step, through the kernel the loop uses (planes in repeat order)
        base.ctx.call("sg_wav_rep_sum_update", C.c_void_p(g.data_ptr()), R, B * T, None, None, C.c_void_p(xa.data_ptr()),
                      C.c_void_p(lower.data_ptr()), C.c_void_p(upper.data_ptr()), STEP, atk.grad_sign, base._stream())
    assert torch.equal(adv, xa), (name, float((adv - xa).abs().max()))
    assert not torch.equal(adv, x)
    # the final pass: one repeat, forward only, at it = max_iter
    h, _ = _replay_chain(base, chain, keys, xa, ITERS, 0)
    d_, s_, l_, _ = base.loss_grad(h, y, atk.loss, want_grad=False)
    assert torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(loss, l_)
    assert success.bool().tolist() == (d_ != y).tolist()
    # one repeat per pass (G = 1): the groups' carried sum and collected records give the same bits as G = 2
    monkeypatch.setenv("SG_EOT_MAX_ROWS", str(B))
    grouped = run()
    monkeypatch.delenv("SG_EOT_MAX_ROWS")
    for a, b in zip((adv, success, dec, scores, loss, ltr, dtr), grouped):
        assert torch.equal(a, b), name
    # through the attack: the same seed twice gives the same audio, another seed another
    kw = dict(EOT_size=R, EOT_batch_size=R)
    a1, a2, a3 = (_attack(base, [(0, d) for d in make(s)], x, y, **kw)[0] for s in (1, 1, 2))
    assert torch.equal(a1, a2) and torch.equal(a1, adv) and not torch.equal(a1, a3)


def test_at_chain_takes_the_device_loop_only_on_request(base, xy, monkeypatch):
    """by default an attack against AT keeps the step loop and its noise (the two routes key AT differently)"""
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import AS, AT
    from speakerguard_amd.model.defended_model import defended_model
    x, y = xy
    calls = _count_calls(base, monkeypatch)
    atk = PGD(defended_model(base, [(0, AS(3)), (0, AT(25, seed=1))]), **dict(KW, EOT_size=2, EOT_batch_size=2))
    atk.attack(x, y)
    assert CALL not in calls and calls.count("sg_an_loss_grad") == ITERS + 1
    del calls[:]
    atk.fuse_randomised_input_defenses = True
    atk.attack(x, y)
    assert calls.count(CALL) == 1 and "sg_an_loss_grad" not in calls


# ---------------------------------------------------------------- 4. chain + FeCo
@pytest.mark.parametrize("name", ["AS3", "QT"])
@pytest.mark.parametrize("off", ["fuse_defended", "fuse_input_defenses"])
def test_chain_and_feco_equal_step_loop(base, xy_feco, name, off, monkeypatch):
    from speakerguard_amd.defense.feature_level import FeCoDefense
    x, y = xy_feco
    defense = [(0, _chains()[name]()[0]), (1, FeCoDefense(0.5))]
    calls = _count_calls(base, monkeypatch)
    adv, succ = _attack(base, defense, x, y)
    assert calls.count(CALL) == 1 and "sg_an_loss_grad" not in calls, calls
    del calls[:]
    ref, rsucc = _attack(base, defense, x, y, **{off: False})
    assert CALL not in calls and calls.count("sg_an_loss_grad") == ITERS + 1
    assert torch.equal(adv, ref) and succ == rsucc, (name, float((adv - ref).abs().max()))
    assert not torch.equal(adv, x) and float((adv - x).abs().max()) <= EPS + 1e-7


def test_chain_and_random_feco_with_eot_equal_replay(base, xy_feco):
    """AS(3) in front of FeCoDefense(init='random'), EOT 2: a replay of the passes through the per-stage entry points with the
    per-pass keys (tests/test_gpu_feco.py::test_audionet_feco_fused_loop's replay behind the smoothing)"""
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense import AS
    from speakerguard_amd.defense.feature_level import FeCoDefense
    x, y = xy_feco
    spec = SEC4SR_CrossEntropy()
    lower, upper = _bounds(x)
    R = 2
    d0, feco = AS(3), FeCoDefense(0.5, init='random', seed=0)
    _fresh(base)
    adv, success, dec, scores, loss, ltr, dtr = base.pgd_run_defended_feco(x, y, lower, upper, spec, STEP, ITERS, 1, [d0], feco,
                                                                           eot_size=R, eot_batch_size=R, trace=True)
    assert feco.calls == 1
    key = base.last_fused_seed
    replay = FeCoDefense(0.5, init='random', seed=123)  # keys are given explicitly below
    xa = x.clone()
    for it in range(ITERS):
        sm, sv0 = d0.fwd(xa)
        feats, front = base.frontend_forward(sm)  # only the clustering is random: one chain and front-end pass per step
        dsum, lsum, decs = None, None, []
        for r in range(R):
            comp, sv = replay.fwd(feats, seed=base.fused_pass_seed(key, it, r))
            d_, _, l_, g = base.loss_grad(comp, y, spec, flag=1)
            lsum = l_ if lsum is None else lsum + l_
            decs.append(d_.cpu().tolist())
            df = replay.bwd(sv, g)
            dsum = df if dsum is None else dsum + df  # feature-level sum in repeat order
        assert np.array_equal(lsum.cpu().numpy() / np.float32(R), ltr[it].cpu().numpy()), it
        assert dtr[it].cpu().tolist() == [Counter(decs[r][b] for r in range(R)).most_common(1)[0][0] for b in range(B)]
        g = d0.bwd(sv0, base.frontend_backward(front, dsum))
        base.pgd_update(xa, g.contiguous(), lower, upper, STEP, 1)
    assert torch.equal(adv, xa) and not torch.equal(adv, x)
    comp, _ = replay.fwd(base.compute_feat(d0.fwd(xa)[0], flag=1), seed=base.fused_pass_seed(key, ITERS, 0))
    d_, s_ = base.make_decision(comp, flag=1)
    assert torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(ltr[ITERS], loss) and torch.equal(dtr[ITERS], dec)
    assert success.bool().tolist() == (d_ != y).tolist()


# ---------------------------------------------------------------- 5. shard invariance
def test_shards_of_a_chain_equal_the_whole(base, xy):
    from speakerguard_amd.defense import AS
    x, y = xy
    make = lambda: [(0, AS(3))]  # noqa: E731
    whole = _attack(base, make(), x, y)[0]
    head = _attack(base, make(), x[0:2], y[0:2])[0]
    tail = _attack(base, make(), x[2:3], y[2:3], index_offset=2)[0]
    assert torch.equal(whole, torch.cat((head, tail), 0)) and not torch.equal(whole, x)


def test_shards_of_a_chain_and_random_feco(base, xy_feco, monkeypatch):
    """(2, 1): the two utterances of the first shard run the device loop and reproduce the whole batch bit for bit; FeCo needs
    two rows, so the single utterance keeps the step loop (where the reference drops empty clusters: another model), and only
    that and the perturbation bound are asserted for it"""
    from speakerguard_amd.defense import AS
    from speakerguard_amd.defense.feature_level import FeCoDefense
    x, y = xy_feco
    kw = dict(EOT_size=2, EOT_batch_size=2)
    make = lambda: [(0, AS(3)), (1, FeCoDefense(0.5, init='random', seed=3))]  # noqa: E731
    calls = _count_calls(base, monkeypatch)
    whole = _attack(base, make(), x, y, **kw)[0]
    head = _attack(base, make(), x[0:2], y[0:2], **kw)[0]
    assert calls.count(CALL) == 2 and "sg_an_loss_grad" not in calls
    assert torch.equal(whole[0:2], head) and not torch.equal(whole, x)
    shifted = _attack(base, make(), x[0:2], y[0:2], index_offset=1, **kw)[0]  # as "global utterances 1, 2": other clusterings
    assert not torch.equal(shifted, head)
    del calls[:]
    tail = _attack(base, make(), x[2:3], y[2:3], index_offset=2, **kw)[0]
    assert CALL not in calls and "sg_an_loss_grad" in calls
    assert bool(torch.isfinite(tail).all()) and float((tail - x[2:3]).abs().max()) <= EPS + 1e-7


# ---------------------------------------------------------------- 6. refusals
def _stage(kind, param=0.0, tag=None, noise=None):
    from speakerguard_amd import _native as N
    st = N.WavStage()
    st.tag = N.SG_WAV_STAGE_DEFENSE if tag is None else tag
    st.u.defense.kind, st.u.defense.param = N.SG_TD[kind], param
    if noise is not None:
        st.u.defense.noise_dev = noise.data_ptr()
    return st


def test_refusals_leave_the_audio_untouched(base, xy):
    from speakerguard_amd import _native as N
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    x, y = xy
    lower, upper = _bounds(x)
    noise = torch.zeros(B, T, device=DEV)
    good, at = _stage("AS", 3.0), _stage("AT", 25.0)
    feco = N.FecoParams()
    feco.k, feco.max_iter, feco.random_init = 16, 10, 0
    cases = {  # name: (stages, EOT size, EOT batch size, feco, rows)
        "0 stages": ([], 1, 1, None, B),
        "9 stages": ([good] * (N.SG_WAV_CHAIN_MAX + 1), 1, 1, None, B),
        "unknown tag": ([_stage("AS", 3.0, tag=7)], 1, 1, None, B),
        "noise_dev": ([_stage("AT", 25.0, noise=noise)], 1, 1, None, B),
        "EOT 3 in batches of 2": ([good], 3, 2, None, B),
        "AT with feco": ([good, at], 1, 1, feco, B),
        "feco with B = 1": ([good], 1, 1, feco, 1),
    }
    p = N.PgdParams()
    p.loss = SEC4SR_CrossEntropy(reduction='none', task='CSI').native()
    p.step_size, p.max_iter, p.grad_sign = STEP, ITERS, 1
    xa = x.clone()
    outs = (torch.empty(B, device=DEV, dtype=torch.uint8), torch.empty(B, device=DEV, dtype=torch.int64),
            torch.empty(B, base.num_spks, device=DEV), torch.empty(B, device=DEV))
    lib, h = base.ctx.lib, base.ctx.handle
    for what, (stages, eot, eot_bs, f, rows) in cases.items():
        arr = (N.WavStage * max(1, len(stages)))(*stages)
        p.eot_size, p.eot_batch_size = eot, eot_bs
        rc = lib.sg_an_pgd_run_defended(h, N._ptr(xa), N._ptr(y), N._ptr(lower), N._ptr(upper), rows, T, C.byref(p), arr, len(stages),
                                        None if f is None else C.byref(f), *[N._ptr(t) for t in outs], None, None, base._stream())
        assert rc == 1, (what, rc, lib.sg_last_error(h))  # SG_ERR_ARG
        assert lib.sg_last_error(h), what
    torch.cuda.synchronize()
    assert torch.equal(xa, x)  # nothing was launched
