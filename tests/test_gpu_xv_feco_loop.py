"""FeCo inside the device-resident x-vector PGD loop (sg_xv_pgd_run_feco) on the GPU.

Shapes: B = 3 utterances of T = 16001 samples (odd: B * T is no multiple of 4), which the front-end cuts into 100 frames; FeCo at
ratio 0.5 leaves k = 50 -- enough for the TDNN context (32), and the frame counts in front of and behind the defense differ.
max_iter = 3.  Everything is bit-equality: the loop issues the launches of the single-stage entry points in the same order on the
same data, so there is no tolerance to choose.

  * deterministic FeCo, no dither: ``PGD.attack`` through the loop == the same attack through the step loop
    (``fuse_defended = False``), which tests/test_gpu_feco.py holds to the oracle's autograd;
  * dither and / or random init, EOT 2: a replay of every pass through ``frontend_forward`` / ``FeCoDefense.fwd`` / ``loss_grad`` /
    the ``bwd``s / ``pgd_update`` with the keys ``fused_pass_seed`` derives from the two recorded base keys.  With dither the
    repeats are summed at the waveform, without (only the defense is random) at the feature level, in repeat order;
  * EOT 4 forced into two groups == one group;
  * the row-wise clustering launch alone == one single-row launch per row with that row's key and utterance index;
  * a batch of 4 cut as 2 + 2 with the shards' index offsets == the uncut batch.
"""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, F, K = 3, 16001, 100, 50
EPS, STEP, ITERS = 0.002, 0.0004, 3
KW = dict(epsilon=EPS, step_size=STEP, max_iter=ITERS, batch_size=4, verbose=0)
ENTRY = "sg_xv_pgd_run_feco"


@pytest.fixture(scope="module")
def bases(xv_weights):
    from speakerguard_amd.model.xv_plda import xv_plda
    return {d: xv_plda.from_weights(xv_weights, device=DEV, dither=d, dither_seed=9) for d in (0.0, 1.0)}


@pytest.fixture(scope="module")
def xy(bases):
    from speakerguard_amd import _native as N
    from speakerguard_amd import synth
    assert N.load().sg_xv_num_frames(T) == F and int(F * 0.5) == K
    x = torch.from_numpy(synth.make_waveforms(4, T, seed=21)).to(DEV)
    return x, bases[0.0].make_decision(x)[0]


def _fresh(base):
    base._noise_epoch = 0
    base.begin_attack()
    base.begin_batch(0)


def _bounds(x):
    return torch.clamp(x - EPS, min=-1).contiguous(), torch.clamp(x + EPS, max=1).contiguous()


def _count_calls(base, monkeypatch):
    calls, call = [], base.ctx.call

    def counting(name, *a):
        calls.append(name)
        return call(name, *a)
    monkeypatch.setattr(base.ctx, "call", counting)
    return calls


def _attack(base, level, feco, x, y, index_offset=0, **attrs):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.model.defended_model import defended_model
    kw = dict(KW, **{k: attrs.pop(k) for k in list(attrs) if k in ("EOT_size", "EOT_batch_size", "batch_size")})
    atk = PGD(defended_model(base, [(level, feco)]), **kw)
    atk.index_offset = index_offset
    for k, v in attrs.items():
        setattr(atk, k, v)
    base._noise_epoch = 0
    return atk.attack(x, y)


# ---------------------------------------------------------------- 4. deterministic: the loop == the step loop
@pytest.mark.parametrize("level", [1, 2])
def test_deterministic_loop_equals_step_loop(bases, xy, level, monkeypatch):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import FeCoDefense
    base, (x, y) = bases[0.0], xy
    x, y = x[:B], y[:B]
    calls = _count_calls(base, monkeypatch)
    adv, succ = _attack(base, level, FeCoDefense(0.5), x, y)
    assert calls.count(ENTRY) == 1 and "sg_xv_loss_grad" not in calls, calls
    del calls[:]
    ref, rsucc = _attack(base, level, FeCoDefense(0.5), x, y, fuse_defended=False)
    assert ENTRY not in calls and calls.count("sg_xv_loss_grad") == ITERS + 1
    assert torch.equal(adv, ref) and succ == rsucc, float((adv - ref).abs().max())
    assert not torch.equal(adv, x) and float((adv - x).abs().max()) <= EPS + 1e-7
    # the state at the final pass, as the loop hands it out, against the step loop's last model call on its own result
    spec = SEC4SR_CrossEntropy()
    lower, upper = _bounds(x)
    _fresh(base)
    out = base.pgd_run_feco(x, y, lower, upper, spec, STEP, ITERS, 1, FeCoDefense(0.5), trace=True, level=level)
    xa, success, dec, scores, loss, ltr, dtr = out
    assert torch.equal(xa, ref)
    feats = base.compute_feat(ref, flag=level)
    d_, s_, l_, _ = base.loss_grad(FeCoDefense(0.5).fwd(feats)[0], y, spec, flag=level, want_grad=False)
    assert torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(loss, l_)
    assert torch.equal(ltr[ITERS], loss) and torch.equal(dtr[ITERS], dec)
    assert success.bool().tolist() == (d_ != y).tolist() == succ


# ---------------------------------------------------------------- 5. randomised: the loop == a replay of its passes
CASES = {"a-dither-even": (1.0, "even"), "b-dither-random": (1.0, "random"), "c-random-only": (0.0, "random")}


def _pass(base, replay, level, xa, y, spec, dkey, fkey, it, r, want_grad=True):
    """one repeat through the single-stage entry points -> (decisions, scores, loss, cotangent at FeCo's input level, front)"""
    feats, front = base.frontend_forward(xa, dither_seed=base.fused_pass_seed(dkey, it, r))
    if level == 2:
        feats = base.comput_feat_from_feat(feats)
    comp, sv = replay.fwd(feats, seed=base.fused_pass_seed(fkey, it, r), row_keys=(0, 0, 0))
    d_, s_, l_, g = base.loss_grad(comp, y, spec, flag=level, want_grad=want_grad)
    return d_, s_, l_, (replay.bwd(sv, g) if want_grad else None), front


def _to_wave(base, level, front, df):
    return base.frontend_backward(front, base.cmvn_backward(df) if level == 2 else df)


def _run_loop(base, level, init, x, y, R, seed=3):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import FeCoDefense
    lower, upper = _bounds(x)
    _fresh(base)
    feco = FeCoDefense(0.5, init=init, seed=seed)
    out = base.pgd_run_feco(x, y, lower, upper, SEC4SR_CrossEntropy(), STEP, ITERS, 1, feco, eot_size=R, eot_batch_size=R, trace=True,
                            level=level)
    assert feco.calls == 1
    return out


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_randomised_loop_equals_replay(bases, xy, case, level):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import FeCoDefense
    dither, init = CASES[case]
    base, (x, y) = bases[dither], xy
    x, y = x[:B], y[:B]
    spec, R = SEC4SR_CrossEntropy(), 2
    lower, upper = _bounds(x)
    adv, success, dec, scores, loss, ltr, dtr = _run_loop(base, level, init, x, y, R)
    dkey, fkey = base.last_fused_seed, base.last_fused_feco_seed
    replay = FeCoDefense(0.5, init=init, seed=123)  # its keys are given explicitly
    xa = x.clone()
    for it in range(ITERS):
        tot, lsum, decs, front = None, None, [], None
        for r in range(R):
            d_, _, l_, df, front = _pass(base, replay, level, xa, y, spec, dkey, fkey, it, r)
            # dither: every repeat has its own front-end pass, the sum is taken at the waveform; only the defense random: the
            # repeats share one front-end pass and are summed at FeCo's input level -- both in repeat order
            g = _to_wave(base, level, front, df) if dither else df
            tot = g if tot is None else tot + g
            lsum = l_ if lsum is None else lsum + l_
            decs.append(d_.cpu().tolist())
        if not dither:
            tot = _to_wave(base, level, front, tot)
        assert np.array_equal(lsum.cpu().numpy() / np.float32(R), ltr[it].cpu().numpy()), (case, level, it)
        assert dtr[it].cpu().tolist() == [Counter(decs[r][b] for r in range(R)).most_common(1)[0][0] for b in range(B)]
        base.pgd_update(xa, tot.contiguous(), lower, upper, STEP, 1)
    assert torch.equal(adv, xa), (case, level, float((adv - xa).abs().max()))
    assert not torch.equal(adv, x)
    d_, s_, l_, _, _ = _pass(base, replay, level, xa, y, spec, dkey, fkey, ITERS, 0, want_grad=False)  # the final pass: one repeat
    assert torch.equal(dec, d_) and torch.equal(scores, s_) and torch.equal(loss, l_)
    assert torch.equal(ltr[ITERS], loss) and torch.equal(dtr[ITERS], dec)
    assert success.bool().tolist() == (d_ != y).tolist()


def test_randomised_configurations_take_the_loop_only_on_request(bases, xy, monkeypatch):
    """by default an attack with dither or random init keeps the step loop and its noise (the two routes key both differently)"""
    from speakerguard_amd.defense.feature_level import FeCoDefense
    base, (x, y) = bases[1.0], xy
    calls = _count_calls(base, monkeypatch)
    kw = dict(EOT_size=2, EOT_batch_size=2)
    _attack(base, 1, FeCoDefense(0.5, init='random', seed=3), x[:B], y[:B], **kw)
    assert ENTRY not in calls and calls.count("sg_xv_loss_grad") == ITERS + 1  # (one call of 2 B rows per step)
    del calls[:]
    a1 = _attack(base, 1, FeCoDefense(0.5, init='random', seed=3), x[:B], y[:B], fuse_randomised_feco=True, **kw)[0]
    assert calls.count(ENTRY) == 1 and "sg_xv_loss_grad" not in calls
    # the same seed twice gives the same audio, another seed another
    a2, a3 = (_attack(base, 1, FeCoDefense(0.5, init='random', seed=s), x[:B], y[:B], fuse_randomised_feco=True, **kw)[0] for s in (3, 4))
    assert torch.equal(a1, a2) and not torch.equal(a1, a3) and float((a1 - x[:B]).abs().max()) <= EPS + 1e-7


# ---------------------------------------------------------------- 6. grouping
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case", ["b-dither-random", "c-random-only"])
def test_two_groups_equal_one(bases, xy, case, level, monkeypatch):
    """EOT 4 as 2 + 2 repeats (SG_EOT_MAX_ROWS = 6 rows per pass).  With dither the overlap-add carries the first group's sum;
    with only the defense random the feature-level sum is carried and ONE adjoint follows the second group."""
    dither, init = CASES[case]
    base, (x, y) = bases[dither], xy
    monkeypatch.delenv("SG_EOT_MAX_ROWS", raising=False)
    one = _run_loop(base, level, init, x[:B], y[:B], 4)
    monkeypatch.setenv("SG_EOT_MAX_ROWS", str(2 * B))
    two = _run_loop(base, level, init, x[:B], y[:B], 4)
    # the knob counted: a stage trace of either form shows one clustering launch per pass -- ITERS steps of one or two groups,
    # and the final pass
    n_fwd = lambda: sum(name == "xv_feco_fwd" for name, _ in base.trace_stages(lambda: _run_loop(base, level, init, x[:B], y[:B], 4)))  # noqa: E731
    assert n_fwd() == 2 * ITERS + 1
    monkeypatch.delenv("SG_EOT_MAX_ROWS")
    assert n_fwd() == ITERS + 1
    for a, b in zip(one, two):
        assert torch.equal(a, b), (case, level)
    assert not torch.equal(one[0], x[:B])


# ---------------------------------------------------------------- 7. the row-wise clustering launch alone
@pytest.mark.parametrize("two_cu", [-1, 0], ids=["two-cu", "one-cu"])
@pytest.mark.parametrize("random_init", [1, 0], ids=["random", "even"])
def test_rowwise_clustering_equals_single_row_calls(two_cu, random_init):
    from speakerguard_amd import _native as N
    from speakerguard_amd.metric.metric import _context
    from speakerguard_amd.model._engine_ops import REP_KEY_STRIDE
    Bk, R, Fk, D, k, iters, seed, index_base = 3, 2, 98, 30, 49, 10, 0x1234567890ABCDEF, 11
    dev = torch.device(DEV)
    ctx, s = _context(dev), N.current_stream_ptr(dev)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(R * Bk, Fk, D, generator=g).to(dev)  # every row differs
    ids = torch.full((R * Bk, Fk), -7, device=dev, dtype=torch.int32)
    out = torch.full((R * Bk, k, D), float("nan"), device=dev)
    cnt = torch.full((R * Bk, k), -7, device=dev, dtype=torch.int32)
    ctx.call("sg_feco_set_two_cu", two_cu)
    try:
        ctx.call("sg_feco_kmeans_compress_rows", N._ptr(feats), Bk, Fk, D, k, iters, random_init, C.c_uint64(seed), index_base, R,
                 N._ptr(ids), N._ptr(out), N._ptr(cnt), s)
        for r in range(R):
            for u in range(Bk):
                row = r * Bk + u
                i1 = torch.empty(1, Fk, device=dev, dtype=torch.int32)
                o1 = torch.empty(1, k, D, device=dev)
                c1 = torch.empty(1, k, device=dev, dtype=torch.int32)
                ctx.call("sg_feco_kmeans_compress", N._ptr(feats[row:row + 1].contiguous()), 1, Fk, D, k, iters, random_init,
                         C.c_uint64((seed + r * REP_KEY_STRIDE) & 0xFFFFFFFFFFFFFFFF), index_base + u, 1, N._ptr(i1), N._ptr(o1), N._ptr(c1), s)
                assert torch.equal(ids[row], i1[0]) and torch.equal(cnt[row], c1[0]) and torch.equal(out[row], o1[0]), (r, u)
    finally:
        ctx.call("sg_feco_set_two_cu", -1)
    assert int(cnt.sum()) == R * Bk * Fk and int(ids.min()) >= 0 and int(ids.max()) < k
    if random_init:  # the repeats of an utterance start from different frames, and so do the utterances of a repeat
        assert not torch.equal(ids[0], ids[Bk]) and not torch.equal(ids[0], ids[1])


# ---------------------------------------------------------------- 8. shards
@pytest.mark.parametrize("level", [1, 2])
def test_shards_equal_the_whole(bases, xy, level):
    """noise -- dither and initial frames -- depends on (utterance, step, repeat) only: 4 utterances cut as 2 + 2, each shard
    with its index offset, reproduce the uncut batch"""
    from speakerguard_amd.defense.feature_level import FeCoDefense
    base, (x, y) = bases[1.0], xy
    kw = dict(EOT_size=2, EOT_batch_size=2, fuse_randomised_feco=True)
    make = lambda: FeCoDefense(0.5, init='random', seed=3)  # noqa: E731
    whole = _attack(base, level, make(), x, y, **kw)[0]
    head = _attack(base, level, make(), x[0:2], y[0:2], **kw)[0]
    tail = _attack(base, level, make(), x[2:4], y[2:4], index_offset=2, **kw)[0]
    assert torch.equal(whole, torch.cat((head, tail), 0)) and not torch.equal(whole, x)
    shifted = _attack(base, level, make(), x[2:4], y[2:4], index_offset=1, **kw)[0]  # as other global utterances: other noise
    assert not torch.equal(shifted, tail)
