"""FeCo with the cosine distance on the device (sg_feco_kmeans_compress_metric, ``FeCoDefense(other_param='cos')``): ids, cluster
means and counts bit for bit against the contract's restatement (tests/feco_cos_restate.py), the L2 metric against the entries it
stands for, the repeat forms against single-row calls, the gradient against autograd, and the defense under PGD through the
step-by-step route."""
import ctypes as C

import numpy as np
import pytest
import torch

import feco_cos_restate as R
from conftest import log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
L2, COS = 0, 1


def _ctx():
    from speakerguard_amd.metric.metric import _context
    return _context(DEV)


def _metric(feat, B, k, metric, random_init=0, seed=0, index_base=0, reps=1, row_wise=0, max_iter=10):
    """sg_feco_kmeans_compress_metric on feat ((B,F,D), or (reps*B,F,D) when row_wise) -> ids, out, counts on reps*B rows"""
    from speakerguard_amd import _native as N
    feat = feat.to(DEV).contiguous()
    F, D = feat.shape[1:]
    ids = torch.full((reps * B, F), -7, device=DEV, dtype=torch.int32)
    out = torch.full((reps * B, k, D), float('nan'), device=DEV)
    counts = torch.full((reps * B, k), -7, device=DEV, dtype=torch.int32)
    _ctx().call("sg_feco_kmeans_compress_metric", N._ptr(feat), B, F, D, k, max_iter, metric, random_init, C.c_uint64(seed),
                int(index_base), reps, row_wise, N._ptr(ids), N._ptr(out), N._ptr(counts), N.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return ids, out, counts


def _compress(feat, ids, k):
    from speakerguard_amd import _native as N
    feat = feat.to(DEV).contiguous()
    B, F, D = feat.shape
    out = torch.empty(B, k, D, device=DEV)
    counts = torch.empty(B, k, device=DEV, dtype=torch.int32)
    _ctx().call("sg_feco_compress", N._ptr(feat), N._ptr(ids), B, F, D, k, N._ptr(out), N._ptr(counts), N.current_stream_ptr(DEV))
    return out, counts


_POOL = {}


def _features(B, F, D, seed=70):
    """oracle-style features (mean |x| 6 .. 10, like the CPU test's): D 30 the oracle's MFCC, 32 its log-mel, wider ones the
    MFCC with log-mel columns behind it; the first F frames of 3 s utterances (more frames than those have: row b is the utterances
    b, b + 1, b + 2, b, ... one after the other -- from frame 900 on it repeats its own frames, exact ties)"""
    from oracle import audionet as oan
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    if F > 300:
        f = _features(3, 300, D, seed)
        return torch.cat([f.roll(-i, 0) for i in range((F + 299) // 300)], dim=1)[:B, :F].contiguous()
    if seed not in _POOL:
        x = torch.from_numpy(synth.make_waveforms(3, 48000, seed=seed))
        mfcc = kaldi_mfcc.mfcc_batch(x * 32768.0).float()
        logmel = oan.preprocess(x.reshape(3, -1)).transpose(1, 2).float()
        n = min(mfcc.shape[1], logmel.shape[1])
        _POOL[seed] = torch.cat([mfcc[:, :n], logmel[:, :n]], dim=2).contiguous()
    pool = _POOL[seed]
    assert B <= pool.shape[0] and F <= pool.shape[1]
    f = pool[:B, :F, 30:62] if D == 32 else pool[:B, :F, :D]
    assert 6.0 <= f.abs().mean().item() <= 10.0
    return f.contiguous()


def _restated(feat, k, seed=None, index_base=0, max_iter=10):
    """ids (B,F), out (B,k,D), counts (B,k) of the restatement; utterance b has global index index_base + b"""
    ids, out, counts = [], [], []
    for b in range(feat.shape[0]):
        x = feat[b].numpy()
        frames = R.init_frames(x.shape[0], k, seed, index_base + b)
        i = R.kmeans_ids(x, k, max_iter, frames)
        o, c = R.compress(x, i, k)
        ids.append(i), out.append(o), counts.append(c)
    return np.stack(ids), np.stack(out), np.stack(counts)


def _same_bits(got, want):
    ids, out, counts = got
    return (np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
            and np.array_equal(counts.cpu().numpy(), want[2]))


SHAPES = [(50, 25, 30),     # one centroid tile, D padded to 32
          (200, 100, 32),   # several tiles, chunked units, two-CU eligible
          (300, 150, 32),   # the schedule the kernel's comments are written for
          (70, 14, 40),     # DPAD 64, never paired
          (33, 33, 30),     # k = F
          (40, 1, 30),      # k = 1
          (1025, 65, 32)]   # 33 frame tiles: no unit table (dealt in the kernel), the slow member lists, frames not in LDS


@pytest.mark.parametrize("F,k,D", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_bit_equal_to_the_restatement(F, k, D):
    feat = _features(3, F, D)
    want = {None: _restated(feat, k), 21: _restated(feat, k, 21, 5)}
    ctx = _ctx()
    try:
        for two_cu in (-1, 0):
            ctx.call("sg_feco_set_two_cu", two_cu)
            for seed in (None, 21):
                got = _metric(feat, 3, k, COS, int(seed is not None), seed or 0, 5)
                differ = int((got[0].cpu().numpy() != want[seed][0]).sum())
                assert _same_bits(got, want[seed]), (two_cu, seed, "%d ids differ" % differ)
                out2, counts2 = _compress(feat, got[0], k)
                assert torch.equal(got[1], out2) and torch.equal(got[2], counts2)
    finally:
        ctx.call("sg_feco_set_two_cu", -1)
    assert not np.array_equal(want[None][0], want[21][0]) or k in (1, F)
    log("cosine FeCo %dx%dx%d: ids, means, counts bit-equal to the restatement (even + seeded, one and two CUs), empty clusters %d"
        % (F, k, D, int((want[None][2] == 0).sum())))


def test_degenerate_rows_stay_finite_and_equal_the_restatement():
    """the first five frames all zero -- initial centroids with n_j = 0 -- and two identical frames: exact ties"""
    feat = _features(3, 40, 30)[2:3].clone()
    feat[0, :5] = 0
    feat[0, 21] = feat[0, 20]
    for k in (20, 40):
        for seed in (None, 4):
            st = {}
            x = feat[0].numpy()
            ids = R.kmeans_ids(x, k, 10, R.init_frames(40, k, seed, 0), stats=st)
            assert st['ties'] > 0 and (seed is not None or st['zero_norm'] >= 3)
            got = _metric(feat, 1, k, COS, int(seed is not None), seed or 0, 0)
            out, counts = R.compress(x, ids, k)
            assert _same_bits(got, (ids[None], out[None], counts[None])), (k, seed)
            assert torch.isfinite(got[1]).all() and int(got[0].min()) >= 0 and int(got[0].max()) < k and int(got[2].sum()) == 40
            assert int(got[0][0, 20]) == int(got[0][0, 21])


def test_l2_metric_is_the_old_entries_bit_for_bit():
    from speakerguard_amd import _native as N
    ctx, s = _ctx(), N.current_stream_ptr(DEV)
    B, F, D, k, reps = 3, 200, 32, 100, 2
    feat = _features(B, F, D).to(DEV)
    rows = torch.cat([feat, feat.flip(1)]).contiguous()  # (reps * B, F, D): the repeats' own features
    for entry, src, row_wise, random_init in (("sg_feco_kmeans_compress", feat, 0, 1), ("sg_feco_kmeans_compress_rows", rows, 1, 1),
                                              ("sg_feco_kmeans_compress_rows", rows, 1, 0)):
        ids = torch.empty(reps * B, F, device=DEV, dtype=torch.int32)
        out = torch.empty(reps * B, k, D, device=DEV)
        counts = torch.empty(reps * B, k, device=DEV, dtype=torch.int32)
        ctx.call(entry, N._ptr(src), B, F, D, k, 10, random_init, C.c_uint64(77), 3, reps, N._ptr(ids), N._ptr(out), N._ptr(counts), s)
        got = _metric(src, B, k, L2, random_init, 77, 3, reps, row_wise)
        assert torch.equal(got[0], ids) and torch.equal(got[1], out) and torch.equal(got[2], counts), entry
        cos = _metric(src, B, k, COS, random_init, 77, 3, reps, row_wise)
        assert not torch.equal(cos[0], ids)  # another distance, other clusters
    with pytest.raises(N.NativeError):
        _metric(feat, B, k, 2)
    with pytest.raises(N.NativeError):  # repeats of the evenly started clustering coincide
        _metric(feat, B, k, COS, 0, 0, 0, 2, 0)


def test_cosine_repeat_forms_equal_single_row_calls():
    """reps = 3 on shared features and row_wise with reps = 2: instance (u, r) is the single-row call with key
    seed + r * 0xC2B2AE3D27D4EB4F and utterance index_base + u"""
    B, F, D, k, seed, base = 2, 70, 30, 35, 1234567, 9
    feat = _features(B, F, D)
    ids, out, counts = _metric(feat, B, k, COS, 1, seed, base, 3, 0)
    for r in range(3):
        for u in range(B):
            one = _metric(feat[u:u + 1], 1, k, COS, 1, (seed + r * R.REP_KEY) & 0xFFFFFFFFFFFFFFFF, base + u)
            row = r * B + u
            assert torch.equal(ids[row], one[0][0]) and torch.equal(out[row], one[1][0]) and torch.equal(counts[row], one[2][0]), (r, u)
    assert not torch.equal(ids[:B], ids[B:2 * B])
    rows = torch.cat([feat, _features(3, F, D)[1:3].flip(1)]).contiguous()  # every repeat has features of its own
    for random_init in (1, 0):
        ids, out, counts = _metric(rows, B, k, COS, random_init, seed, base, 2, 1)
        for r in range(2):
            for u in range(B):
                row = r * B + u
                one = _metric(rows[row:row + 1], 1, k, COS, random_init, (seed + r * R.REP_KEY) & 0xFFFFFFFFFFFFFFFF, base + u)
                assert torch.equal(ids[row], one[0][0]) and torch.equal(out[row], one[1][0]) and torch.equal(counts[row], one[2][0])


def test_gradient_is_autograd_through_the_reference_step():
    """the same backward kernel as the L2 defense, the same tolerance (tests/test_gpu_feco.py: 1e-6 absolute)"""
    from oracle import feco
    from speakerguard_amd.defense.feature_level import FeCoDefense
    rs = np.random.RandomState(6)
    base = rs.randn(1, 10, 4).astype(np.float32)
    single = torch.from_numpy(np.repeat(base, 3, axis=1))  # 30 frames, 10 distinct: k = 15 leaves clusters empty
    for feat in (_features(2, 60, 30), torch.cat([single, single.flip(1)]), single):
        B, F, D = feat.shape
        d = FeCoDefense(0.5, other_param='cos')
        out, saved = d.fwd(feat.to(DEV))
        ids, k = saved[0].cpu().numpy(), F // 2
        x = feat.clone().requires_grad_(True)
        want = [feco.compress_from_ids(x[b], ids[b], k, force=B > 1) for b in range(B)]
        want = torch.stack(want)
        assert tuple(out.shape) == tuple(want.shape)
        if B == 1:
            assert want.shape[1] < k  # empty clusters were dropped
        g = torch.from_numpy(rs.randn(*want.shape).astype(np.float32))
        (want * g).sum().backward()
        got = d.bwd(saved, g.to(DEV))
        # forward: both sides are float32 means of at most n frames of magnitude <= M, the device's summed in ascending order,
        # torch.mean's pairwise: each within (n - 1) u M of the exact mean, plus the division's rounding, u = 2^-24
        n, M = int(saved[1].max()), feat.abs().max().item()
        assert (out.cpu() - want.detach()).abs().max().item() <= (2 * (n - 1) + 2) * 2.0 ** -24 * M
        assert (got.cpu() - x.grad).abs().max().item() < 1e-6


@pytest.fixture(scope="module")
def xv(xv_weights):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=DEV, dither=0.0)


@pytest.fixture(scope="module")
def an():
    from speakerguard_amd import synth
    from speakerguard_amd.model.audionet_csine import audionet_csine
    return audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV)


@pytest.fixture(scope="module")
def waves():
    from speakerguard_amd import synth
    return torch.from_numpy(synth.make_waveforms(4, 32000, seed=72)).to(DEV)


def test_reference_signature_route(xv, waves):
    from speakerguard_amd.defense.feature_level import FeCo, FeCoDefense
    f = xv.compute_feat(waves, flag=1)
    got = FeCo(f, 'kmeans', 0.5, 'cos')
    assert torch.equal(got, FeCoDefense(0.5, other_param='cos')(f))
    assert not torch.equal(got, FeCo(f, 'kmeans', 0.5, 'L2'))
    with pytest.raises(AssertionError):
        FeCoDefense(0.5, other_param='cos')(f[:, :, :29])  # feature_level.py:183: an even dimension
    with pytest.raises(NotImplementedError):
        FeCo(f, 'kmeans', 0.5, 'cosine')


@pytest.mark.parametrize("which,level", [("xv", 1), ("xv", 2), ("an", 1)])
def test_pgd_against_the_cosine_defense_takes_the_step_route(which, level, xv, an, waves):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    base = xv if which == "xv" else an
    dm = defended_model(base, defense=[(level, FeCoDefense(0.5, other_param='cos'))])
    y = dm.make_decision(waves)[0]
    atk = PGD(dm, epsilon=0.002, step_size=0.0004, max_iter=5, batch_size=4, verbose=0)
    assert atk._device_route(4) is None
    assert PGD(defended_model(base, defense=[(level, FeCoDefense(0.5))]), verbose=0)._device_route(4) is not None
    adv, success = atk.attack(waves, y)
    assert (adv - waves).abs().max().item() <= 0.002 + 1e-7 and adv.abs().max().item() <= 1.0
    l0 = dm.loss_grad(waves, y, SEC4SR_CrossEntropy(), want_grad=False)[2]
    l1 = dm.loss_grad(adv, y, SEC4SR_CrossEntropy(), want_grad=False)[2]
    log("PGD-5 vs cosine FeCo at level %d of %s: CE loss %s -> %s, success %s" % (level, which, l0.cpu().numpy().round(3),
                                                                                l1.cpu().numpy().round(3), success))
    assert (l1 >= l0 - 1e-4).all()  # untargeted CE ascent


def test_randomised_cosine_defense_with_eot_is_reproducible(an, waves):
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    y = defended_model(an, defense=[(1, FeCoDefense(0.5, other_param='cos'))]).make_decision(waves)[0]

    def run(seed):
        d = FeCoDefense(0.5, other_param='cos', init='random', seed=seed)
        a = PGD(defended_model(an, defense=[(1, d)]), epsilon=0.002, step_size=0.0004, max_iter=3, batch_size=4, EOT_size=2,
                EOT_batch_size=1, verbose=0)
        assert a._device_route(4) is None
        an._noise_epoch = 0
        adv, succ = a.attack(waves, y)
        return adv, succ, d.calls

    a1, s1, calls = run(5)
    a2, s2, _ = run(5)
    a3, _, _ = run(6)
    assert calls >= 3 * 2  # the step loop calls the defense once per step and repeat (and for the final decisions)
    assert torch.equal(a1, a2) and list(s1) == list(s2) and not torch.equal(a1, a3)
    assert (a1 - waves).abs().max().item() <= 0.002 + 1e-7
