"""FeCo with warped k-means on the device (csrc/k_feco_warped.hip, defense.feature_level.WarpedFeCoDefense): the kernel against
the contract's restatement bit for bit, against the reference's own code (tests/golden/feco_warped_ref.npz), its keyed random
init, its refusals, and PGD through the defended x-vector and AudioNet models on the host-chained path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import feco_warped_restate as R
from conftest import GOLDEN, log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _walk(B, F, D, seed):
    rs = np.random.RandomState(seed)
    return np.cumsum(rs.randn(B, F, D).astype(np.float32) * 0.3, axis=1).astype(np.float32)


def _mfcc(B, F, seed):
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, F * 160, seed=seed))
    with torch.no_grad():
        return XvPlda(synth.make_xv_weights()).compute_feat(x, flag=1).numpy().astype(np.float32)


def _logmel(B, seed):
    from oracle.audionet import AudioNet
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=seed))
    with torch.no_grad():
        return AudioNet(synth.make_audionet_state_dict(seed=0, num_class=251)).compute_feat(x, flag=1).numpy().astype(np.float32)


def _check_rows(tag, feats, d, out, saved, init, delta=0.0, key=0, index_base=0):
    ids, counts, (B, F, D, k) = saved
    out, ids, counts = out.cpu().numpy(), ids.cpu().numpy(), counts.cpu().numpy()
    bnd, sweeps = d.last_boundaries.cpu().numpy(), d.last_sweeps.cpu().numpy()
    for b in range(B):
        r = R.warped(feats[b], k, init, delta, key=key, utt=index_base + b)
        assert np.array_equal(out[b], r["means"]), (tag, b, np.abs(out[b] - r["means"]).max())
        assert np.array_equal(bnd[b], r["bnd"]), (tag, b)
        assert np.array_equal(ids[b], r["init_ids"]) and np.array_equal(counts[b], r["init_counts"]), (tag, b)
        assert sweeps[b] == r["sweeps"] > 0, (tag, b, sweeps[b], r["sweeps"])
    return sweeps


SHAPES = [  # tag, B, F, D, ratio, init, delta, features
    ("mfcc 64x300x30 k150", 64, 300, 30, 0.5, "ts", 0.0, "mfcc"),
    ("logmel 8x300x32 k60", 8, 300, 32, 0.2, "ts", 0.0, "logmel"),
    ("mfcc 3x60x30 k30", 3, 60, 30, 0.5, "random", 0.0, "mfcc"),
    ("mfcc 2x1200x30 k600", 2, 1200, 30, 0.5, "ts", 0.0, "mfcc"),
    ("walk 4x200x64 k100 delta", 4, 200, 64, 0.5, "ts", 0.1, "walk"),
    ("walk 2x1200x64 k1200 (k = F, frames and means off LDS)", 2, 1200, 64, 1.0, "random", 0.0, "walk"),
    ("walk 3x50x30 k1", 3, 50, 30, 0.02, "ts", 0.0, "walk"),
    ("walk 3x40x30 k=F", 3, 40, 30, 1.0, "random", 0.0, "walk"),  # (TS at k = F is degenerate unless the path is even)
    ("walk 5x300x30 k150 random", 5, 300, 30, 0.5, "random", 0.0, "walk"),
]


@pytest.mark.parametrize("tag,B,F,D,ratio,init,delta,kind", SHAPES, ids=[s[0].split(" (")[0] for s in SHAPES])
def test_kernel_matches_restatement_bit_for_bit(tag, B, F, D, ratio, init, delta, kind):
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    feats = {"mfcc": lambda: _mfcc(B, F, 21), "logmel": lambda: _logmel(B, 22), "walk": lambda: _walk(B, F, D, 23)}[kind]()
    assert feats.shape == (B, F, D)
    d = WarpedFeCoDefense(ratio, init, delta=delta)
    key = 0x1234567890ABCDEF
    out, saved = d.fwd(torch.from_numpy(feats).to(DEV), seed=key, row_keys=(17, 0, 0))
    assert saved[2][3] == int(F * ratio)
    sw = _check_rows(tag, feats, d, out, saved, init, delta, key=key, index_base=17)
    log("warped %s: bit-exact, sweeps %d..%d" % (tag, sw.min(), sw.max()))


def test_kernel_matches_the_reference_fixture():
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    z = np.load(os.path.join(GOLDEN, "feco_warped_ref.npz"))
    cases = json.loads(str(z["meta"]))["cases"]
    for tag in cases:
        x, ratio, init, delta = z[tag + "_feat"], float(z[tag + "_ratio"]), str(z[tag + "_init"]), float(z[tag + "_delta"])
        d = WarpedFeCoDefense(ratio, init, delta=delta)
        feat = torch.from_numpy(x[None]).to(DEV)
        given = None if init == "ts" else torch.from_numpy(z[tag + "_init_bnd"][None])  # the reference's recorded draw
        out, saved = d.fwd(feat, boundaries=given)
        assert np.array_equal(d.last_boundaries.cpu().numpy()[0], z[tag + "_bnd"]), tag
        np.testing.assert_allclose(out.cpu().numpy()[0], z[tag + "_out"], rtol=0, atol=1e-5 * np.abs(x).max(), err_msg=tag)
        g = d.bwd(saved, torch.from_numpy(z[tag + "_cot"][None]).to(DEV))
        np.testing.assert_allclose(g.cpu().numpy()[0], z[tag + "_dfeat"], rtol=0, atol=1e-6, err_msg=tag)
    log("warped: %d reference cases, boundaries equal, means and gradient within tolerance" % len(cases))


def test_keyed_random_init():
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    F, D, ratio = 300, 30, 0.5
    k = int(F * ratio)
    feats = _walk(8, F, D, 31)
    x = torch.from_numpy(feats).to(DEV)
    d = WarpedFeCoDefense(ratio, "random", seed=5)
    a, sa = d.fwd(x)
    ba = d.last_boundaries.clone()
    b, _ = d.fwd(x)  # the next call draws afresh
    assert not torch.equal(ba, d.last_boundaries) and not torch.equal(a, b)
    ids0 = sa[0].cpu().numpy()
    for r in range(8):  # the initial cut: k distinct sorted frames in [1, F-1] after 0, restated
        b0 = np.flatnonzero(np.diff(ids0[r])) + 1
        assert len(b0) == k - 1 and b0.min() >= 1 and b0.max() <= F - 1
        assert np.array_equal(np.concatenate([[0], b0]), R.random_boundaries(d.call_seed(0), r, F, k))
    # one call on 8 rows == calls on rows 0-2 and 3-7 with the matching keys
    key = 0xDEADBEEF12345
    whole, sw = d.fwd(x, seed=key, row_keys=(40, 0, 0))
    bw = d.last_boundaries.clone()
    p1, _ = d.fwd(x[:3], seed=key, row_keys=(40, 0, 0))
    b1 = d.last_boundaries.clone()
    p2, _ = d.fwd(x[3:], seed=key, row_keys=(43, 0, 0))
    assert torch.equal(whole, torch.cat([p1, p2])) and torch.equal(bw, torch.cat([b1, d.last_boundaries]))
    # EOT repeats: 2 x 4 rows in one call == the second repeat on its own (rows that start inside a repeat)
    rep, _ = d.fwd(x, seed=key, row_keys=(40, 0, 4))
    q2, _ = d.fwd(x[4:], seed=key, row_keys=(40, 4, 4))
    assert torch.equal(rep[4:], q2)
    q1, _ = d.fwd(x[4:], seed=(key + 0xC2B2AE3D27D4EB4F) & 0xFFFFFFFFFFFFFFFF, row_keys=(40, 0, 0))
    assert not torch.equal(rep[:4], rep[4:])
    _check_rows("repeat 1", feats[4:], d, q1, _, "random", key=(key + 0xC2B2AE3D27D4EB4F) & 0xFFFFFFFFFFFFFFFF, index_base=40)
    assert torch.equal(rep[4:], q1)


def _raw_call(feats, k, mode=0, boundaries=None):
    from speakerguard_amd import _native as N
    from speakerguard_amd.metric.metric import _context
    B, F, D = feats.shape
    ctx = _context(DEV)
    out = torch.full((B, max(k, 1), D), 7.0, device=DEV)
    bnd = torch.zeros(B, max(k, 1), dtype=torch.int32, device=DEV) if boundaries is None else boundaries.to(DEV).int().contiguous()
    ids = torch.empty(B, F, dtype=torch.int32, device=DEV)
    counts = torch.empty(B, max(k, 1), dtype=torch.int32, device=DEV)
    sweeps = torch.empty(B, dtype=torch.int32, device=DEV)
    rc = ctx.lib.sg_feco_warped(ctx.handle, N._ptr(feats), B, F, D, k, mode, C.c_double(0.0), C.c_uint64(1), C.c_int64(0), 0,
                                N._ptr(bnd), N._ptr(ids), N._ptr(counts), N._ptr(out), N._ptr(sweeps),
                                N.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, ctx.lib.sg_last_error(ctx.handle).decode(), out, sweeps


def test_refusals():
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    z = np.load(os.path.join(GOLDEN, "feco_warped_ref.npz"))
    deg, kd = z["degenerate_feat"], int(z["degenerate_k"])
    good = _walk(1, 40, 30, 3)[0]
    feats = torch.from_numpy(np.stack([good, deg])).to(DEV)
    rc, msg, out, sweeps = _raw_call(feats, kd)
    assert rc == 1 and "row 1" in msg, (rc, msg)
    assert bool(torch.isfinite(out).all()) and float(out[1].abs().max()) == 0.0 and int(sweeps[1]) == -1 and int(sweeps[0]) > 0
    with pytest.raises(ValueError, match="row 0"):
        WarpedFeCoDefense(0.5, "ts")(torch.from_numpy(deg[None]).to(DEV))
    with pytest.raises(ValueError):  # given boundaries that do not rise
        WarpedFeCoDefense(0.5, "ts").fwd(torch.from_numpy(good[None]).to(DEV), boundaries=torch.tensor([[0] + [3] * 19]))
    x = torch.zeros(1, 1201, 30, device=DEV)
    assert _raw_call(x, 600)[0] == 1
    with pytest.raises(ValueError):
        WarpedFeCoDefense(0.5, "ts")(x)
    assert _raw_call(torch.zeros(1, 100, 65, device=DEV), 50)[0] == 1
    assert _raw_call(torch.zeros(1, 100, 30, device=DEV), 0)[0] == 1
    assert _raw_call(torch.zeros(1, 100, 30, device=DEV), 101)[0] == 1
    for ratio in (0.001, 1.5):
        with pytest.raises(ValueError):
            WarpedFeCoDefense(ratio, "ts")(torch.zeros(1, 100, 30, device=DEV))


def test_pgd10_through_warped_feco_on_xv_plda(xv_weights):
    """PGD-10 against defended_model(xv_plda, [(1, WarpedFeCoDefense(0.5, 'ts'))]) on 8 utterances x 3 s, host-chained,
    vs an oracle loop: the oracle x-vector model + the restatement with the reference's autograd quirk + torch autograd.
    eps 0.0005 leaves one utterance un-fooled.  (The segmentation is discrete: once the two trajectories differ in a sample,
    boundaries can move differently and the paths part faster than through the L2 k-means -- at eps 0.002 ~22 % of the
    samples differ after ten steps, with equal outcomes; here ~4 %.)"""
    from oracle import attacks as oatk
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.model.xv_plda import xv_plda
    from test_gpu_full_configs import _compare
    eps, step, K, B, ratio = 0.0005, 0.0001, 10, 8, 0.5
    hip, ora = xv_plda.from_weights(xv_weights, device=DEV, dither=0.0), XvPlda(xv_weights, faithful=False, freeze=True)

    class OracleDefended:
        threshold = -np.inf

        def make_decision(self, xx):
            feats = ora.compute_feat(xx, flag=1)
            k = int(feats.shape[1] * ratio)
            comp = [R.torch_with_quirk(feats[b], R.warped(feats[b].detach().numpy(), k, "ts")) for b in range(feats.shape[0])]
            return ora.make_decision(torch.stack(comp), flag=1)

    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=3))
    dm, om = defended_model(hip, defense=[(1, WarpedFeCoDefense(ratio, 'ts'))]), OracleDefended()
    y = dm.make_decision(x.to(DEV))[0].cpu()
    with torch.no_grad():
        assert om.make_decision(x)[0].tolist() == y.tolist()
    atk = PGD(dm, task="CSI", epsilon=eps, step_size=step, max_iter=K, batch_size=B, verbose=0)
    assert atk._device_route(B) is None  # the host-chained path
    adv, succ = atk.attack(x.to(DEV), y.to(DEV))
    oadv, osucc = oatk.PGD(om, task="CSI", epsilon=eps, step_size=step, max_iter=K, batch_size=B).attack(x, y)

    def odec(a):
        with torch.no_grad():
            return om.make_decision(a)[0]
    _compare("PGD-10 vs warped-FeCo-defended xv_plda x 8 x 3 s", x, adv, succ, oadv, osucc, lambda a: dm.make_decision(a)[0],
             odec, eps, K)


def test_level2_gradient_through_warped_feco_on_xv_plda(xv_weights):
    """Level 2 (after CMVN) on the host-chained path: loss and gradient agree with the oracle + restatement + autograd."""
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.model.xv_plda import xv_plda
    B, ratio = 4, 0.5
    hip, ora = xv_plda.from_weights(xv_weights, device=DEV, dither=0.0), XvPlda(xv_weights, faithful=False, freeze=True)
    dm = defended_model(hip, defense=[(2, WarpedFeCoDefense(ratio, 'ts'))])
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=5))
    y = torch.arange(B) % 10
    loss_fn = SEC4SR_CrossEntropy(reduction='none', task='CSI')
    _, _, loss, g = dm.loss_grad(x.to(DEV), y.to(DEV), loss_fn)
    xo = x.clone().requires_grad_(True)
    cm = ora.compute_feat(xo, flag=2)
    k = int(cm.shape[1] * ratio)
    comp = torch.stack([R.torch_with_quirk(cm[b], R.warped(cm[b].detach().numpy(), k, "ts")) for b in range(B)])
    oloss = torch.nn.functional.cross_entropy(ora.forward(comp, flag=2), y, reduction='none')
    oloss.sum().backward()
    np.testing.assert_allclose(loss.cpu().numpy(), oloss.detach().numpy(), rtol=2e-3, atol=2e-3)
    go, gh = xo.grad.flatten(1), g.cpu().flatten(1)
    cos = torch.nn.functional.cosine_similarity(go, gh, dim=1)
    log("warped level 2: loss max |diff| %.2e, gradient cosine min %.6f" % ((loss.cpu() - oloss.detach()).abs().max(), cos.min()))
    assert float(cos.min()) > 0.999


def test_audionet_level1_random_eot():
    """AudioNet with warped FeCo ('random') at level 1, PGD-5 with EOT 2 on 4 utterances: the host-chained loop runs, the
    defended cross-entropy does not fall, and the result stays in the eps ball."""
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.defended_model import defended_model
    eps, step, K, B = 0.002, 0.0004, 5, 4
    hip = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=DEV)
    dm = defended_model(hip, defense=[(1, WarpedFeCoDefense(0.5, 'random', seed=3))])
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=3)).to(DEV)
    y = hip.make_decision(x)[0]

    def ce(a):
        with torch.no_grad():
            return float(np.mean([torch.nn.functional.cross_entropy(dm.score(a), y).item() for _ in range(4)]))
    atk = PGD(dm, task="CSI", epsilon=eps, step_size=step, max_iter=K, batch_size=B, EOT_size=2, EOT_batch_size=2, verbose=0)
    assert atk._device_route(B) is None
    before = ce(x)
    adv, succ = atk.attack(x, y)
    after = ce(adv)
    log("AudioNet + warped FeCo (random), PGD-5 EOT 2: CE %.4f -> %.4f, success %d/%d" % (before, after, sum(bool(s) for s in succ), B))
    assert after >= before and (adv - x).abs().max().item() <= eps + 1e-7
