"""The wide FeCo k-means on the device (sg_feco_kmeans_compress_wide, csrc/k_feco_wide.hip; 65 <= D <= 128): ids, cluster means
and counts bit for bit against the contract's restatement (tests/feco_wide_restate.py), the seeded form and its keys, the
longest utterance the entry takes, and ``FeCoDefense``'s routing by width."""
import ctypes as C

import numpy as np
import pytest
import torch

import feco_wide_restate as R
from conftest import load_golden, log
from test_ivector_cpu import MODELS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LONGEST_F = 833  # D 72, ratio 0.5: k = 416 = kp, 146 864 bytes of LDS; k = 417 needs a 14th centroid tile (k_feco_wide.hip header)


def _ctx():
    from speakerguard_amd.metric.metric import _context
    return _context(DEV)


def _wide(feat, k, random_init=0, seed=0, index_base=0, max_iter=10):
    from speakerguard_amd import _native as N
    feat = feat.to(DEV).contiguous()
    B, F, D = feat.shape
    ids = torch.full((B, F), -7, device=DEV, dtype=torch.int32)
    out = torch.full((B, k, D), float('nan'), device=DEV)
    counts = torch.full((B, k), -7, device=DEV, dtype=torch.int32)
    _ctx().call("sg_feco_kmeans_compress_wide", N._ptr(feat), B, F, D, k, max_iter, random_init, C.c_uint64(seed), int(index_base),
                N._ptr(ids), N._ptr(out), N._ptr(counts), N.current_stream_ptr(DEV))
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


def _restated(feat, k, seed=None, index_base=0, max_iter=10):
    """ids (B,F), out (B,k,D), counts (B,k), steps of the restatement; utterance b has global index index_base + b"""
    ids, out, counts, steps = [], [], [], []
    for b in range(feat.shape[0]):
        x = feat[b].numpy()
        st = {}
        i = R.kmeans_ids(x, k, max_iter, R.init_frames(x.shape[0], k, seed, index_base + b), stats=st)
        o, c = R.compress(x, i, k)
        ids.append(i), out.append(o), counts.append(c), steps.append(st['steps'])
    return np.stack(ids), np.stack(out), np.stack(counts), steps


def _check(name, feat, k):
    """even and seeded form of one shape: ids, means and counts bit-equal to the restatement, counts = bincount, out / counts
    equal to the stand-alone sg_feco_compress of the ids"""
    feat = feat.float().contiguous()
    B, F, D = feat.shape
    for seed in (None, 21):
        want = _restated(feat, k, seed, 5)
        ids, out, counts = _wide(feat, k, int(seed is not None), seed or 0, 5)
        got = ids.cpu().numpy()
        assert got.min() >= 0 and got.max() < k
        differ = int((got != want[0]).sum())
        assert differ == 0, (name, seed, "%d ids differ" % differ)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), (name, seed)
        assert np.array_equal(counts.cpu().numpy(), want[2]), (name, seed)
        for b in range(B):
            assert np.array_equal(counts[b].cpu().numpy(), np.bincount(got[b], minlength=k)), (name, seed, b)
        out2, counts2 = _compress(feat, ids, k)
        assert torch.equal(out, out2) and torch.equal(counts, counts2), (name, seed)
        log("wide FeCo %-22s (%d, %d, %d) k %d %s: ids, means, counts bit-equal to the restatement; empty clusters %d, steps %s"
            % (name, B, F, D, k, "seeded" if seed is not None else "even", int((want[2] == 0).sum()), want[3]))


def _iv_model(white_box=False, dither=0.0):
    from speakerguard_amd import synth
    from speakerguard_amd.model.iv_plda import iv_plda
    return iv_plda.from_weights(synth.make_iv_weights(**MODELS["a"]), device=DEV, dither=dither, white_box=white_box)


@pytest.mark.parametrize("level", [2, 3])
def test_real_iv_features_bit_equal(level):
    """the workload's shape: delta (level 2) and CMVN (level 3) features of 3 x 3 s, ratio 0.5"""
    from speakerguard_amd import synth
    m = _iv_model()
    x = torch.from_numpy(synth.make_waveforms(3, 48000, seed=70)).to(DEV)
    feat = m.compute_feat(x, flag=level).cpu()
    assert feat.shape[0] == 3 and feat.shape[2] == 72
    _check("iv level %d" % level, feat, int(feat.shape[1] * 0.5))


SYNTH = [(2, 77, 72, 0.3),    # one centroid tile, a frame-tile remainder
         (1, 90, 65, 0.4),    # odd width, a half-filled last group of 8
         (1, 40, 128, 0.5),   # full width
         (2, 300, 96, 0.04)]  # few clusters, more frame tiles than waves


@pytest.mark.parametrize("B,F,D,ratio", SYNTH, ids=["%dx%dx%d" % s[:3] for s in SYNTH])
def test_synthetic_shapes_bit_equal(B, F, D, ratio):
    rng = np.random.default_rng(F + D)
    centres = rng.standard_normal((7, D)) * 4
    feat = centres[rng.integers(0, 7, (B, F))] + rng.standard_normal((B, F, D)) * 1.5
    _check("synthetic", torch.from_numpy(feat.astype(np.float32)), int(F * ratio))


@pytest.mark.parametrize("name", ["duplicates", "offset", "k1", "kF"])
def test_degenerate_rows_bit_equal(name):
    x, k = R.degenerate_rows()[name]
    _check(name, torch.from_numpy(x)[None], k)


def test_sliding_cmvn_one_utterance_drops_empty_clusters():
    """(1, 331, 72): CMVN's 300-frame window slides, and with B = 1 FeCoDefense drops the empty clusters"""
    from speakerguard_amd.defense.feature_level import FeCoDefense
    m = _iv_model()
    raw = torch.from_numpy(load_golden("iv_ref.npz")["raw_331"]).to(DEV)
    feat = m.comput_feat_from_feat(raw, 1, 3)
    assert tuple(feat.shape) == (1, 331, 72)
    k = 165
    _check("iv cmvn F=331", feat.cpu(), k)
    want = _restated(feat.cpu(), k)
    out, saved = FeCoDefense(0.5).fwd(feat)
    live = np.nonzero(want[2][0] > 0)[0]
    assert tuple(out.shape) == (1, live.size, 72) and saved[3] is False
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want[1][0][live].view(np.uint32))
    # a start that leaves clusters empty for certain: the defense on the duplicated rows
    x, kd = R.degenerate_rows()["duplicates"]
    wd = _restated(torch.from_numpy(x)[None], kd)
    out, saved = FeCoDefense(0.5).fwd(torch.from_numpy(x)[None].to(DEV))
    live = np.nonzero(wd[2][0] > 0)[0]
    assert 0 < live.size < kd and tuple(out.shape) == (1, live.size, 72) and saved[4] is not None
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), wd[1][0][live].view(np.uint32))
    g = FeCoDefense(0.5)
    o, sv = g.fwd(torch.from_numpy(x)[None].to(DEV))
    d = g.bwd(sv, torch.ones_like(o))
    assert tuple(d.shape) == (1, 80, 72) and torch.isfinite(d).all()
    log("wide FeCo B = 1: F=331 keeps %d of %d clusters, the duplicated rows %d of %d" % (int((want[2][0] > 0).sum()), k, live.size, kd))


def test_longest_utterance_and_the_refusal_behind_it():
    from speakerguard_amd import _native as N
    rng = np.random.default_rng(3)
    F = LONGEST_F
    feat = torch.from_numpy((rng.standard_normal((1, F, 72)) * 3).astype(np.float32))
    feat[0] += torch.from_numpy(np.repeat(rng.standard_normal((F // 7 + 1, 72)) * 5, 7, axis=0)[:F].astype(np.float32))
    _check("longest", feat, int(F * 0.5))
    for F2 in (F + 1, (F // 32 + 1) * 32):  # 834, and 864: the next multiple of 32
        with pytest.raises(N.NativeError, match="too long"):
            _wide(torch.zeros(1, F2, 72), int(F2 * 0.5))


def test_seeded_form_keys():
    rng = np.random.default_rng(8)
    feat = torch.from_numpy((rng.standard_normal((3, 100, 72)) * 3).astype(np.float32))
    k = 50
    want = _restated(feat, k, 21, 5)
    full = _wide(feat, k, 1, 21, 5)
    assert np.array_equal(full[0].cpu().numpy(), want[0])
    for u in range(3):  # keyed by position: row u of a call at index_base 5 = row 0 of a one-row call at index_base 5 + u
        one = _wide(feat[u:u + 1], k, 1, 21, 5 + u)
        assert all(torch.equal(a[u:u + 1], b) for a, b in zip(full, one)), u
    other = _wide(feat, k, 1, 22, 5)
    assert not torch.equal(full[0], other[0])
    assert not torch.equal(full[0], _wide(feat, k)[0])
    log("wide FeCo seeded (3, 100, 72): ids equal the restatement fed feco_random_init, rows keyed by index_base + row, seeds 21 / 22 differ")


def test_width_routing_on_the_device():
    from speakerguard_amd import _native as N
    from speakerguard_amd.defense.feature_level import FeCoDefense
    rng = np.random.default_rng(9)
    feat = torch.from_numpy((rng.standard_normal((2, 100, 72)) * 3).astype(np.float32)).to(DEV)
    out, saved = FeCoDefense(0.5).fwd(feat)
    assert tuple(out.shape) == (2, 50, 72)
    ids, o2, c2 = _wide(feat, 50)
    assert torch.equal(saved[0], ids) and torch.equal(out, o2) and torch.equal(saved[1], c2)
    with pytest.raises(N.NativeError):
        FeCoDefense(0.5, other_param='cos').fwd(feat)
    # the narrow entry keeps refusing 65 columns, and the wide one 64 and 129
    ctx = _ctx()
    f65 = torch.zeros(2, 40, 65, device=DEV)
    i, o, c = torch.empty(2, 40, device=DEV, dtype=torch.int32), torch.empty(2, 20, 65, device=DEV), torch.empty(2, 20, device=DEV, dtype=torch.int32)
    rc = ctx.lib.sg_feco_kmeans_compress(ctx.handle, N._ptr(f65), 2, 40, 65, 20, 10, 0, C.c_uint64(0), 0, 1, N._ptr(i), N._ptr(o), N._ptr(c),
                                         N.current_stream_ptr(DEV))
    assert rc == 1 and b"0 < D <= 64" in ctx.lib.sg_last_error(ctx.handle)
    for D in (64, 129):
        with pytest.raises(N.NativeError, match="65 <= D <= 128"):
            _wide(torch.zeros(2, 40, D), 20)
