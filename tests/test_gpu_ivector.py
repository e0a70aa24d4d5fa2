"""GMM / i-vector / PLDA system on the GPU (speakerguard_amd.model.iv_plda, csrc/k_ivector.hip): every stage against float64
truth under the reference's own error, decisions, the wav flag, invariance under batching and chunking, the decision-only
attacks, enrolment and sharding.  Shapes: the fixtures' (tests/golden/make_golden_ivector.py) -- models A = (C 16, R 24) and
B = (C 80, R 100: tile remainders), F in {2, 13, 100, 331} frames, 5 / 5 / 3 / 1 utterances; model C = (C 272, R 262), F 13 and
100 with 3 and 2 utterances: the smallest sizes at which every 256-wide loop and grid dimension of csrc/k_ivector.hip takes a
second, partial pass (a second loglik column block with a quarter-filled wave, a second ``cb`` pass of 16 components, 17 lin
slices, a second stride of 6 live threads in the solve and the tail, a last Cholesky panel of 2 columns), and calls of 19 and 33
rows of it for the second and third group of 16 utterances of the assembly kernels."""
import numpy as np
import pytest
import torch

import iv_restate as R
from conftest import load_golden, log
from test_ivector_cpu import CASES, CASES_OF, FILES, MODEL_CASE_IDS, MODEL_CASES, MODELS, checksum

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sys_(dev):
    """per model: (weights, fixture, float64 truth, engine model with the dither off)"""
    from speakerguard_amd import synth
    from speakerguard_amd.model.iv_plda import iv_plda
    out = {}
    for tag, name in FILES.items():
        g = load_golden(name)
        w = synth.make_iv_weights(**MODELS[tag])
        assert checksum(w) == g["meta"][tag]["weights_sha256"]
        out[tag] = (w, g, R.IvRestated(w), iv_plda.from_weights(w, device=dev, dither=0.0))
    return out


_TRUTH = {}


def truth_chain(sys_, tag, F):
    """float64 truth of a fixture's case, computed once per module and left unchanged (model C: seconds of numpy work)"""
    if (tag, F) not in _TRUTH:
        _, g, truth, _ = sys_[tag]
        t = truth.chain(g["x_%d" % F])
        t["extract_alone"] = np.stack([truth.extract(a, b) for a, b in zip(g["zeroth_%d" % F], g["first_%d" % F])])
        for v in t.values():
            v.setflags(write=False)
        _TRUTH[tag, F] = t
    return _TRUTH[tag, F]


def err(a, truth):
    return float(np.abs(np.asarray(a, np.float64) - truth).max())


def judge(what, got, ref, truth):
    """the rule of every stage: err_gpu <= max(4 err_ref, 2^-20 max|q|); the measured ratio goes to the parity log"""
    e_gpu, e_ref, top = err(got, truth), err(ref, truth), float(np.abs(truth).max())
    bound = max(4.0 * e_ref, FLOOR * top)
    log("iv_parity %-34s err_gpu %.3e  err_ref %.3e  max|q| %.3e  err_gpu/bound %.3f" % (what, e_gpu, e_ref, top, e_gpu / bound))
    assert np.all(np.isfinite(np.asarray(got)))
    assert e_gpu <= bound, (what, e_gpu, e_ref, bound)


@pytest.mark.parametrize("F,B", CASES)
def test_delta_and_cmvn_against_truth(sys_, dev, F, B):
    _, g, _, m = sys_["a"]
    raw = g["raw_%d" % F]
    delta_t = R.add_delta(raw)
    cmvn_t = R.cmvn(delta_t)
    x = torch.from_numpy(raw).to(dev)
    delta = m.comput_feat_from_feat(x, 1, 2)
    judge("delta F=%d" % F, delta.cpu().numpy(), g["delta_%d" % F], delta_t)
    judge("cmvn F=%d" % F, m.comput_feat_from_feat(x, 1, 3).cpu().numpy(), g["cmvn_%d" % F], cmvn_t)
    # delta -> cmvn alone, fed the reference's own delta rows: against the truth computed from those rows
    judge("cmvn from delta F=%d" % F, m.comput_feat_from_feat(torch.from_numpy(g["delta_%d" % F]).to(dev), 2, 3).cpu().numpy(),
          g["cmvn_%d" % F], R.cmvn(g["delta_%d" % F]))
    # a raw row of 30 columns (the MFCC's own output) reads as its first 24
    wide = torch.cat([x, torch.full((B, F, 6), 7.0, device=dev)], 2).contiguous()
    out = torch.empty(B, F, 72, device=dev)
    from speakerguard_amd import _native as N
    m.ctx.call("sg_iv_delta_cmvn", N._ptr(wide), B, F, 30, N._ptr(out), None, m._stream())
    assert torch.equal(out, delta)


@pytest.mark.parametrize("F,B,tag", MODEL_CASES, ids=MODEL_CASE_IDS)
def test_stages_against_truth(sys_, dev, tag, F, B):
    """statistics, i-vector, embedding, scores: each stage fed the TRUTH's inputs of that stage where it has an entry of its
    own (statistics from the fixture's frames, the i-vector from float32-rounded true statistics), then the whole chain"""
    w, g, truth, m = sys_[tag]
    x = g["x_%d" % F]
    t = truth_chain(sys_, tag, F)
    xd = torch.from_numpy(x).to(dev)
    n, f = m.stats(xd)
    assert np.isfinite(n.cpu().numpy()).all()  # the x30 frame: a finite softmax
    judge("%s zeroth F=%d" % (tag, F), n.cpu().numpy(), g["zeroth_%d" % F], t["zeroth"])
    judge("%s first F=%d" % (tag, F), f.cpu().numpy(), g["first_%d" % F], t["first"])
    np.testing.assert_allclose(n.sum(1).cpu().numpy(), F, rtol=1e-5)
    # the extractor alone: both sides from the same float32 statistics (the reference's recorded ones)
    n_ref, f_ref = g["zeroth_%d" % F], g["first_%d" % F]
    iv_t = t["extract_alone"]
    iv = m.extract(torch.from_numpy(n_ref).to(dev), torch.from_numpy(f_ref).to(dev))
    judge("%s extract alone F=%d" % (tag, F), iv.cpu().numpy(), g["ivector_%d" % F], iv_t)
    # the chain from the frames
    dec, scores, emb, ivec = m._forward(xd, 3, want_emb=True, want_ivector=True)
    judge("%s ivector F=%d" % (tag, F), ivec.cpu().numpy(), g["ivector_%d" % F], t["ivector"])
    judge("%s emb F=%d" % (tag, F), emb.cpu().numpy(), g["emb_%d" % F], t["emb"])
    judge("%s scores F=%d" % (tag, F), scores.cpu().numpy(), g["scores_%d" % F], t["scores"])
    assert dec.cpu().tolist() == g["decisions_%d" % F].tolist()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_all_decisions_equal_the_reference(sys_, dev, tag):
    _, g, _, m = sys_[tag]
    raws = sys_["a"][1]
    for F, B in CASES_OF[tag]:
        for nb in sorted({1, min(3, B), B}):
            dec, _ = m.make_decision(torch.from_numpy(g["x_%d" % F][:nb]).to(dev), flag=3)
            assert dec.cpu().tolist() == g["decisions_%d" % F][:nb].tolist(), (F, nb)
            dec, sc = m.make_decision(torch.from_numpy(raws["raw_%d" % F][:nb]).to(dev), flag=1)
            assert dec.cpu().tolist() == g["raw_decisions_%d" % F][:nb].tolist(), (F, nb)
        dec2, _ = m.make_decision(torch.from_numpy(raws["delta_%d" % F][:B]).to(dev), flag=2)
        assert dec2.cpu().tolist() == g["raw_decisions_%d" % F].tolist()


def test_wav_flag(sys_, dev):
    """T = 16000, dither 0: the raw features are bit-equal to the first 24 columns of the x-vector front-end's; the rest of
    the chain stays within the rule against truth fed those features (the reference cannot run its MFCC here: the floor)"""
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    w, _, truth, m = sys_["a"]
    x = torch.from_numpy(synth.make_waveforms(3, 16000, seed=21)).to(dev)
    xv = xv_plda.from_weights(synth.make_xv_weights(), device=dev, dither=0.0)
    raw = m.compute_feat(x, 1)
    assert raw.shape == (3, 100, 24) and torch.equal(raw, xv.compute_feat(x, 1)[:, :, :24])
    t = truth.chain(R.cmvn(R.add_delta(raw.cpu().numpy())))
    ref32 = R.IvRestated(w, dtype=np.float32).chain(R.cmvn(R.add_delta(raw.cpu().numpy(), np.float32), np.float32))
    dec, scores, emb, ivec = m._forward(x, 0, want_emb=True, want_ivector=True)
    for k, got in (("ivector", ivec), ("emb", emb), ("scores", scores)):
        judge("wav %s" % k, got.cpu().numpy(), ref32[k], t[k])
    assert dec.cpu().tolist() == t["decisions"].tolist()
    assert torch.equal(m.compute_feat(x, 3), m.comput_feat_from_feat(raw, 1, 3))


def test_invariance_under_batching(sys_, dev):
    for tag in ("a", "b"):
        _, g, _, m = sys_[tag]
        x = torch.from_numpy(g["x_13"]).to(dev)
        full = m._forward(x, 3, want_emb=True, want_ivector=True)
        again = m._forward(x, 3, want_emb=True, want_ivector=True)
        for a, b in zip(full, again):
            assert torch.equal(a, b)
        for i in range(5):
            one = m._forward(x[i:i + 1], 3, want_emb=True, want_ivector=True)
            for a, b in zip(full, one):
                assert torch.equal(a[i:i + 1], b), (tag, i)
        n, f = m.stats(x)
        n1, f1 = m.stats(x[3:4])
        assert torch.equal(n[3:4], n1) and torch.equal(f[3:4], f1)


def group_rows(w, g, B0=16):
    """a call of model C whose last rows are the fixture's three utterances of 13 frames, behind B0 rows of other frames"""
    from speakerguard_amd import synth
    return np.concatenate([synth.make_iv_frames(w, B0, 13, seed=77), g["x_13"]])


def test_second_utterance_group_against_truth(sys_, dev):
    """19 rows of model C, flag 3: the assembly kernels' second group of 16 utterances (blockIdx.y / z = 1, nb = 3) holds the
    fixture's utterances -- judged against truth under the rule, and bit-equal to the 3-row call; then sg_iv_extract alone"""
    w, g, _, m = sys_["c"]
    t = truth_chain(sys_, "c", 13)
    x19 = torch.from_numpy(group_rows(w, g)).to(dev)
    assert x19.shape == (19, 13, 72)
    full = m._forward(x19, 3, want_emb=True, want_ivector=True)
    three = m._forward(x19[16:], 3, want_emb=True, want_ivector=True)
    dec, scores, emb, ivec = full
    judge("c 19 rows ivector F=13", ivec[16:].cpu().numpy(), g["ivector_13"], t["ivector"])
    judge("c 19 rows emb F=13", emb[16:].cpu().numpy(), g["emb_13"], t["emb"])
    judge("c 19 rows scores F=13", scores[16:].cpu().numpy(), g["scores_13"], t["scores"])
    assert dec[16:].cpu().tolist() == g["decisions_13"].tolist()
    for a, b in zip(full, three):
        assert torch.equal(a[16:], b)
    # the extractor's entry with B = 19: rows 16 .. 18 are the reference's recorded statistics
    n16, f16 = m.stats(x19[:16])
    n = torch.cat([n16, torch.from_numpy(g["zeroth_13"]).to(dev)]).contiguous()
    f = torch.cat([f16, torch.from_numpy(g["first_13"]).to(dev)]).contiguous()
    iv = m.extract(n, f)
    assert iv.shape == (19, MODELS["c"]["R"])
    judge("c 19 rows extract alone F=13", iv[16:].cpu().numpy(), g["ivector_13"], t["extract_alone"])
    assert torch.equal(iv[16:], m.extract(n[16:].contiguous(), f[16:].contiguous()))
    assert torch.equal(iv[:16], m.extract(n[:16].contiguous(), f[:16].contiguous()))


def test_a_33_row_call_equals_its_rows(sys_, dev):
    """model C, groups of 16, 16 and 1 utterances: the first and last row of every group equal the same row sent alone"""
    w, g, _, m = sys_["c"]
    x = torch.from_numpy(group_rows(w, g, 30)).to(dev)
    assert x.shape[0] == 33
    full = m._forward(x, 3, want_emb=True, want_ivector=True)
    for i in (0, 15, 16, 31, 32):
        one = m._forward(x[i:i + 1], 3, want_emb=True, want_ivector=True)
        for a, b in zip(full, one):
            assert torch.equal(a[i:i + 1], b), i


def test_a_1001_row_call_equals_its_chunks(sys_, dev):
    """NES sends 50 n + 1 rows: the library cuts them into chunks of 64; every row equals the same row sent in other company"""
    _, g, _, m = sys_["a"]
    rs = np.random.RandomState(7)
    raw = torch.from_numpy(rs.randn(1001, 13, 24).astype(np.float32)).to(dev)
    dec, scores, emb, ivec = m._forward(raw, 1, want_emb=True, want_ivector=True)
    for lo, hi in ((0, 1), (60, 70), (63, 64), (64, 65), (500, 577), (1000, 1001)):
        part = m._forward(raw[lo:hi], 1, want_emb=True, want_ivector=True)
        for a, b in zip((dec, scores, emb, ivec), part):
            assert torch.equal(a[lo:hi], b), (lo, hi)


def test_wav_chunks_keep_their_dither(sys_, dev):
    """70 one-second rows with the dither ON cross the 64-row chunk: row 64 .. 69 draw the noise of their place in the call"""
    from speakerguard_amd import synth
    from speakerguard_amd.model.iv_plda import iv_plda
    w = sys_["a"][0]
    m = iv_plda.from_weights(w, device=dev, dither=1.0, dither_seed=5)
    x = torch.from_numpy(synth.make_waveforms(70, 4000, seed=2)).to(dev)
    key = 1234567
    full = m._forward(x, 0, want_ivector=True, dither_seed=key)
    m._row_base = 64
    try:
        tail = m._forward(x[64:], 0, want_ivector=True, dither_seed=key)
    finally:
        m._row_base = 0
    assert torch.equal(full[3][64:], tail[3]) and torch.equal(full[1][64:], tail[1])
    other = m._forward(x[64:], 0, want_ivector=True, dither_seed=key)
    assert not torch.equal(full[3][64:], other[3])  # (the dither is on: another place, another noise)


def test_loss_and_enroll_override(sys_, dev):
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
    w, g, truth, m = sys_["a"]
    x = torch.from_numpy(g["x_100"]).to(dev)
    dec0, sc0 = m.make_decision(x, flag=3)
    y = torch.tensor([0, 1, 2], device=dev)
    dec, sc, loss, grad = m.loss_grad(x, y, SEC4SR_CrossEntropy(), flag=3, want_grad=False)
    assert grad is None and torch.equal(sc, sc0) and torch.equal(dec, dec0)
    want = torch.nn.functional.cross_entropy(sc0.cpu().double(), y.cpu(), reduction="none")
    np.testing.assert_allclose(loss.cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6)
    _, _, lm, _ = m.loss_grad(x, y, SEC4SR_MarginLoss(targeted=False, confidence=0.0, task="CSI", threshold=None, clip_max=True),
                              flag=3, want_grad=False)
    assert torch.isfinite(lm).all()
    with pytest.raises(NotImplementedError, match="gradient is not built"):
        m.loss_grad(x, y, SEC4SR_CrossEntropy(), flag=3)
    # per-call enroll_embs: two of the speakers, in another order; the model's own set is untouched afterwards
    sub = torch.from_numpy(w["enroll"][[2, 0]]).to(dev)
    d2, s2 = m.make_decision(x, flag=3, enroll_embs=sub)
    assert torch.equal(s2, sc0[:, [2, 0]]) and s2.shape == (3, 2)
    assert torch.equal(m.make_decision(x, flag=3)[1], sc0)
    m.set_enroll(threshold=1e9)
    try:
        assert m.make_decision(x, flag=3)[0].cpu().tolist() == [-1, -1, -1]
    finally:
        m.set_enroll(threshold=-np.inf)


def test_fakebob_matches_oracle_with_shared_noise(sys_, dev):
    """FAKEBOB / NES on model A, 2 x 1 s, 3 iterations, both sides drawing the NES noise from the same seeded CPU generator; the
    oracle attack queries the float64 restatement.  The bound of tests/test_gpu_xv.py's shared-noise test."""
    from oracle import attacks as oatk
    from speakerguard_amd import synth
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    w, _, _, m = sys_["a"]
    om = R.IvOracleModel(w)
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=32))
    y = om.make_decision(x)[0]
    assert m.make_decision(x.to(dev))[0].cpu().tolist() == y.tolist()
    kw = dict(task="CSI", epsilon=0.002, max_iter=3, max_lr=0.0005, min_lr=1e-6, samples_per_draw=8,
              samples_per_draw_batch_size=4, sigma=0.001, stop_early=True, stop_early_iter=2, batch_size=1)
    g = torch.Generator().manual_seed(5)
    oadv, osucc = oatk.FAKEBOB(om, noise_fn=lambda shape: torch.randn(shape, generator=g), **kw).attack(x.clone(), y)
    g2 = torch.Generator().manual_seed(5)
    adv, succ = FAKEBOB(m, verbose=0, noise_fn=lambda shape: torch.randn(shape, generator=g2), **kw).attack(x.to(dev), y.to(dev))
    diff = (adv.cpu() - oadv).abs()
    frac = float((diff > 1e-7).float().mean())
    log("iv FAKEBOB-3: samples differing %.3f%%, success hip=%s oracle=%s" % (100 * frac, succ, osucc))
    assert succ == osucc
    assert frac < 0.05 and diff.max().item() <= 2 * 0.002 + 1e-6


def test_kenan_and_siren_run(sys_, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.Kenan import Kenan
    from speakerguard_amd.attack.SirenAttack import SirenAttack
    m = sys_["a"][3]
    x = torch.from_numpy(synth.make_waveforms(2, 16000, seed=33)).to(dev)
    y = m.make_decision(x)[0]
    adv, succ = Kenan(m, atk_name="fft", max_iter=3, verbose=0, batch_size=2).attack(x, y)
    assert adv.shape == x.shape and torch.isfinite(adv).all()
    dec = m.make_decision(adv)[0]
    assert [bool(s) for s in succ] == (dec != y).cpu().tolist()
    eps = 0.002
    adv, succ = SirenAttack(m, task="CSI", epsilon=eps, max_epoch=1, max_iter=2, n_particles=4, batch_size=2, verbose=0).attack(x, y)
    assert (adv - x).abs().max().item() <= eps + 1e-6 and adv.abs().max().item() <= 1.0
    dec = m.make_decision(adv)[0]
    assert [bool(s) for s in succ] == (dec != y).cpu().tolist()


def test_query_sharded_model_takes_it(sys_, dev):
    """the row-sharding proxy of the black-box attacks takes the model as it is: a rank's slice of a call equals those rows
    of the whole call (emulated ranks: ``_call_rows``)"""
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.shard import QueryShardedModel
    m = sys_["a"][3]
    x = torch.from_numpy(sys_["a"][1]["raw_13"]).to(dev)
    y = torch.tensor([0, 1, 2, 3, 0], device=dev)
    sm = QueryShardedModel(m)
    spec = SEC4SR_CrossEntropy()
    full = sm.loss_grad(x, y, spec, want_grad=False, flag=1)
    assert full[3] is None
    for lo, hi in ((0, 2), (2, 5)):
        part = sm._call_rows(x, y, spec, lo, hi, False, {"flag": 1})
        for a, b in zip(full[:3], part[:3]):
            assert torch.equal(a[lo:hi], b)
    assert torch.equal(sm.make_decision(x, flag=1)[1], full[1])


def test_enroll_takes_it(sys_, dev):
    """speakerguard_amd.enroll needs ``embedding`` and ``score(enroll_embs=)``: the mean embedding of a speaker's utterances, the
    z-norm statistics of others' against it, and the scores of a model that enrolled it"""
    from speakerguard_amd import synth
    from speakerguard_amd.enroll import enroll_speaker, znorm_stats
    from speakerguard_amd.set_threshold import set_threshold
    m = sys_["a"][3]
    x = torch.from_numpy(synth.make_waveforms(4, 16000, seed=44))
    emb = enroll_speaker(m, [x[0], x[1]])
    want = (m.embedding(x[0:1].to(dev)) + m.embedding(x[1:2].to(dev))) / 2
    assert emb.shape == (1, 10) and torch.equal(emb, want)
    mean, std = znorm_stats(m, emb, [x[2], x[3]])
    s = m.score(x[2:4].to(dev), enroll_embs=emb).flatten().cpu().numpy().astype(np.float64)
    assert abs(mean - s.mean()) <= 1e-6 * abs(s).max() and abs(std - s.std()) <= 1e-6 * abs(s).max()
    thr, frr, far = set_threshold(s + 50.0, s, device=dev)
    assert np.isfinite(thr) and frr == 0.0 and far == 0.0


# ---- the PLDA back end at its corner shapes (tests/plda_cases.py): D = 150, S = 1, 27 / 28, 64 / 65 (the counts at which the
# x-vector tail, which shares the scoring, changes path); one white-box model of 65 speakers, a case enrols the first S
@pytest.fixture(scope="module")
def backend_case(dev):
    import plda_cases as P
    from speakerguard_amd.model.iv_plda import iv_plda
    w = P.iv_weights()
    return w, iv_plda.from_weights(w, device=dev, dither=0.0, white_box=True), torch.from_numpy(P.waveforms()).to(dev)


@pytest.mark.parametrize("S", [1, 27, 28, 64, 65])
def test_backend_corner_shapes_against_float64_scores(backend_case, S):
    """scores against the float64 log-likelihood ratio of the model's OWN returned embedding under the rule of ``judge`` (the
    reference: the same recomputation in float32), decisions = the float64 arg-max outside the tie margin"""
    import plda_cases as P
    w, m, x = backend_case
    m.set_enroll(w["enroll"][:S])
    dec, scores, emb, _ = m._forward(x, 0, want_emb=True)
    emb = emb.cpu().numpy()
    truth = P.llr(emb, w["enroll"][:S], w["plda_psi"])
    yard = P.llr(emb, w["enroll"][:S], w["plda_psi"], np.float32).astype(np.float64)
    assert scores.shape == (P.B, S)
    judge("back-end corner D=%d S=%d scores" % (P.D, S), scores.cpu().numpy(), yard, truth)
    clear = P.top_two_margin(truth) > P.iv_score_bound(truth, yard)
    assert clear.mean() >= 0.9 and (dec.cpu().numpy()[clear] == truth.argmax(1)[clear]).all()


@pytest.mark.parametrize("S", [1, 27, 28, 64, 65])
def test_backend_corner_shapes_override_and_reenrol_bit_for_bit(backend_case, S):
    """the x-vector file's override test on this model: a permuted subset through ``enroll_embs=`` gives the matching columns of
    the full-table scores, and a smaller table enrolled and the full one enrolled again the first ones, bit for bit"""
    import plda_cases as P
    w, m, x = backend_case
    full = w["enroll"][:S]
    m.set_enroll(full)
    sc0 = m.score(x)
    idx = P.subset(S)
    sub = m.score(x, enroll_embs=torch.from_numpy(full[idx].copy()).to(x.device))
    assert sub.shape == (P.B, len(idx)) and torch.equal(sub, sc0[:, torch.from_numpy(idx).to(x.device)])
    assert m.num_spks == S and torch.equal(m.score(x), sc0)
    m.set_enroll(full[:max(1, S // 2)])
    assert m.score(x).shape == (P.B, max(1, S // 2))
    m.set_enroll(full)
    assert torch.equal(m.score(x), sc0)


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("loss_name", ["Entropy", "Margin"])
def test_backend_corner_shapes_gradient_is_row_invariant(backend_case, loss_name, S):
    """loss_grad from the waveform: finite, and three rows in one call bit-equal to the same rows one at a time"""
    import plda_cases as P
    from speakerguard_amd.attack.utils import resolve_loss
    w, m, x = backend_case
    m.set_enroll(w["enroll"][:S])
    spec, _ = resolve_loss(loss_name, targeted=False, task='CSI', threshold=None, clip_max=False)
    y = (torch.arange(P.B) % S).to(x.device)
    dec, sc, loss, grad = m.loss_grad(x, y, spec, flag=0)
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all() and grad.shape == x.shape
    for i in range(P.B):
        d1, s1, l1, g1 = m.loss_grad(x[i:i + 1], y[i:i + 1], spec, flag=0)
        assert torch.equal(g1, grad[i:i + 1]) and torch.equal(s1, sc[i:i + 1]) and torch.equal(l1, loss[i:i + 1]) and torch.equal(d1, dec[i:i + 1])
