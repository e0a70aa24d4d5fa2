"""Every AudioNet layer, both directions, pinned in situ to the float32 fmaf chain -- on the readbacks of ONE per-layer pass.

The determinism contract (DESIGN.md "Tolerances") says an output element of a contraction is one fmaf chain in the documented
k order (oracle/conv_chain.c) whichever kernel ``launch_conv_gemm`` picks.  The per-layer AudioNet pass (SG_AN_FUSED=0) is the
yardstick of the fused CNN kernels, and it launches contractions no other test reaches: the 128 x 32 tile kernel at N = 64 / 32,
same padding (tap_base -1 forward, +1 with tap_step -1 backward: a tap row outside the utterance must read as zero, not as the
neighbouring utterance's frame), and the 16 x 16 / QUAD32 / QUAD64 branches at 6 and 12 chunks.  Here a feature-level
``loss_grad`` (flag 1: the front-end does not enter; cross-entropy, labels one past the decisions) runs per layer, every buffer
is read back (``read_activation``, ``read_gradient`` = sg_an_debug_gradient) and every stage is restated on the pass's own
upstream readback and compared over every element, bit for bit (``an_stages.stage_checks``; tools proved on the CPU with planted
defects in tests/test_an_stages_power.py):

  forward   pre == pre-filter chain(features); every un-pooled layer == conv_chain(previous readback, wf[l], ..., 3, 1, -pad,
            bias); every pooled readback == restated pooling of its un-pooled readback; embedding == max over time of conv8
  backward  for l = 7 .. 1 what conv l's data gradient writes == conv_chain(dact_l, wb[l], ..., 3, -1, +pad, mask = the
            un-pooled ReLU output the engine uses, none into a pooled layer or the pre-filter); each dact below a pool ==
            restated pooling backward(act_unpooled, dpool); d loss / d log-mel == transposed pre-filter chain(dpre); the zero
            pattern of dact7 == the head rule (first arg-max frame, only where the maximum is > 0)

The split sums with no single chain (fc, d emb) are held against float64 on the engine's own embedding readback, with float32
torch on the CPU as the yardstick: per utterance, engine error <= C x yardstick error + FLOOR_SCORE x max |truth|
(truth.POLICY; the rule of test_pool_and_split_k_fc1_against_float64_on_the_engines_own_tdnn5).

Then the fused forms on the same inputs (SG_AN_FUSED=1, head inside the backward, planned cut and 1 / 3 slices): scores, loss,
d loss / d log-mel and the eight activation layers ``torch.equal`` to the pinned per-layer run.

Grid (B, F) and the path ``conv_plan`` (sg_internal.h) picks at 256 CUs for the 14 contractions of a pass, read from the
launcher: AudioNet asks for tile 2 with packed weights where N = 128 (forward conv3 .. conv6, data gradients of conv4 .. conv7)
and for the 128 x 32 tile kernel otherwise; tile 2 takes 16 x 16 blocks while ceil(M / 16) x 8 <= 2800 (M <= 5600), else
QUAD32 from 8 chunks while fewer than 256 64-row tiles exist, else QUAD64; M = B x Tout forward, B x Tin backward with
(Tin, Tout) = (300, 300) (150, 150) x 3 (75, 75) x 2 (37, 35) at F = 300; 6 chunks at conv3 forward and conv7 backward, 12 on
the other N = 128 launches.  fwd: conv2 .. conv8; bwd: in launch order, the data gradients of conv8 .. conv2
(``an_stages.path_table``, held against this table and against tests/native/conv_launch_table.expected on the CPU):

    (1, 300) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (1, 300) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (3, 101) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (3, 101) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (37, 300) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (37, 300) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (38, 300) fwd: TILE_128x32 QUAD64 QUAD32 QUAD32 S16 TILE_128x32 TILE_128x32
    (38, 300) bwd: TILE_128x32 S16 S16 QUAD32 QUAD32 TILE_128x32 TILE_128x32
    (64, 300) fwd: TILE_128x32 QUAD64 QUAD32 QUAD32 S16 TILE_128x32 TILE_128x32
    (64, 300) bwd: TILE_128x32 S16 S16 QUAD32 QUAD32 TILE_128x32 TILE_128x32
    (110, 300) fwd: TILE_128x32 QUAD64 QUAD64 QUAD64 QUAD32 TILE_128x32 TILE_128x32
    (110, 300) bwd: TILE_128x32 QUAD64 QUAD32 QUAD64 QUAD64 TILE_128x32 TILE_128x32
    (5, 126) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (5, 126) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 25) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 25) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 24) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 24) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 126) fwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32
    (2, 126) bwd: TILE_128x32 S16 S16 S16 S16 TILE_128x32 TILE_128x32

(37 | 38, 300): the 16 x 16 block edge on conv3 (M = 5550 | 5700); (64, 300): QUAD32 on the 12-chunk launches with M = 9600,
QUAD64 on the 6-chunk forward one, 16 x 16 blocks where M = 4800; (110, 300): M = 16500 >= 16384, QUAD64 on the 12-chunk
launches at 150 frames, QUAD32 at 75 frames (M = 8250) and QUAD64 on the 6-chunk data gradient of conv7 -- the only case with
QUAD64 in the backward; (5, 126): 126 -> 63 -> 31 -> 15 frames, odd at the second and third pool; (2, 25): odd at the first;
(2, 24): the shortest the stack accepts, one frame at conv8.  (2, 126) "tied": every frame of an utterance is the same
32-vector, so interior frames of every layer are bit-identical and the pooled pairs and the head's maximum tie at positive
values.  The data gradient of conv2 (N = 32) and of conv3 (N = 64) take the 128 x 32 tile kernel as that of conv8 does.
"""
import numpy as np
import pytest
import torch

import an_fold
import an_stages
import truth
import xv_fold
from conftest import log
from speakerguard_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = [(B, Fr, False) for B, Fr in an_stages.GRID] + [an_stages.TIES + (True,)]
KNOBS = ("SG_AN_FUSED", "SG_AN_HEAD", "SG_AN_ONE", "SG_AN_SLICES")
FORWARD = ("pre-filter forward", "forward", "pool after", "embedding")


def _id(c):
    return "B%d_F%d%s" % (c[0], c[1], "_tied" if c[2] else "")


case_param = pytest.mark.parametrize("case", CASES, ids=_id)


@pytest.fixture(scope="module")
def sd():
    from speakerguard_amd import synth
    return synth.make_audionet_state_dict(seed=0, num_class=251)


@pytest.fixture(scope="module")
def hip(sd):
    from speakerguard_amd.model.audionet_csine import audionet_csine
    return audionet_csine.from_weights(sd, device=DEV)


@pytest.fixture(scope="module")
def fd(sd):
    return an_fold.fold(sd)


def _ce():
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    return SEC4SR_CrossEntropy()


def _knobs(mp, **kw):
    for k in KNOBS:
        mp.delenv(k, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


_PASS = {}  # the latest case only


def _engine_pass(hip, fd, case):
    """The per-layer pass of a case, once: the readbacks as ``an_stages.stage_checks`` takes them (numpy), the device outputs
    the fused forms are compared with, and the verdict of every stage (None: same bits in every element)."""
    if case not in _PASS:
        _PASS.clear()
        B, Fr, ties = case
        feats = an_stages.case_feats(B, Fr, ties)
        Tin, Tout = an_fold.layer_frames(Fr)
        x = torch.from_numpy(feats.copy()).to(DEV)
        with pytest.MonkeyPatch.context() as mp:
            _knobs(mp, SG_AN_FUSED="0")
            dec0 = hip.make_decision(x, flag=1)[0]
            y = (dec0 + 1) % hip.num_spks  # not the decisions: the loss and its gradient are far from zero
            emb = hip.embedding(x, flag=1)
            dec, scores, loss, grad = hip.loss_grad(x, y, _ce(), flag=1)
            raw = {k: hip.read_gradient(k) for k in sorted(N.SG_AN_GRAD)}
            layers = [hip.read_activation(i, B).clone() for i in range(1, 9)]
        assert torch.equal(dec, dec0)
        cpu = lambda t: t.cpu().numpy()
        rb = dict(feats=feats, pre=cpu(raw["pre"]), emb=cpu(emb), dpre=cpu(raw["dpre"]), grad=cpu(grad), act=[None] * 7, pool={},
                  dact=[cpu(raw["dact%d" % (l + 1)]) for l in range(7)], dpool={})
        for l in range(7):
            if an_fold.POOL[l]:
                rb["act"][l] = cpu(raw["act%d_unpooled" % (l + 1)])
                rb["pool"][l] = cpu(layers[l + 1])
                rb["dpool"][l] = cpu(raw["dpool%d" % (l + 1)])
                assert rb["pool"][l].shape == (B, Tout[l] // 2, an_fold.COUT[l]) and rb["dpool"][l].shape == rb["pool"][l].shape
            else:
                rb["act"][l] = cpu(layers[l + 1])
            assert rb["act"][l].shape == (B, Tout[l], an_fold.COUT[l]) and rb["dact"][l].shape == rb["act"][l].shape, l
        assert rb["pre"].shape == (B, Fr, 32) and rb["dpre"].shape == (B, Fr, 32) and rb["grad"].shape == (B, Fr, 32)
        assert torch.equal(layers[0], raw["pre"]), "read_activation(1) and read_gradient('pre') are one buffer"
        verdict = {}
        for name, got, want in an_stages.stage_checks(rb, fd):
            rows = got.shape[1]
            verdict[name] = xv_fold.bit_mismatch(got.reshape(B * rows, -1), want.reshape(B * rows, -1), rows, "%s, %s" % (name, _id(case)))
        _PASS[case] = dict(rb=rb, verdict=verdict, y=y, x=x, scores=scores, loss=loss, grad=grad, layers=layers)
    return _PASS[case]


def _is_forward(name):
    return any(k in name for k in FORWARD)


@case_param
def test_forward_stages_in_situ_are_the_restated_chains(hip, fd, case):
    p = _engine_pass(hip, fd, case)
    names = [n for n in p["verdict"] if _is_forward(n)]
    assert len(names) == 1 + 7 + 3 + 1
    bad = [p["verdict"][n] for n in names if p["verdict"][n] is not None]
    log("AudioNet stages %s forward: %d of %d comparisons same bits (%s)" % (_id(case), len(names) - len(bad), len(names), "; ".join(names)))
    assert not bad, "\n".join(bad)


@case_param
def test_backward_stages_in_situ_are_the_restated_chains(hip, fd, case):
    p = _engine_pass(hip, fd, case)
    names = [n for n in p["verdict"] if not _is_forward(n)]
    assert len(names) == 7 + 3 + 1 + 1
    bad = [p["verdict"][n] for n in names if p["verdict"][n] is not None]
    log("AudioNet stages %s backward: %d of %d comparisons same bits (%s)" % (_id(case), len(names) - len(bad), len(names), "; ".join(names)))
    assert not bad, "\n".join(bad)


@case_param
def test_the_case_tests_something(hip, fd, case):
    """live ReLU masks, non-zero gradients, labels that are not the decisions; the tied case: positive tied pairs in every
    pooled layer of every utterance and a head maximum held by more than one frame -- in the ENGINE's readbacks"""
    p = _engine_pass(hip, fd, case)
    rb = p["rb"]
    failed = [d for d, ok in an_stages.conditions(rb) if not ok]
    assert failed == []
    assert (p["scores"].argmax(1) != p["y"]).all()
    if case[2]:
        for l in an_stages.POOLED:
            n = an_stages.positive_tied_pairs(rb["act"][l])
            log("AudioNet stages %s: positive tied pairs of conv%d per utterance %s" % (_id(case), l + 2, n.tolist()))
            assert (n >= 1).all(), (l, n)
        assert (an_stages.tied_head_maxima(rb["act"][6]) >= 1).all(), "the head's maximum ties at a positive value"


@case_param
def test_head_sums_against_float64_on_the_engines_own_embedding(hip, fd, case):
    """fc and d emb are split float32 sums with no single chain: the engine's scores and the non-zero values of dact7 against
    float64 evaluated on the engine's embedding readback, float32 torch on the CPU as yardstick; per utterance
    engine error <= C x yardstick error + FLOOR_SCORE x max |truth| (truth.POLICY)."""
    p = _engine_pass(hip, fd, case)
    rb, B = p["rb"], case[0]
    y = p["y"].cpu()
    w32, b32 = torch.from_numpy(fd.fc_w), torch.from_numpy(fd.fc_b)

    def head(emb, w, b):
        e = emb.clone().requires_grad_(True)
        s = torch.nn.functional.linear(e, w, b)
        l = torch.nn.functional.cross_entropy(s, y, reduction="none")
        l.backward(torch.ones_like(l))
        return s.detach().double().numpy(), e.grad.double().numpy()
    emb = torch.from_numpy(rb["emb"])
    s64, d64 = head(emb.double(), w32.double(), b32.double())
    s32, d32 = head(emb, w32, b32)
    mask = an_stages.head_mask(rb["act"][6])
    demb = (rb["dact"][6] * mask).sum(1, dtype=np.float64)  # one non-zero term per channel: exact
    live = mask.any(1)
    assert live.any(1).all()
    P = truth.POLICY
    for what, eng, yard, t64 in (("scores", p["scores"].cpu().double().numpy(), s32, s64), ("d emb", np.where(live, demb, 0.0), np.where(live, d32, 0.0), np.where(live, d64, 0.0))):
        e_eng, e_yard = np.abs(eng - t64).max(1), np.abs(yard - t64).max(1)
        bound = P["C"] * e_yard + P["FLOOR_SCORE"] * np.abs(t64).max(1)
        log("AudioNet head %s %s: engine / fp32 torch vs fp64 on the engine's embedding, max over utterances %.3e / %.3e (max |truth| %.3e); "
            "worst engine error over its bound %.2f" % (_id(case), what, e_eng.max(), e_yard.max(), np.abs(t64).max(), (e_eng / bound).max()))
        bad = np.flatnonzero(~(e_eng <= bound))
        assert bad.size == 0, (what, [(int(u), float(e_eng[u]), float(e_yard[u]), float(bound[u])) for u in bad[:8]])


@case_param
def test_fused_forms_equal_the_pinned_per_layer_pass(hip, fd, case):
    """what carries the pins over to k_audionet_fused.hip: the fused CNN with the head inside the backward, at the planned cut
    and at 1 and 3 time slices, on the same features and labels"""
    p = _engine_pass(hip, fd, case)
    B = case[0]
    names = ["scores", "loss", "d loss / d log-mel"] + ["layer %d" % i for i in range(1, 9)]
    ref = [p["scores"], p["loss"], p["grad"]] + p["layers"]
    with pytest.MonkeyPatch.context() as mp:
        for slices in (None, "1", "3"):
            _knobs(mp, SG_AN_FUSED="1", SG_AN_HEAD="1", **({"SG_AN_SLICES": slices} if slices else {}))
            _, sc, ls, g = hip.loss_grad(p["x"], p["y"], _ce(), flag=1)
            got = [sc, ls, g] + [hip.read_activation(i, B) for i in range(1, 9)]
            for n, a, b in zip(names, got, ref):
                assert a.shape == b.shape, (n, slices)
                assert torch.equal(a, b), "%s differs with %s slices: max |diff| %.3e" % (n, slices or "planned", (a - b).abs().max().item())
    log("AudioNet stages %s: fused CNN with the head inside (planned cut, 1 and 3 slices) equals the pinned per-layer pass: "
        "scores, loss, d loss / d log-mel, 8 layers" % _id(case))


def test_the_readback_refuses_what_it_cannot_serve(hip, fd):
    """state, unknown buffer, small capacity: each raises with its message and launches nothing"""
    x = torch.from_numpy(an_stages.case_feats(2, 24).copy()).to(DEV)
    y = torch.tensor([3, 200], device=DEV)

    def refused(match, fn):
        def run():
            with pytest.raises(N.NativeError, match=match):
                fn()
        assert hip.trace_stages(run) == []

    with pytest.MonkeyPatch.context() as mp:
        _knobs(mp, SG_AN_FUSED="1")
        hip.loss_grad(x, y, _ce(), flag=1)
        refused("per-layer form", lambda: hip.read_gradient("dact7"))  # the fused forms keep these tensors in LDS
        _knobs(mp, SG_AN_FUSED="0")
        hip.loss_grad(x, y, _ce(), flag=1)
        assert hip.read_gradient("dact7").shape == (2, 1, 32)
        refused("unknown buffer 15", lambda: hip.read_gradient(15))
        refused("unknown buffer -1", lambda: hip.read_gradient(-1))
        small = torch.empty(2 * 24 * 32 - 1, device=DEV)
        refused("capacity of 1535 floats, the buffer holds 1536",
                lambda: hip.ctx.call("sg_an_debug_gradient", N.SG_AN_GRAD["dpre"], N._ptr(small), small.numel(), None, hip._stream()))
        assert hip.read_gradient("dpre").shape == (2, 24, 32)  # (a refusal does not end the pass's validity)
        hip.loss_grad(x, y, _ce(), flag=1, want_grad=False)
        refused("not an sg_an_loss_grad call with a gradient", lambda: hip.read_gradient("dpre"))
        hip.loss_grad(x, y, _ce(), flag=1)
        hip.make_decision(x, flag=1)
        refused("not an sg_an_loss_grad call with a gradient", lambda: hip.read_gradient("pre"))
