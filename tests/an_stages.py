"""AudioNet's stages between the contractions, restated in numpy, and the stage-by-stage comparison of a pass's readbacks.
TEST INFRASTRUCTURE (a plain module, not a conftest).

Exact restatements (no arithmetic beyond comparisons and selections, so numpy is bit-exact):

* ``pool_fwd``: MaxPool1d(2, 2) along time, an odd last frame dropped (k_audionet.hip an_pool_fwd_kernel);
* ``pool_bwd``: the pooled gradient goes to the FIRST maximum of a pair (torch's rule at ties) and only where that entry
  is > 0 (the ReLU in front of the pool); a dropped odd last frame gets +0 (an_pool_bwd_kernel);
* ``head_mask`` / ``head_dact``: d loss / d conv8 pre-activation is d emb at the FIRST frame holding a channel's maximum over
  time, only where that maximum is > 0, +0 elsewhere (an_tail_kernel).

``stage_checks`` lists every comparison tests/test_gpu_an_stages.py makes on the readbacks of one per-layer pass: each stage
restated on the pass's OWN upstream readback, so a defect shows at the stage that has it.  ``simulate`` produces the same
readbacks from the restatements alone -- an engine double -- and takes the operations as a table (``OPS``), so that
tests/test_an_stages_power.py can plant a defect in one operation and show that ``stage_checks`` (the very comparison the
engine is held to) rejects the result.
"""
from types import SimpleNamespace

import numpy as np

import an_fold
from oracle.conv_chain import conv_chain, prefilter_chain

POOLED = (0, 3, 5)  # conv2, conv5, conv7: the layers followed by a MaxPool (an_fold.POOL)


def pool_fwd(act):
    """(B, Tin, C) -> (B, Tin // 2, C)"""
    T2 = act.shape[1] // 2
    return np.maximum(act[:, 0:2 * T2:2], act[:, 1:2 * T2:2])


def pool_bwd(act, dpool):
    """act (B, Tin, C) the un-pooled ReLU output, dpool (B, Tin // 2, C) -> d pre-activation (B, Tin, C)"""
    B, Tin, C = act.shape
    T2 = Tin // 2
    a0, a1 = act[:, 0:2 * T2:2], act[:, 1:2 * T2:2]
    first = ~(a1 > a0)
    out = np.zeros_like(act)
    out[:, 0:2 * T2:2] = np.where(first & (a0 > 0), dpool, np.float32(0))
    out[:, 1:2 * T2:2] = np.where(~first & (a1 > 0), dpool, np.float32(0))
    return out


def head_mask(act8):
    """(B, T8, 32) -> bool (B, T8, 32): the first frame of each channel's maximum over time, where that maximum is > 0"""
    B, T8, C = act8.shape
    at = act8.argmax(1)  # numpy: the first maximal index
    m = np.zeros(act8.shape, bool)
    b, c = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    m[b, at, c] = act8.max(1) > 0
    return m


def head_dact(act8, demb):
    """d emb (B, 32) routed by ``head_mask`` -> (B, T8, 32)"""
    return np.where(head_mask(act8), demb[:, None, :], np.float32(0)).astype(np.float32)


OPS = SimpleNamespace(conv=conv_chain, prefilter=prefilter_chain, pool_fwd=pool_fwd, pool_bwd=pool_bwd, head_mask=head_mask)


def layer_input(rb, l):
    if l == 0:
        return rb["pre"]
    return rb["pool"][l - 1] if an_fold.POOL[l - 1] else rb["act"][l - 1]


def fwd_conv(ops, fd, a, l, B, Tin, Tout):
    out = ops.conv(a.reshape(B * Tin, an_fold.CIN[l]), fd.wf[l], B, Tin, Tout, 3, 1, -an_fold.PAD[l], bias=fd.bias[l])
    return out.reshape(B, Tout, an_fold.COUT[l])


def bwd_conv(ops, fd, da, l, B, Tin, Tout, mask, wb=None):
    """data gradient of conv l: d out (B, Tout, Cout) -> d in (B, Tin, Cin), under the ReLU mask of the layer below or none"""
    out = ops.conv(da.reshape(B * Tout, an_fold.COUT[l]), (wb or fd.wb)[l], B, Tout, Tin, 3, -1, an_fold.PAD[l],
                   mask=None if mask is None else mask.reshape(B * Tin, an_fold.CIN[l]))
    return out.reshape(B, Tin, an_fold.CIN[l])


def bwd_target(l):
    """(which readback conv l's data gradient writes, the mask layer or None)"""
    if l == 0:
        return ("dpre", None), None
    if an_fold.POOL[l - 1]:
        return ("dpool", l - 1), None
    return ("dact", l - 1), l - 1


def _get(rb, key):
    return rb[key[0]] if key[1] is None else rb[key[0]][key[1]]


def stage_checks(rb, fd, ops=OPS):
    """Every bitwise comparison of one pass: [(name, got, want)] with got / want float32 arrays of one shape (B, rows, C).
    ``rb``: feats, pre, act[0..6] (un-pooled ReLU outputs), pool[l] for l in POOLED, emb, dact[0..6], dpool[l], dpre, grad."""
    B, F = rb["feats"].shape[:2]
    Tin, Tout = an_fold.layer_frames(F)
    out = [("pre-filter forward", rb["pre"], ops.prefilter(rb["feats"], fd.w25, fd.pre_bias, False))]
    for l in range(an_fold.CONVS):
        out.append(("conv%d forward" % (l + 2), rb["act"][l], fwd_conv(ops, fd, layer_input(rb, l), l, B, Tin[l], Tout[l])))
        if an_fold.POOL[l]:
            out.append(("pool after conv%d" % (l + 2), rb["pool"][l], ops.pool_fwd(rb["act"][l])))
    out.append(("embedding = max over time of conv8", rb["emb"][:, None, :], rb["act"][6].max(1)[:, None, :]))
    for l in range(an_fold.CONVS - 1, -1, -1):
        key, ml = bwd_target(l)
        mask = None if ml is None else rb["act"][ml]
        out.append(("conv%d data gradient" % (l + 2), _get(rb, key), bwd_conv(ops, fd, rb["dact"][l], l, B, Tin[l], Tout[l], mask)))
        if key[0] == "dpool":
            out.append(("pool backward below conv%d" % (l + 2), rb["dact"][l - 1], ops.pool_bwd(rb["act"][l - 1], rb["dpool"][l - 1])))
    out.append(("pre-filter transposed", rb["grad"], ops.prefilter(rb["dpre"], fd.w25, 0.0, True)))
    out.append(("zero pattern of d conv8 = head rule", (rb["dact"][6] != 0).astype(np.float32), ops.head_mask(rb["act"][6]).astype(np.float32)))
    return out


def mismatches(rb, fd, ops=OPS):
    """names of the stages of ``stage_checks`` whose readback and restatement differ in any bit of any element"""
    bad = []
    for name, got, want in stage_checks(rb, fd, ops):
        got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
        if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            bad.append(name)
    return bad


def ce_demb(emb, fd, y):
    """float64 cross-entropy head on an embedding (B, 32): scores (B, S), loss (B,), d loss / d emb (B, 32)"""
    w, b = fd.fc_w.astype(np.float64), fd.fc_b.astype(np.float64)
    s = emb.astype(np.float64) @ w.T + b
    z = s - s.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    loss = -np.log(p[np.arange(len(y)), y])
    p[np.arange(len(y)), y] -= 1.0
    return s, loss, p @ w


def simulate(fd, feats, y=None, ops=OPS, wb=None):
    """The readbacks of a per-layer pass on ``feats`` (B, F, 32), produced by the restatements (``ops``; ``wb``: other
    data-gradient weights).  The head's sums are float64 rounded once (the engine's are split float32 sums, judged apart).
    ``y`` None: labels one past the decisions."""
    feats = np.ascontiguousarray(feats, np.float32)
    B, F = feats.shape[:2]
    Tin, Tout = an_fold.layer_frames(F)
    rb = dict(feats=feats, act=[None] * an_fold.CONVS, pool={}, dact=[None] * an_fold.CONVS, dpool={})
    rb["pre"] = ops.prefilter(feats, fd.w25, fd.pre_bias, False)
    for l in range(an_fold.CONVS):
        rb["act"][l] = fwd_conv(ops, fd, layer_input(rb, l), l, B, Tin[l], Tout[l])
        if an_fold.POOL[l]:
            rb["pool"][l] = ops.pool_fwd(rb["act"][l])
    rb["emb"] = rb["act"][6].max(1)
    s, _, _ = ce_demb(rb["emb"], fd, np.zeros(B, int))
    rb["y"] = (s.argmax(1) + 1) % s.shape[1] if y is None else np.asarray(y)
    rb["scores"], rb["loss"], demb = ce_demb(rb["emb"], fd, rb["y"])
    rb["dact"][6] = np.where(ops.head_mask(rb["act"][6]), demb.astype(np.float32)[:, None, :], np.float32(0)).astype(np.float32)
    for l in range(an_fold.CONVS - 1, -1, -1):
        key, ml = bwd_target(l)
        g = bwd_conv(ops, fd, rb["dact"][l], l, B, Tin[l], Tout[l], None if ml is None else rb["act"][ml], wb)
        if key[1] is None:
            rb[key[0]] = g
        else:
            rb[key[0]][key[1]] = g
        if key[0] == "dpool":
            rb["dact"][l - 1] = ops.pool_bwd(rb["act"][l - 1], rb["dpool"][l - 1])
    rb["grad"] = ops.prefilter(rb["dpre"], fd.w25, 0.0, True)
    return rb


def conditions(rb):
    """what a case must satisfy to test anything: [(description, holds)] -- every ReLU mask in use (conv3 / conv4 / conv6 in the
    contractions' epilogue, conv2 / conv5 / conv7 in the pooling backward) between 5 % and 95 % active, every compared
    gradient with a non-zero entry"""
    out = []
    for l in range(6):
        frac = float((rb["act"][l] > 0).mean())
        out.append(("ReLU mask of conv%d active in 5 %% .. 95 %% (%.3f)" % (l + 2, frac), 0.05 < frac < 0.95))
    grads = [("dact%d" % (l + 1), rb["dact"][l]) for l in range(7)] + [("dpool%d" % (l + 1), rb["dpool"][l]) for l in POOLED]
    for name, g in grads + [("dpre", rb["dpre"]), ("d loss / d log-mel", rb["grad"])]:
        out.append(("%s has a non-zero entry" % name, bool(np.any(g != 0))))
    return out


def tied_head_maxima(act8):
    """(B,) number of channels of conv8's output (B, T8, 32) whose maximum over time is > 0 and held by more than one frame"""
    m = act8.max(1, keepdims=True)
    return (((act8 == m) & (m > 0)).sum(1) >= 2).sum(1)


def positive_tied_pairs(act):
    """(B,) number of pooled pairs of an un-pooled layer (B, Tin, C) whose two entries are bit-equal and > 0"""
    T2 = act.shape[1] // 2
    a0, a1 = act[:, 0:2 * T2:2], act[:, 1:2 * T2:2]
    return ((a0 == a1) & (a0 > 0)).sum((1, 2))


# ------------------------------------------------------------------------------------------------- the cases' inputs
# (B, F): the 16 x 16 block edge on conv3 (M = 150 B <= 5600: B = 37 | 38) with B = 1 and a ragged B = 3 below it; QUAD32 on the
# 12-chunk layers at B = 64 and QUAD64 on them from M >= 16384 (B = 110); frame counts odd at the second and third pool
# (126 -> 63 -> 31 -> 15), odd at the first (25), and the shortest the stack accepts (24: one frame at conv8)
GRID = ((1, 300), (3, 101), (37, 300), (38, 300), (64, 300), (110, 300), (5, 126), (2, 25), (2, 24))
TIES = (2, 126)
TIES_SEED = 1
_FEATS = {}


def case_feats(B, F, ties=False):
    """log-mel features (B, F, 32) float32 of seeded waveforms from the oracle's front-end; ``ties``: every frame of an utterance
    is the same seeded 32-vector at the log-mel's scale (N(-15, 8) dB), so the interior frames of every layer are bit-identical.
    The zero padding makes the frames at an utterance's edges differ, and in most channels the largest: TIES_SEED is the first
    seed at which every utterance has a channel whose maximum over time is positive and held by the interior frames
    (tests/test_an_stages_power.py checks it on the restated chain)."""
    key = (B, F, ties)
    if key not in _FEATS and ties:
        v = (np.random.RandomState(TIES_SEED).standard_normal((B, 1, 32)) * 8 - 15).astype(np.float32)
        _FEATS[key] = np.ascontiguousarray(np.repeat(v, F, 1))
        _FEATS[key].setflags(write=False)
    if key not in _FEATS:
        import torch
        from oracle.audionet import preprocess
        from speakerguard_amd import synth
        x = torch.from_numpy(synth.make_waveforms(B, 160 * (F - 1) + 1, seed=2000 + B + F))
        with torch.no_grad():
            f = preprocess(x.reshape(B, -1)).transpose(1, 2).numpy().astype(np.float32)
        assert f.shape == (B, F, 32), f.shape
        f = np.ascontiguousarray(f)
        f.setflags(write=False)
        _FEATS[key] = f
    return _FEATS[key]


# ---------------------------------------------------------------------------------------- the launcher's path per contraction
def conv_path(M, N, total_chunks, num_cus=256, s16_max_blocks=2800):
    """What ``conv_plan`` (speakerguard_amd/csrc/sg_internal.h) picks for an AudioNet contraction with the default knobs:
    AudioNet asks for tile 2 with packed weights where N % 128 == 0 and for tile 1 (the 128 x 32 tile kernel) otherwise, one
    split, nothing forced; tile 2 never reaches stream-K."""
    if N % 128:
        return "TILE_128x32"
    if total_chunks >= 4 and ((M + 15) // 16) * (N // 16) <= s16_max_blocks:
        return "S16"
    return "QUAD32" if total_chunks >= 8 and ((M + 63) // 64) * (N // 128) < num_cus else "QUAD64"


def path_table(B, F):
    """[(direction, conv name, M, N, chunks, path)] of the 14 contractions of a per-layer pass, in launch order"""
    Tin, Tout = an_fold.layer_frames(F)
    rows = []
    for l in range(an_fold.CONVS):
        M, N, ch = B * Tout[l], an_fold.COUT[l], 3 * an_fold.CIN[l] // 32
        rows.append(("fwd", an_fold.NAMES[l], M, N, ch, conv_path(M, N, ch)))
    for l in range(an_fold.CONVS - 1, -1, -1):
        M, N, ch = B * Tin[l], an_fold.CIN[l], 3 * an_fold.COUT[l] // 32
        rows.append(("bwd", an_fold.NAMES[l], M, N, ch, conv_path(M, N, ch)))
    return rows
