"""The float64 truth the hand-coded gradients are judged against.  TEST INFRASTRUCTURE (a plain module, not a conftest).

Two fp32 implementations of the same model -- the HIP engine and the PyTorch-CPU oracle -- reduce in different orders, so
their difference says little about either one's accuracy.  Both are measured here against the SAME oracle evaluated in
float64 (the fp32-rounded constants, wider arithmetic), and the engine is accepted when it is at least about as close to
that truth as the fp32 oracle is, utterance by utterance and 160-sample hop by hop (DESIGN.md "Tolerances").

    fp32, fp64 = evaluate(oracle_model, x, y, Loss("ce"))          # the yardstick and the truth
    rep = check(Side.of(dec, scores, loss, grad), fp32, fp64, ...)  # the policy, one table of constants below
    rep.assert_ok()

tests/test_truth_power.py proves on the CPU that the policy accepts the fp32 oracle and rejects planted defects.
"""
import copy
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)  # 1.19e-7

# ---------------------------------------------------------------------------------------------------------------- policy
# Every constant of the judgement.  `yard` = the fp32 oracle's error against the fp64 truth on the same input.
POLICY = dict(
    # per utterance: judged relative L2 error <= C * yard's (same utterance), and the worst 160-sample hop's RMS error
    # (over the utterance's RMS |g64|) <= C * yard's worst hop.  2: what the issue's prototype separates on (fp32 oracle
    # 6.6e-3 / 4.5e-2 against planted defects from 1.7e-2 / 0.24 upward).
    C=2.0,
    # batch: aggregate RMS error of the judged gradient <= C_AGG * yard's + FLOOR_UTT -- the DESIGN.md claim that the engine
    # is at least as close to the fp64 model as the fp32 oracle is (the floor: where both carry the same error, e.g. a
    # shared fp32 input rounding, the two agree to round-off and either may be the larger).
    C_AGG=1.0,
    # "decided" entries: |g64| > TAU * RMS_u(g64).  No fp32 round-off flips their sign; a disagreement there is a defect.
    TAU=0.5,
    # floors, in units of fp32 eps, for where the yard's own error is round-off (AudioNet: ~1e-6 relative): two
    # independent round-off levels do not stay within 2x of each other.  256 eps = 3.1e-5 on the utterance norm, 2048 eps
    # = 2.4e-4 on the worst hop (a hop holds 160 entries: its RMS is a few-sample statistic).  The planted defects of
    # tests/test_truth_power.py sit at 3e-3 and above.
    FLOOR_UTT=256 * EPS32,
    FLOOR_BLOCK=2048 * EPS32,
    # scores and loss, per utterance: |judged - truth| <= C * (yard's largest error in the batch) + FLOOR_SCORE * max|s64|
    # of that utterance.  The score error is set by the shared conditioning of the front-end (log of weak bands), so the
    # yard's error on one utterance is a noisy scale; its batch maximum is not.  16 eps: the fp32 round-off of the
    # PLDA / logit sums themselves.
    FLOOR_SCORE=16 * EPS32,
)
# two members of a max-pool pair closer than this (relative) are a tie the judged side's pooled output cannot resolve
POOL_TIE = 256 * EPS32
MAX_TIE_BITS = 3  # alternatives tried for the pool ties of an utterance: 2 ** 3 fp64 passes at most
HOP = 160  # the MFCC frame shift: defects local to edge frames, partial tiles and the padding live at this scale


# ---------------------------------------------------------------------------------------------------------------- losses
class Loss:
    """The attack losses (attack/utils.py:7-102, oracle/attacks.py) in the dtype of the scores they are given, plus the
    engine's description of the same loss.  kind: 'ce' | 'margin'."""

    def __init__(self, kind="ce", targeted=False, confidence=0.0, task="CSI", threshold=None, clip_max=True):
        assert kind in ("ce", "margin")
        self.kind, self.targeted, self.confidence, self.task = kind, targeted, confidence, task
        self.threshold, self.clip_max = threshold, (clip_max if kind == "margin" else False)

    def spec(self):
        from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss
        if self.kind == "ce":
            return SEC4SR_CrossEntropy()
        return SEC4SR_MarginLoss(self.targeted, self.confidence, self.task, self.threshold, self.clip_max)

    def __repr__(self):
        if self.kind == "ce":
            return "CE"
        return "Margin %s%s%s" % (self.task, " targeted" if self.targeted else "", " clip" if self.clip_max else "")

    def unclipped(self, s, y):
        if self.kind == "ce":
            return F.cross_entropy(s, y, reduction="none")
        # the reference's rules at ties (attack/utils.py:41-102, tests/test_oracle_losses.py): the confidence is a tensor of
        # the scores' dtype (the threshold, a Python float, rounds to it in the additions); torch.max(t, dim) sends the
        # gradient to the first maximal index; `other` is the max over the row with the label's entry at the -10000 sentinel
        conf, thr = torch.tensor(self.confidence, dtype=s.dtype), self.threshold
        imp_zero = 0.0 * s[y == -1].sum()  # CSI imposters: one 0 * sum over all of them, the batch's sign of zero
        rows = []
        for i in range(s.shape[0]):
            si, yi = s[i], int(y[i])
            if self.task == "SV":
                rows.append(thr + conf - si[0] if (yi == 0) == self.targeted else si[0] + conf - thr)
                continue
            top = si.max(0)[0]
            if yi == -1:
                if self.task == "OSI":
                    rows.append(top + conf - thr if self.targeted else thr + conf - top)
                else:
                    rows.append(imp_zero)
                continue
            onehot = torch.zeros_like(si)
            onehot[yi] = 1
            real = si[yi]
            other = ((1 - onehot) * si - onehot * 10000).max(0)[0]
            if self.targeted:
                rows.append(other + conf - real if self.task == "CSI" else torch.clamp(other, min=thr) + conf - real)
            elif self.task == "CSI":
                rows.append(real + conf - other)
            else:
                rows.append(torch.minimum(top + conf - thr, torch.clamp(real, min=thr) + conf - other))
        return torch.stack(rows)

    def __call__(self, s, y):
        l = self.unclipped(s, y)
        # binary max as the reference's clip (:100): 0.5 to each side at l == 0, where clamp(min=0) passes all of it
        return torch.max(torch.zeros((), dtype=l.dtype), l) if self.clip_max else l


# ---------------------------------------------------------------------------------------------------------------- evaluation
@dataclass
class Side:
    """One implementation's answer on a batch: scores (B, S), loss (B,), d loss / d input (B, ...), all float64."""
    scores: np.ndarray
    loss: np.ndarray
    grad: np.ndarray

    @staticmethod
    def of(scores, loss, grad):
        f = lambda t: (t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64))
        return Side(f(scores), f(loss), f(grad))


def default_forward(model, x):
    return model(x)


def _run(model, x, y, loss, forward, dtype):
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    s = forward(model, xin)
    l = loss(s, y)
    l.backward(torch.ones_like(l))
    return Side.of(s, l, xin.grad)


def evaluate(model, x, y, loss, forward=default_forward, truth_model=None):
    """`model`: an fp32 oracle (oracle.xv_plda.XvPlda, oracle.audionet.AudioNet).  Returns (fp32 Side, fp64 Side): the
    same model and forward evaluated in float32 (the yardstick) and in float64 (the truth).  `forward(model, x) -> scores`
    composes defenses (FeCo with the device's cluster ids) around the model; `truth_model`: an fp64 model to use instead
    of a copy of `model` (tests that plant a defect in the fp32 side only)."""
    m64 = truth_model if truth_model is not None else copy.deepcopy(model).double()
    return _run(model, x, y, loss, forward, torch.float32), _run(m64, x, y, loss, forward, torch.float64)


def evaluate_truth(model64, x, y, loss, forward=default_forward):
    return _run(model64, x, y, loss, forward, torch.float64)


def pattern_truths(model64, acts, x, y, loss, forward=default_forward):
    """The fp64 truth under the judged side's activation pattern: one Side per resolution of the pool ties (pattern_model)."""
    m = pattern_model(model64, acts)
    out = [evaluate_truth(m, x, y, loss, forward)]
    n = int(getattr(m, "pool_ties", torch.zeros(1)).max())
    for c in range(1, 2 ** min(n, MAX_TIE_BITS)):
        out.append(evaluate_truth(pattern_model(model64, acts, c), x, y, loss, forward))
    return out


# ---- the truth under the judged side's own activation pattern (ReLU / max-pool decisions within round-off of a tie)
def pattern_model(model64, acts, choice=0):
    """A copy of the fp64 model whose ReLU (and max-pool) decisions are the judged side's, read back from its activations.
    XvPlda: `acts` = [ReLU output of tdnn1..5, (B, F_l, C_pad) channel-last]; AudioNet: [output of layer 1..8 after its
    pooling, (B, L_l, C)].  A pooled output picks the member of its pair nearest the judged value; AudioNet's embedding (the
    maximum over time of layer 8) is taken at the frame where the judged side's layer 8 is largest.

    A pair whose two members are within round-off of each other (POOL_TIE) does not say which one the judged side took:
    the k-th such pair of an utterance (in layer, channel, position order) takes the nearest member if bit k of `choice`
    is 0, the other one if it is 1.  After a forward, ``m.pool_ties`` holds the number of such pairs per utterance."""
    from oracle import audionet as oan
    from oracle import xv_plda as oxv
    m = copy.deepcopy(model64)
    masks = [torch.as_tensor(np.asarray(a, np.float64)).transpose(1, 2) for a in acts]  # (B, C, L)
    if isinstance(m, oxv.XvPlda):
        def tdnn_layers(x):
            outs, p = [], m.params
            for (name, _, dil), act in zip(oxv.TDNN_SPEC, masks):
                z = F.conv1d(x, p[name + ".weight"], p[name + ".bias"], dilation=dil)
                assert act.shape[2] == z.shape[2], ("activation pattern of another pass", name, act.shape, z.shape)
                a = z * (act[:, :z.shape[1], :z.shape[2]] > 0).to(z.dtype)
                x = F.batch_norm(a, p["bn_" + name + ".running_mean"], p["bn_" + name + ".running_var"],
                                 None, None, False, 0.1, oxv.BN_EPS)
                outs.append((a, x))
            return outs
        m.tdnn_layers = tdnn_layers
        return m
    assert isinstance(m, oan.AudioNet), type(m)

    def layers(feats):
        p = m.p
        x = feats.transpose(1, 2).unsqueeze(1)
        x = m._bn(F.conv2d(x, p["conv1.0.weight"], p["conv1.0.bias"], padding=2), "conv1.1").squeeze(1)
        outs = [x]
        ties = torch.zeros(x.shape[0], dtype=torch.int64)
        for (name, _, _, _, pad, pool), act in zip(oan.CONV_SPEC, masks[1:]):
            if name == "conv8" and x.shape[2] < 3:
                x = x.repeat(1, 1, -(-3 // x.shape[2]))
            z = m._bn(F.conv1d(x, p[name + ".0.weight"], p[name + ".0.bias"], padding=pad), name + ".1")
            assert act.shape[2] == (z.shape[2] // 2 if pool else z.shape[2]), ("activation pattern of another pass", name)
            if pool:
                L = z.shape[2] // 2
                pairs = z[:, :, :2 * L].reshape(z.shape[0], z.shape[1], L, 2)
                pd = pairs.detach()
                pick = (pd - act.unsqueeze(3)).abs().argmin(3, keepdim=True)
                tie = ((pd[..., 0] - pd[..., 1]).abs() <= POOL_TIE * (1 + pd.abs().amax(3))) & (act > 0)
                k = tie.flatten(1).cumsum(1).view_as(tie) - 1 + ties.view(-1, 1, 1)  # index of each tie in its utterance
                other = tie & ((choice >> k.clamp(min=0, max=62)) & 1).bool()
                pick = torch.where(other.unsqueeze(3), 1 - pick, pick)
                ties += tie.flatten(1).sum(1)
                z = pairs.gather(3, pick).squeeze(3)
            x = z * (act > 0).to(z.dtype)
            outs.append(x)
        m.pool_ties = ties
        return outs

    def extract_emb(feats):  # the time maximum of the last layer taken at the judged side's frame
        return layers(feats)[-1].gather(2, masks[-1].argmax(2, keepdim=True)).squeeze(2)
    m.layers, m.extract_emb = layers, extract_emb
    return m


# ---------------------------------------------------------------------------------------------------------------- metrics
def _flat(g):
    return np.asarray(g, np.float64).reshape(g.shape[0], -1)


def utt_error(g, g64):
    g, g64 = _flat(g), _flat(g64)
    return np.linalg.norm(g - g64, axis=1) / np.maximum(np.linalg.norm(g64, axis=1), 1e-300)


def block_error(g, g64, hop=HOP):
    """Per utterance: the largest RMS error over `hop`-entry blocks, over the utterance's RMS |g64| (a last partial
    block counts over its own entries)."""
    g, g64 = _flat(g), _flat(g64)
    B, n = g.shape
    nb = -(-n // hop)
    e2 = np.zeros((B, nb * hop))
    e2[:, :n] = (g - g64) ** 2
    cnt = np.full(nb, float(hop))
    cnt[-1] = n - (nb - 1) * hop
    rms_blocks = np.sqrt(e2.reshape(B, nb, hop).sum(2) / cnt)
    rms_u = np.sqrt((g64 ** 2).mean(1))
    return rms_blocks.max(1) / np.maximum(rms_u, 1e-300)


def decided(g64, tau=None):
    g64 = _flat(g64)
    tau = POLICY["TAU"] if tau is None else tau
    return np.abs(g64) > tau * np.sqrt((g64 ** 2).mean(1, keepdims=True))


def decided_sign(g, g64, tau=None):
    """Per utterance: sign disagreements on entries whose sign no fp32 round-off can flip."""
    return ((np.sign(_flat(g)) != np.sign(_flat(g64))) & decided(g64, tau)).sum(1)


def aggregate_error(g, g64):
    g, g64 = _flat(g), _flat(g64)
    return float(np.sqrt(((g - g64) ** 2).sum() / max((g64 ** 2).sum(), 1e-300)))


def metrics(side, truth, hop=HOP):
    return dict(utt=utt_error(side.grad, truth.grad), block=block_error(side.grad, truth.grad, hop),
                decided_sign=decided_sign(side.grad, truth.grad),
                score=np.abs(side.scores - truth.scores).max(1), loss=np.abs(side.loss - truth.loss),
                aggregate=aggregate_error(side.grad, truth.grad))


# ---------------------------------------------------------------------------------------------------------------- judgement
@dataclass
class Report:
    name: str
    judged: dict
    yard: dict
    failures: list = field(default_factory=list)   # (metric, utterance or -1, value, bound)
    explained: list = field(default_factory=list)  # utterances accepted against the judged side's activation pattern
    zero_loss: int = 0                              # utterances whose loss is clipped to exactly 0 (zero gradient asserted)

    @property
    def failed(self):
        return sorted({f[0] for f in self.failures})

    def line(self):
        j, y = self.judged, self.yard
        fmt = lambda a: "%.2e" % np.max(a)
        return ("%s: judged/yard vs fp64 -- aggregate %.2e/%.2e, utt max %s/%s, block max %s/%s, decided sign %d/%d, "
                "score max %s/%s, loss max %s/%s%s%s%s" % (
                    self.name, j["aggregate"], y["aggregate"], fmt(j["utt"]), fmt(y["utt"]), fmt(j["block"]),
                    fmt(y["block"]), int(np.sum(j["decided_sign"])), int(np.sum(y["decided_sign"])), fmt(j["score"]),
                    fmt(y["score"]), fmt(j["loss"]), fmt(y["loss"]),
                    "; %d zero-loss utterances" % self.zero_loss if self.zero_loss else "",
                    "; accepted on the judged activation pattern: %s" % self.explained if self.explained else "",
                    "; FAILED %s" % self.failures[:8] if self.failures else ""))

    def assert_ok(self):
        assert not self.failures, self.line()


def _bounds(judged, yard, truth, hop, judged_truth=None):
    """(metric, utterance, value, bound) of every violated per-utterance bound; the judged side measured against
    `judged_truth` (default: `truth`), the yard always against `truth`."""
    P, out = POLICY, []
    mj, my = metrics(judged, truth if judged_truth is None else judged_truth, hop), metrics(yard, truth, hop)
    for u in range(judged.grad.shape[0]):
        for name, floor in (("utt", P["FLOOR_UTT"]), ("block", P["FLOOR_BLOCK"])):
            bound = P["C"] * max(my[name][u], floor)
            if not mj[name][u] <= bound:
                out.append((name, u, float(mj[name][u]), float(bound)))
        if mj["decided_sign"][u] != 0:
            out.append(("decided_sign", u, int(mj["decided_sign"][u]), 0))
    return mj, my, out


def check(judged, yard, truth, name="", hop=HOP, clipped=None, pattern_truth=None):
    """Judge `judged` (a Side) against the fp64 `truth`, with the fp32 oracle `yard` on the same input as the yardstick.

    clipped: bool (B,) -- utterances whose loss is clipped to exactly 0: their judged gradient must be exactly zero (and is
      left out of the gradient metrics, whose truth is then zero too).
    pattern_truth: callable () -> Side or [Side], the fp64 truth under the judged side's own activation pattern
      (pattern_truths: one per resolution of the pool ties).  An utterance over a gradient bound is accepted only if it
      meets every bound against one of them; the aggregate then uses that truth for it.  Without it, the utterance fails."""
    P = POLICY
    B = judged.grad.shape[0]
    keep = np.ones(B, bool) if clipped is None else ~np.asarray(clipped, bool)
    failures, zero = [], int((~keep).sum())
    for u in np.nonzero(~keep)[0]:
        if truth.loss[u] != 0 or np.any(_flat(judged.grad)[u] != 0) or np.any(_flat(truth.grad)[u] != 0):
            failures.append(("clipped_zero", int(u), float(np.abs(_flat(judged.grad)[u]).max()), 0.0))
    sub = lambda s: Side(s.scores[keep], s.loss[keep], s.grad[keep])
    idx = np.nonzero(keep)[0]
    j, y, t = sub(judged), sub(yard), sub(truth)
    explained = []
    if idx.size:
        mj, my, bad = _bounds(j, y, t, hop)
        bad_u = sorted({b[1] for b in bad})
        if bad_u and pattern_truth is not None:
            alts = pattern_truth()
            alts = alts if isinstance(alts, (list, tuple)) else [alts]
            for tp in map(sub, alts):
                _, _, bad_p = _bounds(j, y, t, hop, judged_truth=tp)
                still = {b[1] for b in bad_p}
                for u in bad_u:
                    if u not in still and int(idx[u]) not in explained:
                        explained.append(int(idx[u]))
                        t.grad[u] = tp.grad[u]  # that utterance's truth is the pattern one from here on
            explained.sort()
            bad = [b for b in bad if int(idx[b[1]]) not in explained]
            mj = metrics(j, t, hop)
        failures += [(m, int(idx[u]), v, bd) for m, u, v, bd in bad]
        agg_bound = P["C_AGG"] * my["aggregate"] + P["FLOOR_UTT"]  # (a tie at the yard's level is not a failure)
        if not mj["aggregate"] <= agg_bound:
            failures.append(("aggregate", -1, mj["aggregate"], agg_bound))
    else:
        mj = my = {k: np.zeros(1) for k in ("utt", "block", "decided_sign", "score", "loss", "aggregate")}
        mj["aggregate"] = my["aggregate"] = 0.0
    # scores and loss over every utterance (clipped ones included)
    ms_j, ms_y = metrics(judged, truth, hop), metrics(yard, truth, hop)
    smax = np.abs(truth.scores).max(1)
    for key in ("score", "loss"):
        bound = P["C"] * ms_y[key].max() + P["FLOOR_SCORE"] * smax
        for u in np.nonzero(~(ms_j[key] <= bound))[0]:
            failures.append((key, int(u), float(ms_j[key][u]), float(bound[u])))
    mj = dict(mj, score=ms_j["score"], loss=ms_j["loss"])
    my = dict(my, score=ms_y["score"], loss=ms_y["loss"])
    return Report(name, mj, my, failures, explained, zero)


# ---------------------------------------------------------------------------------------------------------------- one step
def one_step_signs(x_adv, x, step):
    """The sign step a one-iteration PGD took, per sample: round((x_adv - x) / step) in {-1, 0, 1}."""
    return np.rint((np.asarray(x_adv, np.float64) - np.asarray(x, np.float64)) / step).reshape(x_adv.shape[0], -1)


def one_step(judged_step, yard_step, g64, grad_sign=1):
    """judged_step / yard_step: the sign each side's single PGD step took, (B, N).  Returns (fraction of samples whose step
    differs from grad_sign * sign(g64) for judged and yard, disagreements on decided entries for judged and yard)."""
    want = grad_sign * np.sign(_flat(g64))
    dm = decided(g64)
    out = []
    for s in (judged_step, yard_step):
        diff = s.reshape(want.shape) != want
        out += [float(diff.mean()), int((diff & dm).sum())]
    return out
