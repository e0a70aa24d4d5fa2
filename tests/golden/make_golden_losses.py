"""Generate tests/golden/loss_ref.npz (build container only): the REFERENCE's own loss stage on designed score tables.

    python tests/golden/make_golden_losses.py      # needs the reference checkout (REF below)

What is pinned: ``attack/utils.py`` ``SEC4SR_CrossEntropy(reduction='none')`` (:7-29) and ``SEC4SR_MarginLoss`` (:31-102),
executed unmodified on the CPU in float32, with torch autograd's d loss / d scores for a cotangent of ones, and the
decision rule of ``model/iv_plda.py`` :188-192 (argmax, first index; -1 unless max > threshold).

Layout.  For every class count S and every (threshold, confidence) variant v there is one score table
``S{S}_v{v}_scores`` (R, S) float32 with its labels ``_labels`` (R,) int64, decisions ``_dec`` (R,) int64 and per-row
annotations (meta["rows"]).  Every loss configuration c of meta["configs"] that applies to S has ``S{S}_v{v}_{c}_loss``
(R,) and ``_grad`` (R, S).  SV runs at S = 1 only, as the reference requires.

The rows are designed so that the reference's autograd rules decide the gradient: ties for the maximum (first index wins
under torch.max(x, dim)), other == real, other == threshold, real == threshold, f_reject == f_mis (torch.minimum: 0.5
each), a margin loss of exactly 0 before the clip (binary torch.max: 0.5 each), max == threshold for the decision, a
saturated cross entropy, every other score at or below the -10000 sentinel, and a threshold that float32 rounds.  Every
equality is made in float32 arithmetic with the float32-rounded threshold and confidence, as the reference computes.
The archive is written with fixed zip timestamps, so a second run reproduces it byte for byte.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SG_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

SIZES = (1, 2, 3, 10, 31, 32, 33, 63, 64, 65, 251, 1024)
# (threshold as a Python float, confidence): dyadic; a threshold float32 rounds to 1.0 with a non-dyadic confidence;
# non-dyadic both
VARIANTS = ((0.5, 0.0), (0.99999999, 0.3), (-0.1, 0.7))
# name -> (kind, task, targeted, clip_max)
CONFIGS = {"ce": ("ce", "CSI", False, False)}
for _task in ("CSI", "OSI", "SV"):
    for _tg in (0, 1):
        for _clip in (0, 1):
            CONFIGS["%s_t%d_c%d" % (_task.lower(), _tg, _clip)] = ("margin", _task, bool(_tg), bool(_clip))
SENTINEL = -10000.0
f32 = np.float32


def _ties(S):
    """Index pairs that tie for the maximum: beginning, middle, end, and across waves / threads at large S."""
    pairs = [(0, 1), (S // 2 - 1, S // 2), (S - 2, S - 1), (0, S - 1)]
    if S > 40:
        pairs.append((3, 40))
    if S > 64:
        pairs.append((5, S - 6))
    if S > 900:
        pairs.append((5, 900))
    if S > 300:
        pairs.append((255, 256))
    out = []
    for p in pairs:
        if p[0] >= 0 and p[0] < p[1] < S and p not in out:
            out.append(p)
    return out


def design(S, thr, conf, rng):
    """(scores (R, S) float32, labels (R,), row names) for one class count and one variant."""
    t, c = f32(thr), f32(conf)
    rows = []

    def base():
        return (rng.integers(-40, 40, S) * 0.25).astype(np.float32)  # [-10, 10), dyadic

    def add(name, s, y):
        rows.append((name, np.asarray(s, np.float32), int(y)))

    # plain rows: label the argmax, another class, an imposter
    s = base()
    add("plain_y_argmax", s, int(np.argmax(s)))
    add("plain_y_other", s, (int(np.argmax(s)) + 1) % S)
    add("plain_imposter", s, -1)
    if S >= 2:
        for a, b in _ties(S):
            s = base()
            s[a] = s[b] = f32(s.max() + 1.0)
            lab = next(j for j in range(S) if j not in (a, b)) if S > 2 else a
            add("tie_max_%d_%d_y%d" % (a, b, lab), s, lab)
            add("tie_max_%d_%d_y_first" % (a, b), s, a)  # other == real
            add("tie_max_%d_%d_y_second" % (a, b), s, b)
            add("tie_max_%d_%d_imposter" % (a, b), s, -1)
        # three-way tie for `other` below a larger real
        if S >= 4:
            s = base()
            m = f32(s.max() + 1.0)
            s[1] = s[S // 2] = s[S - 1] = m
            s[0] = f32(m + 2.0)
            add("tie_other_three_y0", s, 0)
        # other == threshold (OSI targeted clamp and f_mis; label the argmax: f_reject == f_mis)
        s = np.minimum(base(), f32(t - 4.0))
        j, k = S // 3, (S // 3 + 1) % S
        s[j] = f32(t + 2.0)
        s[k] = t
        add("other_eq_thr_y_argmax", s, j)      # f_reject == f_mis
        add("other_eq_thr_y_low", s, (k + 1) % S if (k + 1) % S != j else (k + 2) % S)
        # real == threshold
        s = np.minimum(base(), f32(t - 3.0))
        s[k] = t
        add("real_eq_thr_y_max", s, k)
        s[j] = f32(t + 1.0)
        add("real_eq_thr_y_below_max", s, k)
        # max == threshold (decision: rejected) and a tie at the threshold
        s = np.minimum(base(), f32(t - 1.0))
        s[S - 1] = t
        add("max_eq_thr", s, S - 1)
        s = s.copy()
        s[0] = t
        add("max_eq_thr_tie", s, 0)
        add("max_eq_thr_tie_imposter", s, -1)
        # margin exactly 0 before the clip: CSI untargeted real + c - other, targeted other + c - real
        s = base()
        s[j] = f32(2.5)
        s[k] = f32(s[j] + c)
        s[[i for i in range(S) if i not in (j, k)]] = np.minimum(s[[i for i in range(S) if i not in (j, k)]], f32(-1.0))
        add("zero_margin_untargeted", s, j)
        s = s.copy()
        s[k], s[j] = f32(2.5), f32(f32(2.5) + c)
        add("zero_margin_targeted", s, j)
        # OSI targeted zero margin: clamp(other, thr) + c - real == 0 with other below the threshold
        s = np.minimum(base(), f32(t - 2.0))
        s[j] = f32(t + c)
        add("zero_margin_osi_targeted", s, j)
        # every other score below, and at, the -10000 sentinel
        s = np.full(S, -20000.0, np.float32)
        s[j] = f32(3.0)
        add("others_below_sentinel", s, j)
        s = s.copy()
        s[0 if j else S - 1] = f32(SENTINEL)
        add("other_at_sentinel", s, j)
    else:
        add("single_eq_thr", np.array([t]), 0)
        add("single_eq_thr_imposter", np.array([t]), -1)
        add("single_zero_margin_up", np.array([f32(t + c)]), 0)
        add("single_zero_margin_down", np.array([f32(t - c)]), 0)
        add("single_zero_margin_down_imposter", np.array([f32(t - c)]), -1)
        add("single_below_sentinel", np.array([f32(-20000.0)]), 0)
    # a saturated cross entropy (d/ds_y is exactly 0 in float32), and one that is not quite
    s = base()
    y0 = S // 2
    s[y0] = f32(s.max() + 40.0)
    add("ce_saturated", s, y0)
    s = s.copy()
    s[y0] = f32(np.sort(s)[-2] + 12.0) if S > 1 else s[y0]
    add("ce_near_saturated", s, y0)
    # random rows, not dyadic: the float32 order of thr + c - s decides the low bits
    for r in range(4):
        s = (rng.standard_normal(S) * 3.0).astype(np.float32)
        lab = int(rng.integers(-1, S)) if r else int(np.argmax(s))
        add("random_%d" % r, s, lab)
        if r == 0:
            s2 = s.copy()
            s2[int(np.argmax(s))] = f32(t + f32(rng.standard_normal() * 1e-6))  # max close to the threshold
            add("random_max_near_thr", s2, lab)
    names = [r[0] for r in rows]
    return np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int64), names


def reference_losses():
    sys.path.insert(0, REF)
    from attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss  # the reference module, unmodified
    return SEC4SR_CrossEntropy, SEC4SR_MarginLoss


def run(cfg, scores, labels, thr, conf, CE, MG):
    kind, task, targeted, clip = cfg
    s = torch.from_numpy(scores.copy()).requires_grad_(True)
    y = torch.from_numpy(labels.copy())
    fn = CE(reduction="none") if kind == "ce" else MG(targeted=targeted, confidence=conf, task=task, threshold=thr,
                                                      clip_max=clip)
    loss = fn(s, y)
    loss.backward(torch.ones_like(loss))
    assert loss.dtype == torch.float32 and s.grad.dtype == torch.float32
    return loss.detach().numpy().copy(), s.grad.numpy().copy()


def decide(scores, thr):
    s = torch.from_numpy(scores)
    dec = torch.argmax(s, dim=1)
    mx = torch.max(s, dim=1)[0]
    return torch.where(mx > thr, dec, torch.tensor([-1] * dec.shape[0], dtype=torch.int64)).numpy()


def save(path, arrays):
    """np.savez_compressed with fixed zip timestamps (numpy stamps the current time): byte-reproducible."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    CE, MG = reference_losses()
    rng = np.random.default_rng(20261015)
    out, rows = {}, {}
    for S in SIZES:
        for v, (thr, conf) in enumerate(VARIANTS):
            sc, lab, names = design(S, thr, conf, rng)
            tag = "S%d_v%d" % (S, v)
            out[tag + "_scores"], out[tag + "_labels"], out[tag + "_dec"] = sc, lab, decide(sc, thr)
            rows[tag] = names
            for name, cfg in CONFIGS.items():
                if cfg[1] == "SV" and S != 1:
                    continue
                loss, grad = run(cfg, sc, lab, thr, conf, CE, MG)
                out["%s_%s_loss" % (tag, name)], out["%s_%s_grad" % (tag, name)] = loss, grad
    meta = {
        "generator": "tests/golden/make_golden_losses.py",
        "reference": "SpeakerGuard attack/utils.py SEC4SR_CrossEntropy(reduction='none') and SEC4SR_MarginLoss, unmodified; "
                     "decision rule of model/iv_plda.py:188-192",
        "sizes": list(SIZES), "variants": [list(v) for v in VARIANTS],
        "configs": {k: list(v) for k, v in CONFIGS.items()}, "rows": rows,
        "sv": "SV configurations at S = 1 only",
        "torch": torch.__version__, "numpy": np.__version__,
    }
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(HERE, "loss_ref.npz")
    save(path, out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), "tables", len(rows))


if __name__ == "__main__":
    main()
