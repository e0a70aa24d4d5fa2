"""Generate tests/golden/feco_warped_ref.npz (build container only): the REFERENCE's own warped k-means, forward and
autograd gradient.

    python tests/golden/make_golden_feco_warped.py      # needs the reference checkout (REF below)

What is pinned: ``defense/feature_level.py`` ``warped_kmeans`` (:157-165) -> ``wk_compute`` (:114-154) with ``TS``
(:53-77) or ``random_init`` (:80-85) and ``init`` (:88-107), executed unmodified, plus torch autograd's gradient of its
output for a fixed cotangent (which sees only the INITIAL segment means: :135-136 / :150-151 update ``means.data``).

Harness accommodations, disclosed in the fixture's ``meta``:
  * the module imports ``kmeans_pytorch`` at the top (:13); a placeholder module is put in ``sys.modules`` so that the
    import succeeds.  Warped k-means never calls it (the placeholder raises if it is called).
  * ``TS`` and ``random_init`` are wrapped by recording wrappers that call the originals and keep the boundary tensor they
    return: a clone is the INITIAL boundaries, and the tensor itself -- which ``wk_compute`` moves in place -- holds the
    FINAL boundaries after the call.  ``random_init`` draws from numpy's global generator, seeded here.
Every case records the smallest relative |delta_SQE| margin of its decisions under this repository's restatement
(tests/feco_warped_restate.py); only cases whose decisions are all far from float32 rounding of zero are kept, and the
restatement's TS and final boundaries must equal the reference's exactly.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SG_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import feco_warped_restate as R  # noqa: E402
from oracle.audionet import AudioNet  # noqa: E402
from oracle.xv_plda import XvPlda  # noqa: E402
from speakerguard_amd import synth  # noqa: E402

MIN_MARGIN = 1e-4  # relative |delta_SQE| below which a decision could flip with the reduction order
RECORD = []


def _install():
    mod = types.ModuleType("kmeans_pytorch")

    def kmeans(*a, **kw):
        raise AssertionError("warped k-means must not call kmeans_pytorch")
    mod.kmeans = kmeans
    sys.modules["kmeans_pytorch"] = mod
    sys.path.insert(0, REF)
    import defense.feature_level as fl  # the reference module, unmodified
    for name in ("TS", "random_init"):
        orig = getattr(fl, name)

        def wrapper(feat, k, _orig=orig, _name=name):
            b = _orig(feat, k)
            RECORD.append((_name, b.clone(), b))
            return b
        setattr(fl, name, wrapper)
    return fl


def mfcc(T, n, seed):
    x = torch.from_numpy(synth.make_waveforms(n, T, seed=seed))
    with torch.no_grad():
        return XvPlda(synth.make_xv_weights()).compute_feat(x, flag=1).numpy().astype(np.float32)


def logmel(T, n, seed):
    x = torch.from_numpy(synth.make_waveforms(n, T, seed=seed))
    with torch.no_grad():
        return AudioNet(synth.make_audionet_state_dict(seed=0, num_class=251)).compute_feat(x, flag=1).numpy().astype(np.float32)


def main():
    assert not torch.cuda.is_available()
    fl = _install()
    rs = np.random.RandomState(20261015)
    np.random.seed(20261015)  # random_init's np.random.choice
    walk = np.cumsum(rs.randn(300, 30).astype(np.float32) * 0.3, axis=0).astype(np.float32)
    m300, m60, m1200 = mfcc(48000, 2, 7), mfcc(60 * 160, 1, 8), mfcc(1200 * 160, 1, 9)
    lm = logmel(48000, 2, 10)
    cases = [  # tag, features (n, D), ratio, init, delta
        ("mfcc300_ts", m300[0], 0.5, "ts", 0.0),
        ("mfcc300_ts_r03", m300[1], 0.3, "ts", 0.0),
        ("mfcc60_ts", m60[0], 0.5, "ts", 0.0),
        ("mfcc1200_ts", m1200[0], 0.5, "ts", 0.0),
        ("logmel_ts", lm[0], 0.5, "ts", 0.0),
        ("logmel_ts_r02", lm[1], 0.2, "ts", 0.0),
        ("walk_ts_delta", walk, 0.25, "ts", 0.2),
        ("mfcc300_random", m300[1], 0.5, "random", 0.0),
        ("logmel_random", lm[1], 0.4, "random", 0.0),
        ("mfcc60_random", m60[0], 0.8, "random", 0.0),
    ]
    out, kept, margins = {}, [], {}
    for tag, x, ratio, init, delta in cases:
        RECORD.clear()
        feat = torch.from_numpy(x.copy()).requires_grad_(True)
        y = fl.warped_kmeans(feat, param=ratio, delta=delta, other_param=init)
        cot = torch.from_numpy(rs.randn(*y.shape).astype(np.float32))
        (y * cot).sum().backward()
        (name, b0, bfin), = RECORD
        assert name == ("TS" if init == "ts" else "random_init")
        stats = []
        k = int(x.shape[0] * ratio)
        r = R.warped(x, k, init, delta, boundaries=None if init == "ts" else b0.numpy(), stats=stats)
        margin = min(stats) if stats else 1.0
        same = (np.array_equal(r["init_bnd"], b0.numpy()) and np.array_equal(r["bnd"], bfin.numpy()))
        print("%-16s n %4d D %2d k %3d: margin %.3g, boundaries equal %s, max |means diff| %.3g, sweeps %d" % (
            tag, x.shape[0], x.shape[1], k, margin, same, np.abs(r["means"] - y.detach().numpy()).max(), r["sweeps"]))
        if margin < MIN_MARGIN or not same:
            print("   dropped")
            continue
        kept.append(tag)
        margins[tag] = margin
        out[tag + "_feat"] = x
        out[tag + "_k"] = np.int32(k)
        out[tag + "_ratio"] = np.float64(ratio)
        out[tag + "_delta"] = np.float64(delta)
        out[tag + "_init"] = np.array(init)
        out[tag + "_init_bnd"] = b0.numpy().astype(np.int32)
        out[tag + "_bnd"] = bfin.numpy().astype(np.int32)
        out[tag + "_out"] = y.detach().numpy()
        out[tag + "_cot"] = cot.numpy()
        out[tag + "_dfeat"] = feat.grad.numpy()
    # the degenerate TS init: zero frames and one large jump in the last frame -> [0, 39, 22, 23, ...] (F 40, k 20)
    deg = np.zeros((40, 30), np.float32)
    deg[-1] = 100.0
    RECORD.clear()
    bd = fl.TS(torch.from_numpy(deg), 20).numpy().astype(np.int32)
    assert not R.valid(bd, 40) and np.array_equal(R.ts_boundaries(deg, 20), bd), bd
    out["degenerate_feat"] = deg
    out["degenerate_k"] = np.int32(20)
    out["degenerate_ts_bnd"] = bd
    meta = {
        "generator": "tests/golden/make_golden_feco_warped.py",
        "reference": "SpeakerGuard defense/feature_level.py warped_kmeans / wk_compute / TS / random_init / init, unmodified",
        "accommodation": "sys.modules['kmeans_pytorch'] = placeholder (only so that the import at :13 succeeds; never called); "
                         "TS and random_init wrapped by recording wrappers that return the originals' tensor unchanged "
                         "(clone = initial boundaries, the tensor after the call = final boundaries, moved in place by "
                         "wk_compute); random_init draws from numpy's global generator seeded 20261015",
        "cases": kept, "min_rel_margin": margins, "margin_floor": MIN_MARGIN,
        "degenerate": "TS boundaries of 40 zero frames with the last one at 100, k = 20 (only TS recorded)",
        "torch": torch.__version__, "numpy": np.__version__,
    }
    path = os.path.join(HERE, "feco_warped_ref.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), "cases", kept)


if __name__ == "__main__":
    main()
