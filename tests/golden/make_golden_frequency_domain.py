"""Generate tests/golden/freq_domain_ref.npz (build container only): the REFERENCE's own Butterworth defenses ``LPF`` (:33-70)
and ``BPF`` (:72-112) of ``defense/frequency_domain.py``, forward and autograd gradient, on the CPU, next to the float64 truth.

    python tests/golden/make_golden_frequency_domain.py      # needs the reference checkout (REF below)

The reference module is imported UNMODIFIED behind two disclosed accommodations placed in ``sys.modules`` (neither package
is installed here):
  * ``torchaudio``: an empty module (only ``DS`` uses it, which is not pinned);
  * ``torch_lfilter``: a module whose ``lfilter(b, a, x)`` is an autograd function that runs ``scipy.signal.lfilter`` in
    float64 on the float32 coefficient tensors it is handed (so the reference's cast of b, a to float32 is in effect) and
    returns float32; its backward is the flipped filter, flip(lfilter(b, a, flip(g))).
Per case: parameters and design (order, Wn, float64 sos, largest pole radius of the direct form's ``a`` before and after the
float32 cast) in ``meta``; the input and cotangent (slices of shared arrays); the reference's output and autograd's
gradient; for T <= 259 the float64 truth ``sosfilt(sos, x)`` (clamped like the reference) and its adjoint.  For the four
long cases of the shape sweep the truth is NOT stored -- two float64 arrays of 8195 samples alone would take half the
file's budget -- and the tests recompute it from the recorded sos with the same two lines (``truth`` / ``truth_adjoint``
below); they check that recipe against every truth that IS stored.
The default ``BPF`` is recorded as the fact that the reference's output is non-finite (how many samples, the first one), on
4095 samples: its direct form's poles leave the unit circle with the float32 cast, the output overflows float64 after some
2500 samples (float32 arithmetic would after some 300), and ``clamp`` keeps the NaN that follows.
Inputs sit on the int16 grid with amplitude <= 0.25 so that no pre-clamp value comes near +-1; the clamp case is a square-like
wave of amplitude 0.98 whose overshoot crosses 1 (checked here: fewer than 1 % of its samples lie within 1e-5 of +-1); one
input is int16-scaled.  Cotangents sit on a 2^-8 grid.
Shapes (lpf5000): T over 1, 2, C-1, C, C+1, W-1, W, W+1, P-1, P, P+1, 2P+3 for the kernel's C = 4 samples per lane, W = 256
per wave, P = 4096 per block pass; B = 3 at T = 1, 2, 257, one row elsewhere.  The other filters run on W + 3 = 259 samples.
"""
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SG_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

C, W, P = 4, 256, 4096
T_SHORT, T_LONG = W + 3, 2 * P + 3


class _Lfilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, a, x):
        ctx.b, ctx.a = b.numpy().astype(np.float64), a.numpy().astype(np.float64)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return torch.from_numpy(signal.lfilter(ctx.b, ctx.a, x.detach().numpy().astype(np.float64), axis=0).astype(np.float32))

    @staticmethod
    def backward(ctx, g):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            gx = signal.lfilter(ctx.b, ctx.a, g.numpy().astype(np.float64)[::-1], axis=0)[::-1]
        return None, None, torch.from_numpy(np.ascontiguousarray(gx).astype(np.float32))


def install_accommodations():
    sys.modules["torchaudio"] = types.ModuleType("torchaudio")
    m = types.ModuleType("torch_lfilter")
    m.lfilter = lambda b, a, x: _Lfilter.apply(b, a, x)
    sys.modules["torch_lfilter"] = m


def design(kind, wp, ws, fs=16000, gpass=3, gstop=40):
    """the reference's recipe (:53-57, :93-97), in sos form as well"""
    if kind == "LPF":
        wpn, wsn, btype = 2 * wp / fs, 2 * ws / fs, "low"
    else:
        wpn, wsn, btype = [2 * w / fs for w in wp], [2 * w / fs for w in ws], "bandpass"
    N, Wn = signal.buttord(wpn, wsn, gpass, gstop, analog=False, fs=None)
    b, a = signal.butter(N, Wn, btype=btype, analog=False, output="ba")
    sos = signal.butter(N, Wn, btype=btype, analog=False, output="sos")
    return int(N), np.atleast_1d(Wn).astype(np.float64), b, a, sos


def truth(sos, x, lo, hi):
    """float64: (clamped output, mask, pre-clamp value)"""
    v = signal.sosfilt(sos, np.asarray(x, np.float64), axis=1)
    return np.clip(v, lo, hi), (v >= lo) & (v <= hi), v


def truth_adjoint(sos, g, mask):
    gm = np.where(mask, np.asarray(g, np.float64), 0.0)
    return signal.sosfilt(sos, gm[:, ::-1], axis=1)[:, ::-1]


def main():
    assert not torch.cuda.is_available()
    install_accommodations()
    sys.path.insert(0, REF)
    import defense.frequency_domain as FD  # the reference module, unmodified
    torch.set_num_threads(1)
    rs = np.random.RandomState(20261017)
    out, cases, filters = {}, [], {}
    out["x_short"] = (rs.randint(-8192, 8193, (3, T_SHORT)) / 32768.0).astype(np.float32)
    out["x_long"] = (rs.randint(-8192, 8193, (1, T_LONG)) / 32768.0).astype(np.float32)
    out["cot_short"] = (np.round(rs.randn(3, T_SHORT) * 256) / 256).astype(np.float32)
    out["cot_long"] = (np.round(rs.randn(1, T_LONG) * 256) / 256).astype(np.float32)
    t = np.arange(T_SHORT)
    out["x_clamp"] = (np.round(0.98 * 32768 * np.sign(np.sin(2 * np.pi * t / 97.3 + 0.4))) / 32768.0).astype(np.float32)[None]
    out["x_int16"] = rs.randint(-8192, 8193, (1, T_SHORT)).astype(np.float32)

    FILTERS = [("lpf8000", "LPF", 4000, 8000), ("lpf7000", "LPF", 4000, 7000), ("lpf5000", "LPF", 4000, 5000),
               ("bpf_a", "BPF", [300, 4000], [10, 7000]), ("bpf_b", "BPF", [1000, 4000], [100, 7000]),
               ("bpf_c", "BPF", [500, 3000], [50, 6000]), ("bpf_default", "BPF", [300, 4000], [50, 5000])]
    for name, kind, wp, ws in FILTERS:
        N, Wn, b, a, sos = design(kind, wp, ws)
        a32 = a.astype(np.float32).astype(np.float64)
        filters[name] = dict(kind=kind, wp=wp, param=ws, order=N, Wn=Wn.tolist(), n_sections=int(len(sos)),
                             direct_form_order=int(len(a) - 1), max_abs_a=float(np.abs(a).max()),
                             pole_radius_f64=float(np.abs(np.roots(a)).max()), pole_radius_f32=float(np.abs(np.roots(a32)).max()))
        out[name + "_sos"] = sos
        print(name, "order", N, "sections", len(sos), "pole radius %.4f -> %.4f after the float32 cast" %
              (filters[name]["pole_radius_f64"], filters[name]["pole_radius_f32"]))

    def add(tag, filt, B, T, xk, ck):
        f = filters[filt]
        x, cot = out[xk][:B, :T], out[ck][:B, :T]
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        y = getattr(FD, f["kind"])(xt, wp=f["wp"], param=f["param"])
        finite = bool(torch.isfinite(y).all())
        lo, hi = (-1.0, 1.0) if 0.9 * x.max() <= 1 and 0.9 * x.min() >= -1 else (-32768.0, 32767.0)
        c = dict(tag=tag, filter=filt, B=B, T=T, x=xk, cot=ck, clip=[lo, hi], ref_finite=finite, has_truth=T <= T_SHORT)
        t_out, t_mask, t_v = truth(out[filt + "_sos"], x, lo, hi)
        if finite:
            y.backward(torch.from_numpy(cot.copy()))
            out[tag + "_out"], out[tag + "_grad"] = y.detach().numpy(), xt.grad.numpy()
            c["ref_vs_truth"] = float(np.abs(out[tag + "_out"] - t_out).max() / np.abs(t_out).max())
        else:
            bad = ~np.isfinite(y.detach().numpy())
            c["ref_nonfinite"], c["ref_first_nonfinite"] = int(bad.sum()), int(np.argmax(bad.reshape(-1)))
        if c["has_truth"]:
            out[tag + "_truth"], out[tag + "_truth_adj"] = t_out, truth_adjoint(out[filt + "_sos"], cot, t_mask)
        c["clamped"] = int((~t_mask).sum())
        c["near_clip"] = int((np.minimum(np.abs(t_v - lo), np.abs(t_v - hi)) <= 1e-5 * max(abs(lo), abs(hi))).sum())
        cases.append(c)
        return c

    for T in (1, 2, C - 1, C, C + 1, W - 1, W, W + 1, P - 1, P, P + 1, 2 * P + 3):
        B = 3 if T in (1, 2, W + 1) else 1
        add("lpf5000_B%d_T%d" % (B, T), "lpf5000", B, T, *(("x_short", "cot_short") if T <= T_SHORT else ("x_long", "cot_long")))
    for name, *_ in FILTERS[:-1]:
        if name == "lpf5000":  # (the sweep above)
            continue
        c = add("%s_B1_T%d" % (name, T_SHORT), name, 1, T_SHORT, "x_short", "cot_short")
        assert c["clamped"] == 0 and c["ref_finite"], c
    # (the float64 arithmetic of the accommodation overflows later than float32 would: a few thousand samples, not hundreds)
    c = add("bpf_default_B1_T%d" % (P - 1), "bpf_default", 1, P - 1, "x_long", "cot_long")
    assert c["clamped"] == 0 and not c["ref_finite"], c
    c = add("clamp_lpf5000", "lpf5000", 1, T_SHORT, "x_clamp", "cot_short")
    assert c["clamped"] > 10 and c["near_clip"] <= 0.01 * T_SHORT, c
    c = add("int16_lpf7000", "lpf7000", 1, T_SHORT, "x_int16", "cot_short")
    assert c["clip"] == [-32768.0, 32767.0] and c["clamped"] == 0

    sigs = {}
    for name in ("LPF", "BPF"):
        ps = list(inspect.signature(getattr(FD, name)).parameters.values())
        sigs[name] = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in ps]
    import scipy
    meta = {
        "generator": "tests/golden/make_golden_frequency_domain.py",
        "reference": "SpeakerGuard defense/frequency_domain.py LPF / BPF, unmodified, CPU",
        "accommodation": "sys.modules['torchaudio'] = empty module; sys.modules['torch_lfilter'].lfilter = autograd function "
                         "running scipy.signal.lfilter in float64 on the float32 (b, a) it is handed, backward = flipped filter",
        "truth": "scipy.signal.sosfilt(sos, float64 x) clamped to `clip`; adjoint = flip(sosfilt(sos, flip(cot * mask))); "
                 "stored for has_truth cases, recomputed by the tests for the others",
        "chunk": C, "wave": W, "pass": P, "filters": filters, "cases": cases, "signatures": sigs,
        "torch": torch.__version__, "numpy": np.__version__, "scipy": scipy.__version__,
    }
    path = os.path.join(HERE, "freq_domain_ref.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), len(cases), "cases")
    for c in cases:
        print(c["tag"], {k: c[k] for k in ("ref_finite", "clamped", "near_clip") if k in c}, "ref vs truth %.3g" % c.get("ref_vs_truth", np.nan))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
