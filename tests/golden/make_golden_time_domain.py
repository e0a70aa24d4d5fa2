"""Generate tests/golden/time_domain_ref.npz (build container only): the REFERENCE's own time-domain defenses, forward and
autograd gradient, on the CPU.

    python tests/golden/make_golden_time_domain.py      # needs the reference checkout (REF below)

What is pinned: ``defense/time_domain.py`` ``QT`` / ``QT_Non_Diff`` (:10-44), ``BDR`` (:46-48), ``AT`` (:50-70), ``AS`` (:72-97)
and ``MS`` (:100-127), executed unmodified.  Per case: the parameters (in ``meta``), the input (a slice of a shared array or
an array of its own), the output, and for AS / MS / AT torch autograd's gradient for a recorded cotangent.
  * AT draws ``torch.randn((B, N))`` from the global generator: the generator is seeded, the draw is made once here to record
    it, then the generator is seeded again and the reference is called -- it makes the same draw.
  * MS: the positions ``torch.median`` selected are recorded too, by repeating the reference's pad + unfold (:118-126) here
    and keeping the indices it discards.
  * the call signatures of the five functions are recorded (the Python classes must keep names and defaults).
Inputs sit on the int16 grid (m / 32768, what decoded audio looks like) with all samples of a row distinct and non-zero, so
that no median window holds a tie; the tie case and the full-precision float case are built separately.  Cotangents sit on
a 2^-8 grid.  (Both also keep the compressed file small.)
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SG_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

TS = (1, 2, 255, 256, 257, 4099)


def distinct_rows(rs, B, T):
    """(B,T) float32 in [-1,1) on the int16 grid, every row's samples distinct and non-zero"""
    rows = []
    for _ in range(B):
        m = rs.choice(65535, T, replace=False).astype(np.int64) - 32768  # -32768 .. 32766
        m[m >= 0] += 1                                                    # skip 0: -32768 .. -1, 1 .. 32767
        rows.append(m.astype(np.float32) / np.float32(32768.0))
    return np.stack(rows)


def main():
    assert not torch.cuda.is_available()
    sys.path.insert(0, REF)
    import defense.time_domain as TD  # the reference module, unmodified
    torch.set_num_threads(1)
    rs = np.random.RandomState(20261017)
    out, cases = {}, []
    X = {T: distinct_rows(rs, 3, T) for T in TS}
    COT = {T: (np.round(rs.randn(3, T) * 256) / 256).astype(np.float32) for T in TS}
    COT[4099] = COT[4099][:1]  # (the long cases that take a gradient have one row)
    for T in TS:
        out["x_T%d" % T], out["cot_T%d" % T] = X[T], COT[T]

    def add(tag, kind, B, T, param, x_key, **extra):
        cases.append(dict(tag=tag, kind=kind, B=B, T=T, param=param, x=x_key, **extra))

    def xin(x_key, B):
        return torch.from_numpy(out[x_key][:B].copy())

    # ---- QT / BDR (forward only: the backward is BPDA's identity)
    def qt(tag, x_key, B, T, q, bdr=False):
        x = xin(x_key, B)
        y = TD.BDR(x, param=q) if bdr else TD.QT(x, param=q)
        out[tag + "_out"] = y.numpy()
        add(tag, "BDR" if bdr else "QT", B, T, q, x_key)

    for B, T in ((3, 1), (1, 2), (3, 255), (1, 256), (3, 257), (3, 4099)):
        qt("qt_q128_B%d_T%d" % (B, T), "x_T%d" % T, B, T, 128)
    for q in (1, 3, 256):
        for B, T in ((1, 255), (3, 257)):
            qt("qt_q%d_B%d_T%d" % (q, B, T), "x_T%d" % T, B, T, q)
    qt("bdr_p8_B3_T256", "x_T256", 3, 256, 8, bdr=True)
    qt("bdr_p12_B1_T257", "x_T257", 1, 257, 12, bdr=True)
    out["x_float"] = rs.uniform(-1, 1, (3, 257)).astype(np.float32)        # full-precision floats in [-1, 1)
    out["x_int16"] = (rs.uniform(-0.9, 0.9, (3, 257)) * 32768).astype(np.float32)  # int16-SCALED input (not rounded)
    for q in (3, 128):
        qt("qt_q%d_float" % q, "x_float", 3, 257, q)
        qt("qt_q%d_int16scale" % q, "x_int16", 3, 257, q)
        m = np.arange(-128, 128)
        out["x_half_q%d" % q] = ((m + 0.5) * q / 32768.0).astype(np.float32)[None]   # exact half-way points
        assert np.array_equal(out["x_half_q%d" % q].astype(np.float64) * 32768.0 / q, (m + 0.5)[None])
        qt("qt_q%d_halfway" % q, "x_half_q%d" % q, 1, 256, q)

    # ---- AS / MS
    def smooth(kind, tag, x_key, cot_key, B, T, k, ties=False):
        x = xin(x_key, B).requires_grad_(True)
        cot = torch.from_numpy(out[cot_key][:B].copy())
        y = getattr(TD, kind)(x, param=k)
        (y * cot).sum().backward()
        out[tag + "_out"], out[tag + "_grad"] = y.detach().numpy(), x.grad.numpy()
        if kind == "MS":
            pad = (k - 1) // 2
            roll = torch.nn.functional.pad(x.detach(), (pad, pad), mode="constant", value=0.).unfold(-1, k, 1)
            vals, idx = torch.median(roll, -1)
            assert torch.equal(vals, y.detach())
            out[tag + "_idx"] = idx.numpy().astype(np.int8)  # window position 0 .. k-1
        add(tag, kind, B, T, k, x_key, cot=cot_key, ties=ties)

    shapes = {1: ((3, 1), (1, 2), (1, 256)),
              3: ((3, 1), (1, 2), (3, 255), (1, 256), (3, 257)),
              5: ((3, 1), (1, 2), (1, 255), (3, 257)),
              17: ((3, 1), (1, 2), (1, 255), (1, 257))}
    for kind in ("AS", "MS"):
        for k, sh in shapes.items():
            for B, T in sh:
                smooth(kind, "%s_k%d_B%d_T%d" % (kind.lower(), k, B, T), "x_T%d" % T, "cot_T%d" % T, B, T, k)
    smooth("AS", "as_k17_B1_T4099", "x_T4099", "cot_T4099", 1, 4099, 17)
    smooth("MS", "ms_k5_B1_T4099", "x_T4099", "cot_T4099", 1, 4099, 5)
    # MS with ties: runs of equal samples (clipped at +-1) and zeros touching the pad
    t = rs.uniform(-2.5, 2.5, (3, 257)).astype(np.float32)
    t = np.clip(np.round(t * 8) / 8, -1, 1).astype(np.float32)
    t[0, :4] = 0
    t[1, -5:] = 0
    t[2, :2] = 0
    t[2, -1:] = 0
    out["x_ties"] = t
    for k in (3, 5, 17):
        smooth("MS", "ms_k%d_ties" % k, "x_ties", "cot_T257", 3, 257, k, ties=True)

    # ---- AT
    def at(tag, x_key, cot_key, B, T, snr, seed):
        x = xin(x_key, B).requires_grad_(True)
        cot = torch.from_numpy(out[cot_key][:B].copy())
        torch.manual_seed(seed)
        noise = torch.randn((B, T))
        torch.manual_seed(seed)
        y = TD.AT(x, param=snr)
        (y * cot).sum().backward()
        sig = torch.sqrt(torch.sum((x.detach() / np.sqrt(T)) ** 2, dim=1, keepdims=True) / (10 ** (snr / 10)))
        assert torch.equal(y.detach(), x.detach() + noise * sig), tag  # the recorded draw IS the one the reference made
        out[tag + "_noise"], out[tag + "_out"], out[tag + "_grad"] = noise.numpy(), y.detach().numpy(), x.grad.numpy()
        add(tag, "AT", B, T, snr, x_key, cot=cot_key, seed=seed)

    for i, (B, T) in enumerate(((3, 1), (1, 2), (1, 255), (1, 256), (3, 257), (1, 4099))):
        at("at_snr25_B%d_T%d" % (B, T), "x_T%d" % T, "cot_T%d" % T, B, T, 25, 100 + i)
    at("at_snr10_B1_T257", "x_T257", "cot_T257", 1, 257, 10, 200)
    s = X[256].copy()
    s[1] = 0  # a silent utterance between two others
    out["x_silent"] = s
    at("at_snr25_silent", "x_silent", "cot_T256", 3, 256, 25, 300)
    assert not np.isfinite(out["at_snr25_silent_grad"][1]).any() and np.isfinite(out["at_snr25_silent_grad"][[0, 2]]).all()

    sigs = {}
    for name in ("QT_Non_Diff", "BDR", "AT", "AS", "MS"):
        ps = list(inspect.signature(getattr(TD, name)).parameters.values())
        sigs[name] = [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in ps]
    meta = {
        "generator": "tests/golden/make_golden_time_domain.py",
        "reference": "SpeakerGuard defense/time_domain.py QT / BDR / AT / AS / MS, unmodified, CPU float32",
        "accommodation": "AT: torch.manual_seed(seed), torch.randn((B, N)) recorded, torch.manual_seed(seed) again, then the "
                         "call; MS: torch.median's indices recorded by repeating the reference's pad + unfold",
        "cases": cases, "signatures": sigs, "torch": torch.__version__, "numpy": np.__version__,
    }
    path = os.path.join(HERE, "time_domain_ref.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), len(cases), "cases")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
