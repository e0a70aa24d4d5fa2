"""Times the GMM / i-vector / PLDA forward (speakerguard_amd.model.iv_plda) at the recipe's size -- C 2048, R 400, D 200, S 10,
3 s utterances -- for B = 64 and B = 51 (one FAKEBOB draw of 50 queries + the clean sample for one utterance).

    python tools/iv_bench.py [--out profiles/iv_bench.txt] [--passes 5] [--small] [--grad]

Device-event times of ``make_decision`` (wav in, decisions out) after a warm-up, the stage entries on their own (delta + CMVN,
statistics, extraction), the load time (the host's float64 fold of V and U) and the device bytes of the packed model.
``--grad`` (out: profiles/iv_grad_bench.txt) times ``loss_grad(want_grad=True)`` of a ``white_box=True`` model next to
``make_decision`` in the same run, at flags 0 and 3, and the backward's stage entries (each re-runs its forward stage first).
Per-kernel times come from a ``rocprofv3 --kernel-trace --stats`` run of this script (``--passes 2``), a run of its own.
Model figures quoted beside the times:
  log-likelihood contraction   2 B F C 2700 flop, against the 157.3 TFLOP/s float32 MFMA peak
  assembly of L                the bytes of U (C x R (R + 1) / 2 float32, once per 16 utterances), against 8 TB/s HBM
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.model.iv_plda import iv_plda  # noqa: E402


def timed(fn, passes):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="C 256, R 100: a quick look, not the recipe")
    ap.add_argument("--grad", action="store_true", help="batch 64 only: loss_grad(want_grad=True) next to make_decision")
    a = ap.parse_args()
    C, R, D, S = (256, 100, 50, 10) if a.small else (2048, 400, 200, 10)
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t0 = time.time()
    w = synth.make_iv_weights(seed=0, C=C, R=R, D=D, n_spk=S)
    t1 = time.time()
    m = iv_plda.from_weights(w, device=dev, dither=1.0, white_box=a.grad)
    t2 = time.time()
    P = R * (R + 1) // 2
    Pp, Cp = (P + 255) // 256 * 256, (C + 63) // 64 * 64
    u_bytes, v_bytes, w_bytes = 4 * C * Pp, 4 * C * 72 * R, 4 * 2700 * Cp
    say("iv_plda forward: C %d, R %d, D %d, S %d, 3 s utterances (F 300); ms, median of %d after a warm-up (HIP events)" % (C, R, D, S, a.passes))
    say("synthetic model generated in %.1f s; sg_iv_load (host float64 fold of V and U + upload) %.1f s" % (t1 - t0, t2 - t1))
    say("device bytes of the packed model: U %.1f MB, V^T %.1f MB, W %.1f MB" % (u_bytes / 1e6, v_bytes / 1e6, w_bytes / 1e6))
    for B in ((64,) if a.grad else (64, 51)):
        x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=B)).to(dev)
        F = 300
        say()
        say("batch %d" % B)
        say("  make_decision (wav -> decisions)         %9.3f" % timed(lambda: m.make_decision(x), a.passes))
        raw = m.compute_feat(x, 1)
        say("  delta + CMVN (one launch)                %9.3f" % timed(lambda: m.comput_feat_from_feat(raw, 1, 3), a.passes))
        cm = m.comput_feat_from_feat(raw, 1, 3)
        t_st = timed(lambda: m.stats(cm), a.passes)
        flops = 2.0 * B * F * C * 2700
        say("  statistics (loglik + rowstat + stats)    %9.3f   loglik model: %.1f GFLOP = %.3f ms at the 157.3 TFLOP/s f32-MFMA peak"
            % (t_st, flops / 1e9, flops / 157.3e12 * 1e3))
        n, f = m.stats(cm)
        t_ex = timed(lambda: m.extract(n, f), a.passes)
        groups = (B + 15) // 16
        say("  extraction (assembly + Cholesky solve)   %9.3f   assembly model: U read %d x = %.1f MB = %.3f ms at 8 TB/s"
            % (t_ex, groups, groups * u_bytes / 1e6, groups * u_bytes / 8e12 * 1e3))
        say("  from CMVN features (flag 3)              %9.3f" % timed(lambda: m.make_decision(cm, flag=3), a.passes))
        if a.grad:
            from speakerguard_amd import _native as N
            from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
            spec, y = SEC4SR_CrossEntropy(), torch.zeros(B, dtype=torch.int64, device=dev)
            say("  loss_grad(want_grad=False) (wav)         %9.3f" % timed(lambda: m.loss_grad(x, y, spec, want_grad=False), a.passes))
            say("  loss_grad(want_grad=True)  (wav)         %9.3f   forward + backward, d loss / d wav out"
                % timed(lambda: m.loss_grad(x, y, spec, want_grad=True), a.passes))
            say("  loss_grad(want_grad=True)  (flag 3)      %9.3f" % timed(lambda: m.loss_grad(cm, y, spec, flag=3, want_grad=True), a.passes))
            dw = torch.randn(B, R, device=dev)
            dn, df, dx = torch.empty_like(n), torch.empty_like(f), torch.empty_like(cm)
            s = m._stream()
            say("  extraction + its backward (stage entry)  %9.3f" % timed(lambda: m.ctx.call(
                "sg_iv_extract_backward", N._ptr(n), N._ptr(f), N._ptr(dw), B, N._ptr(dn), N._ptr(df), s), a.passes))
            say("  statistics + their backward (stage entry)%9.3f   transposed contraction model: %.1f GFLOP = %.3f ms at the peak"
                % (timed(lambda: m.ctx.call("sg_iv_stats_backward", N._ptr(cm), B, F, N._ptr(dn), N._ptr(df), N._ptr(dx), s), a.passes),
                   flops / 1e9, flops / 157.3e12 * 1e3))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
