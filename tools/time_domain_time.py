"""Time the native time-domain defenses (csrc/k_time_domain.hip) against the parent commit's only way to do the same thing:
the torch restatement of the reference function wrapped in ``adaptive_attack.BPDA.BPDA``, same box, same run.

At 64 x 48000 samples, for QT, BDR, AS, MS and AT at their default parameters: microseconds per forward and per backward of
the defense alone, with the effective bandwidth of the native direction (the bytes the algorithm has to move over the
time, against the 6.3 TB/s a float4 copy reaches on this part), and milliseconds per PGD step of
``defended_model(xv_plda, [(0, d)])``.  HIP events, warm-up first (clock ramp, code objects), medians; native and torch
measurements alternate.  A table on stdout, and in --out if given.

    python tools/time_domain_time.py [--calls 50] [--attacks 5] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.adaptive_attack.BPDA import BPDA  # noqa: E402
from speakerguard_amd.attack.PGD import PGD  # noqa: E402
from speakerguard_amd.defense import AS, AT, BDR, MS, QT  # noqa: E402
from speakerguard_amd.model.defended_model import defended_model  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402

HBM_COPY_TBS = 6.3  # achievable HBM bandwidth of the MI355X (float4 copy), the yardstick of the bandwidth column


# ---- the reference's functions restated with torch (defense/time_domain.py), as a user of the parent commit would
def qt_torch(audio, param=128):
    scale = bool(0.9 * audio.max() <= 1 and 0.9 * audio.min() >= -1)  # (a host synchronisation, like the reference's `if`)
    a = audio * 32768.0 if scale else audio
    a = torch.round(a / param) * param
    return a / 32768.0 if scale else a


def bdr_torch(audio, param=8, bits=16):
    return qt_torch(audio, 2 ** (bits - param))


def at_torch(audio, param=25):
    a = audio.squeeze(1)
    power = torch.sum((a / math.sqrt(a.shape[1])) ** 2, dim=1, keepdim=True)
    return (a + torch.randn(a.shape, device=a.device) * torch.sqrt(power / 10 ** (param / 10))).view(audio.shape)


def as_torch(audio, param=3):
    w = torch.full((1, 1, param), 1.0 / param, device=audio.device)
    return torch.nn.functional.conv1d(audio, w, padding=(param - 1) // 2)


def ms_torch(audio, param=3):
    pad = (param - 1) // 2
    roll = torch.nn.functional.pad(audio.squeeze(1), (pad, pad), mode="constant", value=0.).unfold(-1, param, 1)
    return torch.median(roll, -1)[0].view(audio.shape)


def timed(fns, n, warm):
    """medians (ms) of several callables, measured in alternation"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--attacks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, K = 64, 48000, 10
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(dev)
    g = torch.randn_like(x)
    xv = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=10), device=dev, dither=0.0)
    y = xv.make_decision(x)[0]
    n = B * T
    # name, native defense, torch forward, torch substitute for the backward (None: BPDA's identity),
    # bytes the native forward / backward must move (reads + writes; AT reads x twice, the backward g twice)
    rows = [("QT", QT(), qt_torch, None, 8 * n, 0),
            ("BDR", BDR(), bdr_torch, None, 8 * n, 0),
            ("AS", AS(), as_torch, as_torch, 8 * n, 8 * n),
            ("MS", MS(), ms_torch, ms_torch, 9 * n, 9 * n),
            ("AT", AT(), at_torch, None, 12 * n, 16 * n)]
    lines = ["%d x %d samples; us per call (median of %d), effective bandwidth of the native kernels against %.1f TB/s; "
             "ms per PGD step of defended_model(xv_plda, [(0, d)]) (PGD-%d, median of %d attacks)" % (B, T, a.calls, HBM_COPY_TBS, K, a.attacks),
             "%-4s %12s %12s %9s %12s %12s %9s %14s %14s" % ("", "fwd native", "fwd torch", "fwd TB/s", "bwd native", "bwd torch",
                                                            "bwd TB/s", "step native ms", "step torch ms")]
    print("\n".join(lines), flush=True)
    for name, d, f_torch, sub, bytes_f, bytes_b in rows:
        wrapped = BPDA(f_torch, sub)
        if name == "AT":  # not BPDA-wrapped in the reference: autograd through the function itself (fresh noise per call)
            wrapped = BPDA(f_torch, f_torch)
        fn, ft = timed([lambda: d.fwd(x), lambda: wrapped.fwd(x)], a.calls, 10)
        sv_n, sv_t = d.fwd(x)[1], wrapped.fwd(x)[1]
        bn, bt = timed([lambda: d.bwd(sv_n, g), lambda: wrapped.bwd(sv_t, g)], a.calls, 10)
        kw = dict(task="CSI", epsilon=0.002, step_size=0.0004, max_iter=K, batch_size=B, verbose=0)
        an, at_ = PGD(defended_model(xv, [(0, d)]), **kw), PGD(defended_model(xv, [(0, wrapped)]), **kw)
        sn, st = timed([lambda: an.attack(x, y), lambda: at_.attack(x, y)], a.attacks, 1)
        tbs = lambda nbytes, ms: ("%9.2f" % (nbytes / (ms * 1e-3) / 1e12)) if nbytes else "%9s" % "-"  # noqa: E731
        lines.append("%-4s %12.1f %12.1f %s %12.1f %12.1f %s %14.3f %14.3f" % (
            name, fn * 1e3, ft * 1e3, tbs(bytes_f, fn), bn * 1e3, bt * 1e3, tbs(bytes_b, bn), sn / K, st / K))
        print(lines[-1], flush=True)
    lines.append("(QT / BDR backward: the identity on both sides, nothing is launched.  AT's torch backward differentiates a "
                 "fresh noise draw: BPDA re-runs its substitute.  A PGD step includes the model's forward and backward.)")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
