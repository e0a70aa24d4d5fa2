"""Time the native down-/up-sampling defense ``DS`` (csrc/k_resample.hip) beside the Butterworth ``LPF`` on the same box, same run.

At 64 x 48000 samples: microseconds per launch of ``DS.fwd`` / ``DS.bwd`` between HIP events through the library's stage trace
(tags ds_fwd / ds_bwd: the kernels alone), the traffic they have to move (read B*T floats, write B*T floats per direction) over
that time, and the fraction of the rate a float4 copy reaches on this part; the same for LPF's cascade kernel (fd_fwd / fd_bwd);
a device-to-device copy of the same bytes as the yardstick measured in the run itself.  Medians after a warm-up.

    python tools/ds_time.py [--calls 50] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import _native as N  # noqa: E402
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.defense import DS, LPF  # noqa: E402
from speakerguard_amd.metric.metric import _context  # noqa: E402

HBM_COPY_TBS = 6.3  # achievable HBM bandwidth of the MI355X (float4 copy), as in tools/time_domain_time.py


def traced(ctx, fn, calls, warm=10):
    """{stage name: median ms} of the launches fn() makes, over `calls` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    cap = 8 * calls
    ctx.call("sg_trace_begin", cap)
    try:
        for _ in range(calls):
            fn()
    finally:
        tags, ms, n = (C.c_int32 * cap)(), (C.c_float * cap)(), C.c_int32()
        ctx.call("sg_trace_end", tags, ms, cap, C.byref(n))
    by = {}
    for i in range(min(n.value, cap)):
        by.setdefault(N.STAGE_NAMES.get(tags[i], str(tags[i])), []).append(float(ms[i]))
    return {k: statistics.median(v) for k, v in by.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T = 64, 48000
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(dev) * 0.5
    g = torch.randn_like(x)
    ctx = _context(dev)
    nbytes = 8 * B * T
    lines = ["%d x %d samples, %.1f MB per direction; us per launch (median of %d, HIP events of the stage trace); "
             "TB/s = those bytes over the time; fraction of the %.1f TB/s a float4 copy reaches" % (B, T, nbytes / 1e6, a.calls, HBM_COPY_TBS)]
    dst = torch.empty_like(x)
    ts = []
    for i in range(a.calls + 10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(x)
        e1.record()
        e1.synchronize()
        if i >= 10:
            ts.append(e0.elapsed_time(e1))
    cp = statistics.median(ts)
    lines.append("%-22s %8.1f us  %5.2f TB/s" % ("torch copy (same bytes)", cp * 1e3, nbytes / (cp * 1e-3) / 1e12))
    for name, d, tf, tb in (("DS()", DS(), "ds_fwd", "ds_bwd"), ("DS(0.33)", DS(0.33), "ds_fwd", "ds_bwd"),
                            ("LPF() 1 section", LPF(), "fd_fwd", "fd_bwd"), ("LPF(5000) 6 sections", LPF(5000), "fd_fwd", "fd_bwd")):
        sv = d.fwd(x)[1]
        f = traced(ctx, lambda: d.fwd(x), a.calls)[tf]
        b = traced(ctx, lambda: d.bwd(sv, g), a.calls)[tb]
        lines.append("%-22s fwd %8.1f us %5.2f TB/s (%4.1f %%)   bwd %8.1f us %5.2f TB/s (%4.1f %%)" % (
            name, f * 1e3, nbytes / (f * 1e-3) / 1e12, 100 * nbytes / (f * 1e-3) / 1e12 / HBM_COPY_TBS,
            b * 1e3, nbytes / (b * 1e-3) / 1e12, 100 * nbytes / (b * 1e-3) / 1e12 / HBM_COPY_TBS))
    lines.append("(LPF moves an int8 mask per sample besides: 27.6 MB per direction; its fractions above count the 24.6 MB of the floats.)")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
