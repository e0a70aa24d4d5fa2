"""Time the native spectrum gate (csrc/k_spectrum.hip) beside the decision it feeds, same box, same run.

Per shape (64 x 48000, 1 x 48000, 64 x 52960): microseconds per ``sg_wav_spectrum_gate`` call and per ``sg_wav_spectrum`` call
(peak only) between HIP events, and next to them the time of ``xv_plda.make_decision`` on the same batch.  Medians after a
warm-up.  The file also takes the compiler's resource lines of the two kernel instances when given (``--resources FILE``:
the -Rpass-analysis=kernel-resource-usage remarks of the build).

    python tools/kenan_bench.py [--calls 30] [--out profiles/kenan_bench.txt] [--resources FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.attack.Kenan import wav_spectrum, wav_spectrum_gate  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402

SHAPES = ((64, 48000), (1, 48000), (64, 52960))


def timed(fn, calls, warm=5):
    """median microseconds of fn() between HIP events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    model = xv_plda.from_weights(synth.make_xv_weights(), device=dev, dither=0.0)
    lines = ["the spectrum gate beside the decision it feeds: us per call, median of %d (HIP events around the host call, so the "
             "wrapper's allocations and the launch are inside)" % a.calls]
    slower = []
    for B, T in SHAPES:
        x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(dev)
        peak = wav_spectrum(x, want_spec=False)[1]
        f = peak / 8
        g = timed(lambda: wav_spectrum_gate(x, f), a.calls)
        p = timed(lambda: wav_spectrum(x, want_spec=False), a.calls)
        d = timed(lambda: model.make_decision(x), a.calls)
        lines.append("%3d x %5d   gate %9.1f us   peak only %9.1f us   xv_plda.make_decision %9.1f us   gate / decision %.2f" %
                     (B, T, g, p, d, g / d))
        if g > d:
            slower.append((B, T))
    lines.append("the gate costs MORE than the decision it feeds at: %s" % (slower if slower else "no shape measured"))
    if a.resources and os.path.exists(a.resources):
        lines.append("")
        lines.append("compiler resource usage of the two instances (sp_kernel<true>: both buffers in LDS; <false>: workspace):")
        keep = ("Function Name", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy", "Spill", "LDS Size", "TotalSGPRs")
        for ln in open(a.resources):
            if "remark:" in ln and any(k in ln for k in keep):
                lines.append("  " + ln.split("remark:", 1)[1].split("[-Rpass")[0].strip())
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
