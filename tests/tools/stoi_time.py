"""Time the native STOI (csrc/k_stoi.hip, C-ABI sg_wav_stoi) at 64 x 48000 and 8 x 48000 samples, fs = 16000.

Per launch: microseconds between the HIP events of the library's stage trace (tags stoi_scale .. stoi_segments: the kernels
alone), median over the calls of a traced run.  Total: HIP events around the whole call on the stream, in a run of its own without
the trace (event records between launches cost a few microseconds), median after a warm-up.  Beside them the wall time of the numpy
restatement (tests/stoi_restate.py) of the same rows on this host with 16 threads -- pystoi is not available, its time cannot be
measured; the restatement is a per-row Python loop over numpy calls, not a tuned program.

    python tests/tools/stoi_time.py [--calls 200] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

for _v in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
    os.environ.setdefault(_v, "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import stoi_restate as R  # noqa: E402
from speakerguard_amd import _native as N  # noqa: E402
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.metric import metric  # noqa: E402

STAGES = ("stoi_scale", "stoi_resample", "stoi_mask", "stoi_bands", "stoi_segments")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    ctx, stream = metric._context(dev), N.current_stream_ptr(dev)
    T, fs = 48000, 16000
    lines = ["sg_wav_stoi, T = %d at fs = %d (30000 samples, 233 frames at 10 kHz); us, medians of %d calls after 20 warm-up calls;"
             % (T, fs, a.calls),
             "stages: HIP events of the stage trace around each launch; total: HIP events around the whole call, trace off;",
             "numpy restatement: wall time of tests/stoi_restate.py over the same rows, once, %s threads" % os.environ["OMP_NUM_THREADS"]]
    for B in (64, 8):
        x = synth.make_waveforms(B, T, seed=3).reshape(B, T).astype(np.float32)
        y = (x + np.random.RandomState(4).uniform(-0.002, 0.002, x.shape)).astype(np.float32)
        b, adv = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        out = torch.empty(B, device=dev, dtype=torch.float64)
        frames = torch.empty(B, device=dev, dtype=torch.int32)

        def call():
            ctx.call("sg_wav_stoi", N._ptr(b), N._ptr(adv), B, T, fs, N._ptr(out), N._ptr(frames), stream)

        for _ in range(20):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize()
        total = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3
        cap = 8 * a.calls
        ctx.call("sg_trace_begin", cap)
        try:
            for _ in range(a.calls):
                call()
        finally:
            tags, ms, n = (C.c_int32 * cap)(), (C.c_float * cap)(), C.c_int32()
            ctx.call("sg_trace_end", tags, ms, cap, C.byref(n))
        by = {}
        for i in range(min(n.value, cap)):
            by.setdefault(N.STAGE_NAMES.get(tags[i], str(tags[i])), []).append(float(ms[i]) * 1e3)
        stage = {k: statistics.median(v) for k, v in by.items()}
        t0 = time.perf_counter()
        want = np.array([R.stoi(x[r], y[r], fs) for r in range(B)])
        cpu = time.perf_counter() - t0
        gap = float(np.abs(out.cpu().numpy() - want).max())
        lines.append("B = %2d: total %8.1f us | %s | sum of stages %8.1f us | numpy restatement %8.3f s (%.0f x) | max |gpu - restated| %.1e"
                     % (B, total, "  ".join("%s %7.1f" % (s[5:], stage.get(s, float("nan"))) for s in STAGES),
                        sum(stage.get(s, 0.0) for s in STAGES), cpu, cpu / (total * 1e-6), gap))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
