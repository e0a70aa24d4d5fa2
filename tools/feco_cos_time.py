"""Time one call of the FeCo forward (clustering + cluster means, one launch) under both distances: the L2 entry
``sg_feco_kmeans_compress`` and ``sg_feco_kmeans_compress_metric`` with SG_FECO_L2 / SG_FECO_COS.

64 x 300 x 32 and 64 x 300 x 30 with k = 150 (3 s utterances at ratio 0.5: log-mel and MFCC widths), even and seeded start, on
oracle-style features (the device's own log-mel / MFCC of synthetic speech-like waveforms).  The configurations alternate in one
process; a window of --batch back-to-back calls is timed between HIP events on the stream the calls are issued on; --warmup
windows per configuration first, then the median of --windows timed windows, with the spread (min .. max) beside it, all in
us per call.  A table on stdout, and in --out if given.

--parent-lib PATH adds another build's library (the parent commit's: its L2 kernels are meant to be identical) to the same
alternation, TWICE, as "parent (a)" and "parent (b)": the difference between the two is the run-to-run spread of one and the
same code, the yardstick for any other difference in the table.  --trace makes three calls per configuration and nothing else:
run it with SG_TUNE=1 SG_FECO_TRACE=1 to get the kernel's phase split of block (0, 0) on stderr (each traced launch synchronises).

    python tools/feco_cos_time.py [--windows 40] [--batch 25] [--warmup 3] [--parent-lib PATH] [--out FILE]
    SG_TUNE=1 SG_FECO_TRACE=1 python tools/feco_cos_time.py --trace
    (recorded: profiles/feco_cos_bench.txt)
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

I32, VP = C.c_int32, C.c_void_p
OLD_ARGS = [VP, VP, I32, I32, I32, I32, I32, I32, C.c_uint64, C.c_int64, I32, VP, VP, VP, VP]
NEW_ARGS = [VP, VP, I32, I32, I32, I32, I32, I32, I32, C.c_uint64, C.c_int64, I32, I32, VP, VP, VP, VP]


def features(dev):
    """{32: log-mel (64, 300, 32), 30: MFCC (64, 300, 30)} from the package's own front-ends"""
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.xv_plda import xv_plda
    x = torch.from_numpy(synth.make_waveforms(64, 48000, seed=3)).to(dev)
    an = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=10), device=dev)
    xv = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=10), device=dev, dither=0.0)
    f32, f30 = an.compute_feat(x, flag=1)[:, :300].contiguous(), xv.compute_feat(x, flag=1)[:, :300].contiguous()
    assert tuple(f32.shape) == (64, 300, 32) and tuple(f30.shape) == (64, 300, 30), (f32.shape, f30.shape)
    return {32: f32, 30: f30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--batch", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.windows >= 20, "median of at least 20 windows"
    dev = torch.device("cuda:0")
    feats = features(dev)
    torch.cuda.synchronize()

    def opened(lib):  # (handles of this tool's own: the package's prototypes stay as they are)
        lib.sg_create.restype, lib.sg_create.argtypes = C.c_int, [I32, C.POINTER(VP)]
        lib.sg_destroy.argtypes = [VP]
        lib.sg_feco_kmeans_compress.restype, lib.sg_feco_kmeans_compress.argtypes = C.c_int, OLD_ARGS
        if hasattr(lib, "sg_feco_kmeans_compress_metric"):
            lib.sg_feco_kmeans_compress_metric.restype, lib.sg_feco_kmeans_compress_metric.argtypes = C.c_int, NEW_ARGS
        ctx = VP()
        assert lib.sg_create(0, C.byref(ctx)) == 0
        return lib, ctx

    lib, ctx = opened(C.CDLL(N.LIB_PATH))
    parent = opened(C.CDLL(os.path.abspath(a.parent_lib))) if a.parent_lib else None
    B, F, k = 64, 300, 150
    stream = torch.cuda.current_stream(dev).cuda_stream
    ids = torch.empty(B, F, device=dev, dtype=torch.int32)
    counts = torch.empty(B, k, device=dev, dtype=torch.int32)
    outs = {D: torch.empty(B, k, D, device=dev) for D in feats}

    def caller(entry, D, seeded):
        f, o = feats[D], outs[D]
        if entry.startswith("parent"):
            plib, pctx = parent
            return lambda: plib.sg_feco_kmeans_compress(pctx, f.data_ptr(), B, F, D, k, 10, seeded, 77, 0, 1, ids.data_ptr(), o.data_ptr(),
                                                        counts.data_ptr(), stream)
        if entry == "L2 entry":
            return lambda: lib.sg_feco_kmeans_compress(ctx, f.data_ptr(), B, F, D, k, 10, seeded, 77, 0, 1, ids.data_ptr(), o.data_ptr(),
                                                       counts.data_ptr(), stream)
        metric = N.SG_FECO_COS if entry == "metric cos" else N.SG_FECO_L2
        return lambda: lib.sg_feco_kmeans_compress_metric(ctx, f.data_ptr(), B, F, D, k, 10, metric, seeded, 77, 0, 1, 0, ids.data_ptr(),
                                                          o.data_ptr(), counts.data_ptr(), stream)

    entries = (["parent (a)"] if parent else []) + ["L2 entry", "metric L2", "metric cos"] + (["parent (b)"] if parent else [])
    cases = [(e, D, s) for D in (32, 30) for s in (0, 1) for e in entries]
    fns = [caller(*c) for c in cases]
    names = ["%-10s 64x300x%d k=150 %s" % (e, D, "seeded" if s else "even  ") for e, D, s in cases]
    if a.trace:
        for name, fn in zip(names, fns):
            for i in range(3):  # the first call arms the trace, the later ones print
                sys.stderr.write("%s call %d: " % (name, i) if i else "")
                sys.stderr.flush()
                assert fn() == 0
                torch.cuda.synchronize()
        return
    def window(fn):
        for _ in range(a.batch):
            assert fn() == 0

    for _ in range(a.warmup):
        for fn in fns:
            window(fn)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(a.windows):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(fn)
            e1.record()
            e1.synchronize()
            ts[i].append(1e3 * e0.elapsed_time(e1) / a.batch)
    lines = ["FeCo forward (one launch per call): us per call, windows of %d back-to-back calls between HIP events, median of %d windows "
             "after %d warm-up windows, configurations alternating%s" % (a.batch, a.windows, a.warmup, "; parent = the parent commit's "
             "library in the same process, listed twice" if parent else ""),
             "%-40s %10s %10s %10s" % ("configuration", "median", "min", "max")]
    for name, t in zip(names, ts):
        lines.append("%-40s %10.1f %10.1f %10.1f" % (name, statistics.median(t), min(t), max(t)))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
