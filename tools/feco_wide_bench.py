"""Time the wide FeCo forward (sg_feco_kmeans_compress_wide, csrc/k_feco_wide.hip) and one PGD step on the level-3-defended
iv_plda; writes section 2 of profiles/feco_wide_bench.txt (section 1, the compiler's resource lines, is kept by hand).

  * per call: the wide entry at (64, 300, 72) and (8, 300, 72), k = 150, even and seeded, on iv_plda's own CMVN features of
    synthetic speech-like waveforms, next to the 64-wide kernel (sg_feco_kmeans_compress) at (64, 300, 64), k = 150, on the first
    64 of the same columns; the configurations alternate in one process, a window of --batch back-to-back calls is timed
    between HIP events, --warmup windows per configuration first, then the median of --windows windows (min .. max beside it);
  * the assignment steps a call takes (read off the ids: the smallest max_iter that already gives the final ids, + 1) and the
    matrix-pipe floor of the header, 12 us per assignment step at 300 x 150 x 72, times the steps of the slowest utterance;
  * one PGD step (loss_grad through the defenses + pgd_update) on defended_model(iv_plda, [(3, FeCoDefense(0.5))]) at 8 x 3 s
    next to the undefended step, the model of profiles/iv_grad_bench.txt (C 2048, R 400, D 200, S 10), alternating.

    python tools/feco_wide_bench.py [--windows 20] [--batch 1000] [--warmup 3] [--out FILE]
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

FLOOR_US_PER_STEP = 12.0  # 50 tile pairs x 36 MFMAs x 64 cycles over four SIMDs at 2.4 GHz (k_feco_wide.hip header)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="PGD steps per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense.feature_level import FeCoDefense
    from speakerguard_amd.metric.metric import _context
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.model.iv_plda import iv_plda
    dev = torch.device("cuda:0")
    m = iv_plda.from_weights(synth.make_iv_weights(seed=0, C=2048, R=400, D=200, n_spk=10), device=dev, dither=0.0, white_box=True)
    wav = torch.from_numpy(synth.make_waveforms(64, 48000 + 400, seed=3)).to(dev)
    cm = m.compute_feat(wav, flag=3)[:, :300].contiguous()
    assert tuple(cm.shape) == (64, 300, 72), cm.shape
    narrow = cm[:, :, :64].contiguous()
    ctx, stream = _context(dev), N.current_stream_ptr(dev)
    B, F, k = 64, 300, 150
    ids = torch.empty(B, F, device=dev, dtype=torch.int32)
    counts = torch.empty(B, k, device=dev, dtype=torch.int32)
    out = torch.empty(B, k, 72, device=dev)

    def wide(nb, seeded, max_iter=10):
        ctx.call("sg_feco_kmeans_compress_wide", N._ptr(cm), nb, F, 72, k, max_iter, seeded, C.c_uint64(77), 0, N._ptr(ids), N._ptr(out),
                 N._ptr(counts), stream)

    def old(nb, seeded):
        ctx.call("sg_feco_kmeans_compress", N._ptr(narrow), nb, F, 64, k, 10, seeded, C.c_uint64(77), 0, 1, N._ptr(ids), N._ptr(out),
                 N._ptr(counts), stream)

    def steps_of(nb, seeded):
        """assignment steps per utterance: the block stops at the first step that changes nothing"""
        wide(nb, seeded)
        final = ids[:nb].clone()
        steps = torch.full((nb,), 10, dtype=torch.int64)
        for mi in range(9, 0, -1):
            wide(nb, seeded, mi)
            same = (ids[:nb] == final).all(dim=1).cpu()
            steps[same] = mi + 1
        return steps.clamp(max=10)

    cases = [("wide  (64, 300, 72) even  ", lambda: wide(64, 0)), ("wide  (64, 300, 72) seeded", lambda: wide(64, 1)),
             ("wide  ( 8, 300, 72) even  ", lambda: wide(8, 0)), ("wide  ( 8, 300, 72) seeded", lambda: wide(8, 1)),
             ("64-wide kernel (64, 300, 64) even  ", lambda: old(64, 0)), ("64-wide kernel (64, 300, 64) seeded", lambda: old(64, 1))]

    def timed(fns, batch):
        for _ in range(a.warmup):
            for fn in fns:
                for _ in range(batch):
                    fn()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(batch):
                    fn()
                e1.record()
                e1.synchronize()
                ts[i].append(1e3 * e0.elapsed_time(e1) / batch)
        return ts

    lines = ["== 2. Time per call on an MI355X (tools/feco_wide_bench.py): us per call, windows of %d back-to-back calls between HIP "
             "events, median of %d windows after %d warm-up windows, configurations alternating in one process" % (a.batch, a.windows, a.warmup),
             "%-40s %10s %10s %10s" % ("configuration (k = 150)", "median", "min", "max")]
    med = {}
    for (name, _), t in zip(cases, timed([fn for _, fn in cases], a.batch)):
        med[name] = statistics.median(t)
        lines.append("%-40s %10.1f %10.1f %10.1f" % (name, med[name], min(t), max(t)))
    for nb, seeded, name in ((64, 0, cases[0][0]), (64, 1, cases[1][0]), (8, 0, cases[2][0]), (8, 1, cases[3][0])):
        st = steps_of(nb, seeded)
        lines.append("%s: assignment steps mean %.1f, max %d -> floor %.0f us (12 us x the slowest utterance's steps); measured / floor %.2f"
                     % (name, st.float().mean().item(), int(st.max()), FLOOR_US_PER_STEP * int(st.max()), med[name] / (FLOOR_US_PER_STEP * int(st.max()))))
    lines.append("wide / 64-wide at 64 utterances: even %.2f, seeded %.2f (1.125 x the multiply-adds; one CU per utterance in both)"
                 % (med[cases[0][0]] / med[cases[4][0]], med[cases[1][0]] / med[cases[5][0]]))

    # ---- one PGD step at 8 x 3 s
    x = wav[:8, :, :48000].contiguous()
    y = m.make_decision(x)[0]
    spec = SEC4SR_CrossEntropy()
    dm = defended_model(m, [(3, FeCoDefense(0.5))])
    lo, hi = torch.full_like(x, -1.0), torch.full_like(x, 1.0)

    def step(model):
        adv = x.clone()

        def run():
            g = model.loss_grad(adv, y, spec)[3]
            m.pgd_update(adv, g.contiguous(), lo, hi, 0.0004, 1)
        return run
    ts = timed([step(m), step(dm)], a.steps)
    lines.append("one PGD step (loss_grad + pgd_update) at 8 x 3 s, iv_plda C 2048 R 400 D 200 S 10, ms, median (min .. max) of %d windows of %d steps:"
                 % (a.windows, a.steps))
    for name, t in zip(("undefended (flag 0)", "[(3, FeCoDefense(0.5))]"), ts):
        lines.append("  %-28s %8.3f  (%.3f .. %.3f)" % (name, statistics.median(t) / 1e3, min(t) / 1e3, max(t) / 1e3))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
