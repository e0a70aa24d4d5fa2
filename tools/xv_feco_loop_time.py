"""Time PGD against xv_plda behind FeCoDefense(0.5) on its two routes: the device-resident loop (``pgd_run_feco``, C-ABI
``sg_xv_pgd_run_feco``) and the step loop over ``defended_model.loss_grad`` / ``pgd_update`` that the same attack takes with
``PGD.fuse_defended = False`` (the yardstick: the only route before the loop existed, unchanged code).

PGD-20 on 64 x 48000 samples, FeCo at level 1 and at level 2, two configurations each:
  (i)  dither 0, deterministic FeCo (one pass per step; the two routes give the same bits);
  (ii) the default dither 1.0, EOT 4 / EOT batch 4, ``init='random'`` (every repeat a row of its own; the loop on request,
       ``fuse_randomised_feco``: its noise keys differ from the step loop's).
The two routes alternate in one process; wall time of ``attack()`` between HIP events (host work included: it is what differs),
one warm-up attack per route, then the median of --attacks timed attacks.  With --trace the device route's stage trace of one
further attack is summed per stage.  A table on stdout, and in --out if given.

    python tools/xv_feco_loop_time.py [--attacks 5] [--trace] [--out FILE]
    (recorded: profiles/xv_feco_loop_bench.txt)
"""
import argparse
import collections
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.attack.PGD import PGD  # noqa: E402
from speakerguard_amd.defense.feature_level import FeCoDefense  # noqa: E402
from speakerguard_amd.model.defended_model import defended_model  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402


def timed(fns, n, warm=1):
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
    return [statistics.median(t) for t in ts], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attacks", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, K = 64, 48000, 20
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(dev)
    w = synth.make_xv_weights(seed=0, D=200, n_spk=10)
    models = {0.0: xv_plda.from_weights(w, device=dev, dither=0.0), 1.0: xv_plda.from_weights(w, device=dev, dither=1.0, dither_seed=1)}
    y = models[0.0].make_decision(x)[0]
    cases = [("(i)  L%d even, dither 0" % lv, lv, 0.0, "even", 1) for lv in (1, 2)] + \
            [("(ii) L%d random, dither 1, EOT4" % lv, lv, 1.0, "random", 4) for lv in (1, 2)]
    lines = ["xv_plda behind FeCoDefense(0.5): PGD-%d, %d x %d samples; ms per attack step, median of %d attacks after one warm-up, "
             "routes alternating" % (K, B, T, a.attacks),
             "step loop = this commit's, PGD.fuse_defended = False: the code path the parent commit took for these models (its kernels "
             "and launches are unchanged; the front-end helpers were only split), measured in the same process on the same box",
             "%-32s %12s %12s %8s   %s" % ("case", "device loop", "step loop", "ratio", "all timed attacks, ms per step (device | step)")]
    print("\n".join(lines), flush=True)
    for name, level, dither, init, eot in cases:
        kw = dict(task="CSI", epsilon=0.002, step_size=0.0004, max_iter=K, batch_size=B, EOT_size=eot, EOT_batch_size=eot, verbose=0)
        dm = defended_model(models[dither], [(level, FeCoDefense(0.5, init=init, seed=0))])
        fused, host = PGD(dm, **kw), PGD(dm, **kw)
        host.fuse_defended = False
        if dither or init == "random":
            fused.fuse_randomised_feco = True  # case (ii): the device loop on request (its noise keys differ)
        assert fused._device_route(B) is not None and host._device_route(B) is None
        (mf, mh), (tf, th) = timed([lambda: fused.attack(x, y), lambda: host.attack(x, y)], a.attacks)
        lines.append("%-32s %12.3f %12.3f %8.3f   %s | %s" % (name, mf / K, mh / K, mf / mh, " ".join("%.3f" % (t / K) for t in tf),
                                                             " ".join("%.3f" % (t / K) for t in th)))
        print(lines[-1], flush=True)
        if a.trace:
            rec = models[dither].trace_stages(lambda: fused.attack(x, y), max_records=1 << 15)
            tot = collections.OrderedDict()
            for stage, ms in rec:
                n, t = tot.get(stage, (0, 0.0))
                tot[stage] = (n + 1, t + ms)
            lines.append("    stage trace, us per step (launches per attack): " +
                         ", ".join("%s %.1f (%d)" % (s, 1e3 * t / K, n) for s, (n, t) in tot.items()))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
