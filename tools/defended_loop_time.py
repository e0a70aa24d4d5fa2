"""Time PGD against xv_plda or audionet_csine behind native input-level defenses on its two routes: the device-resident loop
(``pgd_run_defended``, C-ABI ``sg_xv_pgd_run_defended`` / ``sg_an_pgd_run_defended``) and the step loop over
``defended_model.loss_grad`` / ``pgd_update`` that the same attack took before (``PGD.fuse_input_defenses = False``: the
yardstick, unchanged code).

PGD-20 on 64 x 48000 samples, dither 0.  One case each for QT, BDR, AS(3), MS(3), LPF(5000) and BPF(); AT(25) and
[AS(3), AT(25)] with EOT 4 / 4; with --model audionet also AS(3) and QT in front of FeCoDefense(0.5), evenly and randomly
started (EOT 2), on ``pgd_run_defended_feco``.  The two routes alternate in one process; wall time of ``attack()`` between HIP events
(host work included: it is what differs), one warm-up attack per route, then the median of --attacks timed attacks.  With
--trace the device route's stage trace of one further attack is summed per stage.  A table on stdout, and in --out if given.

    python tools/defended_loop_time.py [--model xv|audionet] [--attacks 5] [--trace] [--out FILE]
    (recorded: profiles/defended_loop_bench.txt for xv, profiles/an_defended_loop_bench.txt for audionet)
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
from speakerguard_amd.defense import AS, AT, BDR, BPF, LPF, MS, QT  # noqa: E402
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
    ap.add_argument("--model", choices=("xv", "audionet"), default="xv")
    ap.add_argument("--attacks", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, K = 64, 48000, 20
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=3)).to(dev)
    if a.model == "audionet":
        from speakerguard_amd.defense.feature_level import FeCoDefense
        from speakerguard_amd.model.audionet_csine import audionet_csine
        xv = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=dev)
    else:
        xv = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=10), device=dev, dither=0.0)
    y = xv.make_decision(x)[0]
    cases = [("QT", [QT()], 1), ("BDR", [BDR()], 1), ("AS(3)", [AS(3)], 1), ("MS(3)", [MS(3)], 1), ("LPF(5000)", [LPF(5000)], 1),
             ("BPF()", [BPF()], 1), ("AT(25) EOT4", [AT(25)], 4), ("AS(3),AT(25) EOT4", [AS(3), AT(25)], 4)]
    cases = [(name, [(0, d) for d in chain], eot) for name, chain, eot in cases]
    if a.model == "audionet":
        cases += [("AS(3)+FeCo", [(0, AS(3)), (1, FeCoDefense(0.5))], 1), ("QT+FeCo", [(0, QT()), (1, FeCoDefense(0.5))], 1),
                  ("AS(3)+FeCo rnd EOT2", [(0, AS(3)), (1, FeCoDefense(0.5, init='random', seed=0))], 2)]
    lines = ["%s: PGD-%d, %d x %d samples, dither 0; ms per attack step, median of %d attacks after one warm-up, routes alternating"
             % (type(xv).__name__, K, B, T, a.attacks),
             "%-20s %12s %12s %8s   %s" % ("chain", "device loop", "step loop", "ratio", "all timed attacks, ms per step (device | step)")]
    print("\n".join(lines), flush=True)
    for name, defense, eot in cases:
        kw = dict(task="CSI", epsilon=0.002, step_size=0.0004, max_iter=K, batch_size=B, EOT_size=eot, EOT_batch_size=eot, verbose=0)
        dm = defended_model(xv, defense)
        fused, host = PGD(dm, **kw), PGD(dm, **kw)
        host.fuse_input_defenses = False
        fused.fuse_randomised_input_defenses = True  # the AT cases: the device loop on request (its noise keys differ)
        (mf, mh), (tf, th) = timed([lambda: fused.attack(x, y), lambda: host.attack(x, y)], a.attacks)
        lines.append("%-20s %12.3f %12.3f %8.3f   %s | %s" % (name, mf / K, mh / K, mf / mh, " ".join("%.3f" % (t / K) for t in tf),
                                                             " ".join("%.3f" % (t / K) for t in th)))
        print(lines[-1], flush=True)
        if a.trace:
            rec = xv.trace_stages(lambda: fused.attack(x, y), max_records=1 << 15)
            tot = collections.OrderedDict()
            for stage, ms in rec:
                n, t = tot.get(stage, (0, 0.0))
                tot[stage] = (n + 1, t + ms)
            lines.append("    stage trace, us per step (launches per attack): " +
                         ", ".join("%s %.1f (%d)" % (s, 1e3 * t / K, n) for s, (n, t) in tot.items()))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
