"""Times PGD-20 on 64 utterances of unequal lengths (speakerguard_amd.model.xv_plda with ``lengths=``) three ways, (a) - (c).

    python tools/ragged_bench.py [--out profiles/ragged_bench.txt] [--runs 7] [--steps 20]

64 utterances, lengths drawn once from a fixed seed, uniformly in 2-4 s; dither 0; epsilon 0.002, step 0.0004, Entropy loss.
  (a) one padded batch of 64 through the device loop (``PGD.attack(x, y, lengths=lengths)``: sg_xv_pgd_run_ragged)
  (b) the same 64 as 64 solo attacks, one utterance per call at its own length -- what a user without ``lengths=`` does
  (c) a uniform batch of 64 x T_max -- the cost ceiling of padding: the same launches as (a) with full front-end work
  (a') / (c'): the device loop call alone (``model.pgd_run`` with and without ``lengths=`` on prepared bounds) -- (a) and (c)
       without what ``attack`` does on the host around it (for (a): the length checks, zeroing the padding of start point and
       bounds, padding the result back), i.e. the comparison of the kernels themselves
Host wall time around each attack, which ends with the success flags on the host (a device synchronise); one warm-up run of
each (workspace, tables, code objects), then `--runs` timed runs in the order a, b, c, a', c', a, b, ...: the median, with the
minimum and maximum as the spread.  Also checked in the same run, because faster and different is not faster: every row of (a)
equals its solo attack of (b) bit for bit.
The ratio (a) / (c) is the one expectation that can be derived: not above 1 beyond the spread, or the length-aware kernels cost
occupancy.  Utterance-steps per second = 64 x steps / time.
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
from speakerguard_amd.attack.PGD import PGD  # noqa: E402
from speakerguard_amd.audio_io import pad_batch  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=64)
    a = ap.parse_args()
    assert a.runs >= 5, "the median of at least 5 runs"
    assert torch.cuda.is_available(), "this measures the GPU: no device, no number"
    dev = torch.device("cuda:0")
    B = a.utterances
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lengths = np.random.RandomState(2024).randint(32000, 64001, size=B)
    waves = [torch.from_numpy(synth.make_waveforms(1, int(t), seed=1000 + b))[0] for b, t in enumerate(lengths)]
    x, lens = pad_batch(waves)
    x = x.to(dev)
    T = x.shape[2]
    uniform = torch.from_numpy(synth.make_waveforms(B, T, seed=77)).to(dev)
    solos = [x[b:b + 1, :, :int(t)].contiguous() for b, t in enumerate(lengths)]
    model = xv_plda.from_weights(synth.make_xv_weights(), device=dev, dither=0.0)
    y = model.make_decision(x, lengths=lens)[0]
    yu = model.make_decision(uniform)[0]
    kw = dict(epsilon=0.002, step_size=0.0004, max_iter=a.steps, verbose=0)
    batch, one = PGD(model, batch_size=B, **kw), PGD(model, batch_size=1, **kw)

    def ragged():
        return batch.attack(x, y, lengths=lens)

    def solo():
        return [one.attack(solos[b], y[b:b + 1]) for b in range(B)]

    def padded():
        return batch.attack(uniform, yu)

    keep = (torch.arange(T).unsqueeze(0) < lens.to(torch.int64).unsqueeze(1)).unsqueeze(1).to(dev)
    zero = torch.zeros((), device=dev)
    lo_r, hi_r = torch.where(keep, torch.clamp(x - 0.002, min=-1), zero), torch.where(keep, torch.clamp(x + 0.002, max=1), zero)
    lo_u, hi_u = torch.clamp(uniform - 0.002, min=-1), torch.clamp(uniform + 0.002, max=1)

    def loop_ragged():
        return model.pgd_run(x, y, lo_r, hi_r, batch.loss, 0.0004, a.steps, batch.grad_sign, lengths=lens)[1].cpu()

    def loop_padded():
        return model.pgd_run(uniform, yu, lo_u, hi_u, batch.loss, 0.0004, a.steps, batch.grad_sign)[1].cpu()

    adv, succ = ragged()
    ref = solo()
    padded()
    loop_ragged()
    loop_padded()
    torch.cuda.synchronize()
    same = all(torch.equal(adv[b, :, :int(t)], ref[b][0][0]) and succ[b] == ref[b][1][0] for b, t in enumerate(lengths))
    times = {"a": [], "b": [], "c": [], "a'": [], "c'": []}
    for _ in range(a.runs):
        for key, fn in (("a", ragged), ("b", solo), ("c", padded), ("a'", loop_ragged), ("c'", loop_padded)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[key].append(time.perf_counter() - t0)
    frames = (lengths + 80) // 160
    say("PGD-%d on %d utterances of unequal lengths, dither 0 (%s)" % (a.steps, B, torch.cuda.get_device_name(0)))
    say("lengths: uniform in 2-4 s, seed 2024: min %d, mean %.0f, max %d samples (T_max); frames %d .. %d; padding %.1f %% of B x T_max"
        % (lengths.min(), lengths.mean(), T, frames.min(), frames.max(), 100.0 * (1.0 - lengths.sum() / float(B * T))))
    say("host wall time per attack (ends with the flags on the host), one warm-up each, then %d runs in the order a b c a' c': median [min .. max] ms" % a.runs)
    med = {}
    for key, what in (("a", "(a) one padded batch of %d, lengths=       " % B), ("b", "(b) %d solo attacks, own length each       " % B),
                      ("c", "(c) uniform batch of %d x T_max (no lengths)" % B), ("a'", "(a') the device loop of (a) alone            "),
                      ("c'", "(c') the device loop of (c) alone            ")):
        ms = 1e3 * np.asarray(times[key])
        med[key] = float(np.median(ms))
        say("  %s %9.1f [%9.1f .. %9.1f]   %8.0f utterance-steps/s" % (what, med[key], ms.min(), ms.max(), B * a.steps / (med[key] * 1e-3)))
    say("(a) / (b) = %.3f   (a) / (c) = %.3f   (a') / (c') = %.3f" % (med["a"] / med["b"], med["a"] / med["c"], med["a'"] / med["c'"]))
    say("every row of (a) equals its solo attack of (b) bit for bit, success flags included: %s" % ("yes" if same else "NO"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
