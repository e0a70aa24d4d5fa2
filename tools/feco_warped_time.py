"""Time FeCo with warped k-means (csrc/k_feco_warped.hip) on the device: one defense call at 64 x 300 x 30 (x-vector MFCC,
k = 150) and at 64 x 300 x 32 (AudioNet log-mel, k = 150), TS and random init, and one PGD-10 attack on 64 utterances x 3 s
against each model defended by WarpedFeCoDefense(0.5, 'ts') at feature level 1 (the host-chained path).  HIP events,
warm-up first, medians; one JSON line per measurement on stdout (and in --out if given).

    python tools/feco_warped_time.py [--calls 30] [--attacks 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.attack.PGD import PGD  # noqa: E402
from speakerguard_amd.defense.feature_level import WarpedFeCoDefense  # noqa: E402
from speakerguard_amd.model.audionet_csine import audionet_csine  # noqa: E402
from speakerguard_amd.model.defended_model import defended_model  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--attacks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B = 64
    x = torch.from_numpy(synth.make_waveforms(B, 48000, seed=3)).to(dev)
    xv = xv_plda.from_weights(synth.make_xv_weights(seed=0, D=200, n_spk=10), device=dev, dither=0.0)
    an = audionet_csine.from_weights(synth.make_audionet_state_dict(seed=0, num_class=251), device=dev)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    for name, model in (("xv_plda MFCC", xv), ("AudioNet log-mel", an)):
        feat = model.compute_feat(x, flag=1).contiguous()
        Bf, F, D = feat.shape
        for init in ("ts", "random"):
            d = WarpedFeCoDefense(0.5, init)
            med, lo, hi = timed(lambda: d.fwd(feat), a.calls, 5)
            sw = d.last_sweeps.cpu()
            emit({"what": "WarpedFeCoDefense.fwd", "features": name, "B": Bf, "F": F, "D": D, "k": int(F * 0.5), "init": init,
                  "median_us": round(med * 1e3, 1), "min_us": round(lo * 1e3, 1), "max_us": round(hi * 1e3, 1),
                  "sweeps_max": int(sw.max()), "sweeps_mean": round(float(sw.float().mean()), 2), "calls": a.calls})
        dm = defended_model(model, defense=[(1, WarpedFeCoDefense(0.5, 'ts'))])
        y = dm.make_decision(x)[0]
        atk = PGD(dm, task="CSI", epsilon=0.002, step_size=0.0004, max_iter=10, batch_size=B, verbose=0)
        assert atk._device_route(B) is None
        med, lo, hi = timed(lambda: atk.attack(x, y), a.attacks, 1)
        emit({"what": "PGD-10 attack, warped FeCo (ts, 0.5) at level 1", "model": name.split()[0], "B": B, "seconds": 3,
              "median_ms_per_attack": round(med, 2), "median_ms_per_step": round(med / 10, 2), "min_ms": round(lo, 2),
              "max_ms": round(hi, 2), "attacks": a.attacks})
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
