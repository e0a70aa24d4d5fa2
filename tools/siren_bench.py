"""Time one SirenAttack iteration on the device-resident swarm (csrc/k_pso.hip) beside the reference's host path, same box,
same run.  Workload: n_particles = 50, T = 48000 (3 s), xv_plda, batch sizes 1 and 8.

Per batch size, medians after a warm-up, every piece between HIP events with a synchronise:
  * the iteration and its split: model call (forward-only loss of n * P queries), ``pso_select`` (launch + the host read of its
    report), ``pso_move`` (draws generated in the kernel);
  * ``pso_move``'s achieved bytes/s against the HBM peak (8.0 TB/s spec, 6.29 TB/s measured float4 copy).  The bytes are
    counted from the shapes, each array read or written once per element (``move_bytes``);
  * the reference's path for the same step, restated (attack/SirenAttack.py:167-174, :99): two numpy float64 draws of
    (n, P, 1, T) on the host, the cast to float32 and the copy to the device, then the update as torch elementwise operators
    on the device -- and the ratio to ``pso_move``, as measured.

With SG_TUNE=1 the two widths of the streaming kernels (SG_PSO_VEC=1 / 4) are timed side by side, and ``--width-batches``
adds batch sizes at which only that is done.

    python tools/siren_bench.py [--iters 20] [--width-batches 16,32,64] [--out profiles/siren_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speakerguard_amd import synth  # noqa: E402
from speakerguard_amd.adaptive_attack.EOT import EOT  # noqa: E402
from speakerguard_amd.attack.SirenAttack import SwarmState  # noqa: E402
from speakerguard_amd.attack.utils import resolve_loss  # noqa: E402
from speakerguard_amd.model.xv_plda import xv_plda  # noqa: E402

P, T = 50, 48000
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def move_bytes(n, P, T):
    """bytes one ``pso_move`` of n continuing rows touches: per (row, particle, sample) loc and vel are read and written and the
    query is written; pbest_loc is read where the particle did not improve and written where it did (one access either way);
    per (row, sample) x, lower, upper and gbest_loc are read; one byte per (row, particle) of improved flags"""
    per_particle = n * P * T * 4 * (2 + 2 + 1 + 1)
    per_row = n * T * 4 * 4
    return per_particle + per_row + n * P


def events(fn, iters, warm=3):
    """median milliseconds of fn() between HIP events, synchronised after every call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def wall(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--width-batches", default="", help="with SG_TUNE=1: batch sizes at which only pso_move / pso_init are timed, "
                    "at both kernel widths (SG_PSO_VEC=1 / 4), e.g. 16,32,64")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = xv_plda.from_weights(synth.make_xv_weights(), device=dev, dither=0.0)
    loss_spec, _ = resolve_loss('Margin', False, 0., 'CSI', None, False)
    eot = EOT(model, loss_spec, 1, 1, False)
    lines = ["SirenAttack, one iteration: n_particles %d, T %d, xv_plda; ms, median of %d after a warm-up (HIP events, synchronised)"
             % (P, T, a.iters)]
    for n in (1, 8):
        x = torch.from_numpy(synth.make_waveforms(n, T, seed=3)).to(dev)
        y = model.make_decision(x)[0]
        eps = 0.002
        lower, upper = torch.clamp(-1 - x, min=-eps), torch.clamp(1 - x, max=eps)
        rows = list(range(n))
        st = SwarmState(n, P, T, dev)
        q = [model.pso_init(st, x, lower, upper, rows, 0, None, 1)]
        eval_y = y.repeat_interleave(P)
        state = {}

        def call_model():
            state["loss"] = eot(q[0], eval_y)[1].view(n, P).contiguous()

        def select():
            state["report"] = model.pso_select(st, state["loss"], rows)

        def move():
            q[0] = model.pso_move(st, x, lower, upper, rows, state["report"][2], [1] * n, 1, 0.5, 1.4961, 1.4961, 2)

        def iteration():
            call_model()
            select()
            move()

        t_init = events(lambda: model.pso_init(st, x, lower, upper, rows, 0, None, 1), a.iters)
        call_model()
        select()
        t_iter = events(iteration, a.iters)
        t_model = events(call_model, a.iters)
        t_select = events(select, a.iters)
        t_move = events(move, a.iters)
        widths = {}
        if os.environ.get("SG_TUNE") == "1":  # the two kernel widths side by side (SG_PSO_VEC is read per call)
            for v in ("1", "4"):
                os.environ["SG_PSO_VEC"] = v
                widths[v] = (events(move, a.iters), events(lambda: model.pso_init(st, x, lower, upper, rows, 0, None, 1), a.iters))
            del os.environ["SG_PSO_VEC"]
        nbytes = move_bytes(n, P, T)
        rate = nbytes / (t_move * 1e-3)

        # ---- the reference's path for the same step, restated
        loc, vel, pb = st.loc.view(n, P, 1, T).clone(), st.vel.view(n, P, 1, T).clone(), st.pbest_loc.view(n, P, 1, T).clone()
        g = st.gbest_loc.view(n, 1, T).clone()
        draws = {}

        def host_draws():  # :167-168
            draws["r1"] = np.random.rand(n, P, 1, T) + 0.00001
            draws["r2"] = np.random.rand(n, P, 1, T) + 0.00001

        def cast_copy():  # :169-170
            draws["t1"] = torch.tensor(draws["r1"], device=dev, dtype=torch.float)
            draws["t2"] = torch.tensor(draws["r2"], device=dev, dtype=torch.float)

        def torch_update():  # :171-174, :99
            v = 0.5 * vel + 1.4961 * draws["t1"] * (pb - loc) + 1.4961 * draws["t2"] * (g.unsqueeze(1) - loc)
            l = loc + v
            l = torch.min(torch.max(l, lower.unsqueeze(1)), upper.unsqueeze(1))
            state["eval_x"] = (l + x.unsqueeze(1)).view(-1, 1, T)

        ref_iters = max(3, a.iters // 4)
        t_draw = wall(host_draws, ref_iters)
        t_copy = wall(cast_copy, ref_iters)
        t_torch = events(torch_update, a.iters)
        t_ref = t_draw + t_copy + t_torch
        lines += [
            "",
            "batch %d (%d queries of %d samples per model call)" % (n, n * P, T),
            "  pso_init (once per epoch)              %9.3f" % t_init,
            "  iteration: model + select + move       %9.3f" % t_iter,
            "    model call (forward-only loss)       %9.3f" % t_model,
            "    pso_select + the host read           %9.3f" % t_select,
            "    pso_move (draws in the kernel)       %9.3f   %.1f MB touched, %.2f TB/s = %.0f %% of the 8.0 TB/s spec, %.0f %% of the "
            "6.29 TB/s float4 copy" % (t_move, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY),
        ] + ["    SG_PSO_VEC=%s: pso_move %.3f, pso_init %.3f" % (v, m, i) for v, (m, i) in widths.items()] + [
            "  the reference's path for the move      %9.3f   = numpy draws %.3f + cast and copy %.3f + torch elementwise %.3f"
            % (t_ref, t_draw, t_copy, t_torch),
            "  reference's path / pso_move            %9.1f x   (draws and copy alone / model call: %.1f x)"
            % (t_ref / t_move, (t_draw + t_copy) / t_model),
        ]
        torch.cuda.empty_cache()
    for n in [int(v) for v in a.width_batches.split(",") if v] if os.environ.get("SG_TUNE") == "1" else []:
        x = torch.from_numpy(synth.make_waveforms(n, T, seed=3)).to(dev)
        lower, upper = torch.clamp(-1 - x, min=-0.002), torch.clamp(1 - x, max=0.002)
        rows, st = list(range(n)), SwarmState(n, P, T, dev)
        model.pso_init(st, x, lower, upper, rows, 0, None, 1)
        st.improved = torch.zeros(n * P, dtype=torch.uint8, device=dev)
        lines.append("")
        for v in ("1", "4"):
            os.environ["SG_PSO_VEC"] = v
            m = events(lambda: model.pso_move(st, x, lower, upper, rows, [-1] * n, [1] * n, 1, 0.5, 1.4961, 1.4961, 2), a.iters)
            i = events(lambda: model.pso_init(st, x, lower, upper, rows, 0, None, 1), a.iters)
            lines.append("batch %d, SG_PSO_VEC=%s: pso_move %.3f (%.2f TB/s), pso_init %.3f" % (n, v, m, move_bytes(n, P, T) / m / 1e9, i))
        del os.environ["SG_PSO_VEC"]
        del st
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
