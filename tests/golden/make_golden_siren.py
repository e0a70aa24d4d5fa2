"""tests/golden/siren_ref.npz: the reference's own ``SirenAttack`` (attack/SirenAttack.py, unmodified) run on the CPU against
tests/toy_model.py's ``ToyModel`` (T = 40: the swarm's draws are the bulk of the fixture -- two (n, P, 1, T) float64 arrays
per iteration -- and T = 40 is the shortest utterance the toy model takes).  Every ``numpy.random.uniform`` /
``numpy.random.rand`` call the attack makes is logged (the functions are wrapped, their results pass through untouched)
and saved in call order, so that a restatement fed the same draws can be compared bit for bit.

Cases: CSI and OSI (threshold 1.5), untargeted and targeted, batch_size 1 and 4, n_particles 5, plus one case with
n_particles 1; max_epoch 3, abort_early_iter 2, abort_early_epoch 2.  max_iter is 6 where the fixture's size allows it and
is cut (CASES below) where it does not: the file must stay below the largest fixture of this directory.  Seeds and
epsilons are chosen so that both abort branches fire, ``delete_found`` removes some but not all utterances of a chunk, and
both outcomes occur; ``meta`` records, per case, how often each of these happened.

Run from the repository root with the reference on the path given as the first argument."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
from toy_model import ToyModel, toy_inputs  # noqa: E402

T, N_SPK, THRESHOLD = 40, 4, 1.5
COMMON = dict(max_epoch=3, abort_early_iter=2, abort_early_epoch=2, verbose=0)
# name: (task, targeted, batch_size, n_particles, epsilon, max_iter, numpy seed[, abort_early_epoch])
# With max_epoch 3 and abort_early_epoch 2 the outer test is made once, at epoch 1, against the initial +inf: it cannot
# fire.  The targeted OSI cases therefore make it at every epoch (abort_early_epoch 1).
CASES = {
    "csi_u_b4": ("CSI", False, 4, 5, 0.02, 4, 5),
    "csi_u_b1": ("CSI", False, 1, 5, 0.02, 3, 5),
    "csi_t_b4": ("CSI", True, 4, 5, 0.1, 4, 5),
    "csi_t_b1": ("CSI", True, 1, 5, 0.1, 4, 5),
    "osi_u_b4": ("OSI", False, 4, 5, 0.02, 4, 5),
    "osi_u_b1": ("OSI", False, 1, 5, 0.02, 3, 5),
    "osi_t_b4": ("OSI", True, 4, 5, 0.1, 6, 5, 1),
    "osi_t_b1": ("OSI", True, 1, 5, 0.1, 4, 5, 1),
    "csi_u_b4_p1": ("CSI", False, 4, 1, 0.02, 6, 6),
}


def run_case(SirenAttack, x, case):
    task, targeted, bs, P, eps, max_iter, seed = case[:7]
    kw = dict(COMMON, abort_early_epoch=case[7]) if len(case) > 7 else COMMON
    model = ToyModel(T=T, n_spk=N_SPK, threshold=THRESHOLD if task == "OSI" else None).eval()
    with torch.no_grad():
        own = model.make_decision(x)[0]
    own = torch.where(own < 0, torch.zeros_like(own), own)
    y = (own + 1) % N_SPK if targeted else own.clone()
    atk = SirenAttack(model, threshold=THRESHOLD if task == "OSI" else None, task=task, targeted=targeted, epsilon=eps,
                      max_iter=max_iter, n_particles=P, batch_size=bs, **kw)
    draws, partial, offset = [], [0], [0]
    gbest = np.full(x.shape[0], np.inf, np.float32)
    uniform, rand, delete_found, attack_batch = np.random.uniform, np.random.rand, atk.delete_found, atk.attack_batch

    def rec_uniform(low=0.0, high=1.0, size=None):
        d = uniform(low=low, high=high, size=size)
        draws.append(d)
        return d

    def rec_rand(*shape):
        d = rand(*shape)
        draws.append(d)
        return d

    def watch_delete(gbests, *a):  # called once per evaluation with the active utterances' global bests (:151-155)
        found = int((gbests < 0).sum())
        partial[0] += int(0 < found < len(gbests))
        gbest[[offset[0] + i for i in a[-1]]] = gbests.numpy()
        return delete_found(gbests, *a)

    def watch_batch(x_batch, y_batch, lower, upper, batch_id):
        offset[0] = batch_id * min(bs, x.shape[0])
        return attack_batch(x_batch, y_batch, lower, upper, batch_id)

    np.random.seed(seed)
    torch.manual_seed(seed)
    np.random.uniform, np.random.rand, atk.delete_found, atk.attack_batch = rec_uniform, rec_rand, watch_delete, watch_batch
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):  # the reference announces its abort branches whatever ``verbose`` says
            adv, success = atk.attack(x.clone(), y)
    finally:
        np.random.uniform, np.random.rand = uniform, rand
    assert [bool(g < 0) for g in gbest] == [bool(s) for s in success]
    stats = {"abort_inner": buf.getvalue().count("Break Inner Loop"), "abort_outer": buf.getvalue().count("Break Outer Loop"),
             "partial_delete": partial[0], "success": [bool(s) for s in success]}
    return y, draws, adv, success, gbest, stats


def main(reference):
    sys.path.insert(0, reference)
    np.infty = np.inf
    from attack.SirenAttack import SirenAttack

    x = toy_inputs(B=4, T=T)
    out, stats = {"x": x.numpy()}, {}
    for name, case in CASES.items():
        y, draws, adv, success, gbest, st = run_case(SirenAttack, x, case)
        out[name + "_y"] = y.numpy()
        out[name + "_adv"] = adv.numpy()
        out[name + "_succ"] = np.array(success, np.bool_)
        out[name + "_gbest"] = gbest
        # the draws in call order, flattened; their shapes beside them
        out[name + "_draws"] = np.concatenate([d.reshape(-1) for d in draws]) if draws else np.zeros(0)
        out[name + "_draw_shapes"] = np.array([d.shape for d in draws], np.int64).reshape(-1, 4)
        stats[name] = st
        print(name, st, len(draws))
    flags = [s for st in stats.values() for s in st["success"]]
    assert True in flags and False in flags, "the fixture must hold both outcomes"
    assert any(st["abort_inner"] for st in stats.values()) and any(st["abort_outer"] for st in stats.values())
    assert any(st["partial_delete"] for st in stats.values())
    assert any(True in stats[n]["success"] for n in stats if "_t_" in n), "no targeted case succeeds"
    path = os.path.join(HERE, "siren_ref.npz")
    np.savez_compressed(path, meta=json.dumps({
        "generator": "tests/golden/make_golden_siren.py", "reference": "attack/SirenAttack.py (unmodified)",
        "toy": "tests/toy_model.py ToyModel(T=40, n_spk=4, seed=7), toy_inputs(B=4, T=40)",
        "accommodations": ["numpy.infty alias"], "torch": torch.__version__, "numpy": np.__version__,
        "common": COMMON, "threshold": THRESHOLD, "cases": {k: list(v) for k, v in CASES.items()}, "stats": stats}), **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
