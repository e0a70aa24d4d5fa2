"""tests/golden/kenan_ref.npz: the reference's own Kenan attack, ``Kenan(model, atk_name='fft')`` (attack/Kenan.py and
attack/_kenan_fft.py, unmodified), run on the CPU against a small seeded toy model -- the model is defined HERE and imported
by tests/test_kenan_host.py, its weights travel in the fixture.  T in {480, 16000}, 6 utterances, batch sizes 1 and 4, 15
iterations, untargeted (against the model's own decisions) and targeted (at the class two further on: the one this toy model can be pushed
to, so that the targeted runs hold successes as well).  Besides the adversarial audio and the
success flags (the audio stored once per distinct result, see ``_adv_is``) the fixture holds every iteration's factors and decisions, captured by wrapping the reference's
``fft_compression`` and the model's ``make_decision`` (the loop itself records neither).

Run from the repository root with the reference on the path given as the first argument."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N_CLASS, N_SEG = 4, 16


class ToyModel(object):
    """scores = features @ W: per 1/16th of the utterance the log energy and the log energy of the first difference (what a
    spectrum gate changes).  CPU float32, deterministic; ``make_decision`` like the library's models."""

    def __init__(self, W):
        self.W = torch.as_tensor(W, dtype=torch.float32)

    def features(self, x):
        n, _, T = x.shape
        seg = x.reshape(n, N_SEG, T // N_SEG)
        e = (seg * seg).mean(2)
        d = seg[:, :, 1:] - seg[:, :, :-1]
        r = (d * d).mean(2)
        return torch.cat([torch.log(e + 1e-6), torch.log(r + 1e-6)], 1)

    def make_decision(self, x):
        x = x.detach().to("cpu", torch.float32)
        scores = self.features(x) @ self.W
        return scores.argmax(1), scores

    def eval(self):
        return self


def make_inputs(T, n=6, seed=0):
    rs = np.random.RandomState(seed + T)
    t = np.arange(T) / float(T)
    x = np.zeros((n, 1, T), np.float32)
    for i in range(n):
        tone = sum(rs.uniform(0.02, 0.3) * np.sin(2 * np.pi * rs.randint(2, T // 8) * t + rs.uniform(0, 6.28)) for _ in range(4))
        env = np.exp(-rs.uniform(0, 3) * t)
        x[i, 0] = (tone * env + rs.uniform(0.005, 0.08) * rs.randn(T)).astype(np.float32)
    # 16-bit audio, as a wav file holds it (and half the bytes in the fixture)
    return (np.round(np.clip(x, -0.95, 0.95) * 32768.0) / 32768.0).astype(np.float32)


def main(reference):
    sys.path.insert(0, reference)
    np.infty = np.inf
    from attack import _kenan_fft
    from attack.Kenan import Kenan

    W = np.random.RandomState(7).randn(2 * N_SEG, N_CLASS).astype(np.float32)
    out = {"W": W}
    outcomes = set()
    for T in (480, 16000):
        x = torch.from_numpy(make_inputs(T))
        out["x_%d" % T] = x.numpy()
        model = ToyModel(W)
        own = model.make_decision(x)[0]
        for targeted in (False, True):
            y = (own + 2) % N_CLASS if targeted else own.clone()
            for bs in (1, 4):
                factors, decisions = [], []
                gate = _kenan_fft.fft_compression
                decide = model.make_decision

                def rec_gate(audio, factor, fs, gate=gate):
                    factors.append(factor.clone().numpy())
                    return gate(audio, factor, fs)

                def rec_decide(a, decide=decide):
                    d, s = decide(a)
                    decisions.append(d.clone().numpy())
                    return d, s

                _kenan_fft.fft_compression, model.make_decision = rec_gate, rec_decide
                try:
                    adv, succ = Kenan(model, atk_name='fft', max_iter=15, targeted=targeted, verbose=0,
                                      batch_size=bs).attack(x.clone(), y)
                finally:
                    _kenan_fft.fft_compression = gate
                    del model.make_decision
                key = "T%d_t%d_b%d" % (T, int(targeted), bs)
                # (iterations, N): the chunks' histories side by side, in chunk order
                n_chunks = len(factors) // 15
                out[key + "_factors"] = np.concatenate([np.stack(factors[c * 15:(c + 1) * 15]) for c in range(n_chunks)], 1)
                out[key + "_decisions"] = np.concatenate([np.stack(decisions[c * 15:(c + 1) * 15]) for c in range(n_chunks)], 1)
                out[key + "_y"] = y.numpy()
                # the audio once per distinct result (float32 noise does not compress): "<key>_adv_is" names the array that holds it
                same = [k for k in sorted(out) if k.endswith("_adv") and k.startswith("T%d_" % T) and np.array_equal(out[k], adv.numpy())]
                if same:
                    out[key + "_adv_is"] = np.array(same[0])
                else:
                    out[key + "_adv"] = adv.numpy()
                out[key + "_succ"] = np.array(succ, np.bool_)
                outcomes.update(bool(s) for s in succ)
                print(key, succ)
    assert outcomes == {True, False}, "the fixture must hold both outcomes"
    np.savez_compressed(os.path.join(HERE, "kenan_ref.npz"), meta=json.dumps({
        "generator": "tests/golden/make_golden_kenan.py", "reference": "attack/Kenan.py, attack/_kenan_fft.py (unmodified)",
        "accommodations": ["numpy.infty alias"], "torch": torch.__version__}), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
