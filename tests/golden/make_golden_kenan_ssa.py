"""tests/golden/kenan_ssa_ref*.npz: the reference's own ``ssa`` route -- attack/_kenan.py ``ssa_compression`` / ``atk_bst``,
attack/ssa_core.py ``ssa`` / ``inv_ssa`` and attack/Kenan.py, all unmodified -- run on the CPU.

Part (i), reconstruction.  T = 40, 60, 100, 480, 4000, 16000 (W = 2, 3, 5, 24, 200, 800), the first two utterances of
tests/golden/make_golden_kenan.py's ``make_inputs(T)``, quantised as attack/Kenan.py:31-34 does it, and the factors 50, 25, 75,
12.5, 87.5, 97 and 1.  T = 20 (W = 1) has no reference: ``ssa`` cuts its trajectory matrix with ``yy[:-dim + 1]``, which is
empty at dim = 1, and ``inv_ssa`` fails on it; the tests hold that length to tests/ssa_restate.py alone (``inputs(20)``: that
generator cannot draw its tone frequencies below T = 24 either, so it is the first 20 samples of ``make_inputs(24)``).  Per case ``T<T>_u<u>_f<j>``:
  * ``ref64_T<T>`` (2, 7, T): the float64 output of ``inv_ssa``.  The reference's int16 output is NOT stored beside it: it is
    ``np.asarray(ref64, dtype=np.int16)`` by the reference's own line (_kenan.py:112), which this generator asserts against what
    ``ssa_compression`` returned, and which ``ref16`` below repeats on load;
  * ``ecase_T<T>`` (2, 7): E_case = max |tests/ssa_restate.py (eigh route) - reference| in float64 -- the gap between two LAPACK
    routes to the same projector: the conditioning of the case, not the code under test;
  * ``rank_T<T>`` (7,), ``xq_T<T>`` (2, T) int16 the quantised input.
A committed file holds at most 1 MiB, and float64 noise does not compress: T = 4000 and each utterance of T = 16000 have a file
of their own (``kenan_ssa_ref_T4000.npz``, ``kenan_ssa_ref_T16000_u0.npz``, ``..._u1.npz``; ``load`` below puts them together).

Part (ii), the attack.  ``Kenan(model, atk_name='ssa', max_iter=15)`` on make_golden_kenan.py's ``ToyModel`` (weights in the
fixture: the first seed whose runs hold both outcomes in both modes), T = 480 and 4000, six utterances, untargeted (against the
model's own decision on the int16-scale audio) and targeted (at the class ``shift`` further on).  ``ssa_compression`` and
``make_decision`` are wrapped to record every query's factor, rank and decision, and the final decision.  Per run
``T<T>_t<0|1>``: ``_adv`` (6, T) int16, ``_succ``, ``_y``, ``_count`` queries per utterance, ``_factors`` / ``_ranks`` /
``_decisions`` those queries end to end, ``_final``.

Run from the repository root with the reference on the path given as the first argument."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
T_CASES = (40, 60, 100, 480, 4000, 16000)
FACTORS = (50, 25, 75, 12.5, 87.5, 97, 1)
OWN_FILE = {4000: ("kenan_ssa_ref_T4000.npz",), 16000: ("kenan_ssa_ref_T16000_u0.npz", "kenan_ssa_ref_T16000_u1.npz")}


def kenan_generator():
    spec = importlib.util.spec_from_file_location("make_golden_kenan", os.path.join(HERE, "make_golden_kenan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(T, n=2):
    """(n, 1, T) float32 in [-1, 1]"""
    gen = kenan_generator()
    return gen.make_inputs(T)[:n] if T >= 24 else np.ascontiguousarray(gen.make_inputs(24)[:n, :, :T])


def ref16(ref64):
    """the reference's cast (_kenan.py:112)"""
    return np.asarray(ref64, dtype=np.int16)


def load(golden_dir=HERE):
    """every file of the fixture as one dict (``ref64_T4000`` and ``ref64_T16000`` put back together)"""
    def npz(name):
        d = np.load(os.path.join(golden_dir, name), allow_pickle=False)
        return {k: d[k] for k in d.files}
    out = npz("kenan_ssa_ref.npz")
    out["meta"] = json.loads(str(out["meta"]))
    out["ref64_T4000"] = npz(OWN_FILE[4000][0])["ref64"]
    out["ref64_T16000"] = np.stack([npz(f)["ref64"] for f in OWN_FILE[16000]])
    return out


def main(reference):
    import ssa_restate as sr
    sys.path.insert(0, reference)
    np.infty = np.inf
    from attack import _kenan
    from attack.Kenan import Kenan
    from attack.ssa_core import inv_ssa
    gen = kenan_generator()
    out, own = {}, {}

    # ---- part (i)
    for T in T_CASES:
        W = sr.window(T)
        x = inputs(T)
        xq = np.stack([sr.quantise(row) for row in x[:, 0]])
        # attack/Kenan.py:31-34 on the utterance alone
        for u in range(2):
            xb = x[u:u + 1]
            assert 0.9 * xb.max() <= 1 and 0.9 * xb.min() >= -1
            assert np.array_equal((xb * (2 ** 15)).astype(np.int16).flatten(), xq[u])
        ref64 = np.zeros((2, len(FACTORS), T))
        ecase = np.zeros((2, len(FACTORS)))
        ranks = np.zeros(len(FACTORS), np.int32)
        for u in range(2):
            pc = v = None
            evec = sr.eigh_rows(sr.covariance(xq[u]))[1]
            for j, f in enumerate(FACTORS):
                got16, pc, v = _kenan.ssa_compression(xq[u], f, 16000, pc=pc, v=v)
                k = int(W * f / 100)
                k = 1 if k == 0 else k
                ranks[j] = k
                ref64[u, j] = inv_ssa(pc, v, np.arange(0, k, 1))
                assert np.array_equal(ref16(ref64[u, j]), got16)
                mine = sr.reconstruct64(xq[u], sr.projector(evec, k))
                ecase[u, j] = np.abs(mine - ref64[u, j]).max()
                assert np.array_equal(sr.low16(mine), got16), (T, u, j)
            print("T", T, "W", W, "u", u, "E_case", ecase[u])
        out["xq_T%d" % T], out["ecase_T%d" % T], out["rank_T%d" % T] = xq, ecase, ranks
        if T == 4000:
            own[OWN_FILE[T][0]] = ref64
        elif T == 16000:
            own[OWN_FILE[T][0]], own[OWN_FILE[T][1]] = ref64[0], ref64[1]
        else:
            out["ref64_T%d" % T] = ref64

    # ---- part (ii)
    def runs(Wt, shift):
        res = {}
        for T in (480, 4000):
            Wn = sr.window(T)
            x = torch.from_numpy(gen.make_inputs(T))
            model = gen.ToyModel(Wt)
            q16 = torch.from_numpy(np.stack([sr.quantise(r) for r in x.numpy()[:, 0]]).astype(np.float32)).unsqueeze(1)
            own_dec = model.make_decision(q16)[0]
            for targeted in (False, True):
                y = (own_dec + shift) % gen.N_CLASS if targeted else own_dec.clone()
                factors, ranks, decisions = [], [], []
                comp, decide = _kenan.ssa_compression, model.make_decision

                def rec_comp(audio_image, factor, fs, percent=True, pc=None, v=None, comp=comp):
                    k = int(Wn * factor / 100)
                    factors.append(float(factor)), ranks.append(1 if k == 0 else k)
                    return comp(audio_image, factor, fs, percent=percent, pc=pc, v=v)

                def rec_decide(a, decide=decide):
                    d, s = decide(a)
                    decisions.append(int(d.item()))
                    return d, s

                _kenan.ssa_compression, model.make_decision = rec_comp, rec_decide
                try:
                    advs, succ, count, final, qd = [], [], [], [], []
                    for i in range(x.shape[0]):  # (the reference takes one utterance at a time anyway)
                        nf, nd = len(factors), len(decisions)
                        adv, s = Kenan(model, atk_name='ssa', max_iter=15, targeted=targeted, verbose=0).attack(x[i:i + 1].clone(), y[i:i + 1])
                        assert adv.dtype == np.int16 and len(decisions) - nd == len(factors) - nf + 1
                        advs.append(adv.reshape(-1)), succ.append(bool(s[0])), count.append(len(factors) - nf)
                        qd += decisions[nd:-1]
                        final.append(decisions[-1])
                finally:
                    _kenan.ssa_compression = comp
                    del model.make_decision
                key = "T%d_t%d" % (T, int(targeted))
                res.update({key + "_adv": np.stack(advs), key + "_succ": np.array(succ, np.bool_), key + "_y": y.numpy(),
                            key + "_count": np.array(count, np.int32), key + "_factors": np.array(factors, np.float64),
                            key + "_ranks": np.array(ranks, np.int32), key + "_decisions": np.array(qd, np.int64),
                            key + "_final": np.array(final, np.int64)})
        return res

    def both(res, t):
        f = np.concatenate([res["T%d_t%d_succ" % (T, t)] for T in (480, 4000)])
        return f.any() and not f.all()

    for seed in range(200):
        Wt = np.random.RandomState(seed).randn(2 * gen.N_SEG, gen.N_CLASS).astype(np.float32)
        hit = None
        for shift in (1, 2, 3):
            res = runs(Wt, shift)
            if both(res, 0) and both(res, 1):
                hit = shift
                break
            if not both(res, 0):
                break  # (the untargeted runs do not depend on the shift)
        if hit:
            break
    assert hit, "no toy weights with both outcomes in both modes"
    print("toy weights: seed", seed, "shift", hit, {k: v.tolist() for k, v in res.items() if k.endswith("_succ") or k.endswith("_count")})
    out.update(res)
    out["W_toy"] = Wt

    meta = json.dumps({"generator": "tests/golden/make_golden_kenan_ssa.py",
                       "reference": "attack/Kenan.py, attack/_kenan.py, attack/ssa_core.py (unmodified)",
                       "accommodations": ["numpy.infty alias"], "factors": list(FACTORS), "toy_seed": seed, "toy_shift": hit,
                       "torch": torch.__version__, "numpy": np.__version__})
    np.savez_compressed(os.path.join(HERE, "kenan_ssa_ref.npz"), meta=meta, **out)
    for name, arr in own.items():
        np.savez_compressed(os.path.join(HERE, name), ref64=arr)
    for name in ["kenan_ssa_ref.npz"] + list(own):
        size = os.path.getsize(os.path.join(HERE, name))
        print(name, size)
        assert size < (1 << 20), name


if __name__ == "__main__":
    main(sys.argv[1])
