"""The native singular spectrum analysis (csrc/k_ssa.hip: sg_ssa_decompose / sg_ssa_reconstruct) and the Kenan SSA attack on it
(speakerguard_amd/attack/KenanSSA.py).

Quantised audio and lag covariance are integers: exact against tests/ssa_restate.py.  Eigenpairs are held to 64 W 2^-53 against
that exact matrix (orthogonality, residual / |C|_F) and against ``eigh`` (eigenvalues / l_max).  The float64 reconstruction is
held to the REFERENCE's own float64 (tests/golden/kenan_ssa_ref*.npz) within 8 E_case, E_case being the fixture's gap between
two LAPACK routes to the same projector; the int16 output is the reference's exactly, except where the reference's float64
value lies within 8 E_case of a nonzero integer (one step allowed there, at most 0.01 % of a case).  T = 20 (W = 1), where the
reference fails, is held to the restatement.  Measured ratios are logged."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ssa_restate as sr
from conftest import GOLDEN, log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T_ALL = (20, 40, 60, 100, 480, 4000, 16000)
BOUND = 64 * 2.0 ** -53


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN, _GOLD, _DEC = [], [], {}


def gen():
    if not _GEN:
        _GEN.append(_module("make_golden_kenan_ssa"))
    return _GEN[0]


def golden():
    if not _GOLD:
        _GOLD.append(gen().load(GOLDEN))
    return _GOLD[0]


def _case(T):
    """made once per T, shared, never changed: the two utterances, the restatement's integers, the native decomposition"""
    if T not in _DEC:
        from speakerguard_amd.attack.KenanSSA import ssa_decompose
        x = gen().inputs(T)
        xq = np.stack([sr.quantise(r) for r in x[:, 0]])
        C = np.stack([sr.covariance(q) for q in xq])
        st = ssa_decompose(torch.from_numpy(x).to(DEV), want_cov=True)
        torch.cuda.synchronize()
        _DEC[T] = dict(x=x, xq=xq, C=C, st=st)
    return _DEC[T]


@pytest.mark.parametrize("T", T_ALL)
def test_decompose(T):
    c = _case(T)
    st, W = c["st"], sr.window(T)
    assert st["W"] == W
    assert np.array_equal(st["xq"].cpu().numpy(), c["xq"])
    cov = st["cov"].cpu().numpy()
    assert np.array_equal(cov, c["C"].astype(np.float64)) and np.array_equal(cov.astype(np.int64), c["C"])
    lam, E, sweeps = st["eval"].cpu().numpy(), st["evec"].cpu().numpy(), st["sweeps"].cpu().tolist()
    for u in range(2):
        C = c["C"][u].astype(np.float64)
        orth = np.abs(E[u] @ E[u].T - np.eye(W)).max()
        resid = np.abs(C @ E[u].T - E[u].T * lam[u]).max() / np.linalg.norm(C)
        lam_t = sr.eigh_rows(C)[0]
        dlam = np.abs(lam[u] - lam_t).max() / lam_t.max()
        log("kenan ssa decompose T=%d W=%d u=%d: sweeps %d, |VtV-I| %.2e, |CV-VL|/|C|_F %.2e, |l-l_eigh|/l_max %.2e (bound %.2e)"
            % (T, W, u, sweeps[u], orth, resid, dlam, BOUND * W))
        assert orth <= BOUND * W and resid <= BOUND * W and dlam <= BOUND * W
        assert (np.diff(lam[u]) <= 0).all()
        assert (1 <= sweeps[u] < 30) or W == 1


@pytest.mark.parametrize("T", T_ALL[1:])
def test_reconstruction_against_the_reference(T):
    from speakerguard_amd.attack.KenanSSA import ssa_reconstruct
    g, c = golden(), _case(T)
    assert np.array_equal(g["xq_T%d" % T], c["xq"])
    for j, k in enumerate(g["rank_T%d" % T]):
        out, out64 = ssa_reconstruct(c["st"], [int(k)] * 2, want64=True)
        out, out64 = out[:, 0].cpu().numpy(), out64.cpu().numpy()
        assert np.array_equal(out, sr.low16(out64).astype(np.float32))  # the float32 output is the cast of the float64 one
        for u in range(2):
            ref, e = g["ref64_T%d" % T][u, j], float(g["ecase_T%d" % T][u, j])
            dev = float(np.abs(out64[u] - ref).max())
            near = (np.abs(ref - np.round(ref)) <= 8 * e) & (np.round(ref) != 0)
            step = np.abs(out[u].astype(np.int64) - gen().ref16(ref).astype(np.int64))
            log("kenan ssa reconstruct T=%d u=%d factor %g k=%d: E_case %.3e native %.3e ratio %.2f (margin 8); int16: %d differ, "
                "%d of %d samples undecided" % (T, u, g["meta"]["factors"][j], k, e, dev, dev / e, int((step != 0).sum()),
                                                int(near.sum()), T))
            assert dev <= 8 * e, (T, u, j, dev, e)
            assert not step[~near].any() and (step[near] <= 1).all()
            assert near.sum() <= 1e-4 * T


def test_window_of_one_is_the_identity():
    from speakerguard_amd.attack.KenanSSA import ssa_reconstruct
    c = _case(20)
    out, out64 = ssa_reconstruct(c["st"], [1, 1], want64=True)
    assert np.array_equal(out[:, 0].cpu().numpy(), c["xq"].astype(np.float32))
    want = np.stack([sr.reconstruct64(q, sr.projector(np.ones((1, 1)), 1)) for q in c["xq"]])
    assert np.array_equal(out64.cpu().numpy(), want)


@pytest.mark.parametrize("T", [100, 480, 4000])
def test_a_batch_equals_its_utterances_alone_and_two_runs_agree(T):
    from speakerguard_amd.attack.KenanSSA import ssa_decompose, ssa_reconstruct
    c = _case(T)
    W = sr.window(T)
    # three rows: utterance 0, silence (done at once, while the others still sweep), utterance 1
    x3 = torch.from_numpy(np.stack([c["x"][0], np.zeros_like(c["x"][0]), c["x"][1]])).to(DEV)
    st3 = ssa_decompose(x3)
    ranks = [max(1, W // 3), 1, W]
    r3, r3_64 = ssa_reconstruct(st3, ranks, want64=True)
    assert st3["sweeps"][1].item() == 0 and not bool(r3[1].any())
    for row, u in ((0, 0), (2, 1)):
        for key in ("xq", "eval", "evec", "sweeps"):
            assert torch.equal(st3[key][row], c["st"][key][u]), key  # ... as in the batch of two
        alone = ssa_decompose(x3[row:row + 1])
        for key in ("xq", "eval", "evec", "sweeps"):
            assert torch.equal(alone[key][0], st3[key][row]), key
        a, a64 = ssa_reconstruct(alone, [ranks[row]], want64=True)
        assert torch.equal(a[0], r3[row]) and torch.equal(a64[0], r3_64[row])
        b, b64 = ssa_reconstruct(st3, [ranks[row]], rows=[row], want64=True)
        assert torch.equal(b[0], r3[row]) and torch.equal(b64[0], r3_64[row])
    again, again64 = ssa_reconstruct(st3, ranks, want64=True)
    assert torch.equal(again, r3) and torch.equal(again64, r3_64)


def test_quantise_scale_decision_and_wrap():
    """per utterance: [-1, 1] audio is scaled, int16-scale audio is not; beyond the int16 range the low 16 bits stay"""
    from speakerguard_amd.attack.KenanSSA import ssa_decompose
    rs = np.random.RandomState(5)
    x = np.stack([0.3 * rs.randn(100), 9000.0 * rs.randn(100), 30000.0 * rs.randn(100), 0.2 * rs.randn(100)]).astype(np.float32)
    x[0, 3], x[3, 5], x[3, 6] = 1.0, 1.11, -1.111  # 32768 wraps; 0.9 * 1.11 <= 1 still scales, and wraps
    x[2, 7], x[2, 8] = 3e9, -3e9
    for bits in (16, 8):
        st = ssa_decompose(torch.from_numpy(x).to(DEV).unsqueeze(1), bits=bits)
        want = np.stack([sr.quantise(r, bits) for r in x])
        assert np.array_equal(st["xq"].cpu().numpy(), want)
    assert np.abs(x[2] * 1.0).max() > 40000 and want[3, 5] != 0


def test_refusals_leave_the_outputs_untouched():
    import ctypes as C
    from speakerguard_amd import _native as N
    from speakerguard_amd.metric.metric import _context
    ctx, s = _context(DEV), N.current_stream_ptr(DEV)
    lib, h, P = ctx.lib, ctx.handle, N._ptr
    T, W = 480, 24
    x = torch.zeros((2, T), device=DEV)
    xq = torch.full((2, T), 7, dtype=torch.int16, device=DEV)
    lam = torch.full((2, W), 7.0, dtype=torch.float64, device=DEV)
    E = torch.full((2, W, W), 7.0, dtype=torch.float64, device=DEV)
    sw = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    out = torch.full((2, T), 7.0, device=DEV)
    out64 = torch.full((2, T), 7.0, dtype=torch.float64, device=DEV)
    k = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    dec = lambda *a: lib.sg_ssa_decompose(*a)  # noqa: E731
    rec = lambda *a: lib.sg_ssa_reconstruct(*a)  # noqa: E731
    rcs = [dec(None, P(x), 2, T, 16, P(xq), P(lam), P(E), P(sw), None, s),
           dec(h, None, 2, T, 16, P(xq), P(lam), P(E), P(sw), None, s),
           dec(h, P(x), 2, T, 16, None, P(lam), P(E), P(sw), None, s),
           dec(h, P(x), 2, T, 16, P(xq), None, P(E), P(sw), None, s),
           dec(h, P(x), 2, T, 16, P(xq), P(lam), None, P(sw), None, s),
           dec(h, P(x), 2, T, 16, P(xq), P(lam), P(E), None, None, s),
           rec(None, P(xq), P(E), k(1, 1), 2, T, P(out), P(out64), s),
           rec(h, None, P(E), k(1, 1), 2, T, P(out), P(out64), s),
           rec(h, P(xq), None, k(1, 1), 2, T, P(out), P(out64), s),
           rec(h, P(xq), P(E), None, 2, T, P(out), P(out64), s),
           rec(h, P(xq), P(E), k(1, 1), 2, T, None, P(out64), s)]
    for B, Tb in ((0, T), (-1, T), (65536, T), (2, 19), (2, 0), (2, -5), (1, (1 << 22) + 1)):
        rcs.append(dec(h, P(x), B, Tb, 16, P(xq), P(lam), P(E), P(sw), None, s))
        rcs.append(rec(h, P(xq), P(E), k(1, 1), B, Tb, P(out), P(out64), s))
    for bits in (0, 17, -1):
        rcs.append(dec(h, P(x), 2, T, bits, P(xq), P(lam), P(E), P(sw), None, s))
    for ranks in ((0, 1), (1, W + 1), (-3, 1), (W, 0)):
        rcs.append(rec(h, P(xq), P(E), k(*ranks), 2, T, P(out), P(out64), s))
    torch.cuda.synchronize()
    assert rcs == [1] * len(rcs)  # SG_ERR_ARG
    for t in (xq, lam, E, sw, out, out64):
        assert bool((t == 7).all())
    assert rec(h, P(xq), P(E), k(1, W), 2, T, P(out), None, s) == 0  # (the bounds themselves are accepted)
    from speakerguard_amd.attack.KenanSSA import ssa_decompose
    with pytest.raises(ValueError):
        ssa_decompose(torch.zeros((1, 1, 19), device=DEV))


# ---------------------------------------------------------------- the attack
@pytest.mark.parametrize("T", [480, 4000])
def test_attack_reproduces_the_reference_histories(T):
    from speakerguard_amd.attack.KenanSSA import KenanSSA
    g = golden()
    kg = _module("make_golden_kenan")
    model = kg.ToyModel(g["W_toy"])
    x = torch.from_numpy(kg.make_inputs(T)).to(DEV)
    for targeted in (0, 1):
        key = "T%d_t%d" % (T, targeted)
        count = g[key + "_count"]
        split = lambda flat: [list(v) for v in np.split(np.asarray(flat), np.cumsum(count)[:-1])]  # noqa: E731
        runs = []
        for bs in (1, 4):
            atk = KenanSSA(model, max_iter=15, targeted=bool(targeted), verbose=0, batch_size=bs)
            adv, succ = atk.attack(x, torch.from_numpy(g[key + "_y"]))
            assert adv.device.type == "cuda" and adv.dtype == torch.float32 and tuple(adv.shape) == (6, 1, T)
            assert atk.factor_history == split(g[key + "_factors"])
            assert atk.rank_history == split(g[key + "_ranks"])
            assert atk.decision_history == split(g[key + "_decisions"])
            assert list(succ) == [bool(v) for v in g[key + "_succ"]]
            differ = int((adv[:, 0].cpu().numpy() != g[key + "_adv"].astype(np.float32)).sum())
            log("kenan ssa attack toy T=%d targeted=%d bs=%d: %d of %d samples differ from the reference's audio" % (T, targeted, bs, differ, 6 * T))
            assert differ <= 1e-4 * 6 * T
            runs.append(adv)
        assert torch.equal(runs[0], runs[1])


def test_attack_on_xv_plda():
    """the shortest utterance xv_plda takes (T = 5040, W = 252): every flag is what a final make_decision says"""
    from speakerguard_amd.attack.KenanSSA import KenanSSA, ssa_decompose, ssa_reconstruct
    from test_gpu_time_domain import XV_T, _models
    model = _models()[0][1]()
    rs = np.random.RandomState(0)
    x = torch.from_numpy(np.clip(np.array([a * rs.randn(1, XV_T) for a in (0.05, 0.1, 0.2, 0.3)]), -0.95, 0.95).astype(np.float32)).to(DEV)
    st = ssa_decompose(x)
    q = st["xq"].to(torch.float32).unsqueeze(1)
    own = model.make_decision(q)[0]
    n_spk = model.make_decision(q)[1].shape[1]
    for targeted in (False, True):
        y = (own + 1) % n_spk if targeted else own.clone()
        atk = KenanSSA(model, max_iter=6, targeted=targeted, verbose=0, batch_size=4)
        adv, succ = atk.attack(x, y)
        dec = model.make_decision(adv)[0].cpu().tolist()
        log("kenan ssa attack xv_plda targeted=%d: success %s ranks %s" % (targeted, succ, atk.rank_history))
        for i in range(4):
            assert succ[i] == ((dec[i] == int(y[i])) == targeted)
            hits = [j for j, d in enumerate(atk.decision_history[i]) if (d == int(y[i])) == targeted]
            if hits:  # the audio is the reconstruction at the rank of the last hit ...
                again = ssa_reconstruct(st, [atk.rank_history[i][hits[-1]]], rows=[i])
                assert torch.equal(adv[i], again[0])
            else:     # ... or the quantised input
                assert torch.equal(adv[i], q[i])
            assert 1 <= len(atk.rank_history[i]) <= 6 and all(1 <= k <= 252 for k in atk.rank_history[i])
