"""speakerguard_amd.attack.KenanSSA's loop against the reference's own run (tests/golden/kenan_ssa_ref*.npz, written by
tests/golden/make_golden_kenan_ssa.py), with the numpy restatement of the native route (tests/ssa_restate.py) injected as
``decompose=`` / ``reconstruct=``: audio, flags, and every query's factor, rank and decision must come out exactly.  And the
restatement itself: against the reference's reconstructions (int16 equal everywhere), its Jacobi iteration against ``eigh``.
CPU only: the native kernels are the GPU suite's business (tests/test_gpu_kenan_ssa.py)."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import ssa_restate as sr
from conftest import GOLDEN, log
from speakerguard_amd import _native
from speakerguard_amd.attack.KenanSSA import KenanSSA


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _module("make_golden_kenan_ssa")


@pytest.fixture(scope="module")
def golden(gen):
    return gen.load(GOLDEN)


def _split(flat, count):
    return [list(v) for v in np.split(np.asarray(flat), np.cumsum(count)[:-1])]


def _run(golden, T, targeted, bs):
    model = _module("make_golden_kenan").ToyModel(golden["W_toy"])
    x = torch.from_numpy(_module("make_golden_kenan").make_inputs(T))
    atk = KenanSSA(model, max_iter=15, targeted=bool(targeted), verbose=0, batch_size=bs, decompose=sr.decompose,
                   reconstruct=sr.reconstruct)
    adv, succ = atk.attack(x.clone(), torch.from_numpy(golden["T%d_t%d_y" % (T, targeted)]))
    return atk, adv, succ


ATTACKS = [(T, t, b) for T in (480, 4000) for t in (0, 1) for b in (1, 4)]


@pytest.mark.parametrize("T,targeted,bs", ATTACKS)
def test_loop_reproduces_the_reference(golden, T, targeted, bs):
    g, key = golden, "T%d_t%d" % (T, targeted)
    atk, adv, succ = _run(g, T, targeted, bs)
    assert adv.dtype == torch.float32 and tuple(adv.shape) == (6, 1, T)
    assert np.array_equal(adv[:, 0].numpy(), g[key + "_adv"].astype(np.float32))
    assert list(succ) == [bool(v) for v in g[key + "_succ"]]
    count = g[key + "_count"]
    assert [len(f) for f in atk.factor_history] == count.tolist()
    assert atk.factor_history == _split(g[key + "_factors"], count)  # Python floats against float64: exact
    assert atk.rank_history == _split(g[key + "_ranks"], count)
    assert atk.decision_history == _split(g[key + "_decisions"], count)
    # the flag is the final decision's, not a sticky one
    want = g[key + "_final"] == g[key + "_y"] if targeted else g[key + "_final"] != g[key + "_y"]
    assert list(succ) == want.tolist()


@pytest.mark.parametrize("T,targeted", [(480, 0), (480, 1), (4000, 1)])
def test_batch_size_does_not_show(golden, T, targeted):
    a1, adv1, s1 = _run(golden, T, targeted, 1)
    a4, adv4, s4 = _run(golden, T, targeted, 4)
    assert torch.equal(adv1, adv4) and s1 == s4
    assert (a1.factor_history, a1.rank_history, a1.decision_history) == (a4.factor_history, a4.rank_history, a4.decision_history)


def test_fixture_holds_both_outcomes_in_both_modes(golden):
    for t in (0, 1):
        f = np.concatenate([golden["T%d_t%d_succ" % (T, t)] for T in (480, 4000)])
        assert f.any() and not f.all()
    # ... and runs that end early (the rank stops changing) beside runs that use every iteration
    counts = np.concatenate([golden["T%d_t%d_count" % (T, t)] for T in (480, 4000) for t in (0, 1)])
    assert counts.min() < 15 and counts.max() == 15


def test_constructor_mirrors_the_reference():
    sig = inspect.signature(KenanSSA.__init__).parameters
    names = list(sig)
    assert names[:9] == ["self", "model", "max_iter", "raster_width", "early_stop", "targeted", "verbose", "BITS", "batch_size"]
    assert [sig[n].default for n in names[2:9]] == [15, 100, False, False, 1, 16, 1]
    assert names[9:] == ["decompose", "reconstruct"] and all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[9:])
    assert KenanSSA.chunk_coupling is None and KenanSSA.workspace_limit == 4 << 30
    atk = KenanSSA(object(), early_stop=True)
    assert atk.early_stop is True and atk.batch_size == 1 and atk.atk_name == 'ssa'


def test_chunk_size():
    class Coupled(object):
        batch_coupled = True
    atk = KenanSSA(object(), batch_size=64)
    assert atk.chunk_size(100, 480) == 64 and atk.chunk_size(10, 480) == 10
    assert atk.chunk_size(100, 48000) == (4 << 30) // (3 * 2400 * 2400 * 8)  # 31: the workspace cap
    atk.workspace_limit = 1
    assert atk.chunk_size(100, 48000) == 1
    assert KenanSSA(Coupled(), batch_size=64).chunk_size(100, 480) == 1


def test_asserts_of_the_reference():
    atk = KenanSSA(object(), verbose=0, decompose=sr.decompose, reconstruct=sr.reconstruct)
    with pytest.raises(AssertionError, match="Mono"):
        atk.attack(torch.zeros(2, 2, 480), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="equal"):
        atk.attack(torch.zeros(2, 1, 480), torch.zeros(3, dtype=torch.int64))


def test_native_path_refuses_a_cpu_tensor():
    with pytest.raises(_native.NativeError):
        KenanSSA(object(), verbose=0).attack(torch.zeros(1, 1, 480), torch.zeros(1, dtype=torch.int64))


def test_window():
    lib = _native.load()
    for T, W in ((20, 1), (39, 1), (40, 2), (60, 3), (100, 5), (480, 24), (4000, 200), (16000, 800), (48000, 2400), (60000, 3000),
                 (1 << 22, 3000)):
        assert lib.sg_ssa_window(T) == W == sr.window(T) == min(int(T * 0.05), 3000)
    for T in (19, 0, -1, (1 << 22) + 1):
        assert lib.sg_ssa_window(T) == -1
        with pytest.raises(ValueError):
            sr.window(T)


# ---------------------------------------------------------------- the restatement
def test_quantise():
    x = np.array([0.5, -0.25, 1.0 / 3, -1.0 / 3, 0.99997, 0.0], np.float32)
    assert sr.quantise(x).tolist() == [16384, -8192, 10922, -10922, 32767, 0]  # scaled, toward zero
    assert sr.quantise(x, bits=8).tolist() == [64, -32, 42, -42, 127, 0]
    assert sr.quantise(np.array([1.0, -0.5], np.float32)).tolist() == [-32768, -16384]  # 32768 wraps
    assert sr.quantise(np.array([1.2, -0.5, 3.9], np.float32)).tolist() == [1, 0, 3]  # 0.9 * 3.9 > 1: int16 scale already
    assert sr.quantise(np.array([40000.7, -70000.2, np.nan, 1e12], np.float32)).tolist() == [40000 - 65536, -70000 + 131072 - 65536, 0, -1]


@pytest.mark.parametrize("T", [40, 60, 100, 480, 4000, 16000])
def test_restatement_equals_the_reference(golden, gen, T):
    """int16 equal everywhere; the float64 gap is what the fixture recorded as E_case (logged; a different LAPACK may move it)"""
    g = golden
    worst = 0.0
    for u in range(2):
        xq = g["xq_T%d" % T][u]
        assert np.array_equal(xq, sr.quantise(gen.inputs(T)[u, 0]))
        C = sr.covariance(xq)
        if T <= 480:
            assert np.array_equal(C, sr.covariance_direct(xq))
        evec = sr.eigh_rows(C)[1]
        for j, k in enumerate(g["rank_T%d" % T]):
            mine = sr.reconstruct64(xq, sr.projector(evec, int(k)))
            ref = g["ref64_T%d" % T][u, j]
            worst = max(worst, float(np.abs(mine - ref).max() / g["ecase_T%d" % T][u, j]))
            assert np.array_equal(sr.low16(mine), gen.ref16(ref)), (T, u, j)
    log("kenan ssa restatement T=%d: float64 gap to the reference at most %.2f x the recorded E_case" % (T, worst))


@pytest.mark.parametrize("T", [20, 40, 100, 480])
def test_taps_and_edges_are_the_fold(gen, T):
    xq = sr.quantise(gen.inputs(T)[0, 0])
    W = sr.window(T)
    evec = sr.jacobi(sr.covariance(xq))[1]
    for k in sorted({1, max(1, W // 2), W}):
        a, b = sr.reconstruct64(xq, sr.projector(evec, k)), sr.reconstruct_direct64(xq, evec, k)
        assert np.abs(a - b).max() <= 1e-9 * max(1, np.abs(xq).max())
    # full rank (and W = 1 whatever the rank) gives the utterance back
    assert np.array_equal(sr.low16(np.round(sr.reconstruct64(xq, sr.projector(evec, W)))), xq)


@pytest.mark.parametrize("T", [20, 40, 60, 100, 480, 4000])
def test_jacobi_against_eigh(gen, T):
    W = sr.window(T)
    bound = 64 * W * 2.0 ** -53
    for u in range(2):
        C = sr.covariance(sr.quantise(gen.inputs(T)[u, 0])).astype(np.float64)
        lam, E, sweeps = sr.jacobi(C)
        lam_t = sr.eigh_rows(C)[0]
        orth = np.abs(E @ E.T - np.eye(W)).max()
        resid = np.abs(C @ E.T - E.T * lam).max() / np.linalg.norm(C)
        dlam = np.abs(lam - lam_t).max() / lam_t.max()
        log("kenan ssa jacobi restated T=%d W=%d u=%d: sweeps %d, |VtV-I| %.2e, |CV-VL|/|C|_F %.2e, |l-l_eigh|/l_max %.2e (bound %.2e)"
            % (T, W, u, sweeps, orth, resid, dlam, bound))
        assert orth <= bound and resid <= bound and dlam <= bound
        assert (np.diff(lam) <= 0).all() and 1 <= sweeps < sr.MAX_SWEEPS or W == 1


def test_silence():
    x = torch.zeros(2, 1, 100)
    lam, E, sweeps = sr.jacobi(sr.covariance(sr.quantise(x[0, 0].numpy())))
    assert sweeps == 0 and not lam.any() and np.array_equal(E, np.eye(5))
    state, q = sr.decompose(x)
    assert not q.any() and not sr.reconstruct(state, [1, 5]).any()


def test_pairs_cover_every_pair_once():
    for n in (2, 4, 6, 24, 200):
        seen = set()
        for r in range(n - 1):
            p, q = sr.pairs(n, r)
            assert (p < q).all() and len(set(p.tolist()) | set(q.tolist())) == n
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2
