"""The power of model C's fixture (tests/golden/iv_ref_c.npz, iv_grad_ref_c.npz), proved on the CPU in the spirit of
tests/test_truth_power.py: the sizes C = 272 and R = 262 send every 256-wide loop of csrc/k_ivector.hip and k_ivector_bwd.hip
through a second, partial pass -- but a test notices a kernel that drops that pass only if what the pass adds is larger than
what the rule of the GPU tests (``judge``: err <= max(4 err_ref, 2^-20 max|truth|)) lets through.

Accept: the plain float32 restatement (tests/iv_restate.py, iv_restate_grad.py with dtype float32) of model C's F = 100 case
passes ``judge`` on the i-vector and on the gradient.  Reject: the same float32 restatement with ONE defect planted fails it:
  components  components 256 and up left out of the assembly of L and lin      (a ``cb`` loop that runs once)
  rows        rows 256 and up of the solved vector left at their right-hand side (a thread loop without its stride)
  panel       the last two Cholesky columns left unfactored                      (a panel loop that drops its remainder)
  dn_slice    only the first d n slice (packed entries p < 8192) summed          (iv_slice_sum with NS = 1)
The first three are judged on the i-vector, the last on the cross-entropy gradient (d n is a backward quantity).  This is a
condition on the INPUTS: should a defect pass, the fixture's inputs have to change, not the rule."""
import numpy as np
import pytest

import iv_restate as R
import iv_restate_grad as G
import test_gpu_ivector as fwd
import test_gpu_ivector_grad as bwd
from conftest import load_golden
from speakerguard_amd import synth
from test_ivector_cpu import FILES, GRAD_FILES, MODELS, checksum

F, SPAN, DN_SLICE = 100, 256, 8192  # the case; the kernels' thread / component span; kIvDnSlice of csrc/sg_internal.h


class Planted(R.IvRestated):
    """the float32 forward with at most one defect of the assembly or the solve.

    The two long contractions are grouped as the reference groups them (gmm.py:120-131: x . (S_c x), sums of 72 terms;
    ivector_extract.py:106-107: V_c = M_c^T Sigma_c^-1, U_c = V_c M_c per component, then one sum over the components).
    ``IvRestated``'s own einsums run each of them as ONE sequential chain (5184 terms per log-likelihood, 19 584 per entry of L),
    which costs nothing in float64 but in float32 leaves L 8 x farther from truth than the reference's float32 (measured at this
    case: 5.3e-4 against 6.7e-5 of max|L| = 160) and the i-vector at 1.6 x the rule's bound -- an error of the yardstick's
    summation order that neither the reference nor the kernels (float64 accumulators) have."""

    def __init__(self, weights, defect=None, dtype=np.float32):
        super().__init__(weights, dtype=dtype)
        self.defect = defect
        self.V = np.matmul(self.w["extractor"].transpose(0, 2, 1), self.w["sigma_inv"])  # (C, R, 72)
        self.U = np.matmul(self.V, self.w["extractor"])                                  # (C, R, R)
        assert self.V.dtype == self.U.dtype == dtype

    def loglik(self, x):
        w = self.w
        x = np.asarray(x, self.dt)
        Sx = np.matmul(w["invcovars"][None], x[:, None, :, None])[..., 0]                # (F, C, 72)
        ll = x @ w["means_invcovars"].T - self.dt(0.5) * np.matmul(Sx, x[:, :, None])[..., 0]
        return ll + w["gconsts"]

    def system(self, n, f):
        n, f = np.array(n, self.dt), np.array(f, self.dt)
        if self.defect == "components":
            n[SPAN:], f[SPAN:] = 0, 0
        L = np.eye(self.R, dtype=self.dt) + (n[:, None, None] * self.U).sum(0)
        lin = np.matmul(self.V, f[:, :, None]).sum((0, 2))
        return L, lin

    def extract(self, n, f):
        L, lin = self.system(n, f)
        lin = lin.copy()
        lin[0] += self.w["ivector_offset"]
        if self.defect == "panel":
            Gf = np.linalg.cholesky(L)
            Gf[:, self.R - 2:] = np.tril(L)[:, self.R - 2:]  # a left-looking factorisation: an unvisited column still holds L's
            iv = np.linalg.solve(Gf.T, np.linalg.solve(Gf, lin))
        else:
            iv = np.linalg.solve(L, lin)
        if self.defect == "rows":
            iv[SPAN:] = lin[SPAN:]
        iv[0] -= self.w["ivector_offset"]
        return iv


class PlantedAdjoint(G.IvAdjoint):
    """the float32 adjoint behind ``Planted``'s forward, whose d n sums the first `keep` entries of the packed upper triangle
    only (IvAdjoint.solve otherwise)"""

    def __init__(self, weights, keep=None, dtype=np.float32):
        super().__init__(weights, dtype)
        self.f = Planted(weights, None, dtype)
        self.w = self.f.w
        self.keep = keep

    def solve(self, n, f, dw):
        L, lin = self.f.system(n, f)
        lin = lin.copy()
        lin[0] += self.w["ivector_offset"]
        Gf = np.linalg.cholesky(L)
        tri = lambda A, b: np.linalg.solve(A, b)
        s = tri(Gf.T, tri(Gf, lin))
        lam = tri(Gf.T, tri(Gf, np.asarray(dw, self.dt)))
        dLsym = -(np.outer(lam, s) + np.outer(s, lam))
        dLsym[np.diag_indices(self.Rk)] *= 0.5
        iu = np.triu_indices(self.Rk)  # row by row: the kernels' packed order
        keep = slice(None, self.keep)
        dn = self.U[:, iu[0][keep], iu[1][keep]] @ dLsym[iu][keep]
        df = np.einsum("crd,r->cd", self.V, lam)
        return dn.astype(self.dt), df.astype(self.dt)


@pytest.fixture(scope="module")
def case():
    g, gf = load_golden(FILES["c"]), load_golden(GRAD_FILES["c"])
    w = synth.make_iv_weights(**MODELS["c"])
    assert checksum(w) == g["meta"]["c"]["weights_sha256"] == gf["meta"]["weights_sha256"]
    x, y = g["x_%d" % F], gf["y_ce_f3_%d" % F]
    assert MODELS["c"]["C"] > SPAN and MODELS["c"]["R"] > SPAN and MODELS["c"]["R"] % 4 == 2
    assert MODELS["c"]["R"] * (MODELS["c"]["R"] + 1) // 2 > 4 * DN_SLICE
    truth = R.IvRestated(w).chain(x)
    _, g_truth, _ = G.IvGrad(w).loss_and_grad(x, y, "ce", 3)
    return dict(w=w, x=x, y=y, iv_ref=g["ivector_%d" % F], iv_truth=truth["ivector"], g_ref=gf["grad_ce_f3_%d" % F], g_truth=g_truth)


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    """``judge`` as the GPU tests apply it, without its lines in the parity log: nothing here is a measurement of the engine"""
    monkeypatch.setattr(fwd, "log", lambda msg: None)
    monkeypatch.setattr(bwd, "log", lambda msg: None)


def ivector(case, defect):
    return Planted(case["w"], defect).chain(case["x"])["ivector"]


def gradient(case, keep):
    adj = PlantedAdjoint(case["w"], keep)
    return np.stack([adj.chain(u, int(l), "ce", 3) for u, l in zip(case["x"], case["y"])])


def test_plain_float32_restatement_passes(case):
    plain = Planted(case["w"])
    assert plain.loglik(case["x"][0]).dtype == np.float32
    assert R.IvRestated(case["w"]).loglik(case["x"][0]) == pytest.approx(plain.loglik(case["x"][0]), rel=1e-4, abs=1e-3)
    fwd.judge("power: plain ivector", ivector(case, None), case["iv_ref"], case["iv_truth"])
    plain = gradient(case, None)
    bwd.judge("power: plain gradient", plain, case["g_ref"], case["g_truth"])
    # the regrouped sums and PlantedAdjoint's copy of ``solve`` change nothing but the rounding: in float64 they are IvAdjoint
    x0, y0 = case["x"][0], int(case["y"][0])
    want = G.IvAdjoint(case["w"]).chain(x0, y0, "ce", 3)
    assert np.abs(PlantedAdjoint(case["w"], None, np.float64).chain(x0, y0, "ce", 3) - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("defect", ["components", "rows", "panel"])
def test_forward_defect_fails_the_rule_on_the_ivector(case, defect):
    got = ivector(case, defect)
    assert np.isfinite(got).all()
    with pytest.raises(AssertionError):
        fwd.judge("power: %s" % defect, got, case["iv_ref"], case["iv_truth"])


def test_first_dn_slice_alone_fails_the_rule_on_the_gradient(case):
    got = gradient(case, DN_SLICE)
    assert np.isfinite(got).all()
    with pytest.raises(AssertionError):
        bwd.judge("power: dn_slice", got, case["g_ref"], case["g_truth"])
