"""The gradient of the GMM / i-vector / PLDA chain, twice: (1) tests/iv_restate.py's forward as a differentiable torch float64
function (delta, CMVN, statistics, solve, tail; the length normalisation's norm detached as the reference's ``.item()``; the
``2 * 3.1415926`` constant; the losses of oracle/attacks.py in float64) -- autograd through it is the truth; (2) the adjoint
formulas the kernels of csrc/k_ivector_bwd.hip implement, written out by hand in numpy (``dtype=np.float32`` runs them in the
reference's own precision).  tests/test_ivector_grad_cpu.py pins (1) to ``IvRestated.chain`` and (2) to (1)."""
import numpy as np
import torch

import iv_restate as R

DIM, CEPS = R.DIM, R.CEPS
IU = np.triu_indices(DIM)


# ----------------------------------------------------------------------------- (1) the differentiable forward
def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def add_delta_t(raw):
    """(B, F, 24) torch -> (B, F, 72)"""
    F = raw.shape[1]
    s1, s2 = R.delta_scales()
    t = torch.arange(F)
    blocks = [raw]
    for sc in (s1, s2):
        half = (len(sc) - 1) // 2
        acc = 0
        for j in range(-half, half + 1):
            acc = acc + raw[:, torch.clamp(t + j, 0, F - 1), :] * float(sc[j + half])
        blocks.append(acc)
    return torch.cat(blocks, 2)


def cmvn_matrix(F):
    """A (F, F): cmvn = delta - A delta, A[t, f] = 1 / (we - ws) inside frame t's window"""
    A = np.zeros((F, F))
    for t in range(F):
        ws, we = R.cmvn_window(t, F)
        A[t, ws:we] = 1.0 / (we - ws)
    return A


def cmvn_t(delta):
    return delta - torch.einsum("tf,bfc->btc", t64(cmvn_matrix(delta.shape[1])), delta)


def loss_t(scores, y, loss):
    """oracle/attacks.py's cross_entropy_loss / margin_loss (untargeted, CSI, confidence 0, clip_max) on ONE float64 score row"""
    if loss == "ce":
        return torch.logsumexp(scores, 0) - scores[y]
    assert loss == "margin"
    onehot = torch.zeros_like(scores)
    onehot[y] = 1
    other = torch.max((1 - onehot) * scores - onehot * 10000, 0)[0]
    return torch.clamp(scores[y] - other, min=0)


class IvGrad:
    def __init__(self, weights, threshold=None):
        self.np = R.IvRestated(weights, threshold)
        self.w = {k: t64(v) for k, v in weights.items()}
        self.C, _, self.R = self.w["extractor"].shape
        self.D = self.w["lda"].shape[0]
        self.V, self.U = (t64(a) for a in R.pack_vu(weights["extractor"], weights["sigma_inv"]))

    # ---- stages (one utterance)
    def stats(self, x):
        w = self.w
        ll = x @ w["means_invcovars"].T - 0.5 * torch.einsum("fi,cij,fj->fc", x, w["invcovars"], x) + w["gconsts"]
        post = torch.softmax(ll, 1)
        return post.sum(0), post.T @ x

    def extract(self, n, f):
        L = torch.eye(self.R, dtype=torch.float64) + torch.einsum("c,crs->rs", n, self.U)
        lin = torch.einsum("crd,cd->r", self.V, f)
        e0 = torch.zeros(self.R, dtype=torch.float64)
        e0[0] = self.w["ivector_offset"]
        return torch.linalg.solve(L, lin + e0) - e0

    def scores(self, iv, enroll=None):
        w, D = self.w, self.D
        e = w["lda"][:, -1] + w["lda"][:, :-1] @ (iv - w["emb_mean"])
        e = e * (np.sqrt(D) / float(torch.linalg.norm(e.detach())))  # .item(): a constant in the backward
        tr = w["plda_transform"] @ (e - w["plda_mean"])
        psi = w["plda_psi"]
        emb = tr * torch.sqrt(D / torch.dot(1.0 / (psi + 1.0), tr ** 2))
        enroll = w["enroll"] if enroll is None else enroll
        var = 1.0 + psi / (psi + 1.0)
        log2pi = float(np.log(2 * 3.1415926))
        given = -0.5 * (torch.log(var).sum() + log2pi * D + ((emb - psi / (psi + 1.0) * enroll) ** 2 / var).sum(1))
        without = -0.5 * (torch.log(psi + 1.0).sum() + log2pi * D + torch.dot(emb ** 2, 1.0 / (psi + 1.0)))
        return given - without, emb

    def chain(self, cm):
        """CMVN features (B, F, 72) torch -> dict of torch stages (IvRestated.chain's keys)"""
        out = {k: [] for k in ("zeroth", "first", "ivector", "emb", "scores")}
        for x in cm:
            n, f = self.stats(x)
            iv = self.extract(n, f)
            sc, emb = self.scores(iv)
            for k, v in zip(("zeroth", "first", "ivector", "emb", "scores"), (n, f, iv, emb, sc)):
                out[k].append(v)
        return {k: torch.stack(v) for k, v in out.items()}

    def features(self, x, flag):
        """the input of `flag` (1 raw, 2 delta, 3 cmvn) -> CMVN features"""
        if flag == 1:
            x = add_delta_t(x)
        return cmvn_t(x) if flag <= 2 else x

    def loss_and_grad(self, x, y, loss, flag=3):
        """numpy input of `flag` (B, F, w), labels (B) -> (loss (B), grad (shape of x), scores (B, S)) in float64"""
        xt = t64(x).requires_grad_(True)
        sc = self.chain(self.features(xt, flag))["scores"]
        ls = torch.stack([loss_t(s, int(l), loss) for s, l in zip(sc, y)])
        ls.sum().backward()
        return ls.detach().numpy(), xt.grad.numpy(), sc.detach().numpy()


class IvGradOracleModel:
    """what oracle.attacks' white-box attacks ask of a model: ``make_decision`` on torch waveforms WITH the autograd graph --
    the oracle's Kaldi MFCC with the dither off (its first 24 cepstra, computed in float64), then the float64 chain"""

    def __init__(self, weights, threshold=None):
        self.g = IvGrad(weights, threshold)
        self.threshold = self.g.np.threshold

    def scores(self, x):
        from oracle import kaldi_mfcc
        from oracle.xv_plda import check_input_range
        x = check_input_range(x)
        raw = torch.stack([kaldi_mfcc.mfcc(u.double())[:, :CEPS].double() for u in x])
        return self.g.chain(self.g.features(raw, 1))["scores"]

    def make_decision(self, x):
        sc = self.scores(x).float()
        dec = sc.argmax(1)
        return torch.where(sc.max(1)[0] > self.threshold, dec, torch.full_like(dec, -1)), sc


# ----------------------------------------------------------------------------- (2) the adjoints by hand, numpy
def dscores_np(scores, y, loss):
    """d loss / d scores of one row (loss_device.h's cross-entropy and untargeted CSI margin with clip_max)"""
    s = np.asarray(scores, np.float64)
    g = np.zeros_like(s)
    if loss == "ce":
        p = np.exp(s - s.max())
        g = p / p.sum()
        g[y] -= 1.0
        return g
    rest = s.copy()
    rest[y] = -np.inf
    k = int(rest.argmax())  # the first maximal index, as torch.max(t, 0)
    if s[y] - s[k] > 0:
        g[y], g[k] = 1.0, -1.0
    return g


class IvAdjoint:
    """steps 1-6 of the backward on parameters held in `dtype` arithmetic"""

    def __init__(self, weights, dtype=np.float64):
        self.dt = dtype
        self.f = R.IvRestated(weights, dtype=dtype)
        self.w = self.f.w
        V, U = R.pack_vu(weights["extractor"], weights["sigma_inv"])
        self.V, self.U = V.astype(dtype), U.astype(dtype)  # (C, R, 72), (C, R, R)
        self.W = R.pack_w(weights["means_invcovars"], weights["invcovars"]).astype(dtype)  # (C, 2700)
        self.C, self.Rk, self.D = self.f.C, self.f.R, self.f.D

    def tail(self, iv, dsc):
        """step 1: d loss / d scores (S) -> d loss / d i-vector (R); the norm of the length normalisation is a constant"""
        w, D, dt = self.w, self.D, self.dt
        e1 = np.asarray(iv, dt) - w["emb_mean"]
        e2 = w["lda"][:, -1] + w["lda"][:, :-1] @ e1
        ratio = np.sqrt(dt(D)) / np.linalg.norm(e2)
        e4 = w["plda_transform"] @ (e2 * ratio - w["plda_mean"])
        psi = w["plda_psi"]
        q = np.dot(1.0 / (psi + 1.0), e4 ** 2)
        fac = np.sqrt(D / q)
        e5 = e4 * fac
        r = psi / (psi + 1.0)
        de5 = (np.asarray(dsc, dt)[:, None] * (-(e5 - r * w["enroll"]) / (1.0 + r) + e5 / (psi + 1.0))).sum(0)
        de4 = fac * de5 - np.dot(de5, e4) * (fac / q) * e4 / (psi + 1.0)
        de2 = ratio * (w["plda_transform"].T @ de4)
        return w["lda"][:, :-1].T @ de2

    def solve(self, n, f, dw):
        """steps 2 + 3: d loss / d w -> (d n (C), d f (C, 72)) by lambda = L^-1 dw, dL = -lambda s^T"""
        L, lin = self.f.system(n, f)
        lin = lin.copy()
        lin[0] += self.w["ivector_offset"]
        G = np.linalg.cholesky(L)
        tri = lambda A, b: np.linalg.solve(A, b)
        s = tri(G.T, tri(G, lin))        # the solved vector, before the offset leaves entry 0
        lam = tri(G.T, tri(G, np.asarray(dw, self.dt)))
        dLsym = -(np.outer(lam, s) + np.outer(s, lam))
        dLsym[np.diag_indices(self.Rk)] *= 0.5
        iu = np.triu_indices(self.Rk)
        dn = self.U[:, iu[0], iu[1]] @ dLsym[iu]          # sum over the packed upper triangle
        df = np.einsum("crd,r->cd", self.V, lam)
        return dn.astype(self.dt), df.astype(self.dt)

    def stats(self, x, dn, df):
        """steps 4 + 5: (d n, d f) -> d x (F, 72)"""
        dt = self.dt
        x = np.asarray(x, dt)
        _, _, post = self.f.stats(x)
        dgam = np.asarray(dn, dt) + x @ np.asarray(df, dt).T
        r = (post * dgam).sum(1, keepdims=True)
        dll = post * (dgam - r)
        dx = post @ np.asarray(df, dt)
        dz = dll @ self.W                                  # (F, 2700): never materialised on the GPU
        dx = dx + dz[:, :DIM]
        pair = dz[:, DIM:]
        ci = pair * x[:, IU[1]] * np.where(IU[0] == IU[1], 2.0, 1.0).astype(dt)   # dx_i += dz_ij x_j (2 dz_ii x_i)
        cj = pair * x[:, IU[0]] * (IU[0] != IU[1])                                   # dx_j += dz_ij x_i, i < j
        for k in range(DIM):
            dx[:, k] += ci[:, IU[0] == k].sum(1) + cj[:, IU[1] == k].sum(1)
        return dx

    def cmvn(self, dcm):
        """step 6a: (F, 72) -> (F, 72): a frame receives from every window that contains it"""
        dcm = np.asarray(dcm, self.dt)
        return dcm - cmvn_matrix(dcm.shape[0]).astype(self.dt).T @ dcm

    def delta(self, dd):
        """step 6b: (F, 72) -> (F, 24): edge frames collect the clamped taps"""
        dd = np.asarray(dd, self.dt)
        F = dd.shape[0]
        out = dd[:, :CEPS].copy()
        s1, s2 = R.delta_scales()
        t = np.arange(F)
        for blk, sc in ((1, s1), (2, s2)):
            half = (len(sc) - 1) // 2
            for j in range(-half, half + 1):
                np.add.at(out, np.clip(t + j, 0, F - 1), dd[:, blk * CEPS:(blk + 1) * CEPS] * self.dt(sc[j + half]))
        return out

    def chain(self, x, y, loss, flag=3):
        """one utterance's input of `flag` -> d loss / d x by steps 1-6 (the forward in this object's dtype)"""
        x = np.asarray(x, self.dt)
        delta = R.add_delta(x[None], self.dt)[0] if flag == 1 else x
        cm = R.cmvn(delta[None], self.dt)[0] if flag <= 2 else x
        n, f, _ = self.f.stats(cm)
        iv = self.f.extract(n, f)
        sc = self.f.scores(self.f.process_emb(iv))
        dn, df = self.solve(n, f, self.tail(iv, dscores_np(sc, y, loss)))
        g = self.stats(cm, dn, df)
        if flag <= 2:
            g = self.cmvn(g)
        return self.delta(g) if flag == 1 else g
