"""numpy restatement of the GMM / i-vector / PLDA forward (reference model/iv_plda.py, _iv_plda/gmm.py,
_iv_plda/ivector_extract.py, _xv_plda/plda.py): float64 arithmetic on the float32-parsed parameters -- the truth the GPU
stages and the reference's own float32 outputs are both measured against -- plus the packing the kernels read
(W, V, U of csrc/k_ivector.hip).  ``IvRestated(weights, dtype=np.float32)`` runs the same formulas in float32."""
import numpy as np

DIM, CEPS, WINDOW = 72, 24, 300


def delta_scales():
    """get_scales(window=3, order=2) in the reference's float32 order (iv_plda.py:277-293) -> (s1 (7,), s2 (13,)) float32"""
    inv = np.float32(1.0 / 28.0)
    s1 = (np.arange(-3, 4).astype(np.float32) * inv).astype(np.float32)
    cur = np.zeros(13, np.float32)
    for j in range(-3, 4):
        for k in range(-3, 4):
            cur[j + k + 6] = np.float32(cur[j + k + 6] + np.float32(j) * s1[k + 3])
    return s1, (cur * inv).astype(np.float32)


def add_delta(raw, dtype=np.float64):
    """(B, F, >= 24) -> (B, F, 72): iv_plda.py:248-274, frame index clamped to [0, F - 1]"""
    raw = np.asarray(raw, dtype=dtype)[:, :, :CEPS]
    B, F, _ = raw.shape
    s1, s2 = delta_scales()
    out = np.zeros((B, F, DIM), dtype=dtype)
    out[:, :, :CEPS] = raw
    t = np.arange(F)
    for blk, sc in ((1, s1), (2, s2)):
        half = (len(sc) - 1) // 2
        for j in range(-half, half + 1):
            out[:, :, blk * CEPS:(blk + 1) * CEPS] += raw[:, np.clip(t + j, 0, F - 1), :] * dtype(sc[j + half])
    return out


def cmvn_window(t, F):
    ws = t - WINDOW // 2
    we = ws + WINDOW
    if ws < 0:
        we -= ws
        ws = 0
    if we > F:
        ws -= we - F
        we = F
        ws = max(ws, 0)
    return ws, we


def cmvn(delta, dtype=np.float64):
    """sliding 300-frame centred mean subtraction, iv_plda.py:296-377, as exact window means"""
    delta = np.asarray(delta, dtype=dtype)
    B, F, _ = delta.shape
    cs = np.concatenate([np.zeros((B, 1, delta.shape[2]), np.float64), np.cumsum(delta.astype(np.float64), axis=1)], axis=1)
    out = np.empty_like(delta)
    for t in range(F):
        ws, we = cmvn_window(t, F)
        out[:, t] = delta[:, t] - ((cs[:, we] - cs[:, ws]) / (we - ws)).astype(dtype)
    return out


def zpos(i, j):
    """position of x_i x_j (i <= j) in z = [x ; x_i x_j]"""
    return DIM + i * DIM - i * (i - 1) // 2 + (j - i)


def pack_w(means_invcovars, invcovars):
    """W (C, 2700): ll = gconst + Z W^T with W_c = [mi_c ; -S_c,ii / 2 ; -S_c,ij (i < j)] in float64"""
    mi, S = np.asarray(means_invcovars, np.float64), np.asarray(invcovars, np.float64)
    C = mi.shape[0]
    W = np.zeros((C, DIM + DIM * (DIM + 1) // 2))
    W[:, :DIM] = mi
    iu = np.triu_indices(DIM)
    val = -0.5 * (S[:, iu[0], iu[1]] + S[:, iu[1], iu[0]])
    val[:, iu[0] == iu[1]] *= 0.5
    W[:, DIM:] = val  # np.triu_indices walks the upper triangle row by row: the order of zpos
    return W


def make_z(x):
    x = np.asarray(x, np.float64)
    iu = np.triu_indices(DIM)
    return np.concatenate([x, x[..., iu[0]] * x[..., iu[1]]], axis=-1)


def pack_vu(extractor, sigma_inv):
    """V (C, R, 72) = M_c^T Sigma_c^-1 and U (C, R, R) = V_c M_c in float64"""
    M, Sg = np.asarray(extractor, np.float64), np.asarray(sigma_inv, np.float64)
    V = np.einsum("cer,ced->crd", M, Sg)
    return V, np.einsum("crd,cds->crs", V, M)


class IvRestated:
    """the forward on parameters held in `dtype` arithmetic (float64: truth; float32: the reference's own precision)"""

    def __init__(self, weights, threshold=None, dtype=np.float64):
        self.dt = dtype
        self.w = {k: np.asarray(v, dtype=dtype) for k, v in weights.items()}
        self.threshold = threshold if threshold else -np.inf
        self.C, _, self.R = self.w["extractor"].shape
        self.D = self.w["lda"].shape[0]
        self._v = None

    def loglik(self, x):
        """(F, 72) -> (F, C): gmm.py:120-131"""
        w = self.w
        x = np.asarray(x, self.dt)
        ll = x @ w["means_invcovars"].T
        ll = ll - 0.5 * np.einsum("fi,cij,fj->fc", x, w["invcovars"], x)
        return ll + w["gconsts"]

    def stats(self, x):
        """(F, 72) -> zeroth (C), first (C, 72): gmm.py:133-171"""
        ll = self.loglik(x)
        e = np.exp(ll - ll.max(axis=1, keepdims=True))
        post = e / e.sum(axis=1, keepdims=True)
        return post.sum(0), post.T @ np.asarray(x, self.dt), post

    def system(self, n, f):
        w = self.w
        if self._v is None:  # a function of the weights alone: computed once (half of this call's time at C = 272, R = 262)
            self._v = np.einsum("cer,ced->crd", w["extractor"], w["sigma_inv"])
        V = self._v
        L = np.eye(self.R, dtype=self.dt) + np.einsum("c,crd,cds->rs", np.asarray(n, self.dt), V, w["extractor"])
        lin = np.einsum("crd,cd->r", V, np.asarray(f, self.dt))
        return L, lin

    def extract(self, n, f):
        """ivector_extract.py:98-114"""
        L, lin = self.system(n, f)
        lin = lin.copy()
        lin[0] += self.w["ivector_offset"]
        iv = np.linalg.solve(L, lin)
        iv[0] -= self.w["ivector_offset"]
        return iv

    def process_emb(self, iv):
        """iv_plda.py:411-443"""
        w = self.w
        e = np.asarray(iv, self.dt) - w["emb_mean"]
        e = w["lda"][:, -1] + w["lda"][:, :-1] @ e
        e = e * (np.sqrt(self.dt(self.D)) / np.linalg.norm(e))
        tr = w["plda_transform"] @ (e - w["plda_mean"])
        fac = np.sqrt(self.D / np.dot(1.0 / (w["plda_psi"] + 1.0), tr ** 2))
        return tr * fac

    def scores(self, emb, enroll=None):
        """plda.py:140-190, num_examples = 1"""
        psi = self.w["plda_psi"]
        enroll = self.w["enroll"] if enroll is None else np.asarray(enroll, self.dt)
        var = 1.0 + psi / (psi + 1.0)
        log2pi = np.log(self.dt(2 * 3.1415926))
        given = -0.5 * (np.log(var).sum() + log2pi * self.D + ((emb - psi / (psi + 1.0) * enroll) ** 2 / var).sum(1))
        without = -0.5 * (np.log(psi + 1.0).sum() + log2pi * self.D + np.dot(emb ** 2, 1.0 / (psi + 1.0)))
        return given - without

    def chain(self, cm):
        """CMVN features (B, F, 72) -> dict of every later stage"""
        out = {"zeroth": [], "first": [], "ivector": [], "emb": [], "scores": []}
        for x in cm:
            n, f, _ = self.stats(x)
            iv = self.extract(n, f)
            emb = self.process_emb(iv)
            for k, v in zip(("zeroth", "first", "ivector", "emb", "scores"), (n, f, iv, emb, self.scores(emb))):
                out[k].append(v)
        out = {k: np.stack(v) for k, v in out.items()}
        out["decisions"] = self.decide(out["scores"])
        return out

    def decide(self, scores):
        dec = scores.argmax(1).astype(np.int64)
        return np.where(scores.max(1) > self.threshold, dec, -1)


class IvOracleModel:
    """what oracle.attacks asks of a model (``make_decision`` on torch waveforms), answered by the restatement: the oracle's
    Kaldi MFCC with the dither off (its first 24 cepstra), then the float64 chain; scores come back as float32"""

    def __init__(self, weights, threshold=None):
        self.r = IvRestated(weights, threshold)
        self.threshold = self.r.threshold

    def features(self, x):
        from oracle import kaldi_mfcc
        from oracle.xv_plda import check_input_range
        x = check_input_range(x.detach().cpu().float())
        return np.stack([kaldi_mfcc.mfcc(u).numpy()[:, :CEPS] for u in x]).astype(np.float32)

    def make_decision(self, x):
        import torch
        out = self.r.chain(cmvn(add_delta(self.features(x))))
        return torch.from_numpy(out["decisions"]), torch.from_numpy(out["scores"].astype(np.float32))
