"""The route of speakerguard_amd/csrc/k_ssa.hip restated in numpy (float64 and exact integers): quantise, the integer lag
covariance by its recurrence, the Jacobi iteration in the kernel's pair order (``jacobi``; ``eigh`` is the truth beside it), the
projector, the taps, the interior filter, the edge sums and the cast to int16.  The formulas are the kernel's; the summation
orders are numpy's (the GPU suite holds the kernel to bounds, not to these bits).

``decompose`` / ``reconstruct`` at the bottom have the signatures speakerguard_amd.attack.KenanSSA takes as ``decompose=`` and
``reconstruct=``."""
import numpy as np

MAX_W, MIN_T, MAX_T, MAX_SWEEPS = 3000, 20, 1 << 22, 30
EPS = 2.0 ** -52


def window(T):
    if T < MIN_T or T > MAX_T:
        raise ValueError("T outside %d .. %d" % (MIN_T, MAX_T))
    return min(int(T * 0.05), MAX_W)


def low16(v):
    """float -> int32 toward zero (NaN: 0, beyond int32: its nearest end) -> the low 16 bits as int16"""
    v = np.asarray(v, np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    i = np.trunc(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16).view(np.int16)


def quantise(x, bits=16):
    """one utterance (T,) float32 -> int16 (attack/Kenan.py:31-34, per utterance)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    hi, lo = np.float32(np.fmax.reduce(x)), np.float32(np.fmin.reduce(x))
    if np.float32(0.9) * hi <= np.float32(1) and np.float32(0.9) * lo >= np.float32(-1):
        x = x * np.float32(2.0 ** (bits - 1))
    return low16(x)


def covariance(xq, W=None):
    """C[a][b] = sum_{p<t} x[p+a] x[p+b], int64: the first row as dot products, every diagonal as a running sum of
    x[a+t] x[b+t] - x[a] x[b]"""
    x = np.asarray(xq).astype(np.int64)
    T = x.shape[0]
    W = window(T) if W is None else W
    t = T - W + 1
    C = np.zeros((W, W), np.int64)
    for d in range(W):
        first = int(np.dot(x[:t], x[d:d + t]))
        n = W - d
        step = x[t:t + n - 1] * x[t + d:t + d + n - 1] - x[:n - 1] * x[d:d + n - 1]
        diag = first + np.concatenate([[0], np.cumsum(step)])
        idx = np.arange(n)
        C[idx, idx + d] = diag
        C[idx + d, idx] = diag
    return C


def covariance_direct(xq, W=None):
    """the same matrix from the trajectory matrix (the check of the recurrence)"""
    x = np.asarray(xq).astype(np.int64)
    T = x.shape[0]
    W = window(T) if W is None else W
    t = T - W + 1
    X = np.stack([x[a:a + t] for a in range(W)], 1)
    return X.T @ X


def pairs(n, r):
    """round r of the round-robin over n (even) indices -> (p, q) arrays, p < q"""
    k = np.arange(n // 2)
    a = np.where(k == 0, n - 1, (r + k) % (n - 1))
    b = np.where(k == 0, r, (r + (n - 1) - k) % (n - 1))
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(C):
    """two-sided cyclic Jacobi in the kernel's order and its closing Newton-Schulz step -> (eigenvalues descending, eigenvectors
    as ROWS, sweeps that rotated)"""
    A = np.array(C, np.float64)
    W = A.shape[0]
    V = np.eye(W)
    n = W + (W & 1)
    sweeps = 0
    for sweep in range(MAX_SWEEPS + 1):
        if sweep == MAX_SWEEPS:
            raise RuntimeError("still rotating after %d sweeps" % MAX_SWEEPS)
        rotated = 0
        for r in range(n - 1):
            p, q = pairs(n, r)
            ok = q < W
            p, q = p[ok], q[ok]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            with np.errstate(all="ignore"):
                rot = (apq != 0) & ~(np.abs(apq) <= EPS * np.sqrt(np.abs(app * aqq)))
                theta = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            rot &= t != 0
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            rot &= s != 0
            if not rot.any():
                continue
            p, q, c, s, t = p[rot], q[rot], c[rot], s[rot], t[rot]
            new_pp, new_qq = app[rot] - t * apq[rot], aqq[rot] + t * apq[rot]
            rotated += int(rot.sum())
            for M in (A, V):  # M <- M J
                x, y = M[:, p].copy(), M[:, q].copy()
                M[:, p], M[:, q] = c * x - s * y, s * x + c * y
            x, y = A[p, :].copy(), A[q, :].copy()  # A <- J^T A
            A[p, :], A[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            A[p, p], A[q, q], A[p, q], A[q, p] = new_pp, new_qq, 0.0, 0.0
        if rotated == 0:
            break
        sweeps += 1
    lam = np.diag(A).copy()
    V = V @ (1.5 * np.eye(W) - 0.5 * (V.T @ V))  # one Newton-Schulz step: the rotations' accumulated loss of orthogonality
    order = np.lexsort((np.arange(W), -lam))  # descending, ties by index
    return lam[order], np.ascontiguousarray(V[:, order].T), sweeps


def eigh_rows(C):
    """numpy.linalg.eigh, in the kernel's layout: (eigenvalues descending, eigenvectors as rows)"""
    lam, V = np.linalg.eigh(np.asarray(C, np.float64))
    return lam[::-1].copy(), np.ascontiguousarray(V[:, ::-1].T)


def projector(evec, k):
    return evec[:k].T @ evec[:k]


def taps(P):
    W = P.shape[0]
    return np.array([np.trace(P, offset=d) for d in range(-(W - 1), W)])


def reconstruct64(xq, P):
    """the float64 value of every sample before the cast: interior filter, edge sums, the division by min(m+1, W, T-m)"""
    x = np.asarray(xq).astype(np.float64)
    T, W = x.shape[0], P.shape[0]
    t = T - W + 1
    z = np.zeros(T)
    z[W - 1:t] = np.correlate(x, taps(P), "valid")
    if W > 1:
        i = np.arange(W)
        # M[u][i] = sum_l x[u+l] P[i][l] for the rows u the edges need
        left = np.stack([x[u:u + W] for u in range(W - 1)]) @ P.T           # u = 0 .. W-2
        right = np.stack([x[u:u + W] for u in range(t - W + 1, t)]) @ P.T   # u = t-W+1 .. t-1
        for m in range(W - 1):
            ii = i[:m + 1]
            z[m] = left[m - ii, ii].sum()
        for m in range(t, T):
            ii = i[m - t + 1:]
            z[m] = right[m - ii - (t - W + 1), ii].sum()
    m = np.arange(T)
    return z / np.minimum(np.minimum(m + 1, W), T - m)


def reconstruct_direct64(xq, evec, k):
    """the same through the trajectory matrix and an explicit fold (small T only: the check of taps and edges)"""
    x = np.asarray(xq).astype(np.float64)
    T, W = x.shape[0], evec.shape[1]
    t = T - W + 1
    X = np.stack([x[a:a + t] for a in range(W)], 1)
    Xh = X @ projector(evec, k)
    z, times = np.zeros(T), np.zeros(T)
    for i in range(W):
        z[i:i + t] += Xh[:, i]
        times[i:i + t] += 1
    return z / times


# ---------------------------------------------------------------- what KenanSSA takes as decompose= / reconstruct=
def decompose(audio, bits=16, eig=eigh_rows):
    """audio (N, 1, T) float32 tensor -> (state: per utterance (int16 audio, eigenvectors as rows), the int16 audio as a
    (N, 1, T) float32 tensor)"""
    import torch
    a = audio.detach().cpu().numpy()
    state = []
    for row in a[:, 0]:
        xq = quantise(row, bits)
        state.append((xq, eig(covariance(xq))[1]))
    return state, torch.from_numpy(np.stack([s[0] for s in state]).astype(np.float32)[:, None, :])


def reconstruct(state, ranks, rows=None):
    """state, one rank per utterance of ``rows`` (default: all) -> (len(rows), 1, T) float32 tensor holding int16 values"""
    import torch
    rows = range(len(state)) if rows is None else rows
    out = [low16(reconstruct64(state[r][0], projector(state[r][1], int(k)))).astype(np.float32) for r, k in zip(rows, ranks)]
    return torch.from_numpy(np.stack(out)[:, None, :])
