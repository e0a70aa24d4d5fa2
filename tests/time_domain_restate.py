"""TEST INFRASTRUCTURE (checker only; never imported by the product).

The five time-domain defenses' contracts (speakerguard_amd/csrc/k_time_domain.hip header) restated in numpy, float32
operation for float32 operation: what the kernels must reproduce bit for bit wherever the arithmetic is exactly
restatable (everything except the library logf / cosf inside the generated noise)."""
import numpy as np

from oracle import philox

F32 = np.float32
REPEAT_STRIDE = 0xC2B2AE3D27D4EB4F
AT_DOMAIN = 0xA7000000
ROW_THREADS = 1024
MASK64 = (1 << 64) - 1


def fmaf(a, b, c):
    """float32 fused multiply-add, exactly: a*b is exact in float64; the sum is rounded to ODD in float64 (TwoSum tells
    whether it was inexact and in which direction), which makes the final rounding to float32 the correct single one."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exact: s + err == p + c
    inexact = (err != 0) & np.isfinite(s)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(inexact & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def rows(x):
    x = np.asarray(x, F32)
    return x.reshape(1, -1) if x.ndim == 1 else x.reshape(x.shape[0], -1)


# ---------------------------------------------------------------- QT / BDR
def qt_scale(x):
    """32768 if the whole call lies in the [-1, 1] float domain (time_domain.py:31, float32 like torch), else 1"""
    x = rows(x)
    return F32(32768.0) if F32(0.9) * x.max() <= F32(1) and F32(0.9) * x.min() >= F32(-1) else F32(1.0)


def qt(x, q=128, scale=None):
    x = rows(x)
    s = qt_scale(x) if scale is None else F32(scale)
    q = F32(q)
    v = np.rint((x * s) / q).astype(F32) * q
    return (v / s).astype(F32) if s != 1 else v


def bdr(x, param=8, bits=16):
    return qt(x, 2 ** (bits - param))


# ---------------------------------------------------------------- AS
def _padded(x, h):
    return np.pad(rows(x), ((0, 0), (h, h)))


def avg_smooth(x, k=3):
    """forward AND backward (the operator is symmetric): one fmaf chain in tap order, from 0"""
    assert k % 2 == 1 and 1 <= k <= 31
    h, T = (k - 1) // 2, rows(x).shape[1]
    xp, w = _padded(x, h), F32(1.0 / k)
    acc = np.zeros(rows(x).shape, F32)
    for j in range(k):
        acc = fmaf(w, xp[:, j:j + T], acc)
    return acc


# ---------------------------------------------------------------- MS
def median_smooth(x, k=3):
    """-> (out, sel): the window element of rank (k-1)/2 under (value, window position); sel = its offset from the centre"""
    assert k % 2 == 1 and 1 <= k <= 31
    h = (k - 1) // 2
    win = np.lib.stride_tricks.sliding_window_view(_padded(x, h), k, axis=1)  # (B, T, k)
    pos = np.argsort(win, axis=2, kind="stable")[:, :, h]                     # stable: equal values keep window order
    out = np.take_along_axis(win, pos[:, :, None], axis=2)[:, :, 0]
    return out.astype(F32), (pos - h).astype(np.int8)


def median_smooth_bwd(sel, g, k):
    """gx[i] = sum over t = i-h .. i+h ascending, inside the row, of (sel[t] == i - t ? g[t] : 0), from 0"""
    g, h = rows(g), (k - 1) // 2
    B, T = g.shape
    gp, sp = np.pad(g, ((0, 0), (h, h))), np.pad(sel.astype(np.int32), ((0, 0), (h, h)), constant_values=127)
    acc = np.zeros((B, T), F32)
    for d in range(-h, h + 1):  # t = i + d
        acc = acc + np.where(sp[:, h + d:h + d + T] == -d, gp[:, h + d:h + d + T], F32(0))
    return acc.astype(F32)


def median_pad_mass(sel, g, k):
    """float64 sum of the cotangents whose selected element is a pad zero (dropped by the backward)"""
    h = (k - 1) // 2
    T = sel.shape[1]
    src = np.arange(T)[None, :] + sel.astype(np.int64)
    return rows(g).astype(np.float64)[(src < 0) | (src >= T)].sum()


# ---------------------------------------------------------------- AT
def row_sum(terms):
    """the reduction tree: thread j of 1024 adds its terms j, j + 1024, ... in order from 0; the 64 lanes of a wave combine
    by v += v[lane ^ o], o = 32 .. 1; the 16 wave sums are added in wave order"""
    terms = np.asarray(terms, F32)
    B, T = terms.shape
    n = -(-T // ROW_THREADS)
    padded = np.zeros((B, n * ROW_THREADS), F32)
    padded[:, :T] = terms
    chunks, live = padded.reshape(B, n, ROW_THREADS), (np.arange(n * ROW_THREADS) < T).reshape(n, ROW_THREADS)
    acc = np.zeros((B, ROW_THREADS), F32)
    for i in range(n):
        acc = np.where(live[i], acc + chunks[:, i], acc)  # (a thread past the row's end adds nothing, not even +0)
    acc = acc.reshape(B, ROW_THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    s = acc[:, 0, 0]
    for w in range(1, ROW_THREADS // 64):
        s = s + acc[:, w, 0]
    return s.astype(F32)


def at_snr(param):
    return F32(10.0 ** (param / 10.0))


def at_forward(x, noise, param=25):
    """-> (out, sigma, P)"""
    x, noise = rows(x), rows(noise)
    T = x.shape[1]
    v = x * F32(1.0 / np.sqrt(float(T)))
    P = row_sum(v * v)
    sigma = np.sqrt(P / at_snr(param)).astype(F32)
    return fmaf(noise, sigma[:, None], x), sigma, P


def at_backward(x, noise, g, sigma, P, param=25):
    x, noise, g = rows(x), rows(noise), rows(g)
    T = x.shape[1]
    dot = row_sum(g * noise)
    den = (F32(T) * at_snr(param)) * sigma
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(P == 0, F32(0), dot / den).astype(F32)
    return fmaf(x, coef[:, None], g)


def at_row_key(seed, index_base, row_base, rep_rows, b):
    """(key, utterance) of row b of a call: sg_dither's derivation"""
    g = row_base + b
    rep = g // rep_rows if rep_rows > 0 else 0
    return (seed + rep * REPEAT_STRIDE) & MASK64, index_base + (g - rep * rep_rows)


def at_normal(key, utt, T):
    """(T,) float32 unit normals of (global) utterance `utt`: Box-Muller on words 0 and 1 of
    philox(counter = (t, AT_DOMAIN, utt lo, utt hi), key)"""
    k0, k1 = philox._key(key)
    r0, r1, _, _ = philox.philox4x32_10(np.arange(T), AT_DOMAIN, int(utt) & 0xFFFFFFFF, (int(utt) >> 32) & 0xFFFFFFFF, k0, k1)
    return (np.sqrt(F32(-2.0) * np.log(philox._uniform(r0))) * np.cos(F32(6.283185307179586) * philox._uniform(r1))).astype(F32)


def at_noise(seed, index_base, row_base, rep_rows, B, T):
    return np.stack([at_normal(*at_row_key(seed, index_base, row_base, rep_rows, b), T) for b in range(B)])
