"""TEST INFRASTRUCTURE (checker only; never imported by the product).

The frequency-domain defenses' contract (speakerguard_amd/csrc/k_freq_domain.hip header) restated in numpy, float32
operation for float32 operation: the second-order-section cascade as the chunked parallel scan the kernel runs, the clamp,
the mask, and the backward as the same sequence on the reversed row.  What the kernel must reproduce bit for bit."""
import numpy as np

from time_domain_restate import fmaf, rows

F32 = np.float32
C = 4            # samples per lane (kFdChunk)
LANES = 64
WAVES = 16
W = C * LANES    # samples per wave
P = W * WAVES    # samples per block pass
MAX_SECTIONS = 16


def _mul(a, b):
    """2x2 float64 product, (m00, m01, m10, m11), written out like fd_tables' mat_mul"""
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3])


def stable(a1, a2):
    return abs(a2) < 1.0 and abs(a1) < 1.0 + a2


def tables(sos):
    """float64 (S,6) sos -> per section dict of float32 tables, exactly fd_tables; ValueError where the kernel refuses"""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    if not 1 <= len(sos) <= MAX_SECTIONS:
        raise ValueError("1 .. 16 sections")
    out = []
    for row in sos:
        if not np.isfinite(row).all() or row[3] == 0:
            raise ValueError("bad coefficient")
        b0, b1, b2, a1, a2 = (F32(row[i] / row[3]) for i in (0, 1, 2, 4, 5))
        if not (stable(row[4] / row[3], row[5] / row[3]) and stable(float(a1), float(a2))):
            raise ValueError("poles not strictly inside the unit circle")
        A = (-float(a1), 1.0, -float(a2), 0.0)
        p, r = (1.0, 0.0, 0.0, 1.0), []
        for _ in range(C):
            r.append((F32(p[0]), F32(p[1])))
            p = _mul(p, A)
        lev, wav = [], []
        for _ in range(6):
            lev.append(tuple(F32(v) for v in p))
            p = _mul(p, p)
        for _ in range(4):
            wav.append(tuple(F32(v) for v in p))
            p = _mul(p, p)
        out.append(dict(b0=b0, b1=b1, b2=b2, na1=F32(-a1), na2=F32(-a2), r=r, lev=lev, wav=wav))
    return out


def _mv(n, o, v):
    return fmaf(n[1], o[1], fmaf(n[0], o[0], v[0])), fmaf(n[3], o[1], fmaf(n[2], o[0], v[1]))


def _shift(a, k, axis):
    """value of the element k places before, along axis (what the lanes below k receive is never used)"""
    out = np.zeros_like(a)
    dst = [slice(None)] * a.ndim
    src = [slice(None)] * a.ndim
    dst[axis], src[axis] = slice(k, None), slice(0, a.shape[axis] - k)
    out[tuple(dst)] = a[tuple(src)]
    return out


def cascade(x, tabs):
    """H x, zero initial state: (B,T) float32 -> (B,T) float32, the kernel's sequence"""
    x = rows(x)
    B, T = x.shape
    n_pass = -(-T // P)
    xp = np.zeros((B, n_pass * P), F32)
    xp[:, :T] = x
    out = np.empty_like(xp)
    lane = np.arange(LANES)
    sp = [(np.zeros(B, F32), np.zeros(B, F32)) for _ in tabs]
    for p in range(n_pass):
        y = xp[:, p * P:(p + 1) * P].reshape(B, WAVES, LANES, C).copy()
        for k, c in enumerate(tabs):
            # (a)
            f = (np.zeros((B, WAVES, LANES), F32), np.zeros((B, WAVES, LANES), F32))
            for i in range(C):
                xi = y[..., i]
                yy = fmaf(c["b0"], xi, f[0])
                s1 = fmaf(c["na1"], yy, fmaf(c["b1"], xi, f[1]))
                s2 = fmaf(c["na2"], yy, (c["b2"] * xi).astype(F32))
                y[..., i] = yy
                f = (s1, s2)
            # (b) in the wave
            v = f
            for d in range(6):
                o = (_shift(v[0], 1 << d, 2), _shift(v[1], 1 << d, 2))
                n = _mv(c["lev"][d], o, v)
                take = lane >= (1 << d)
                v = (np.where(take, n[0], v[0]), np.where(take, n[1], v[1]))
            # over the block
            t = [v[0][:, :, LANES - 1].copy(), v[1][:, :, LANES - 1].copy()]  # (B, WAVES)
            n = _mv(c["wav"][0], sp[k], (t[0][:, 0], t[1][:, 0]))
            t[0][:, 0], t[1][:, 0] = n
            wv = np.arange(WAVES)
            for e in range(4):
                o = (_shift(t[0], 1 << e, 1), _shift(t[1], 1 << e, 1))
                n = _mv(c["wav"][e], o, t)
                take = wv >= (1 << e)
                t = [np.where(take, n[0], t[0]), np.where(take, n[1], t[1])]
            cw = (np.concatenate([sp[k][0][:, None], t[0][:, :-1]], 1), np.concatenate([sp[k][1][:, None], t[1][:, :-1]], 1))
            sp[k] = (t[0][:, -1].copy(), t[1][:, -1].copy())
            u = (np.repeat(cw[0][:, :, None], LANES, 2), np.repeat(cw[1][:, :, None], LANES, 2))
            zero = (np.zeros_like(u[0]), np.zeros_like(u[1]))
            for d in range(6):
                n = _mv(c["lev"][d], u, zero)
                take = ((lane >> d) & 1) == 1
                u = (np.where(take, n[0], u[0]), np.where(take, n[1], u[1]))
            s_in = (_shift(v[0], 1, 2) + u[0], _shift(v[1], 1, 2) + u[1])
            # (c)
            for i in range(C):
                y[..., i] = fmaf(c["r"][i][1], s_in[1], fmaf(c["r"][i][0], s_in[0], y[..., i]))
        out[:, p * P:(p + 1) * P] = y.reshape(B, P)
    return out[:, :T].copy()


def clip_range(x, bits=16):
    """the reference's per-call rule (frequency_domain.py:46-51), float32 like torch"""
    x = rows(x)
    if F32(0.9) * x.max() <= F32(1) and F32(0.9) * x.min() >= F32(-1):
        return F32(-1), F32(1)
    return F32(-2 ** (bits - 1)), F32(2 ** (bits - 1) - 1)


def forward(x, sos, clip=None, bits=16):
    """-> (out, mask int8, pre-clamp value)"""
    lo, hi = clip_range(x, bits) if clip is None else (F32(clip[0]), F32(clip[1]))
    v = cascade(x, tables(sos))
    return np.minimum(np.maximum(v, lo), hi), ((v >= lo) & (v <= hi)).astype(np.int8), v


def backward(g, mask, sos):
    g = np.where(mask != 0, rows(g), F32(0))
    return cascade(g[:, ::-1], tables(sos))[:, ::-1].copy()
