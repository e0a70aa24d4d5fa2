"""Restatements of the spectrum gate (csrc/k_spectrum.hip) for the tests.

``truth_*``   the transform, the gate and the inverse in float64 through numpy's FFT: what the kernel is judged against.
``plan``      the pass plan in plain Python: smooth or Bluestein, the network's length and its radix sequence.
``network_*`` the kernel's own route -- half-length complex trick, Stockham passes, Bluestein, real post-pass -- at a chosen
              precision.  In float64 it must agree with ``truth_*`` to rounding (the route is right); in float32 it is the
              kernel's arithmetic, value for value (no fused multiply-add).
"""
import numpy as np

MAX_T = 1 << 22
LDS_BYTES, LDS_STATIC = 160 * 1024, 256


# ---------------------------------------------------------------- float64 truth
def truth_spectrum(x):
    return np.fft.rfft(np.asarray(x, np.float64), axis=-1)


def truth_gate(x, keep):
    """irfft of the float64 spectrum with the bins outside `keep` zeroed"""
    x = np.asarray(x, np.float64)
    return np.fft.irfft(np.where(keep, truth_spectrum(x), 0), n=x.shape[-1], axis=-1)


def bisection_factors(peak, outcomes="SSSSSSFS"):
    """the factors the attack's bisection queries from peak / 2 (float32, as the loop runs it) when query i succeeds ('S': the
    factor becomes the upper end) or fails ('F': the lower end).  The default path halves six times -- down into the bulk of
    a noisy spectrum --, fails at peak / 128 and bisects upwards to 3 peak / 256."""
    lo, hi = np.float32(0), np.float32(peak)
    f, out = np.float32(hi / np.float32(2)), []
    for o in outcomes:
        out.append(f)
        if o == "S":
            hi = f
        else:
            lo = f
        f = np.float32(np.abs((lo + hi) / np.float32(2)))
    return np.array(out, np.float32)


# ---------------------------------------------------------------- the plan
def plan(T):
    """{'M', 'N', 'bluestein', 'radix', 'lds'} of an even T in 2 .. 2^22"""
    if T < 2 or T > MAX_T or T % 2:
        raise ValueError("T must be even and in 2 .. 2^22")
    M = T // 2
    rest = M
    for f in (2, 3, 5):
        while rest % f == 0:
            rest //= f
    blue = rest != 1
    N = M
    if blue:
        N = 1
        while N < 2 * M - 1:
            N *= 2
    radix, n = [], N
    for f in (4, 2, 3, 5):
        while n % f == 0:
            radix.append(f)
            n //= f
    assert n == 1
    return {"M": M, "N": N, "bluestein": blue, "radix": radix, "lds": 16 * N + LDS_STATIC <= LDS_BYTES}


# ---------------------------------------------------------------- the kernel's route
def _tables(T, p, cdtype):
    M, N = p["M"], p["N"]
    tw = np.exp(-2j * np.pi * np.arange(N) / N)
    post = np.exp(-2j * np.pi * np.arange(M // 2 + 1) / T)
    chirp = bhat = None
    if p["bluestein"]:
        n = np.arange(M, dtype=np.int64)
        chirp = np.exp(-1j * np.pi * ((n * n) % (2 * M)) / M)
        b = np.zeros(N, np.complex128)
        b[:M] = np.conj(chirp)
        b[N - np.arange(1, M)] = np.conj(chirp[1:])
        bhat = np.fft.fft(b) / N
    return [None if t is None else t.astype(cdtype) for t in (tw, post, chirp, bhat)]


def _cmul(a, b):
    """(ar br - ai bi) + i (ar bi + ai br), every product and sum rounded on its own"""
    return (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)


def _butterfly(a, R, rdtype):
    mi = lambda v: v.imag - 1j * v.real  # noqa: E731  (-i v)
    pi = lambda v: -v.imag + 1j * v.real  # noqa: E731  (+i v)
    c = lambda v: rdtype(v)  # noqa: E731
    if R == 2:
        return [a[0] + a[1], a[0] - a[1]]
    if R == 4:
        t0, t1, t2, t3 = a[0] + a[2], a[0] - a[2], a[1] + a[3], mi(a[1] - a[3])
        return [t0 + t2, t1 + t3, t0 - t2, t1 - t3]
    if R == 3:
        t1 = a[1] + a[2]
        t2 = a[0] - c(0.5) * t1
        t3 = c(0.86602540378443864676) * (a[1] - a[2])
        return [a[0] + t1, t2 + mi(t3), t2 + pi(t3)]
    c1, c2 = c(0.30901699437494742410), c(-0.80901699437494742410)
    s1, s2 = c(0.95105651629515357212), c(0.58778525229247312917)
    t1, t2, t3, t4 = a[1] + a[4], a[2] + a[3], a[1] - a[4], a[2] - a[3]
    m1 = (a[0] + c1 * t1) + c2 * t2
    m2 = (a[0] + c2 * t1) + c1 * t2
    n1 = s1 * t3 + s2 * t4
    n2 = s2 * t3 - s1 * t4
    return [(a[0] + t1) + t2, m1 + mi(n1), m2 + mi(n2), m2 + pi(n2), m1 + pi(n1)]


def _network(v, p, tw, rdtype):
    N, s = p["N"], 1
    for R in p["radix"]:
        nb = N // R
        i = np.arange(nb)
        q = i % s
        sp = i - q
        b = _butterfly([v[i + j * nb] for j in range(R)], R, rdtype)
        out = np.empty_like(v)
        o = q + sp * R
        out[o] = b[0]
        for k in range(1, R):
            out[o + s * k] = _cmul(b[k], tw[sp * k])
        v, s = out, s * R
    return v


def _dft(v, p, tabs, rdtype):
    tw, _, chirp, bhat = tabs
    if not p["bluestein"]:
        return _network(v, p, tw, rdtype)
    a = np.zeros(p["N"], v.dtype)
    a[:p["M"]] = _cmul(v, chirp)
    a = _network(a, p, tw, rdtype)
    a = np.conj(_cmul(a, bhat))
    a = _network(a, p, tw, rdtype)
    return _cmul(chirp, np.conj(a[:p["M"]]))


def network_gate(x, factor=None, dtype=np.float32):
    """one row through the kernel's route: (spectrum (M+1) complex, magnitudes, keep or None, output or None)"""
    rdtype = np.dtype(dtype).type
    cdtype = np.complex64 if rdtype is np.float32 else np.complex128
    x = np.asarray(x, rdtype)
    T = x.shape[0]
    p = plan(T)
    M = p["M"]
    tabs = _tables(T, p, cdtype)
    post = tabs[1]
    Z = _dft((x[0::2] + 1j * x[1::2]).astype(cdtype), p, tabs, rdtype)
    X = np.zeros(M + 1, cdtype)
    X[0], X[M] = Z[0].real + Z[0].imag, Z[0].real - Z[0].imag
    k = np.arange(1, M // 2 + 1)
    m = M - k
    A, Bc = Z[k], np.conj(Z[m])
    E, D = rdtype(0.5) * (A + Bc), rdtype(0.5) * (A - Bc)
    w = _cmul(post[k], D)
    t = w.imag - 1j * w.real
    X[m] = np.conj(E - t)
    X[k] = E + t  # (after X[m]: the middle bin of an even M is its own partner and takes this value)
    mag = np.sqrt(X.real * X.real + X.imag * X.imag)
    if factor is None:
        return X, mag, None, None
    keep = ~(mag < rdtype(factor))
    G = np.where(keep, X, 0).astype(cdtype)
    Zi = np.zeros(M, cdtype)
    S, Dd = G[k] + np.conj(G[m]), G[k] - np.conj(G[m])
    cw = _cmul(np.conj(post[k]), Dd)
    u = -cw.imag + 1j * cw.real
    Zi[m] = S - u
    Zi[k] = np.conj(S + u)
    Zi[0] = (G[0].real + G[M].real) - 1j * (G[0].real - G[M].real)
    Y = _dft(Zi, p, tabs, rdtype)
    out = np.empty(T, rdtype)
    inv = rdtype(1.0 / T)
    out[0::2] = Y.real * inv
    out[1::2] = -Y.imag * inv
    return X, mag, keep, out
