"""STOI (Taal, Hendriks, Heusdens, Jensen 2011) as DESIGN.md section 4 states it, restated in plain numpy float64 in the summation
orders of csrc/k_stoi.hip.  Test infrastructure: never imported by the product.

pystoi is not available, so nothing here is pinned by it; tests/test_stoi_restate.py corroborates the resampler against
scipy.signal.resample_poly and the frame spectra against scipy.signal.stft.

``stoi(benign, adver, fs)`` is the contract's evaluation; ``stoi(..., variant=True)`` is the same algorithm with every reduction
order reversed and a DFT by matrix in place of ``rfft``: the distance between the two is the algorithm's own round-off at that input.

The orders (``variant=False``), all float64, no fused multiply-add:
  resampler      output m = 5 u + p:  acc = 0; for j = 0 .. 122: acc += G[p][j] * x[8 u - 58 + j]  (x zero outside the signal)
  sum of 256     (frame energy) s[l] = ((a[l] + a[l+64]) + a[l+128]) + a[l+192], l < 64; then halves added: s[:32] + s[32:], ... to one
  band           ascending bin;  segment sums (norms, means, correlation) ascending frame
  final sum      c[q], q = 15 j + band: t[i] = c[i] + c[i+256] + c[i+512] + ... (ascending), i < 256; then halves added down to one
"""
import numpy as np

FS, FRAME, HOP, NFFT, NBANDS, MINFREQ = 10000, 256, 128, 512, 15, 150
N, BETA, DYN = 30, -15.0, 40.0
EPS = np.finfo(float).eps
RS_UP, RS_DOWN, RS_HALF = 5, 8, 290      # 16 kHz -> 10 kHz, taps -290 .. 290
RS_J0, RS_W = -58, 123                   # branch window: source samples 8 u + RS_J0 + j, j < RS_W
NOT_ENOUGH = 1e-5


def input_rule(x):
    """reference metric.py:10-14 per signal: float64 of the float32 samples, divided by 2^15 unless -1 <= max <= 1"""
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    return x if -1 <= x.max() <= 1 else x / 32768.0


def resample_window():
    """Octave's resample filter for 5/8, normalised to unit sum (581 taps)"""
    fc = 1.0 / (2 * max(RS_UP, RS_DOWN))
    rolloff = fc / 10
    L = int(np.ceil((60 - 8) / (28.714 * rolloff)))
    assert L == RS_HALF
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * (2 * RS_UP * fc * np.sinc(2 * fc * t))
    return h / np.sum(h)


def resample_branches():
    """G[p][j] = 5 h[290 + 8 p - 5 (RS_J0 + j)], zero where the tap is outside the filter"""
    h = RS_UP * resample_window()
    G = np.zeros((RS_UP, RS_W))
    for p in range(RS_UP):
        for j in range(RS_W):
            d = RS_DOWN * p - RS_UP * (RS_J0 + j)
            if -RS_HALF <= d <= RS_HALF:
                G[p, j] = h[RS_HALF + d]
    return G


def resample_16k(x, variant=False):
    """x (T) float64 at 16 kHz -> ceil(5 T / 8) samples at 10 kHz: the direct polyphase sum"""
    T = x.shape[0]
    n = -(-RS_UP * T // RS_DOWN)
    G = resample_branches()
    units = -(-n // RS_UP)
    lo = -RS_J0
    xp = np.zeros(lo + RS_DOWN * units + RS_W + RS_J0 + 8)
    xp[lo:lo + T] = x
    y = np.zeros(units * RS_UP)
    base = RS_DOWN * np.arange(units)  # xp index of source sample 8 u + RS_J0
    for p in range(RS_UP):
        acc = np.zeros(units)
        for j in (range(RS_W - 1, -1, -1) if variant else range(RS_W)):
            acc = acc + G[p, j] * xp[base + j]
        y[p::RS_UP] = acc
    return y[:n]


def to_10k(x, fs, variant=False):
    if fs == FS:
        return x
    if fs == 16000:
        return resample_16k(x, variant)
    raise ValueError("STOI is built for fs = 10000 and fs = 16000, got %r" % (fs,))


def window():
    return np.hanning(FRAME + 2)[1:-1]


def _halve(s):
    while s.shape[0] > 1:
        h = s.shape[0] // 2
        s = s[:h] + s[h:]
    return s[0]


def sum256(a, variant=False):
    """a (256, ...) -> (...), the kernel's order"""
    if variant:
        s = np.zeros(a.shape[1:])
        for i in range(FRAME - 1, -1, -1):
            s = s + a[i]
        return s
    return _halve(((a[0:64] + a[64:128]) + a[128:192]) + a[192:256])


def frames_of(x):
    starts = np.arange(0, x.shape[0] - FRAME, HOP)
    return x[starts[:, None] + np.arange(FRAME)[None, :]]


def frame_energies(x, variant=False):
    """dB energies of the windowed frames of x (the benign signal at 10 kHz)"""
    f = frames_of(x) * window()
    return 20 * np.log10(np.sqrt(sum256((f * f).T, variant)) + EPS)


def silent_mask(e):
    return (np.max(e) - DYN - e) < 0


def threshold_margin(e):
    """smallest distance in dB of a frame energy from the row's keep / drop threshold"""
    return float(np.min(np.abs(np.max(e) - DYN - e)))


def remove_silent(x, mask):
    """the kept windowed frames, overlap-added at hop 128"""
    f = (frames_of(x) * window())[mask]
    K = f.shape[0]
    out = np.zeros((K - 1) * HOP + FRAME)
    out[:K * HOP] += f[:, :HOP].reshape(-1)
    out[HOP:] += f[:, HOP:].reshape(-1)
    return out


def band_edges():
    """[(lo, hi)] * 15: bins lo .. hi - 1 of the 512-point spectrum"""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    k = np.arange(NBANDS)
    lo = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin(np.abs(f - a))), int(np.argmin(np.abs(f - b)))) for a, b in zip(lo, hi)]


def frame_power(x, variant=False):
    """(frames, 257) power spectra of the windowed frames of x"""
    f = frames_of(x) * window()
    if variant:
        n = np.arange(FRAME)
        k = np.arange(NFFT // 2 + 1)
        ang = -2 * np.pi * ((k[:, None] * n[None, :]) % NFFT) / NFFT
        re, im = f @ np.cos(ang).T, f @ np.sin(ang).T
    else:
        s = np.fft.rfft(f, NFFT, axis=1)
        re, im = s.real, s.imag
    return re * re + im * im


def band_values(x, variant=False):
    """(15, frames) one-third-octave band magnitudes"""
    p = frame_power(x, variant)
    out = np.zeros((NBANDS, p.shape[0]))
    for b, (lo, hi) in enumerate(band_edges()):
        acc = np.zeros(p.shape[0])
        for k in (range(hi - 1, lo - 1, -1) if variant else range(lo, hi)):
            acc = acc + p[:, k]
        out[b] = np.sqrt(acc)
    return out


def _seq(a, variant):
    """a (J, 15, 30) -> sum over the last axis, ascending (variant: descending)"""
    s = np.zeros(a.shape[:2])
    for n in (range(N - 1, -1, -1) if variant else range(N)):
        s = s + a[:, :, n]
    return s


def correlations(xb, yb, variant=False):
    """xb, yb (15, M), M >= 30 -> c (J, 15)"""
    M = xb.shape[1]
    J = M - N + 1
    idx = np.arange(J)[:, None] + np.arange(N)[None, :]
    x = np.transpose(xb[:, idx], (1, 0, 2))  # (J, 15, 30)
    y = np.transpose(yb[:, idx], (1, 0, 2))
    nx, ny = np.sqrt(_seq(x * x, variant)), np.sqrt(_seq(y * y, variant))
    y = y * (nx / (ny + EPS))[:, :, None]
    y = np.minimum(y, x * (1 + 10 ** (-BETA / 20)))
    x = x - (_seq(x, variant) / N)[:, :, None]
    y = y - (_seq(y, variant) / N)[:, :, None]
    x = x / (np.sqrt(_seq(x * x, variant)) + EPS)[:, :, None]
    y = y / (np.sqrt(_seq(y * y, variant)) + EPS)[:, :, None]
    return _seq(y * x, variant)


def final_sum(c, variant=False):
    q = c.reshape(-1)
    if variant:
        s = 0.0
        for v in q[::-1]:
            s = s + v
        return s
    pad = np.zeros(-(-q.shape[0] // 256) * 256)
    pad[:q.shape[0]] = q
    t = np.zeros(256)
    for row in pad.reshape(-1, 256):
        t = t + row
    return _halve(t)


def stoi_parts(benign, adver, fs=16000, variant=False):
    """dict(d, K, energies): the value, the kept frames and the benign frame energies in dB"""
    x, y = input_rule(benign), input_rule(adver)
    if x.shape != y.shape:
        raise ValueError("benign and adversarial audio must have the same length")
    x, y = to_10k(x, fs, variant), to_10k(y, fs, variant)
    if x.shape[0] <= FRAME:
        raise ValueError("the utterance is too short for STOI: %d samples at 10 kHz, more than %d are needed" % (x.shape[0], FRAME))
    e = frame_energies(x, variant)
    mask = silent_mask(e)
    K = int(mask.sum())
    out = dict(K=K, energies=e, d=NOT_ENOUGH)
    if K - 1 < N:
        return out
    xb = band_values(remove_silent(x, mask), variant)
    yb = band_values(remove_silent(y, mask), variant)
    c = correlations(xb, yb, variant)
    out["d"] = float(final_sum(c, variant) / (c.shape[0] * NBANDS))
    return out


def stoi(benign, adver, fs=16000, variant=False):
    return stoi_parts(benign, adver, fs, variant)["d"]
