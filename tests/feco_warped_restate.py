"""numpy float32 restatement of the warped k-means kernel's determinism contract (speakerguard_amd/csrc/k_feco_warped.hip
header), which is the reference's defense/feature_level.py:53-154 with every reduction order fixed.  Bit for bit what the
kernel computes; the reference fixture (tests/golden/feco_warped_ref.npz) checks it against the reference's own code."""
import math

import numpy as np
import torch

from oracle.philox import _key, philox4x32_10

f32 = np.float32
_PERM = [np.arange(64) ^ m for m in (1, 2, 4, 8, 16, 32)]


def bfly(v):
    """(..., D) float32 -> (...,): the xor butterfly over 64 zero-padded lanes (s[d] += s[d ^ m], m = 1, 2, ..., 32)."""
    v = np.asarray(v, dtype=f32)
    s = np.zeros(v.shape[:-1] + (64,), dtype=f32)
    s[..., :v.shape[-1]] = v
    for p in _PERM:
        s = s + s[..., p]
    return s[..., 0]


class Degenerate(ValueError):
    pass


def ts_boundaries(x, k):
    """TS (:53-77), including the surpass fix-up that stops at index 2 (may return non-increasing boundaries)."""
    x = np.asarray(x, dtype=f32)
    n = x.shape[0]
    d = x[1:] - x[:-1]
    nrm = np.sqrt(bfly(d * d)).astype(f32)
    dist = np.add.accumulate(np.concatenate([np.zeros(1, f32), nrm]), dtype=f32)
    seg = f32(dist[n - 1] / f32(k))
    b, index = [0], 0
    for j in range(1, k):
        req = f32(seg * f32(j))
        while index < n and (req > dist[index] or index == b[-1]):
            index += 1
        b.append(index)
    b = np.array(b, dtype=np.int64)
    sur = np.nonzero(b == n)[0]
    if len(sur) == 0:
        return b
    for i, idx in enumerate(sur):
        b[idx] = n - len(sur) + i
    for i in range(sur[0] - 1, 1, -1):
        if b[i] >= b[i + 1]:
            b[i] = b[i + 1] - 1
        else:
            break
    return b


def random_boundaries(key, utt, n, k):
    """random_init (:80-85) keyed like oracle.philox.feco_random_init: the k - 1 frames of lowest (Philox word 0, frame)
    among frames 1 .. n-1, sorted, after 0."""
    k0, k1 = _key(key)
    frames = np.arange(1, n)
    keys = philox4x32_10(frames, 0, int(utt) & 0xFFFFFFFF, (int(utt) >> 32) & 0xFFFFFFFF, k0, k1)[0]
    chosen = np.sort(frames[np.lexsort((frames, keys))[:k - 1]])
    return np.concatenate([[0], chosen]).astype(np.int64)


def valid(b, n):
    b = np.asarray(b)
    return b[0] == 0 and b[-1] < n and bool(np.all(np.diff(b) > 0))


def init_segments(x, b):
    """init (:88-107): counts, segment ids, means summed in ascending frame order from 0.f, / count."""
    x = np.asarray(x, dtype=f32)
    n, k = x.shape[0], len(b)
    ends = np.append(b[1:], n)
    counts = (ends - b).astype(np.int64)
    ids = np.repeat(np.arange(k), counts).astype(np.int32)
    means = np.stack([np.add.accumulate(x[b[i]:ends[i]], axis=0, dtype=f32)[-1] / f32(counts[i]) for i in range(k)])
    return means.astype(f32), ids, counts


def _dsq(x, m_l, m_i, c_l, c_i):
    dl, dj = x - m_l, x - m_i
    s = bfly(np.stack([dl * dl, dj * dj]))
    t_l, t_i = f32(f32(s[0] * f32(c_l)) / f32(c_l + 1)), f32(f32(s[1] * f32(c_i)) / f32(c_i - 1))
    return f32(t_l - t_i), max(abs(float(t_l)), abs(float(t_i)), 1e-30)


def sweep(x, b, delta=0.0, cap=None, stats=None):
    """wk_compute's loop (:118-153) from initial boundaries b: (final means, final boundaries, initial means, init ids,
    init counts, sweeps).  `stats` (a list) collects |delta_SQE| / max(|its two terms|) of every decision (fixture margins)."""
    x = np.asarray(x, dtype=f32)
    n = x.shape[0]
    b = np.array(b, dtype=np.int64)
    k = len(b)
    means0, ids, counts0 = init_segments(x, b)
    means, counts = means0.copy(), counts0.copy()
    cap = 4 * n if cap is None else cap
    sw, moved = 0, True
    while moved and sw < cap:
        moved = False
        sw += 1
        for i in range(k):
            if i > 0:
                begin = int(b[i])
                end = begin + math.floor(int(counts[i]) / 2 * (1 - delta))
                for j in range(begin, end):
                    if counts[i] <= 1:
                        break
                    d, sc = _dsq(x[j], means[i - 1], means[i], int(counts[i - 1]), int(counts[i]))
                    if stats is not None:
                        stats.append(abs(float(d)) / sc)
                    if not d < 0:
                        break
                    moved = True
                    b[i] += 1
                    counts[i] -= 1
                    counts[i - 1] += 1
                    means[i] = means[i] - (x[j] - means[i]) / f32(counts[i])
                    means[i - 1] = means[i - 1] + (x[j] - means[i - 1]) / f32(counts[i - 1])
            if i < k - 1:
                end = int(b[i + 1]) - 1
                begin = end - math.floor(int(counts[i]) / 2 * (1 - delta))
                for j in range(end, begin, -1):
                    if counts[i] <= 1:
                        break
                    d, sc = _dsq(x[j], means[i + 1], means[i], int(counts[i + 1]), int(counts[i]))
                    if stats is not None:
                        stats.append(abs(float(d)) / sc)
                    if not d < 0:
                        break
                    moved = True
                    b[i + 1] -= 1
                    counts[i] -= 1
                    counts[i + 1] += 1
                    means[i] = means[i] - (x[j] - means[i]) / f32(counts[i])
                    means[i + 1] = means[i + 1] + (x[j] - means[i + 1]) / f32(counts[i + 1])
    return means, b, means0, ids, counts0.astype(np.int32), (-2 if moved else sw)


def warped(x, k, init='ts', delta=0.0, key=0, utt=0, boundaries=None, stats=None):
    """One utterance (n, D) -> dict(means (k, D), bnd, init_bnd, init_ids, init_counts, sweeps); raises Degenerate."""
    x = np.asarray(x, dtype=f32)
    n = x.shape[0]
    if boundaries is not None:
        b0 = np.asarray(boundaries, dtype=np.int64)
    elif init == 'ts':
        b0 = ts_boundaries(x, k)
    else:
        b0 = random_boundaries(key, utt, n, k)
    if not valid(b0, n):
        raise Degenerate("initial boundaries do not rise strictly from 0: %s" % b0[:8])
    means, b, _, ids, counts, sw = sweep(x, b0, delta, stats=stats)
    return dict(means=means, bnd=b, init_bnd=b0, init_ids=ids, init_counts=counts, sweeps=sw)


def torch_with_quirk(feat, r):
    """The reference's output as autograd sees it: the value is the final means, the gradient that of the INITIAL segment
    means (feature_level.py:104 builds the graph, :135-136 / :150-151 move the means through `.data`)."""
    segs = [feat[int(a):int(a + c)].mean(dim=0) for a, c in zip(r['init_bnd'], r['init_counts'])]
    m0 = torch.stack(segs)
    return torch.from_numpy(r['means']).to(feat.dtype) + (m0 - m0.detach())
