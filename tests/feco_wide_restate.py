"""numpy float32 restatement of the wide k-means' determinism contract (speakerguard_amd/csrc/k_feco_wide.hip header,
"version 2, wide"): version 2 of oracle/feco.py with the padded width 128 -- ``oracle.feco.centre``, ``half_norms(c, 128)`` and
the C fmaf chain of oracle/conv_chain.c sg_feco_scores at Dp = 128 (called through ``oracle.conv_chain._load()``: the Python
wrapper stops at 64).  Bit for bit what sg_feco_kmeans_compress_wide computes for 65 <= D <= 128.  PARITY UNPINNED by
construction, like the narrow ids: the reference delegates to a randomly initialised third-party k-means.  ``lloyd_f64`` is
the same algorithm in float64 from the same initial frames: what the float32 chain has to agree with on real features."""
import ctypes as C

import numpy as np

from oracle.conv_chain import _load
from oracle.feco import centre, half_norms
from oracle.philox import feco_random_init

f32 = np.float32
PAD = 128


def scores(xp, cp, h):
    """xp (F, Dp), cp (k, Dp), h (k) float32 -> (F, k): the chain from h[j] over Dp columns (any multiple of 8)"""
    xp = np.ascontiguousarray(xp, f32)
    cp = np.ascontiguousarray(cp, f32)
    h = np.ascontiguousarray(h, f32)
    F, Dp = xp.shape
    k = cp.shape[0]
    assert Dp % 8 == 0 and cp.shape[1] == Dp and h.shape == (k,)
    out = np.empty((F, k), f32)
    _load().sg_feco_scores(xp.ctypes.data_as(C.c_void_p), cp.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                           out.ctypes.data_as(C.c_void_p), F, k, Dp)
    return out


def init_frames(F, k, seed=None, utt=0):
    """Even form (seed None): frame floor(j F / k); seeded form: oracle.philox.feco_random_init."""
    if seed is None:
        return np.array([j * F // k for j in range(k)], dtype=np.int64)
    return feco_random_init(seed, utt, F, k)


def _pad(a, lanes):
    out = np.zeros((a.shape[0], lanes), dtype=f32)
    out[:, :a.shape[1]] = a
    return out


def kmeans_ids(x, k, max_iter=10, frames=None, stats=None, lanes=PAD):
    """x (F, D) float32, 65 <= D <= 128 -> int32 ids (F,).  `lanes`: how many columns the chain runs over (the contract: 128;
    any multiple of 8 >= D must give the same ids -- trailing zero groups add nothing); h always comes from the 128-lane
    butterfly.  `stats` (a dict) collects assignment steps, exact ties of the best score and empty clusters."""
    xc, _ = centre(x)
    F, D = xc.shape
    assert 64 < D <= PAD and lanes % 8 == 0 and D <= lanes <= PAD
    xp = _pad(xc, lanes)
    frames = init_frames(F, k) if frames is None else frames
    c = xc[[int(f) for f in frames]].copy()
    st = dict(steps=0, ties=0, empty=0)
    ids = np.full(F, -1, dtype=np.int32)
    for _ in range(max_iter):
        sc = scores(xp, _pad(c, lanes), half_norms(c, PAD))
        new = np.argmax(sc, axis=1).astype(np.int32)  # first maximum: ties to the lowest index
        st['steps'] += 1
        st['ties'] += int(((sc == sc.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        if np.array_equal(new, ids):
            break
        ids = new
        for j in range(k):
            members = np.nonzero(ids == j)[0]
            if members.size == 0:
                st['empty'] += 1
                continue  # keeps its centroid bit for bit
            s = np.zeros(D, dtype=f32)
            for i in members:
                s = s + xc[i]
            c[j] = s / f32(members.size)
    if stats is not None:
        stats.update(st)
    return ids


def compress(x, ids, k):
    """What sg_feco_compress gives for the ids (float32 sums in ascending frame order, the `force` fallback to frame j):
    (out (k, D) float32, counts (k,) int32)."""
    x = np.ascontiguousarray(x, dtype=f32)
    out = np.empty((k, x.shape[1]), dtype=f32)
    counts = np.zeros(k, dtype=np.int32)
    for j in range(k):
        members = np.nonzero(ids == j)[0]
        counts[j] = members.size
        if members.size:
            s = np.zeros(x.shape[1], dtype=f32)
            for i in members:
                s = s + x[i]
            out[j] = s / f32(members.size)
        else:
            out[j] = x[j]
    return out, counts


def lloyd_f64(x, k, max_iter=10, frames=None):
    """The same Lloyd iterations in float64 with plain squared distances: no contract, no chain order, no centring."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    frames = init_frames(F, k) if frames is None else frames
    c = x[[int(f) for f in frames]].copy()
    ids = np.full(F, -1, dtype=np.int32)
    for _ in range(max_iter):
        d2 = (x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :]
        new = np.argmin(d2, axis=1).astype(np.int32)
        if np.array_equal(new, ids):
            break
        ids = new
        for j in range(k):
            members = np.nonzero(ids == j)[0]
            if members.size:
                c[j] = x[members].sum(axis=0) / members.size
    return ids


def iv_features(T, seed, n=4):
    """[('delta', (n, F, 72)), ('cmvn', (n, F, 72))] float32 of n synthetic utterances: oracle MFCC (first 24 cepstra), then
    iv_restate's deltas and CMVN in float32"""
    import torch

    import iv_restate
    from oracle import kaldi_mfcc
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(n, T, seed=seed))
    raw = kaldi_mfcc.mfcc_batch(x * 32768.0).numpy().astype(f32)[:, :, :24]
    delta = iv_restate.add_delta(raw, f32).astype(f32)
    cm = iv_restate.cmvn(delta, f32).astype(f32)
    return [("delta", delta), ("cmvn", cm)]


def degenerate_rows():
    """{name: (x (F, 72), k)}: inputs on which only the contract speaks"""
    rng = np.random.default_rng(11)
    base = (rng.standard_normal((20, 72)) * 3).astype(f32)
    dup = np.tile(base, (4, 1))  # 20 distinct rows 4 x: ties go to the lowest index, empty clusters keep their centroid
    return {"duplicates": (dup, 40), "offset": ((rng.standard_normal((64, 72)) + 300.0).astype(f32), 16),
            "k1": ((rng.standard_normal((33, 72))).astype(f32), 1), "kF": ((rng.standard_normal((37, 72))).astype(f32), 37)}
