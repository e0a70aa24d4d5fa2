"""numpy float32 restatement of the cosine k-means' determinism contract (speakerguard_amd/csrc/k_feco.hip header,
"cosine"): raw frames, unit centroids, score = the C fmaf chain of oracle/conv_chain.c sg_feco_scores started at h = 0.
Bit for bit what sg_feco_kmeans_compress_metric(SG_FECO_COS) computes.  PARITY UNPINNED by construction, like the L2
ids (oracle/feco.py): the reference delegates to a randomly initialised kmeans_pytorch.  ``lloyd_f64`` is the same
algorithm in float64 from the same initial frames: what the float32 chain has to agree with on real features."""
import numpy as np

from oracle.conv_chain import feco_scores
from oracle.philox import feco_random_init

f32 = np.float32
REP_KEY = 0xC2B2AE3D27D4EB4F  # per-repeat stride of the generator key


def dpad(D):
    return 32 if D <= 32 else 64


def tree_sum(v, dp):
    """(k, D) float32 -> (k,): the butterfly s[d] += s[d ^ 1], s[d ^ 2], ... s[d ^ dp/2] over dp zero-padded lanes, lane 0."""
    s = np.zeros((v.shape[0], dp), dtype=f32)
    s[:, :v.shape[1]] = v
    idx = np.arange(dp)
    step = 1
    while step < dp:
        s = s + s[:, idx ^ step]
        step *= 2
    return s[:, 0]


def unit_rows(m, dp):
    """Centroid rows as stored: m / sqrtf(tree sum of the rounded squares), 0 where that sum is 0.  Returns (rows, sums)."""
    m = np.ascontiguousarray(m, dtype=f32)
    n = tree_sum(m * m, dp)
    r = np.sqrt(n).astype(f32)  # correctly rounded
    out = np.zeros_like(m)
    nz = n > 0
    out[nz] = m[nz] / r[nz, None]
    return out, n


def init_frames(F, k, seed=None, utt=0):
    """Even form (seed None): frame floor(j F / k); seeded form: oracle.philox.feco_random_init."""
    if seed is None:
        return np.array([j * F // k for j in range(k)], dtype=np.int64)
    return feco_random_init(seed, utt, F, k)


def kmeans_ids(x, k, max_iter=10, frames=None, stats=None):
    """x (F, D) float32 -> int32 ids (F,).  `stats` (a dict) collects what a test wants to know about the run: assignment
    steps, exact ties of the best score, zero-norm centroids, empty clusters."""
    x = np.ascontiguousarray(x, dtype=f32)
    F, D = x.shape
    dp = dpad(D)
    xp = np.zeros((F, dp), dtype=f32)
    xp[:, :D] = x
    frames = init_frames(F, k) if frames is None else frames
    c, n = unit_rows(x[[int(f) for f in frames]], dp)
    st = dict(steps=0, ties=0, zero_norm=int((n == 0).sum()), empty=0)
    ids = np.full(F, -1, dtype=np.int32)
    zero = np.zeros(k, dtype=f32)
    for _ in range(max_iter):
        cp = np.zeros((k, dp), dtype=f32)
        cp[:, :D] = c
        sc = feco_scores(xp, cp, zero)
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
                continue  # keeps its row bit for bit
            s = np.zeros(D, dtype=f32)
            for i in members:
                s = s + x[i]
            row, nj = unit_rows((s / f32(members.size))[None, :], dp)
            st['zero_norm'] += int(nj[0] == 0)
            c[j] = row[0]
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
    """The same Lloyd iterations in float64 with plain dot products and norms: no contract, no chain order."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    frames = init_frames(F, k) if frames is None else frames

    def unit(m):
        r = np.sqrt((m * m).sum(axis=-1, keepdims=True))
        return np.divide(m, r, out=np.zeros_like(m), where=r > 0)

    c = unit(x[[int(f) for f in frames]])
    ids = np.full(F, -1, dtype=np.int32)
    for _ in range(max_iter):
        new = np.argmax(x @ c.T, axis=1).astype(np.int32)
        if np.array_equal(new, ids):
            break
        ids = new
        for j in range(k):
            members = np.nonzero(ids == j)[0]
            if members.size:
                c[j] = unit(x[members].sum(axis=0) / members.size)
    return ids
