"""FeCo feature-level defense on the native engine; mirrors reference defense/feature_level.py:15-50,168-217
(method 'kmeans', distances 'L2' and 'cos').

``FeCo(feat, method, param, other_param)`` keeps the reference's function signature (forward only).
``FeCoDefense`` is the same transform as an object with ``fwd`` / ``bwd`` so that ``defended_model`` can chain
the hand-coded backward through it (adaptive attacks against a FeCo-defended model).

The cluster ids come from the library's k-means (contract in csrc/k_feco.hip); the reference's ids come from a
randomly initialised third-party k-means and are not reproducible, so parity with the reference exists only for
the step after the ids (cluster means + empty-cluster fallback, :204-216).  ``init='even'`` (default) starts from
evenly spaced frames: one input, one output.  ``init='random'`` starts every call from k distinct random frames like
the reference's k-means does -- a randomised defense, the case expectation-over-transformation attacks are for --
with draws that are a function of (key, utterance row) only (Philox4x32-10).  Called on its own, the key is (seed, call
number); inside ``defended_model`` it comes from the base model's noise bookkeeping -- (seed, attack call, restart, GLOBAL
index of the chunk's first utterance, call number inside the chunk), like the MFCC dither -- so an attack is reproducible
and independent of how the batch is cut into per-GPU shards.
Method 'warped_kmeans' (:53-165) is ``WarpedFeCoDefense`` (and the reference-named ``warped_kmeans`` for one utterance):
contiguous segments, boundaries moved frame by frame (contract in csrc/k_feco_warped.hip).  It is not reachable through the
string route ``FeCo(feat, 'warped_kmeans', ...)``, which keeps refusing it.
``other_param='cos'`` is the reference's cosine distance (:174-182) under a contract of its own (csrc/k_feco.hip header,
"cosine": raw frames, unit centroids, largest dot product wins; a zero centroid scores 0 where the reference would give NaN):
same ``init`` / keys / ``max_iter`` / ``force`` handling, same backward (the gradient depends on the ids only).  Like the
reference (:183) it asserts an even feature dimension.  It runs under every attack through the step-by-step route; the
device-resident PGD loops cluster with L2 and refuse it (``FGSM._device_route`` never offers them one).
"""
import ctypes as C

import torch

from .. import _native as N
from ..metric.metric import _context
from ..model._engine_ops import REP_KEY_STRIDE

WIDE_MIN_D = 65  # from this width on the L2 clustering is sg_feco_kmeans_compress_wide (csrc/k_feco_wide.hip; up to 128)


class FeCoDefense:
    # the reference's `force` flag follows the size of the MODEL CALL (feature_level.py:33: feat.shape[0] > 1): a call with
    # one utterance drops empty clusters, a larger one fills them in.  Whoever re-cuts a batch (shard.py) must not turn an
    # utterance of a multi-utterance call into a call of its own, or the other way round.
    batch_coupled = True

    def __init__(self, param=0.5, method='kmeans', other_param='L2', max_iter=10, init='even', seed=0):
        if method != 'kmeans':
            raise NotImplementedError('Currently FEATURE COMPRESSION only supports kmeans on the native engine')
        if other_param not in ('L2', 'cos'):
            raise NotImplementedError("other_param must be 'L2' or 'cos' (:174)")
        if init not in ('even', 'random'):
            raise ValueError("init must be 'even' or 'random'")
        self.param, self.max_iter, self.init, self.seed = param, max_iter, init, int(seed)
        self.other_param = other_param
        self.calls = 0       # fwd calls so far: every call of the randomised defense draws fresh initial frames
        self.index_base = 0  # global index of row 0 (set by sharded callers)

    def call_seed(self, call):
        """Generator key of fwd call number `call` (0-based)."""
        from ..model._engine_ops import mix64
        return mix64(self.seed ^ 0x4665436F, call)

    # ---- forward with saved state ------------------------------------------------------------------
    def fwd(self, feat, seed=None, ids=None, row_keys=None):
        """feat (B,F,D) -> (compressed (B,k,D) [or (1,k',D) with empty clusters dropped when B == 1], saved).
        `seed`: explicit generator key for this call of the randomised defense (tests replay the fused loop's keys).
        `row_keys` = (index_base, row_base, rep_rows) as in sg_dither (speakerguard_hip.h): which global utterance and
        which EOT repeat every row of `feat` is -- repeat r draws from key + r * REP_KEY_STRIDE, like repeat r of the
        device loop (sg_an_pgd_run_feco); default: row b is utterance ``self.index_base + b``.
        `ids` (B,F) int32: cluster ids from elsewhere -- only the reference's step after the clustering runs
        (feature_level.py:204-216; tests/golden/feco_ref.npz pins it against the reference's own code)."""
        feat = feat.to(torch.float32).contiguous()
        if not feat.is_cuda:
            raise N.NativeError("FeCo runs on the HIP device only")
        B, F, D = feat.shape
        if self.other_param == 'cos':
            assert D % 2 == 0  # :183 (kmeans_pytorch's cosine distance)
        k = int(F * self.param)  # :184
        ctx, s = _context(feat.device), N.current_stream_ptr(feat.device)
        out = torch.empty(B, k, D, device=feat.device, dtype=torch.float32)
        counts = torch.empty(B, k, device=feat.device, dtype=torch.int32)
        if ids is not None:
            ids = ids.to(device=feat.device, dtype=torch.int32).contiguous()
            if tuple(ids.shape) != (B, F):
                raise ValueError("ids must have shape (B, F)")
            ctx.call("sg_feco_compress", N._ptr(feat), N._ptr(ids), B, F, D, k, N._ptr(out), N._ptr(counts), s)
        else:
            ids = torch.empty(B, F, device=feat.device, dtype=torch.int32)
            key = 0
            if self.init == 'random':
                key = self.call_seed(self.calls) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
            self.calls += 1
            # clustering + cluster means (:204-216) in one launch per EOT repeat the rows belong to (normally one)
            index_base, row_base, rep_rows = row_keys if row_keys is not None else (self.index_base, 0, 0)
            b0 = 0
            while b0 < B:
                g = row_base + b0
                rep = g // rep_rows if rep_rows > 0 else 0
                u = g - rep * rep_rows
                nb = min(B - b0, rep_rows - u) if rep_rows > 0 else B
                sl = slice(b0, b0 + nb)
                if self.other_param == 'cos':
                    ctx.call("sg_feco_kmeans_compress_metric", N._ptr(feat[sl]), nb, F, D, k, self.max_iter, N.SG_FECO_COS,
                             int(self.init == 'random'), C.c_uint64((key + rep * REP_KEY_STRIDE) & 0xFFFFFFFFFFFFFFFF),
                             int(index_base + u), 1, 0, N._ptr(ids[sl]), N._ptr(out[sl]), N._ptr(counts[sl]), s)
                elif D >= WIDE_MIN_D:  # 65 .. 128 columns (iv_plda's levels 2 and 3): the wide kernel, same keys
                    ctx.call("sg_feco_kmeans_compress_wide", N._ptr(feat[sl]), nb, F, D, k, self.max_iter, int(self.init == 'random'),
                             C.c_uint64((key + rep * REP_KEY_STRIDE) & 0xFFFFFFFFFFFFFFFF), int(index_base + u),
                             N._ptr(ids[sl]), N._ptr(out[sl]), N._ptr(counts[sl]), s)
                else:
                    ctx.call("sg_feco_kmeans_compress", N._ptr(feat[sl]), nb, F, D, k, self.max_iter, int(self.init == 'random'),
                             C.c_uint64((key + rep * REP_KEY_STRIDE) & 0xFFFFFFFFFFFFFFFF), int(index_base + u), 1,
                             N._ptr(ids[sl]), N._ptr(out[sl]), N._ptr(counts[sl]), s)
                b0 += nb
        force = B > 1  # :33 force=feat.shape[0] > 1
        keep = None
        if not force and bool((counts == 0).any()):
            keep = torch.nonzero(counts[0] > 0).flatten()  # :209-212: empty clusters are skipped
            out = out.index_select(1, keep)
        return out, (ids, counts, (B, F, D, k), force, keep)

    def bwd(self, saved, dout):
        ids, counts, (B, F, D, k), force, keep = saved
        dout = dout.to(torch.float32)
        if keep is not None:
            full = torch.zeros(B, k, D, device=dout.device, dtype=torch.float32)
            full.index_copy_(1, keep, dout)
            dout = full
        dout = dout.contiguous()
        dfeat = torch.empty(B, F, D, device=dout.device, dtype=torch.float32)
        _context(dout.device).call("sg_feco_compress_backward", N._ptr(dout), N._ptr(ids), N._ptr(counts), B, F, D, k,
                                   1 if force else 0, N._ptr(dfeat), N.current_stream_ptr(dout.device))
        return dfeat

    def __call__(self, feat):
        return self.fwd(feat)[0]


class WarpedFeCoDefense:
    """FeCo with warped k-means (feature_level.py:53-165): each utterance's F frames cut into k = int(F * param) contiguous
    segments, started from TS (``other_param='ts'``) or from a random cut (``'random'``), the boundaries moved while the
    squared error falls; the output is the k segment means.  ``fwd`` / ``bwd`` chain the gradient like ``FeCoDefense``.

    The reference moves the means through ``.data`` (:135-136, :150-151), so autograd sees only the means of the INITIAL
    segmentation: ``bwd`` returns exactly that gradient (sg_feco_compress_backward with the initial ids and counts).
    ``other_param='random'`` is a randomised defense keyed like ``FeCoDefense(init='random')``: ``init == 'random'`` makes
    ``defended_model`` hand it the base model's keys.  Warped k-means has no ``force``: every utterance is independent."""
    batch_coupled = False

    def __init__(self, param=0.5, other_param='ts', delta=0.0, seed=0):
        if other_param not in ('ts', 'random'):
            raise ValueError("other_param must be 'ts' or 'random' (:160)")
        if not 0.0 <= float(delta) <= 1.0:
            raise ValueError("delta must lie in [0, 1]")
        self.param, self.other_param, self.delta, self.seed = param, other_param, float(delta), int(seed)
        self.init = 'random' if other_param == 'random' else 'ts'
        self.calls = 0       # fwd calls so far: every call of the randomised defense draws fresh initial boundaries
        self.index_base = 0  # global index of row 0 (set by sharded callers)
        self.last_sweeps = None

    def call_seed(self, call):
        """Generator key of fwd call number `call` (0-based)."""
        from ..model._engine_ops import mix64
        return mix64(self.seed ^ 0x5766436F, call)

    def fwd(self, feat, seed=None, row_keys=None, boundaries=None):
        """feat (B,F,D) -> (segment means (B,k,D), saved).  `seed` / `row_keys`: as ``FeCoDefense.fwd`` (random init only).
        `boundaries` (B,k) int: initial boundaries from elsewhere (tests, replaying a reference run); they must rise strictly
        from 0.  Raises ValueError if k = int(F * param) is outside [1, F] or a row's initial boundaries do not rise strictly
        (a degenerate TS init: the reference would return NaN)."""
        feat = feat.to(torch.float32).contiguous()
        if not feat.is_cuda:
            raise N.NativeError("FeCo runs on the HIP device only")
        B, F, D = feat.shape
        k = int(F * self.param)  # :163
        if not 1 <= k <= F:
            raise ValueError("warped k-means needs 1 <= k = int(F * param) <= F (F %d, param %r)" % (F, self.param))
        dev = feat.device
        ctx, s = _context(dev), N.current_stream_ptr(dev)
        out = torch.empty(B, k, D, device=dev, dtype=torch.float32)
        ids = torch.empty(B, F, device=dev, dtype=torch.int32)
        counts = torch.empty(B, k, device=dev, dtype=torch.int32)
        sweeps = torch.empty(B, device=dev, dtype=torch.int32)
        if boundaries is not None:
            bnd = torch.as_tensor(boundaries).to(device=dev, dtype=torch.int32).contiguous().clone()
            if tuple(bnd.shape) != (B, k):
                raise ValueError("boundaries must have shape (B, k) = (%d, %d)" % (B, k))
            chunks = [(0, B, 2, 0, 0, 0)]
        else:
            bnd = torch.empty(B, k, device=dev, dtype=torch.int32)
            if self.init == 'random':
                key = self.call_seed(self.calls) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
                index_base, row_base, rep_rows = row_keys if row_keys is not None else (self.index_base, 0, 0)
                if row_base == 0:
                    chunks = [(0, B, 1, key, index_base, rep_rows)]
                else:  # rows that start inside an EOT repeat: one launch per repeat they belong to
                    chunks, b0 = [], 0
                    while b0 < B:
                        g = row_base + b0
                        rep = g // rep_rows if rep_rows > 0 else 0
                        u = g - rep * rep_rows
                        nb = min(B - b0, rep_rows - u) if rep_rows > 0 else B
                        chunks.append((b0, nb, 1, (key + rep * REP_KEY_STRIDE) & 0xFFFFFFFFFFFFFFFF, index_base + u, 0))
                        b0 += nb
            else:
                chunks = [(0, B, 0, 0, 0, 0)]
            self.calls += 1
        for b0, nb, mode, key, ib, rr in chunks:
            sl = slice(b0, b0 + nb)
            rc = ctx.lib.sg_feco_warped(ctx.handle, N._ptr(feat[sl]), nb, F, D, k, mode, C.c_double(self.delta),
                                        C.c_uint64(key), C.c_int64(int(ib)), int(rr), N._ptr(bnd[sl]), N._ptr(ids[sl]),
                                        N._ptr(counts[sl]), N._ptr(out[sl]), N._ptr(sweeps[sl]), s)
            if rc == 1:  # SG_ERR_ARG: a row's initial boundaries (the call's arguments were checked above)
                raise ValueError(ctx.lib.sg_last_error(ctx.handle).decode())
            ctx.check(rc, "sg_feco_warped")
        self.last_sweeps, self.last_boundaries = sweeps, bnd
        return out, (ids, counts, (B, F, D, k))

    def bwd(self, saved, dout):
        ids, counts, (B, F, D, k) = saved
        dout = dout.to(torch.float32).contiguous()
        dfeat = torch.empty(B, F, D, device=dout.device, dtype=torch.float32)
        # every initial segment has frames, so force = 1 adds nothing: d out_i / d x_f = 1 / count_i for f in segment i
        _context(dout.device).call("sg_feco_compress_backward", N._ptr(dout), N._ptr(ids), N._ptr(counts), B, F, D, k, 1,
                                   N._ptr(dfeat), N.current_stream_ptr(dout.device))
        return dfeat

    def __call__(self, feat):
        return self.fwd(feat)[0]


def warped_kmeans(feat, param=0.5, delta=0., other_param="random"):
    """feature_level.py:157-165 for one utterance: feat (n, dim) on the HIP device -> (k, dim), k = int(n * param)."""
    assert torch.is_tensor(feat)
    if other_param not in ("ts", "random"):
        raise ValueError("other_param must be 'ts' or 'random'")
    d = WarpedFeCoDefense(param=param, other_param=other_param, delta=delta)
    d.calls = _WK_CALLS[0]  # the random form draws afresh on every call, like the reference's np.random.choice
    _WK_CALLS[0] += 1
    return d(feat.unsqueeze(0))[0]


_WK_CALLS = [0]


def FeCo(feat, method='kmeans', param=0.5, other_param='L2'):
    return FEATURE_COMPRESSION(feat, method, param, other_param)


def FEATURE_COMPRESSION(feat, method='kmeans', param=0.5, other_param='L2'):
    return FeCoDefense(param=param, method=method, other_param=other_param)(feat)
