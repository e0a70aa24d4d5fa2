"""Kenan's signal-processing black-box attack, the ``ssa`` variant (reference attack/Kenan.py:28-41, attack/_kenan.py:86-112,
:133-178, :181-291 and attack/ssa_core.py): keep the first k components of a singular spectrum analysis of the int16 utterance
and bisect the kept percentage on the model's decision.  The decomposition runs once per utterance and every query is one
rank-k reconstruction, both native (csrc/k_ssa.hip: integer lag covariance, Jacobi eigenvectors, projector / FIR reconstruction
-- no trajectory matrix, no buffer above W x W); the model is queried through ``make_decision`` only.

Faithfulness notes:
  * the audio is quantised to int16 as attack/Kenan.py:31-34 does it, PER UTTERANCE (the reference sees one utterance at a time);
  * factors are Python floats, from ``raster_width / 2`` in steps of ``abs(min + max) / 2``; a query whose decision DIFFERS from
    the label raises ``min``, any other lowers ``max`` (_kenan.py:139-161 -- also in a targeted run); the rank of a factor is
    ``max(1, int(W * factor / 100))``, W = min(int(0.05 T), 3000), and the loop stops when the next rank equals this one;
  * ``mistranscribed`` changes only on a hit; the returned flag comes from ONE final ``make_decision`` on the result (:288-289),
    it is not sticky; ``early_stop`` is accepted and unused;
  * the model is queried with, and the result returned as, int16-SCALE float32 audio.  The reference returns an int16 ndarray
    (1, 1, T) per utterance; here it is a float32 tensor (N, 1, T) on the input's device holding the same integers;
  * ``batch_size`` is honoured (the reference forces 1): the utterances of a chunk share the native calls, each keeps its own
    bisection and is left out of the queries once complete; an utterance's result equals its ``batch_size=1`` result bit for bit.
    A ``batch_coupled`` model gets chunks of one.  The chunk is capped so that the native workspace (about 3 W^2 float64 per
    utterance) stays below ``workspace_limit`` bytes.
"""
from .utils import refuse_lengths
import ctypes as C

import numpy as np
import torch

from .. import _native as N


def ssa_window(T):
    """W = min(int(0.05 T), 3000) (_kenan.py:97-100); ValueError where the native calls refuse T"""
    w = int(N.load().sg_ssa_window(int(T)))
    if w < 1:
        raise ValueError("the ssa variant needs 20 <= T <= 2^22 (T %d)" % T)
    return w


def ssa_decompose(audio, bits=16, want_cov=False):
    """(N, 1, T) float32 on a GPU -> dict: ``xq`` (N, T) int16, ``eval`` (N, W) and ``evec`` (N, W, W; row j = eigenvector j)
    float64, ``sweeps`` (N,) int32, and with ``want_cov`` the exact lag covariance ``cov`` (N, W, W) float64"""
    if not isinstance(audio, torch.Tensor) or audio.dim() != 3 or audio.shape[1] != 1:
        raise ValueError("the decomposition takes a (N, 1, T) tensor")
    from ..metric.metric import _context
    ctx = _context(audio.device)  # (a CPU tensor: NativeError)
    x = audio.detach().to(torch.float32).contiguous()
    n, T = x.shape[0], x.shape[2]
    W = ssa_window(T)
    dev = x.device
    st = dict(T=T, W=W, xq=torch.empty((n, T), dtype=torch.int16, device=dev),
              eval=torch.empty((n, W), dtype=torch.float64, device=dev),
              evec=torch.empty((n, W, W), dtype=torch.float64, device=dev),
              sweeps=torch.empty((n,), dtype=torch.int32, device=dev),
              cov=torch.empty((n, W, W), dtype=torch.float64, device=dev) if want_cov else None)
    ctx.call("sg_ssa_decompose", N._ptr(x), n, T, int(bits), N._ptr(st["xq"]), N._ptr(st["eval"]), N._ptr(st["evec"]),
             N._ptr(st["sweeps"]), N._ptr(st["cov"]), N.current_stream_ptr(dev))
    return st


def ssa_reconstruct(st, ranks, rows=None, want64=False):
    """the rank-``ranks[i]`` reconstruction of utterance ``rows[i]`` (default: all) of a decomposition -> (len(rows), 1, T)
    float32 holding int16 values; with ``want64`` also the float64 values before the cast (len(rows), T)"""
    from ..metric.metric import _context
    xq, evec = st["xq"], st["evec"]
    ctx = _context(xq.device)
    if rows is not None and list(rows) != list(range(xq.shape[0])):
        idx = torch.as_tensor(list(rows), dtype=torch.int64, device=xq.device)
        xq, evec = xq.index_select(0, idx).contiguous(), evec.index_select(0, idx).contiguous()
    n, T = xq.shape
    ranks = [int(k) for k in ranks]
    if len(ranks) != n:
        raise ValueError("one rank per utterance: %d for %d" % (len(ranks), n))
    k = (C.c_int32 * n)(*ranks)
    out = torch.empty((n, 1, T), dtype=torch.float32, device=xq.device)
    out64 = torch.empty((n, T), dtype=torch.float64, device=xq.device) if want64 else None
    ctx.call("sg_ssa_reconstruct", N._ptr(xq), N._ptr(evec), k, n, T, N._ptr(out), N._ptr(out64), N.current_stream_ptr(xq.device))
    return (out, out64) if want64 else out


def native_decompose(audio, bits=16):
    """-> (state, the quantised audio (N, 1, T) float32): what ``KenanSSA(decompose=)`` stands in for"""
    st = ssa_decompose(audio, bits)
    return st, st["xq"].to(torch.float32).unsqueeze(1)


def native_reconstruct(state, ranks, rows):
    """what ``KenanSSA(reconstruct=)`` stands in for"""
    return ssa_reconstruct(state, ranks, rows)


class KenanSSA(object):

    chunk_coupling = None  # utterances are independent: shard.ShardedAttack may cut anywhere
    workspace_limit = 4 << 30  # bytes of native workspace a chunk may ask for

    def __init__(self, model, max_iter=15, raster_width=100, early_stop=False, targeted=False, verbose=1, BITS=16, batch_size=1, *,
                 decompose=None, reconstruct=None):
        self.model = model  # remember to call model.eval()
        self.atk_name = 'ssa'
        self.max_iter = max_iter
        self.raster_width = raster_width
        self.targeted = targeted
        self.verbose = verbose
        self.BITS = BITS
        self.early_stop = early_stop
        self.batch_size = batch_size
        # decompose(audio (n,1,T), bits) -> (state, quantised audio (n,1,T) float32); reconstruct(state, ranks, rows) ->
        # (len(rows),1,T) float32 of int16 values: the native ones unless given
        self.decompose = native_decompose if decompose is None else decompose
        self.reconstruct = native_reconstruct if reconstruct is None else reconstruct
        self.factor_history = None
        self.rank_history = None
        self.decision_history = None

    def _rank(self, W, factor):
        k = int(W * factor / 100)  # _kenan.py:102-103
        return 1 if k == 0 else k

    def _decide(self, audio):
        d, _ = self.model.make_decision(audio)
        return [int(v) for v in torch.as_tensor(d).reshape(-1).tolist()]

    def atk_bst(self, data, og_label):
        """_kenan.py:181-291 for every utterance of the chunk -> (audio (n,1,T) float32 in int16 scale, success list,
        per utterance the lists of its queries' factors, ranks and decisions)"""
        n, T = data.shape[0], data.shape[2]
        W = min(int(T * 0.05), 3000)
        labels = [int(v) for v in torch.as_tensor(og_label).reshape(-1).tolist()]
        state, quantised = self.decompose(data, self.BITS)
        mistranscribed = quantised.clone()
        lo = [0] * n
        hi = [self.raster_width] * n
        factor = [self.raster_width / 2] * n
        factors, ranks, decisions = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
        active = list(range(n)) if self.max_iter > 0 else []
        itr = 0
        while active:
            k = [self._rank(W, factor[p]) for p in active]
            perturbed = self.reconstruct(state, k, active)
            transcribed = self._decide(perturbed)
            if self.verbose:
                print('Iter: {} ori: {} atk: {} f: {} k: {}'.format(itr + 1, [labels[p] for p in active], transcribed,
                                                                      [factor[p] for p in active], k))
            still = []
            for j, p in enumerate(active):
                factors[p].append(factor[p]), ranks[p].append(k[j]), decisions[p].append(transcribed[j])
                if (labels[p] != transcribed[j] and not self.targeted) or (labels[p] == transcribed[j] and self.targeted):
                    mistranscribed[p] = perturbed[j].to(mistranscribed.device)
                if transcribed[j] != labels[p]:  # bst_atk_factor :139-161: pca / svd / ssa
                    lo[p] = factor[p]
                else:
                    hi[p] = factor[p]
                factor[p] = abs(lo[p] + hi[p]) / 2
                if self._rank(W, factor[p]) != k[j]:  # (complete: the rank would not change)
                    still.append(p)
            itr += 1
            active = still if itr < self.max_iter else []
        final = self._decide(mistranscribed)
        succ = [bool((final[p] != labels[p] and not self.targeted) or (final[p] == labels[p] and self.targeted)) for p in range(n)]
        return mistranscribed, succ, factors, ranks, decisions

    def attack_batch(self, x_batch, y_batch, batch_id, fs=16_000):
        adv, success, factors, ranks, decisions = self.atk_bst(x_batch, y_batch)
        self.factor_history += factors
        self.rank_history += ranks
        self.decision_history += decisions
        return adv, success

    def chunk_size(self, n_audios, T):
        W = max(1, min(int(T * 0.05), 3000))
        fit = max(1, int(self.workspace_limit // (3 * W * W * 8)))
        size = 1 if bool(getattr(self.model, "batch_coupled", False)) else self.batch_size
        return max(1, min(size, n_audios, fit))

    def attack(self, x, y, fs=16_000, lengths=None):
        refuse_lengths(self, lengths)
        n_audios, n_channels, T = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        # per utterance: every query's factor (Python floats), rank and decision, in query order
        self.factor_history, self.rank_history, self.decision_history = [], [], []
        batch_size = self.chunk_size(n_audios, T)
        n_batches = int(np.ceil(n_audios / float(batch_size)))
        for batch_id in range(n_batches):
            x_batch = x[batch_id * batch_size:(batch_id + 1) * batch_size]  # (batch_size, 1, max_len)
            y_batch = y[batch_id * batch_size:(batch_id + 1) * batch_size]
            adver_x_batch, success_batch = self.attack_batch(x_batch, y_batch, batch_id, fs=fs)
            if batch_id == 0:
                adver_x = adver_x_batch
                success = success_batch
            else:
                adver_x = torch.cat((adver_x, adver_x_batch), 0)
                success += success_batch
        return adver_x, success
