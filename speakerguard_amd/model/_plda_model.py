"""What ``xv_plda`` and ``iv_plda`` share on the host: the Kaldi text parsers of the back-end files, the enrolled-speaker
bookkeeping, the dither draws, the MFCC front-end call and the scoring API (``forward`` / ``score`` / ``make_decision`` /
``embedding``) over each model's ``<_entry>_forward`` / ``_set_enroll`` / ``_enroll_override`` (the PLDA back end of
csrc/plda_backend.hip)."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _native as N
from ._engine_ops import EngineOps, _f32


# ---------------------------------------------------------------------------- file parsers
def parse_mean_file(path):
    """Kaldi text vector `` [ v0 v1 ... ]`` (format read at reference model/utils.py:50-60)."""
    with open(path) as f:
        toks = f.readline().split()
    return np.array([float(t) for t in toks[1:-1]], dtype=np.float32)


def parse_transform_mat_file(path):
    """Kaldi text matrix: `` [`` then one row per line, last row closed by ``]`` (model/utils.py:63-80)."""
    rows = []
    with open(path) as f:
        for line in f.readlines()[1:]:
            toks = line.replace("]", " ").split()
            if toks:
                rows.append([float(t) for t in toks])
    return np.array(rows, dtype=np.float32)


def parse_plda_file(path):
    """Kaldi text PLDA: ``<Plda> [ mean ]``, matrix, `` [ psi ]`` (model/_xv_plda/plda.py:27-49)."""
    with open(path) as f:
        lines = f.readlines()
    mean = np.array([float(t) for t in lines[0].split()[2:-1]], dtype=np.float32)
    D = mean.shape[0]
    rows = []
    for line in lines[2:2 + D]:
        rows.append([float(t) for t in line.replace("]", " ").split()])
    psi = np.array([float(t) for t in lines[2 + D].split()[1:-1]], dtype=np.float32)
    return mean, np.array(rows, dtype=np.float32), psi


def parse_enroll_model_file(path):
    """Rows ``id path znorm_mean znorm_std``; each path holds a (1, D) tensor (model/utils.py:21-47)."""
    info = np.loadtxt(path, dtype=str, comments=None)
    if info.ndim == 1:
        info = info[np.newaxis, :]
    spk_ids = list(info[:, 0])
    z_means = info[:, 2].astype(np.float32)
    z_stds = info[:, 3].astype(np.float32)
    embs = [torch.load(p, map_location="cpu").reshape(1, -1).float().numpy() for p in info[:, 1]]
    return spk_ids, z_means, z_stds, np.concatenate(embs, 0)


class PldaModel(EngineOps):
    """A model names its C entries' prefix (``_entry``: "sg_xv" / "sg_iv"), the keyword of ``_forward``'s fourth output
    (``_fourth``: "want_tdnn" / "want_ivector") and that output's width (``_fourth_width``)."""
    range_type = "origin"

    def _thr(self):
        return float(self.threshold) if np.isfinite(self.threshold) else -math.inf

    def _init_backend(self, weights, w, threshold, dither, dither_seed, spk_ids, emb_width, hp):
        """The half of ``_init`` the models share: threshold and dither attributes, the (D, emb_width + 1) LDA check, the
        placeholder enroll table, the back-end fields of the weight struct `w` (same names in XvWeights and IvWeights) and the
        mirrored torch attributes.  The model fills its own fields and makes the ``<_entry>_load`` call."""
        self.threshold = threshold if threshold else -np.inf  # iv_plda.py:73
        self.dither = float(dither)
        self.dither_seed = int(dither_seed)
        self._draw = 0
        lda = _f32(weights["lda"])
        D = lda.shape[0]
        if lda.shape[1] != emb_width + 1:
            raise ValueError("transform matrix must be (D, %d): LDA with offset column (iv_plda.py:430)" % (emb_width + 1))
        enroll = weights.get("enroll")
        self._has_enroll = enroll is not None
        if enroll is None:
            enroll = np.zeros((1, D), np.float32)  # scoring then needs enroll_embs= at call time
        enroll = _f32(enroll).reshape(-1, D)
        w.D, w.S = D, enroll.shape[0]
        w.emb_mean, w.lda = hp(weights["emb_mean"]), hp(lda)
        w.plda_mean, w.plda_transform, w.plda_psi = hp(weights["plda_mean"]), hp(weights["plda_transform"]), hp(weights["plda_psi"])
        w.enroll = hp(enroll)
        w.threshold = self._thr()
        self.dim = D
        self.num_spks = enroll.shape[0]
        self.spk_ids = spk_ids if spk_ids is not None else [str(i) for i in range(self.num_spks)]
        self.enroll_embs = torch.from_numpy(enroll).to(self.device)
        self.emb_mean = torch.from_numpy(_f32(weights["emb_mean"])).to(self.device)
        self.transform_mat = torch.from_numpy(lda).to(self.device)

    # ------------------------------------------------------------------ plumbing
    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device and torch.device(device).index not in (None, self.device.index):
            raise N.NativeError("the engine context is bound to %s" % self.device)
        return self

    def next_dither_seed(self):
        """Draws the generator key the next pass would use (and advances the draw counter like that pass would)."""
        key = self.noise_seed(self.dither_seed, self._draw)
        self._draw += 1
        return key

    def _dither(self, noise=None, seed=None):
        d = N.Dither()
        d.dither = self.dither
        # global utterance index of row 0, offset inside the full call (shard.QueryShardedModel), rows per EOT repeat
        d.index_base, d.row_base, d.rep_rows = self.row_keys()
        d.noise_dev = None if noise is None else noise.data_ptr()
        if seed is not None:  # explicit generator key (tests re-play the fused loop's per-pass seeds)
            d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            return d
        d.seed = self.next_dither_seed()  # every forward draws fresh noise, like the reference's global RNG
        return d

    def set_enroll(self, enroll_embs=None, threshold=None):
        """Replace the enrolled speakers and/or the decision threshold on the device."""
        if threshold is not None:
            self.threshold = threshold
        if enroll_embs is not None:
            e = _f32(enroll_embs).reshape(-1, self.dim)
            self.ctx.call(self._entry + "_set_enroll", e.ctypes.data_as(C.c_void_p), e.shape[0], self._thr())
            self.enroll_embs = torch.from_numpy(e).to(self.device)
            self.num_spks = e.shape[0]
            self._has_enroll = True
        else:
            self.ctx.call(self._entry + "_set_enroll", None, self.num_spks, self._thr())

    def _enroll_for_call(self, enroll_embs):
        """Device table (S, D) for a per-call ``enroll_embs=`` override, or None for the model's own set."""
        if enroll_embs is None:
            if not self._has_enroll:
                raise AssertionError("no enrolled speakers: pass enroll_embs (iv_plda.py:162-163)")
            return None
        if not isinstance(enroll_embs, torch.Tensor):
            enroll_embs = torch.from_numpy(_f32(enroll_embs))
        return enroll_embs.to(self.device, torch.float32).reshape(-1, self.dim).contiguous()

    def _mfcc(self, x, dither_noise=None, dither_seed=None):
        """wav (B,1,T) -> (raw MFCC (B,F,30), (x, scale, dz)): the call's scale decision, one dither draw, the x-vector
        front-end's MFCC (both models' front end); the second value is what ``sg_xv_mfcc_backward`` needs again."""
        x, B, T = self._prep(x, 0)
        F = N.load().sg_xv_num_frames(T)
        scale = torch.empty(1, device=self.device, dtype=torch.float32)
        feats = torch.empty(B, F, 30, device=self.device, dtype=torch.float32)
        s = self._stream()
        self.ctx.call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), s)
        dz = self._dither(dither_noise, dither_seed)
        self.ctx.call("sg_xv_mfcc", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(feats), s)
        return feats, (x, scale, dz)

    # ------------------------------------------------------------------ reference API
    def _forward(self, x, flag, want_emb=False, dither_noise=None, enroll=None, dither_seed=None, lengths=None, **want):
        """-> (decisions, scores, embedding or None, the model's fourth output or None: asked for by its keyword ``_fourth``).
        `lengths`: x is a padded batch of unequal lengths (``EngineOps._lengths_args``; the x-vector model only)."""
        want_fourth = want.pop(self._fourth, False)
        if want:
            raise TypeError("_forward() got an unexpected keyword argument %r" % sorted(want)[0])
        x, B, TF = self._prep(x, flag)
        if lengths is not None:
            if dither_noise is not None:
                raise ValueError("an explicit dither tensor is not supported with lengths=")
            lengths = self._lengths_args(lengths, B, TF, flag)
        n_spk = self.num_spks if enroll is None else enroll.shape[0]
        dec = torch.empty(B, device=self.device, dtype=torch.int64)
        scores = torch.empty(B, n_spk, device=self.device, dtype=torch.float32)
        emb = torch.empty(B, self.dim, device=self.device, dtype=torch.float32) if want_emb else None
        fourth = torch.empty(B, self._fourth_width, device=self.device, dtype=torch.float32) if want_fourth else None
        dz = self._dither(dither_noise, dither_seed)
        if enroll is not None:
            self.ctx.call(self._entry + "_enroll_override", N._ptr(enroll), enroll.shape[0])
        try:
            if lengths is None:
                self.ctx.call(self._entry + "_forward", N._ptr(x), B, TF, flag, C.byref(dz), N._ptr(dec), N._ptr(scores), N._ptr(emb),
                              N._ptr(fourth), self._stream())
            else:
                self.ctx.call(self._entry + "_forward_ragged", N._ptr(x), N._ptr(lengths[0]), lengths[1].ctypes.data_as(C.c_void_p), B, TF,
                              C.byref(dz), N._ptr(dec), N._ptr(scores), N._ptr(emb), N._ptr(fourth), self._stream())
        finally:
            if enroll is not None:
                self.ctx.call(self._entry + "_enroll_override", None, 0)
                enroll.record_stream(torch.cuda.current_stream(self.device))  # the pass may still be reading it
        return dec, scores, emb, fourth

    def embedding(self, x, flag=0):
        return self._forward(x, flag, want_emb=True)[2]

    def forward(self, x, flag=0, return_emb=False, enroll_embs=None, dither_seed=None, lengths=None):
        """`lengths`: x is a padded batch (B, 1, T_max) of utterances of unequal lengths, int32 sample counts (B,): row b is scored as
        utterance b alone at its own length (the x-vector model; ``audio_io.pad_batch`` builds both).  `enroll_embs`: a per-call table, as in the reference (iv_plda.py:155-165); `dither_seed`: explicit generator key of
        this pass's dither (a caller that scores an input and then asks ``loss_grad`` for the gradient of the SAME noise
        realisation passes one key to both: defended_model 'average')."""
        enroll = self._enroll_for_call(enroll_embs)
        _, scores, emb, _ = self._forward(x, flag, want_emb=return_emb, enroll=enroll, dither_seed=dither_seed, lengths=lengths)
        return (scores, emb) if return_emb else scores

    __call__ = forward

    def score(self, x, flag=0, enroll_embs=None, lengths=None):
        return self.forward(x, flag=flag, enroll_embs=enroll_embs, lengths=lengths)

    def make_decision(self, x, flag=0, enroll_embs=None, lengths=None):
        """-> (decisions int64 (B,), scores (B, n_spk)); iv_plda.py:182-194.  `lengths`: see ``forward``."""
        enroll = self._enroll_for_call(enroll_embs)
        dec, scores, _, _ = self._forward(x, flag, enroll=enroll, lengths=lengths)
        return dec, scores
