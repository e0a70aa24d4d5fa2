"""GMM i-vector + PLDA speaker model on the HIP engine; the gradient is opt-in (``white_box=True``).

Host-side mirror of reference model/iv_plda.py: same constructor files, same method names and argument meaning, same
``allowed_flags`` / ``range_type`` / ``threshold`` / ``spk_ids`` attributes.  All arithmetic runs in
``libspeakerguard_hip.so`` (csrc/k_ivector.hip, csrc/k_ivector_bwd.hip); torch only owns the tensors.

The default model is the decision path -- ``make_decision`` / ``score`` / ``forward`` / ``embedding`` / ``compute_feat`` and
``loss_grad(want_grad=False)`` -- which is all the black-box attacks (FAKEBOB / NES, SirenAttack, Kenan) ask of a model; on it
``loss_grad(want_grad=True)`` raises ``NotImplementedError``.  ``iv_plda(..., white_box=True)`` / ``from_weights(...,
white_box=True)`` enables the hand-coded gradient (``sg_iv_loss_grad``: the adjoint of the tail, the solve, the assembly, the
statistics and softmax, the log-likelihoods, CMVN, deltas and the MFCC) at every flag, so FGSM / PGD / CWinf / CW2 run on it
through their step loop.  It is opt-in because a white-box model keeps per-chunk state a decision query should not pay for:
the solved vector and lambda in float64 and a second (frames, C) buffer.  There is no device-resident loop: ``pgd_run*`` raise
on every instance and ``device_loops = False`` sends the attacks to the step loop over ``loss_grad`` / ``pgd_update``.

Differences a caller can observe, all deliberate: ``dither`` / ``dither_seed`` are constructor arguments keyed exactly as in
``xv_plda`` (default 1.0 like the reference, which draws from the global torch RNG); ``gmm_frame_bs`` is accepted and
ignored (the log-likelihoods are one contraction, chunked by the library); there is no Gaussian pruning, as in the reference.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _native as N
from ._engine_ops import EngineOps, _f32
from .xv_plda import parse_enroll_model_file, parse_mean_file, parse_plda_file, parse_transform_mat_file

BITS = 16
IV_CEPS, IV_DIM = 24, 72
_NO_GRAD = ("the i-vector gradient is not built: iv_plda is a forward-only model (decision-only attacks: FAKEBOB, SirenAttack, "
            "Kenan); %s needs the gradient through the GMM posteriors and the i-vector solve")


# ---------------------------------------------------------------------------- file parsers (Kaldi text)
def _floats(line):
    return [float(t) for t in line.replace("[", " ").replace("]", " ").split()]


def _read_tri(lines, at, n):
    """n lower-triangular rows starting at lines[at] (row j: j + 1 values) -> (full symmetric (n, n), next line index)"""
    m = np.zeros((n, n), dtype=np.float32)
    for j in range(n):
        v = _floats(lines[at + j])
        if len(v) != j + 1:
            raise ValueError("row %d of a packed symmetric matrix holds %d values, expected %d" % (j, len(v), j + 1))
        m[j, :j + 1] = v
        m[:j + 1, j] = v
    return m, at + n


def parse_fgmm_file(path):
    """Kaldi text ``final.ubm`` (format read at reference _iv_plda/gmm.py:32-81) -> dict of float32 arrays: gconsts (C),
    gmm_weights (C), means_invcovars (C, dim), invcovars (C, dim, dim) full symmetric."""
    with open(path) as f:
        lines = f.readlines()
    out, i = {}, 0
    while i < len(lines):
        line = lines[i]
        if "<GCONSTS>" in line:
            out["gconsts"] = np.array(line.split()[2:-1], dtype=np.float32)
        elif "<WEIGHTS>" in line:
            out["gmm_weights"] = np.array(line.split()[2:-1], dtype=np.float32)
        elif "<MEANS_INVCOVARS>" in line:
            n = out["gconsts"].shape[0]
            out["means_invcovars"] = np.array([_floats(l) for l in lines[i + 1:i + 1 + n]], dtype=np.float32)
            i += n
        elif "<INV_COVARS>" in line:
            n, dim = out["means_invcovars"].shape
            mats, at = [], i + 1
            for c in range(n):
                if c:
                    at += 1  # the one filler line between consecutive components
                m, at = _read_tri(lines, at, dim)
                mats.append(m)
            out["invcovars"] = np.stack(mats)
            i = at - 1
        i += 1
    missing = [k for k in ("gconsts", "gmm_weights", "means_invcovars", "invcovars") if k not in out]
    if missing:
        raise ValueError("%s: no %s section" % (path, ", ".join(missing)))
    return out


def parse_ie_file(path):
    """Kaldi text ``final.ie`` (format read at reference _iv_plda/ivector_extract.py:28-70) -> dict: extractor (C, dim, R),
    sigma_inv (C, dim, dim) full symmetric, ivector_offset."""
    with open(path) as f:
        lines = f.readlines()
    out, n, i = {}, None, 0
    while i < len(lines):
        line = lines[i]
        if "<w_vec>" in line:
            n = len(line.split()[2:-1])
        elif "<M>" in line:
            mats, at = [], i + 1
            for c in range(n):
                if c:
                    at += 1
                rows = []
                while True:
                    rows.append(_floats(lines[at]))
                    at += 1
                    if "]" in lines[at - 1]:
                        break
                mats.append(rows)
            out["extractor"] = np.array(mats, dtype=np.float32)
            i = at - 1
        elif "<SigmaInv>" in line:
            dim = out["extractor"].shape[1]
            mats, at = [], i + 1
            for c in range(n):
                if c:
                    at += 1
                m, at = _read_tri(lines, at, dim)
                mats.append(m)
            out["sigma_inv"] = np.stack(mats)
            i = at - 1
        elif "<IvectorOffset>" in line:
            out["ivector_offset"] = np.float32(line.split()[1])
        i += 1
    missing = [k for k in ("extractor", "sigma_inv", "ivector_offset") if k not in out]
    if missing:
        raise ValueError("%s: no %s section" % (path, ", ".join(missing)))
    return out


class iv_plda(EngineOps):
    allowed_flags = [0, 1, 2, 3]  # 0: wav; 1: raw feat; 2: delta feat; 3: cmvn feat (iv_plda.py:75-77)
    range_type = "origin"
    _feat_widths = {1: IV_CEPS, 2: IV_DIM, 3: IV_DIM}
    device_loops = False  # no pgd_run*: attack.FGSM._device_route sends every attack to the step loop

    def __init__(self, fgmm_file, extractor_file, plda_file, mean_file, transform_mat_file, model_file=None, threshold=None,
                 device="cuda:0", gmm_frame_bs=200, dither=1.0, dither_seed=0, white_box=False):
        weights = dict(parse_fgmm_file(fgmm_file))
        weights.update(parse_ie_file(extractor_file))
        weights["plda_mean"], weights["plda_transform"], weights["plda_psi"] = parse_plda_file(plda_file)
        weights["emb_mean"] = parse_mean_file(mean_file)
        weights["lda"] = parse_transform_mat_file(transform_mat_file)
        spk_ids = None
        if model_file is not None:
            spk_ids, self.z_norm_means, self.z_norm_stds, weights["enroll"] = parse_enroll_model_file(model_file)
        self._white_box = bool(white_box)
        self._init(weights, threshold, device, dither, dither_seed, spk_ids)

    @classmethod
    def from_weights(cls, weights, threshold=None, device="cuda:0", dither=1.0, dither_seed=0, white_box=False):
        """Build from in-memory arrays (see speakerguard_amd.synth.make_iv_weights)."""
        self = cls.__new__(cls)
        self._white_box = bool(white_box)
        self._init(weights, threshold, device, dither, dither_seed, None)
        return self

    def _init(self, weights, threshold, device, dither, dither_seed, spk_ids):
        hp = self._open(device)  # host arrays must outlive sg_iv_load
        self.threshold = threshold if threshold else -np.inf  # iv_plda.py:73
        self.dither = float(dither)
        self.dither_seed = int(dither_seed)
        self._draw = 0
        ext = _f32(weights["extractor"])
        Cn, dim, R = ext.shape
        if dim != IV_DIM or _f32(weights["means_invcovars"]).shape != (Cn, IV_DIM):
            raise ValueError("the engine's i-vector front-end is 24 cepstra + deltas: feature dimension must be %d" % IV_DIM)
        lda = _f32(weights["lda"])
        D = lda.shape[0]
        if lda.shape[1] != R + 1:
            raise ValueError("transform matrix must be (D, %d): LDA with offset column (iv_plda.py:430)" % (R + 1))
        enroll = weights.get("enroll")
        self._has_enroll = enroll is not None
        if enroll is None:
            enroll = np.zeros((1, D), np.float32)  # scoring then needs enroll_embs= at call time
        enroll = _f32(enroll).reshape(-1, D)
        w = N.IvWeights()
        w.C, w.R, w.D, w.S = Cn, R, D, enroll.shape[0]
        w.gconsts, w.means_invcovars = hp(weights["gconsts"]), hp(weights["means_invcovars"])
        w.invcovars, w.extractor, w.sigma_inv = hp(weights["invcovars"]), hp(ext), hp(weights["sigma_inv"])
        w.ivector_offset = float(weights["ivector_offset"])
        w.emb_mean, w.lda = hp(weights["emb_mean"]), hp(lda)
        w.plda_mean, w.plda_transform, w.plda_psi = hp(weights["plda_mean"]), hp(weights["plda_transform"]), hp(weights["plda_psi"])
        w.enroll = hp(enroll)
        w.threshold = float(self.threshold) if np.isfinite(self.threshold) else -math.inf
        self.ctx.call("sg_iv_load", C.byref(w))
        self.num_gaussians, self.ivector_dim, self.dim = Cn, R, D
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

    def _prep(self, x, flag):
        assert flag in self.allowed_flags
        x = x.to(self.device, torch.float32).contiguous()
        if flag == 0:
            assert x.dim() == 3 and x.shape[1] == 1, "wav input must be (B, 1, T)"
            return x, x.shape[0], x.shape[2]
        width = self._feat_widths[flag]
        assert x.dim() == 3 and x.shape[2] == width, "flag-%d input must be (B, F, %d)" % (flag, width)
        return x, x.shape[0], x.shape[1]

    def _dither(self, noise=None, seed=None):
        d = N.Dither()
        d.dither = self.dither
        d.index_base, d.row_base, d.rep_rows = self.row_keys()
        d.noise_dev = None if noise is None else noise.data_ptr()
        if seed is not None:
            d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            return d
        d.seed = self.noise_seed(self.dither_seed, self._draw)
        self._draw += 1  # every forward draws fresh noise, like the reference's global RNG
        return d

    def set_enroll(self, enroll_embs=None, threshold=None):
        """Replace the enrolled speakers and/or the decision threshold on the device."""
        if threshold is not None:
            self.threshold = threshold
        thr = float(self.threshold) if np.isfinite(self.threshold) else -math.inf
        if enroll_embs is not None:
            e = _f32(enroll_embs).reshape(-1, self.dim)
            self.ctx.call("sg_iv_set_enroll", e.ctypes.data_as(C.c_void_p), e.shape[0], thr)
            self.enroll_embs = torch.from_numpy(e).to(self.device)
            self.num_spks = e.shape[0]
            self._has_enroll = True
        else:
            self.ctx.call("sg_iv_set_enroll", None, self.num_spks, thr)

    def _enroll_for_call(self, enroll_embs):
        if enroll_embs is None:
            if not self._has_enroll:
                raise AssertionError("no enrolled speakers: pass enroll_embs (iv_plda.py:162-163)")
            return None
        if not isinstance(enroll_embs, torch.Tensor):
            enroll_embs = torch.from_numpy(_f32(enroll_embs))
        return enroll_embs.to(self.device, torch.float32).reshape(-1, self.dim).contiguous()

    # ------------------------------------------------------------------ reference API
    def compute_feat(self, x, flag=1, dither_noise=None):
        """wav (B,1,T) -> raw (B,F,24) / delta (B,F,72) / CMVN (B,F,72) features; iv_plda.py:86-109.  The 24-cepstrum MFCC
        is the first 24 columns of the x-vector front-end's 30 (same mel bank, lifter by column index, c0 <- energy)."""
        assert flag in (1, 2, 3)
        x, B, T = self._prep(x, 0)
        F = N.load().sg_xv_num_frames(T)
        scale = torch.empty(1, device=self.device, dtype=torch.float32)
        feats = torch.empty(B, F, 30, device=self.device, dtype=torch.float32)
        s = self._stream()
        self.ctx.call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), s)
        dz = self._dither(dither_noise)
        self.ctx.call("sg_xv_mfcc", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(feats), s)
        raw = feats[:, :, :IV_CEPS].contiguous()
        return raw if flag == 1 else self.comput_feat_from_feat(raw, 1, flag)

    def comput_feat_from_feat(self, feats, ori_flag=1, des_flag=2):
        """(sic, name as at iv_plda.py:112) raw -> delta / CMVN, delta -> CMVN"""
        assert ori_flag in (1, 2) and des_flag in (2, 3) and des_flag > ori_flag
        feats, B, F = self._prep(feats, ori_flag)
        out = torch.empty(B, F, IV_DIM, device=self.device, dtype=torch.float32)
        if ori_flag == 1:
            delta, cmvn = (out, None) if des_flag == 2 else (None, out)
            self.ctx.call("sg_iv_delta_cmvn", N._ptr(feats), B, F, IV_CEPS, N._ptr(delta), N._ptr(cmvn), self._stream())
            return out
        # delta -> CMVN: a delta row read as a raw row of width 72 gives itself back in column block 0; the CMVN of the kernel
        # acts column by column, so the CMVN of the 72 columns is its first block over three passes of 24 columns each
        parts = []
        for blk in range(3):
            cm = torch.empty(B, F, IV_DIM, device=self.device, dtype=torch.float32)
            src = feats[:, :, blk * IV_CEPS:]
            self.ctx.call("sg_iv_delta_cmvn", C.c_void_p(src.data_ptr()), B, F, IV_DIM, None, N._ptr(cm), self._stream())
            parts.append(cm[:, :, :IV_CEPS])
        return torch.cat(parts, 2).contiguous()

    def add_delta(self, feats):
        return self.comput_feat_from_feat(feats, 1, 2)

    def cmvn(self, feats):
        return self.comput_feat_from_feat(feats, 2, 3)

    def stats(self, feats):
        """Zeroth_First_Stats of CMVN features (B,F,72) -> (zeroth (B,C), first (B,C,72)); _iv_plda/gmm.py:166-171"""
        feats, B, F = self._prep(feats, 3)
        n = torch.empty(B, self.num_gaussians, device=self.device, dtype=torch.float32)
        f = torch.empty(B, self.num_gaussians, IV_DIM, device=self.device, dtype=torch.float32)
        self.ctx.call("sg_iv_stats", N._ptr(feats), B, F, N._ptr(n), N._ptr(f), self._stream())
        return n, f

    def extract(self, zeroth, first):
        """Extractivector on statistics -> raw i-vectors (B,R); _iv_plda/ivector_extract.py:98-114"""
        zeroth = zeroth.to(self.device, torch.float32).contiguous()
        first = first.to(self.device, torch.float32).contiguous()
        B = zeroth.shape[0]
        assert zeroth.shape == (B, self.num_gaussians) and first.shape == (B, self.num_gaussians, IV_DIM)
        w = torch.empty(B, self.ivector_dim, device=self.device, dtype=torch.float32)
        self.ctx.call("sg_iv_extract", N._ptr(zeroth), N._ptr(first), B, N._ptr(w), self._stream())
        return w

    def _forward(self, x, flag, want_emb=False, want_ivector=False, dither_noise=None, enroll=None, dither_seed=None):
        x, B, TF = self._prep(x, flag)
        n_spk = self.num_spks if enroll is None else enroll.shape[0]
        dec = torch.empty(B, device=self.device, dtype=torch.int64)
        scores = torch.empty(B, n_spk, device=self.device, dtype=torch.float32)
        emb = torch.empty(B, self.dim, device=self.device, dtype=torch.float32) if want_emb else None
        ivec = torch.empty(B, self.ivector_dim, device=self.device, dtype=torch.float32) if want_ivector else None
        dz = self._dither(dither_noise, dither_seed)
        if enroll is not None:
            self.ctx.call("sg_iv_enroll_override", N._ptr(enroll), enroll.shape[0])
        try:
            self.ctx.call("sg_iv_forward", N._ptr(x), B, TF, flag, C.byref(dz), N._ptr(dec), N._ptr(scores), N._ptr(emb),
                          N._ptr(ivec), self._stream())
        finally:
            if enroll is not None:
                self.ctx.call("sg_iv_enroll_override", None, 0)
                enroll.record_stream(torch.cuda.current_stream(self.device))
        return dec, scores, emb, ivec

    def embedding(self, x, flag=0):
        return self._forward(x, flag, want_emb=True)[2]

    def ivector(self, x, flag=0):
        """the raw i-vector (B,R), before mean subtraction / LDA / PLDA (parity tests)"""
        return self._forward(x, flag, want_ivector=True)[3]

    def forward(self, x, flag=0, return_emb=False, enroll_embs=None, dither_seed=None):
        enroll = self._enroll_for_call(enroll_embs)
        _, scores, emb, _ = self._forward(x, flag, want_emb=return_emb, enroll=enroll, dither_seed=dither_seed)
        return (scores, emb) if return_emb else scores

    __call__ = forward

    def score(self, x, flag=0, enroll_embs=None):
        return self.forward(x, flag=flag, enroll_embs=enroll_embs)

    def make_decision(self, x, flag=0, enroll_embs=None):
        """-> (decisions int64 (B,), scores (B, n_spk)); iv_plda.py:182-194."""
        enroll = self._enroll_for_call(enroll_embs)
        dec, scores, _, _ = self._forward(x, flag, enroll=enroll)
        return dec, scores

    # ------------------------------------------------------------------ engine protocol used by attack.*
    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, dither_noise=None, dither_seed=None):
        """make_decision + per-example loss (+ d loss / d x, the shape of x, on a ``white_box=True`` model) in one native call
        -> (decisions, scores, loss, grad or None).  On the default model ``want_grad=True`` raises."""
        if want_grad and not getattr(self, "_white_box", False):
            raise NotImplementedError(_NO_GRAD % "loss_grad(want_grad=True)")
        x, y, B, TF, outs = self._loss_grad_args(x, y, loss_spec, flag, want_grad)
        dz = self._dither(dither_noise, dither_seed)
        spec = loss_spec.native()
        if want_grad:
            self.ctx.call("sg_iv_loss_grad", N._ptr(x), N._ptr(y), B, TF, flag, C.byref(spec), C.byref(dz),
                          *[N._ptr(t) for t in outs], self._stream())
            return outs
        self.ctx.call("sg_iv_loss", N._ptr(x), N._ptr(y), B, TF, flag, C.byref(spec), C.byref(dz),
                      *[N._ptr(t) for t in outs[:3]], self._stream())
        return outs

    def pgd_run(self, *args, **kwargs):
        raise NotImplementedError(_NO_GRAD % "pgd_run (FGSM / PGD)")

    def pgd_run_defended(self, *args, **kwargs):
        raise NotImplementedError(_NO_GRAD % "pgd_run_defended")

    def pgd_run_feco(self, *args, **kwargs):
        raise NotImplementedError(_NO_GRAD % "pgd_run_feco")
