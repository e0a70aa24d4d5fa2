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

import numpy as np
import torch

from .. import _native as N
from ._engine_ops import _f32
from ._plda_model import PldaModel, parse_enroll_model_file, parse_mean_file, parse_plda_file, parse_transform_mat_file

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


class iv_plda(PldaModel):
    """The back end, the enrolled speakers and the scoring API: ``PldaModel``."""
    allowed_flags = [0, 1, 2, 3]  # 0: wav; 1: raw feat; 2: delta feat; 3: cmvn feat (iv_plda.py:75-77)
    _feat_widths = {1: IV_CEPS, 2: IV_DIM, 3: IV_DIM}
    device_loops = False  # no pgd_run*: attack.FGSM._device_route sends every attack to the step loop
    _entry, _fourth = "sg_iv", "want_ivector"  # the fourth output: the raw i-vector (B, R)
    _fourth_width = property(lambda self: self.ivector_dim)

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
        ext = _f32(weights["extractor"])
        Cn, dim, R = ext.shape
        if dim != IV_DIM or _f32(weights["means_invcovars"]).shape != (Cn, IV_DIM):
            raise ValueError("the engine's i-vector front-end is 24 cepstra + deltas: feature dimension must be %d" % IV_DIM)
        w = N.IvWeights()
        self._init_backend(weights, w, threshold, dither, dither_seed, spk_ids, R, hp)
        w.C, w.R = Cn, R
        w.gconsts, w.means_invcovars = hp(weights["gconsts"]), hp(weights["means_invcovars"])
        w.invcovars, w.extractor, w.sigma_inv = hp(weights["invcovars"]), hp(ext), hp(weights["sigma_inv"])
        w.ivector_offset = float(weights["ivector_offset"])
        self.ctx.call("sg_iv_load", C.byref(w))
        self.num_gaussians, self.ivector_dim = Cn, R

    # ------------------------------------------------------------------ plumbing
    def _prep(self, x, flag):
        assert flag in self.allowed_flags
        x = x.to(self.device, torch.float32).contiguous()
        if flag == 0:
            assert x.dim() == 3 and x.shape[1] == 1, "wav input must be (B, 1, T)"
            return x, x.shape[0], x.shape[2]
        width = self._feat_widths[flag]
        assert x.dim() == 3 and x.shape[2] == width, "flag-%d input must be (B, F, %d)" % (flag, width)
        return x, x.shape[0], x.shape[1]

    # ------------------------------------------------------------------ reference API
    def compute_feat(self, x, flag=1, dither_noise=None):
        """wav (B,1,T) -> raw (B,F,24) / delta (B,F,72) / CMVN (B,F,72) features; iv_plda.py:86-109.  The 24-cepstrum MFCC
        is the first 24 columns of the x-vector front-end's 30 (same mel bank, lifter by column index, c0 <- energy)."""
        assert flag in (1, 2, 3)
        feats, _ = self._mfcc(x, dither_noise)
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

    # ---- front-end stages with their backward (used when a feature-level defense sits between them: defended_model) ----
    def frontend_forward(self, x, dither_seed=None):
        """wav (B,1,T) -> (raw features (B,F,24), saved) with the state the backward needs (same scale, same dither).
        `dither_seed`: explicit generator key of this pass's dither."""
        feats, saved = self._mfcc(x, dither_seed=dither_seed)
        return feats[:, :, :IV_CEPS].contiguous(), saved

    def frontend_backward(self, saved, d_raw):
        """d loss / d raw features (B,F,24) -> d loss / d wav (B,1,T): the 24 columns padded into the 30 of the x-vector
        front-end's MFCC adjoint (columns 24 .. 29 do not reach this model), with the forward's scale and dither key."""
        if not getattr(self, "_white_box", False):
            raise NotImplementedError(_NO_GRAD % "frontend_backward")
        x, scale, dz = saved
        B, T = x.shape[0], x.shape[2]
        d_raw, _, F = self._prep(d_raw, 1)
        d30 = torch.zeros(B, F, 30, device=self.device, dtype=torch.float32)
        d30[:, :, :IV_CEPS] = d_raw
        grad = torch.empty_like(x)
        self.ctx.call("sg_xv_mfcc_backward", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(d30), N._ptr(grad), self._stream())
        return grad

    def feat_from_feat_backward(self, dout, ori_flag, des_flag):
        """The adjoint of ``comput_feat_from_feat(., ori_flag, des_flag)`` for one level: d CMVN -> d delta (2, 3), both
        (B,F,72), or d delta -> d raw (B,F,24) (1, 2); sg_iv_delta_cmvn_backward."""
        if not getattr(self, "_white_box", False):
            raise NotImplementedError(_NO_GRAD % "feat_from_feat_backward")
        assert (ori_flag, des_flag) in ((1, 2), (2, 3))
        dout, B, F = self._prep(dout, des_flag)
        if des_flag == 3:
            din = torch.empty(B, F, IV_DIM, device=self.device, dtype=torch.float32)
            self.ctx.call("sg_iv_delta_cmvn_backward", N._ptr(dout), 3, B, F, N._ptr(din), None, self._stream())
        else:
            din = torch.empty(B, F, IV_CEPS, device=self.device, dtype=torch.float32)
            self.ctx.call("sg_iv_delta_cmvn_backward", N._ptr(dout), 2, B, F, None, N._ptr(din), self._stream())
        return din

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

    def ivector(self, x, flag=0):
        """the raw i-vector (B,R), before mean subtraction / LDA / PLDA (parity tests)"""
        return self._forward(x, flag, want_ivector=True)[3]

    # ------------------------------------------------------------------ engine protocol used by attack.*
    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, dither_noise=None, dither_seed=None, lengths=None):
        """make_decision + per-example loss (+ d loss / d x, the shape of x, on a ``white_box=True`` model) in one native call
        -> (decisions, scores, loss, grad or None).  On the default model ``want_grad=True`` raises.  `lengths` (a padded batch
        of unequal lengths) is refused: the i-vector engine takes one length per call."""
        self.refuse_lengths(lengths)
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
