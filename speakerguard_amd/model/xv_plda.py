"""x-vector + PLDA speaker model on the HIP engine.

Host-side mirror of reference model/xv_plda.py (and the methods it inherits from
model/iv_plda.py): same constructor files, same method names and argument meaning, same
``allowed_flags`` / ``range_type`` / ``threshold`` / ``spk_ids`` attributes, so that
``attack.*`` and ``defended_model`` callers keep working.  All arithmetic runs in
``libspeakerguard_hip.so``; torch only owns the tensors.

Differences a caller can observe, all deliberate:
  * ``dither`` is an explicit constructor argument (reference hard-codes 1.0 at xv_plda.py:119 and
    draws from the global torch RNG).  Default 1.0 like the reference; the noise comes from a
    counter-based generator keyed by ``dither_seed`` so runs are reproducible.  Use ``dither=0`` for
    bit-reproducible decisions.
  * ``enroll_embs=`` of forward / score / make_decision is a per-call override exactly as in the reference
    (iv_plda.py:155-165): the call scores against the given table, ``self.enroll_embs`` / ``num_spks`` and every
    later call are unaffected (``sg_xv_enroll_override``: no allocation, no synchronisation).
  * gradients come from ``loss_grad`` (hand-coded backward), not from ``loss.backward()``;
    outputs of ``make_decision`` carry no autograd graph.
"""
import ctypes as C
import math
import types

import numpy as np
import torch

from .. import _native as N
from ._engine_ops import EngineOps, _f32

BITS = 16
_TDNN = ("tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5")


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


class xv_plda(EngineOps):
    allowed_flags = [0, 1, 2]  # 0: wav; 1: raw feat; 2: cmvn feat (xv_plda.py:45-47)
    range_type = "origin"
    _feat_width = 30
    _debug_activation = "sg_xv_debug_activation"

    def __init__(self, extractor_file, plda_file, mean_file, transform_mat_file, model_file=None,
                 threshold=None, device="cuda:0", dither=1.0, dither_seed=0):
        sd = torch.load(extractor_file, map_location="cpu") if isinstance(extractor_file, str) else extractor_file
        weights = {"state_dict": {k: v for k, v in sd.items()}}
        weights["plda_mean"], weights["plda_transform"], weights["plda_psi"] = parse_plda_file(plda_file)
        weights["emb_mean"] = parse_mean_file(mean_file)
        weights["lda"] = parse_transform_mat_file(transform_mat_file)
        spk_ids = None
        if model_file is not None:
            spk_ids, self.z_norm_means, self.z_norm_stds, weights["enroll"] = parse_enroll_model_file(model_file)
        self._init(weights, threshold, device, dither, dither_seed, spk_ids)

    @classmethod
    def from_weights(cls, weights, threshold=None, device="cuda:0", dither=1.0, dither_seed=0):
        """Build from in-memory arrays (see speakerguard_amd.synth.make_xv_weights)."""
        self = cls.__new__(cls)
        self._init(weights, threshold, device, dither, dither_seed, None)
        return self

    def _init(self, weights, threshold, device, dither, dither_seed, spk_ids):
        hp = self._open(device)  # host arrays must outlive sg_xv_load
        self.threshold = threshold if threshold else -np.inf  # xv_plda.py:41
        self.dither = float(dither)
        self.dither_seed = int(dither_seed)
        self._draw = 0
        sd = weights["state_dict"]
        w = N.XvWeights()
        for l, name in enumerate(_TDNN):
            w.tdnn_weight[l] = hp(sd[name + ".weight"])
            w.tdnn_bias[l] = hp(sd[name + ".bias"])
            w.bn_mean[l] = hp(sd["bn_" + name + ".running_mean"])
            w.bn_var[l] = hp(sd["bn_" + name + ".running_var"])
        w.fc1_weight, w.fc1_bias = hp(sd["fc1.weight"]), hp(sd["fc1.bias"])
        lda = _f32(weights["lda"])
        D = lda.shape[0]
        if lda.shape[1] != 513:
            raise ValueError("transform matrix must be (D, 513): LDA with offset column (iv_plda.py:430)")
        enroll = weights.get("enroll")
        if enroll is None:
            enroll = np.zeros((1, D), np.float32)  # scoring then needs enroll_embs= at call time
            self._has_enroll = False
        else:
            self._has_enroll = True
        enroll = _f32(enroll).reshape(-1, D)
        w.emb_mean, w.lda = hp(weights["emb_mean"]), hp(lda)
        w.plda_mean, w.plda_transform, w.plda_psi = hp(weights["plda_mean"]), hp(weights["plda_transform"]), hp(weights["plda_psi"])
        w.enroll = hp(enroll)
        w.D, w.S, w.bn_eps = D, enroll.shape[0], 1e-5
        w.threshold = float(self.threshold) if np.isfinite(self.threshold) else -math.inf
        self.ctx.call("sg_xv_load", C.byref(w))
        self.dim = D
        self.num_spks = enroll.shape[0]
        self.spk_ids = spk_ids if spk_ids is not None else [str(i) for i in range(self.num_spks)]
        self.enroll_embs = torch.from_numpy(enroll).to(self.device)
        self.emb_mean = torch.from_numpy(_f32(weights["emb_mean"])).to(self.device)
        self.transform_mat = torch.from_numpy(lda).to(self.device)

    # ------------------------------------------------------------------ plumbing
    def eval(self):
        return self

    def configure_frontend(self, fft_bits=32):
        """Precision of the MFCC's 512-point transforms on the engine (sg_xv_configure): 32 = float32, the reference's own
        (torchaudio 0.6's kaldi.mfcc is float32 end to end, xv_plda.py:114-148) and the default; 64 = float64 transforms
        around the same float32 stages, the form of rounds 1-5 kept as the counterpart."""
        self.ctx.call("sg_xv_configure", int(fft_bits))
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
            self.ctx.call("sg_xv_set_enroll", e.ctypes.data_as(C.c_void_p), e.shape[0], thr)
            self.enroll_embs = torch.from_numpy(e).to(self.device)
            self.num_spks = e.shape[0]
            self._has_enroll = True
        else:
            self.ctx.call("sg_xv_set_enroll", None, self.num_spks, thr)

    def _enroll_for_call(self, enroll_embs):
        """Device table (S, D) for a per-call ``enroll_embs=`` override, or None for the model's own set."""
        if enroll_embs is None:
            if not self._has_enroll:
                raise AssertionError("no enrolled speakers: pass enroll_embs (iv_plda.py:162-163)")
            return None
        if not isinstance(enroll_embs, torch.Tensor):
            enroll_embs = torch.from_numpy(_f32(enroll_embs))
        return enroll_embs.to(self.device, torch.float32).reshape(-1, self.dim).contiguous()

    # ------------------------------------------------------------------ reference API
    def compute_feat(self, x, flag=1, dither_noise=None):
        """wav (B,1,T) -> raw MFCC (flag 1) or CMVN features (flag 2); xv_plda.py:51-67."""
        assert flag in (1, 2)
        x, B, T = self._prep(x, 0)
        F = N.load().sg_xv_num_frames(T)
        scale = torch.empty(1, device=self.device, dtype=torch.float32)
        feats = torch.empty(B, F, 30, device=self.device, dtype=torch.float32)
        s = self._stream()
        self.ctx.call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), s)
        dz = self._dither(dither_noise)
        self.ctx.call("sg_xv_mfcc", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(feats), s)
        return feats if flag == 1 else self.comput_feat_from_feat(feats, 1, 2)

    # ---- front-end stages with their backward (used when a feature-level defense sits between them) ----
    def frontend_forward(self, x, dither_seed=None):
        """wav (B,1,T) -> (raw MFCC (B,F,30), saved) with the state the backward needs (same scale, same dither).
        `dither_seed`: explicit generator key of this pass's dither (tests replay the device loop's per-pass keys)."""
        x, B, T = self._prep(x, 0)
        F = N.load().sg_xv_num_frames(T)
        scale = torch.empty(1, device=self.device, dtype=torch.float32)
        feats = torch.empty(B, F, 30, device=self.device, dtype=torch.float32)
        s = self._stream()
        self.ctx.call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), s)
        dz = self._dither(None, dither_seed)
        self.ctx.call("sg_xv_mfcc", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(feats), s)
        return feats, (x, scale, dz)

    def frontend_backward(self, saved, dfeats):
        """d loss / d raw MFCC (B,F,30) -> d loss / d wav (B,1,T)."""
        x, scale, dz = saved
        B, T = x.shape[0], x.shape[2]
        dfeats = dfeats.to(self.device, torch.float32).contiguous()
        grad = torch.empty_like(x)
        self.ctx.call("sg_xv_mfcc_backward", N._ptr(x), B, T, N._ptr(scale), C.byref(dz), N._ptr(dfeats), N._ptr(grad),
                      self._stream())
        return grad

    def cmvn_backward(self, dout):
        dout, B, F = self._prep(dout, 1)
        din = torch.empty_like(dout)
        self.ctx.call("sg_xv_cmvn_backward", N._ptr(dout), B, F, N._ptr(din), self._stream())
        return din

    def comput_feat_from_feat(self, feats, ori_flag=1, des_flag=2):
        """raw -> CMVN (sic, name as at xv_plda.py:70)."""
        assert ori_flag == 1 and des_flag == 2
        feats, B, F = self._prep(feats, 1)
        out = torch.empty_like(feats)
        self.ctx.call("sg_xv_cmvn", N._ptr(feats), B, F, N._ptr(out), self._stream())
        return out

    def cmvn(self, feats):
        return self.comput_feat_from_feat(feats)

    def _forward(self, x, flag, want_emb=False, want_tdnn=False, dither_noise=None, enroll=None, dither_seed=None):
        x, B, TF = self._prep(x, flag)
        n_spk = self.num_spks if enroll is None else enroll.shape[0]
        dec = torch.empty(B, device=self.device, dtype=torch.int64)
        scores = torch.empty(B, n_spk, device=self.device, dtype=torch.float32)
        emb = torch.empty(B, self.dim, device=self.device, dtype=torch.float32) if want_emb else None
        temb = torch.empty(B, 512, device=self.device, dtype=torch.float32) if want_tdnn else None
        dz = self._dither(dither_noise, dither_seed)
        if enroll is not None:
            self.ctx.call("sg_xv_enroll_override", N._ptr(enroll), enroll.shape[0])
        try:
            self.ctx.call("sg_xv_forward", N._ptr(x), B, TF, flag, C.byref(dz), N._ptr(dec), N._ptr(scores), N._ptr(emb),
                          N._ptr(temb), self._stream())
        finally:
            if enroll is not None:
                self.ctx.call("sg_xv_enroll_override", None, 0)
                enroll.record_stream(torch.cuda.current_stream(self.device))  # the pass may still be reading it
        return dec, scores, emb, temb

    def embedding(self, x, flag=0):
        return self._forward(x, flag, want_emb=True)[2]

    def forward(self, x, flag=0, return_emb=False, enroll_embs=None, dither_seed=None):
        """`dither_seed`: explicit generator key of this pass's dither (a caller that scores an input and then asks
        ``loss_grad`` for the gradient of the SAME noise realisation passes one key to both: defended_model 'average')."""
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

    def tdnn_activation(self, layer):
        """ReLU output of TDNN layer 1..5 from the last pass, (B, F_l, C_l) channel-last (parity tests)."""
        return self.activation_shape(layer)

    # ------------------------------------------------------------------ engine protocol used by attack.*
    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, dither_noise=None, dither_seed=None):
        """make_decision + per-example loss + d loss / d x in one native call (replaces EOT.py:32-35).

        Returns (decisions, scores, loss, grad) with grad shaped like x (None if want_grad=False).
        """
        x, y, B, TF, outs = self._loss_grad_args(x, y, loss_spec, flag, want_grad)
        dz = self._dither(dither_noise, dither_seed)
        spec = loss_spec.native()
        self.ctx.call("sg_xv_loss_grad", N._ptr(x), N._ptr(y), B, TF, flag, C.byref(spec), C.byref(dz),
                      *[N._ptr(t) for t in outs], self._stream())
        return outs

    def _pgd_dither(self, p):
        p.dither = self._dither()
        self.last_fused_seed = int(p.dither.seed)

    # the device loops: which C entry each takes (``EngineOps._pgd_loop`` marshals; neither takes a FeCo block)
    def pgd_run(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size=1, eot_batch_size=1,
                trace=False):
        """attack/FGSM.py:38-70 attack_batch as one device-resident loop, including EOT over the front-end's random
        dither (eot_size fresh-noise passes per gradient step, gradients summed on the device; the traces record each
        step's loss averaged and decision voted over its repeats, like the reference's verbose print)."""
        return self._pgd_loop("sg_xv_pgd_run", x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size,
                              eot_batch_size, trace)

    def pgd_run_defended(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, chain, eot_size=1,
                         eot_batch_size=1, trace=False):
        """``pgd_run`` against this model behind a chain of native waveform-level defenses (defense.time_domain /
        defense.frequency_domain objects, applied in order before the MFCC): the step loop of ``attack_batch`` over
        ``defended_model._loss_grad_through_defenses`` as ONE device-resident call (sg_xv_pgd_run_defended).  Every randomised
        stage (AT) gets one base key, drawn in chain order like ``defended_model._fwd`` draws them; the loop derives the
        key of step ``it``, repeat ``r`` from it as ``fused_pass_seed(key, it, r)``.  ``last_fused_seed`` (the dither's base
        key) and ``last_fused_defense_seeds`` (one entry per stage, None for a deterministic one) let tests replay."""
        return self._pgd_loop("sg_xv_pgd_run_defended", x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size,
                              eot_batch_size, trace, chain=chain)

    # ---- FeCo inside the device loop (sg_xv_pgd_run_feco).  What ``FGSM._device_route`` reads off the base model:
    feco_loop_levels = (1, 2)  # the feature levels a FeCoDefense may sit at (AudioNet's loop: level 1 only, no attribute)
    # The device loop keys the dither and FeCo's random start by (step, repeat), the step loop by draw / call number: for one
    # seed the two routes see different noise.  An attack's result must not change under its user, so a randomised
    # configuration takes the loop only when the attack object opts in (``fuse_randomised_feco``).
    feco_loop_rekeys = True

    def _feco_params(self, feco, T):
        """sg_feco_params of one device loop call, drawn AFTER the dither's key: one base key per call from the model's noise
        bookkeeping (``last_fused_feco_seed`` keeps it; the loop derives ``fused_pass_seed(key, it, r)``), k = int(F * ratio)
        as ``FeCoDefense.fwd`` computes it; a row is keyed by its utterance's GLOBAL index (chunk base + row)."""
        if getattr(feco, 'other_param', 'L2') != 'L2':
            raise N.NativeError("the device loops cluster with the L2 distance only: FeCo with other_param=%r takes the step loop"
                                % (feco.other_param,))
        f = N.FecoParams()
        f.k = int(N.load().sg_xv_num_frames(T) * feco.param)  # feature_level.py:184
        f.max_iter = int(feco.max_iter)
        f.random_init = int(feco.init == 'random')
        f.seed = self.defense_seed(feco.seed)
        feco.calls += 1
        self.last_fused_feco_seed = int(f.seed)
        f.index_base = int(feco.index_base) + self.row_keys()[0]
        return f

    def __getattr__(self, name):
        """``pgd_run_feco`` is offered by every INSTANCE, not as a class attribute: the pinned table of the class's loop
        methods (tests/test_loop_marshalling.py) asserts that the class carries none of that name, and this method's
        marshalling is pinned in a table of its own (tests/test_xv_feco_marshalling.py).  Looked up here -- only when the
        normal lookup fails -- so that nothing is stored on the instance: no reference cycle, and copies and pickles of a
        model offer it like the original."""
        if name == "pgd_run_feco":
            return types.MethodType(_pgd_run_feco, self)
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def time_layer(self, layer, B, T, iters=20):
        ms, fl, rows = C.c_float(), C.c_double(), C.c_int32()
        self.ctx.call("sg_xv_time_layer", layer, B, T, iters, C.byref(ms), C.byref(fl), C.byref(rows), self._stream())
        return ms.value, fl.value, rows.value


def _pgd_run_feco(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, feco, eot_size=1, eot_batch_size=1,
                  trace=False, level=1):
    """``xv_plda.pgd_run_feco`` (every instance offers it: ``xv_plda.__getattr__``): ``pgd_run`` against ``defended_model(self, [(level, feco)])`` as
    ONE device-resident loop (sg_xv_pgd_run_feco) -- MFCC -> FeCo -> CMVN (level 1) or MFCC -> CMVN -> FeCo (level 2) -> TDNN on
    k = int(F * ratio) frames, the hand-chained backward, EOT repeats over the dither and / or FeCo's random start summed on
    the device.  Keys are drawn in this order: the dither's (``last_fused_seed``), FeCo's (``last_fused_feco_seed``); the loop
    derives the key of step ``it``, repeat ``r`` from each as ``fused_pass_seed(key, it, r)``.  `feco`: a FeCoDefense."""
    if level not in self.feco_loop_levels:
        raise ValueError("FeCo runs inside the x-vector device loop at feature level 1 or 2, got %r" % (level,))
    return self._pgd_loop("sg_xv_pgd_run_feco", x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size,
                          eot_batch_size, trace, feco=feco, feco_level=level)
