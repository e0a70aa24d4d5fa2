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
import types

import torch

from .. import _native as N
from ._plda_model import (PldaModel, parse_enroll_model_file, parse_mean_file, parse_plda_file,  # noqa: F401 (re-exported)
                          parse_transform_mat_file)

BITS = 16
_TDNN = ("tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5")


class xv_plda(PldaModel):
    """The back end, the enrolled speakers and the scoring API: ``PldaModel``."""
    allowed_flags = [0, 1, 2]  # 0: wav; 1: raw feat; 2: cmvn feat (xv_plda.py:45-47)
    _feat_width = 30
    _debug_activation = "sg_xv_debug_activation"
    _entry, _fourth, _fourth_width = "sg_xv", "want_tdnn", 512  # the fourth output: fc1's output before the mean subtraction
    takes_lengths = True  # padded batches of unequal lengths: sg_xv_forward_ragged / _loss_grad_ragged / _pgd_run_ragged

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
        sd = weights["state_dict"]
        w = N.XvWeights()
        for l, name in enumerate(_TDNN):
            w.tdnn_weight[l] = hp(sd[name + ".weight"])
            w.tdnn_bias[l] = hp(sd[name + ".bias"])
            w.bn_mean[l] = hp(sd["bn_" + name + ".running_mean"])
            w.bn_var[l] = hp(sd["bn_" + name + ".running_var"])
        w.fc1_weight, w.fc1_bias = hp(sd["fc1.weight"]), hp(sd["fc1.bias"])
        w.bn_eps = 1e-5
        self._init_backend(weights, w, threshold, dither, dither_seed, spk_ids, 512, hp)
        self.ctx.call("sg_xv_load", C.byref(w))

    # ------------------------------------------------------------------ plumbing
    def configure_frontend(self, fft_bits=32):
        """Precision of the MFCC's 512-point transforms on the engine (sg_xv_configure): 32 = float32, the reference's own
        (torchaudio 0.6's kaldi.mfcc is float32 end to end, xv_plda.py:114-148) and the default; 64 = float64 transforms
        around the same float32 stages, the form of rounds 1-5 kept as the counterpart."""
        self.ctx.call("sg_xv_configure", int(fft_bits))
        return self

    # ------------------------------------------------------------------ reference API
    def compute_feat(self, x, flag=1, dither_noise=None):
        """wav (B,1,T) -> raw MFCC (flag 1) or CMVN features (flag 2); xv_plda.py:51-67."""
        assert flag in (1, 2)
        feats, _ = self._mfcc(x, dither_noise)
        return feats if flag == 1 else self.comput_feat_from_feat(feats, 1, 2)

    # ---- front-end stages with their backward (used when a feature-level defense sits between them) ----
    def frontend_forward(self, x, dither_seed=None):
        """wav (B,1,T) -> (raw MFCC (B,F,30), saved) with the state the backward needs (same scale, same dither).
        `dither_seed`: explicit generator key of this pass's dither (tests replay the device loop's per-pass keys)."""
        return self._mfcc(x, dither_seed=dither_seed)

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

    def feat_from_feat_backward(self, dout, ori_flag, des_flag):
        """The adjoint of ``comput_feat_from_feat(., ori_flag, des_flag)``: what ``defended_model`` walks back through, level
        by level, on every base model.  This model has one such step, the CMVN."""
        assert ori_flag == 1 and des_flag == 2
        return self.cmvn_backward(dout)

    def comput_feat_from_feat(self, feats, ori_flag=1, des_flag=2):
        """raw -> CMVN (sic, name as at xv_plda.py:70)."""
        assert ori_flag == 1 and des_flag == 2
        feats, B, F = self._prep(feats, 1)
        out = torch.empty_like(feats)
        self.ctx.call("sg_xv_cmvn", N._ptr(feats), B, F, N._ptr(out), self._stream())
        return out

    def cmvn(self, feats):
        return self.comput_feat_from_feat(feats)

    def tdnn_activation(self, layer):
        """ReLU output of TDNN layer 1..5 from the last pass, (B, F_l, C_l) channel-last (parity tests)."""
        return self.activation_shape(layer)

    def read_gradient(self, what):
        """A buffer of the last ``loss_grad`` call's backward (sg_xv_debug_gradient; parity tests), laid out as that pass
        wrote it: 'demb' (B, 512), 'dact1' .. 'dact5' (B, F_l, C_l), 'dstats' (8, B, 3072) and 'dfeats' (10, B, F, 32) -- the
        split-K slabs -- and, after a waveform pass, 'dfeats_raw' (B, F, 30).  Refused (NativeError) unless that call was the
        last pass of this model."""
        dims = (C.c_int32 * 4)()
        self.ctx.call("sg_xv_debug_gradient", N.SG_GRAD[what], None, 0, dims, self._stream())
        slabs, B, rows, cols = (int(v) for v in dims)
        out = torch.empty(slabs, B, rows, cols, device=self.device, dtype=torch.float32)
        self.ctx.call("sg_xv_debug_gradient", N.SG_GRAD[what], N._ptr(out), out.numel(), None, self._stream())
        if what in ("demb", "dstats"):
            out = out.view(slabs, B, cols)
        return out[0] if slabs == 1 else out

    # ------------------------------------------------------------------ engine protocol used by attack.*
    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, dither_noise=None, dither_seed=None, lengths=None):
        """make_decision + per-example loss + d loss / d x in one native call (replaces EOT.py:32-35).

        Returns (decisions, scores, loss, grad) with grad shaped like x (None if want_grad=False).
        `lengths` (B,) int32: x (B, 1, T_max) is a padded batch of utterances of unequal lengths; row b of every output is that
        of utterance b alone at its own length, and grad is 0 in the padding (sg_xv_loss_grad_ragged).
        """
        x, y, B, TF, outs = self._loss_grad_args(x, y, loss_spec, flag, want_grad)
        if lengths is not None:
            if dither_noise is not None:
                raise ValueError("an explicit dither tensor is not supported with lengths=")
            lens_dev, lens_host = self._lengths_args(lengths, B, TF, flag)
        dz = self._dither(dither_noise, dither_seed)
        spec = loss_spec.native()
        if lengths is not None:
            self.ctx.call("sg_xv_loss_grad_ragged", N._ptr(x), N._ptr(lens_dev), lens_host.ctypes.data_as(C.c_void_p), N._ptr(y), B, TF,
                          C.byref(spec), C.byref(dz), *[N._ptr(t) for t in outs], self._stream())
            return outs
        self.ctx.call("sg_xv_loss_grad", N._ptr(x), N._ptr(y), B, TF, flag, C.byref(spec), C.byref(dz),
                      *[N._ptr(t) for t in outs], self._stream())
        return outs

    def _pgd_dither(self, p):
        p.dither = self._dither()
        self.last_fused_seed = int(p.dither.seed)

    # the device loops: which C entry each takes (``EngineOps._pgd_loop`` marshals; neither takes a FeCo block)
    def pgd_run(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size=1, eot_batch_size=1,
                trace=False, lengths=None):
        """attack/FGSM.py:38-70 attack_batch as one device-resident loop, including EOT over the front-end's random
        dither (eot_size fresh-noise passes per gradient step, gradients summed on the device; the traces record each
        step's loss averaged and decision voted over its repeats, like the reference's verbose print).
        `lengths` (B,) int32: a padded batch of unequal lengths (sg_xv_pgd_run_ragged); no padding sample moves."""
        if lengths is not None:
            return self._pgd_loop("sg_xv_pgd_run_ragged", x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size,
                                  eot_batch_size, trace, lengths=lengths)
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
