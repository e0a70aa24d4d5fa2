"""What every engine-backed model shares: the native attack-state updates (C-ABI: sg_pgd_update, sg_cw2_step,
sg_nes_queries, sg_nes_grad, sg_fakebob_step, sg_pso_init / _select / _move), which the attack classes call through the model so
that the only implementation in the product is the HIP one (tests substitute a CPU double), the noise
bookkeeping, and the ONE marshalling path from a model's ``pgd_run*`` methods to its device-resident PGD
loops (``_pgd_loop``)."""
import ctypes as C

import numpy as np
import torch

from .. import _native as N


_MASK64 = (1 << 64) - 1
# the key strides of the device-resident PGD loops (kStepKey / kRepKey of csrc/sg_internal.h)
STEP_KEY_STRIDE = 0x9E3779B97F4A7C15  # from one PGD step to the next
REP_KEY_STRIDE = 0xC2B2AE3D27D4EB4F   # from one EOT repeat to the next (the kernels' stride for the rows of a pass, sg_dither)


def mix64(*vals):
    """Order-dependent 64-bit hash of integers (splitmix-style); seeds of the engine's counter-based generators."""
    h = 0x9E3779B97F4A7C15
    for v in vals:
        h = ((h ^ (int(v) & _MASK64)) * 0xBF58476D1CE4E5B9) & _MASK64
        h ^= h >> 31
    return h


def fused_pass_seed(base_seed, it, r=0):
    """Generator key of step `it`, EOT repeat `r` of a device-resident PGD loop whose call drew `base_seed` (the dither's,
    a randomised stage's or FeCo's: ``last_fused_seed`` / ``last_fused_defense_seeds``)."""
    return (int(base_seed) + it * STEP_KEY_STRIDE + r * REP_KEY_STRIDE) & _MASK64


def _f32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


class EngineOps:
    """Mixin: ``_open`` sets ``self.ctx`` (N.Context) and ``self.device``; the model names its feature width
    (``_feat_width``) and its debug-activation entry (``_debug_activation``) and has ``num_spks`` / ``allowed_flags``.

    Noise bookkeeping (dither of the MFCC front-end, NES queries, FeCo's random start): the reference draws from the
    process-global torch RNG, which makes an utterance's noise depend on everything that ran before it.  Here every
    draw is keyed by (user seed, attack call, restart, pass number inside the chunk) and, inside the kernels, by the
    GLOBAL index of the utterance (chunk base + row; an EOT repeat moves the key, not the index) -- so the noise an
    utterance sees does not depend on how the batch is chunked or cut into per-GPU shards, wherever the cut falls
    (round 4; rounds 2-3 hashed the chunk base into the key, which tied the invariance to chunk-aligned cuts).
    ``attack()`` calls ``begin_attack`` once, ``_run_batches`` calls ``begin_batch`` per chunk; without them every
    forward simply advances ``_draw`` (fresh noise per call, like the reference).

    What a kernel needs to find "global utterance, repeat" from a row of the call (sg_dither, speakerguard_hip.h):
    ``row_keys()`` = (index base of row 0, offset of this call's row 0 inside the full call, rows per EOT repeat).
    """
    _noise_epoch = 0   # attack() calls so far
    _batch_salt = 0    # restart number + 1 (0: none)
    _index_base = 0    # global index of the first utterance of the chunk being attacked
    _draw = 0          # passes since begin_batch
    _nes_draw = 0      # NES.forward calls since begin_batch
    _def_draw = 0      # calls of a randomised defense (FeCoDefense(init='random'), time_domain.AT) since begin_batch
    _row_base = 0      # position of this call's row 0 inside the full model call it is a slice of (shard.QueryShardedModel)
    _row_scale = 1     # rows every utterance of the chunk contributes to the call (NES: its queries), set by the caller
    _rep_rows = 0      # > 0: the full call's rows are EOT repeats of _rep_rows rows (adaptive_attack/EOT.py sets it)

    def begin_attack(self):
        self._noise_epoch += 1

    def begin_batch(self, index_base=0, salt=0):
        self._index_base, self._batch_salt, self._draw, self._nes_draw, self._def_draw = int(index_base), int(salt), 0, 0, 0

    def noise_seed(self, user_seed, draw):
        return mix64(user_seed, self._noise_epoch, self._batch_salt, draw)

    def row_keys(self):
        """(index_base, row_base, rep_rows) of the model call being made, see sg_dither."""
        return int(self._index_base) * int(self._row_scale), int(self._row_base), int(self._rep_rows)

    def defense_seed(self, user_seed, tag=0x4665436F):
        """Generator key of the next call of a randomised defense sitting on this model (defended_model): keyed like the
        dither -- (seed, attack call, restart, call number inside the chunk) + global utterance index -- so that the clusterings an
        utterance sees do not depend on the shard layout either (rows: ``row_keys()``).  `tag` separates the key domains of
        different defenses (default: FeCo's; defense.time_domain.AT passes its own ``seed_tag``)."""
        key = self.noise_seed(int(user_seed) ^ int(tag), self._def_draw)
        self._def_draw += 1
        return key

    _labels_ok = None  # (label tensor, its version, S, task, loss id) of the last labels check_labels accepted

    def check_labels(self, y, loss_spec, S=None):
        """attack.utils.check_labels before a native call that takes labels, against this model's class count.  The
        tensor last accepted is remembered (a reference to it, and its in-place version counter), so that a loop calling
        the model with the same labels at every step -- CW2, the EOT wrapper -- pays one check, not one device round trip
        per step."""
        from ..attack.utils import check_labels
        if loss_spec.loss_id == N.SG_LOSS_LINEAR:
            return  # (no labels read; leaves the memo to the loss calls around it, defended_model's 'average' order)
        S = self.num_spks if S is None else int(S)
        key = (S, loss_spec.task, loss_spec.loss_id)
        ok = self._labels_ok
        if torch.is_tensor(y) and ok is not None and ok[0] is y and ok[1] == y._version and ok[2:] == key:
            return
        check_labels(y, S, loss_spec)
        self._labels_ok = (y, y._version) + key if torch.is_tensor(y) else None

    def _stream(self):
        return N.current_stream_ptr(self.device)

    def _open(self, device):
        """Bind the model to the GPU `device` and create its engine context.  Returns ``hp``: host array -> pointer to its
        float32 copy for a weight struct; the copies live as long as ``hp`` (they must outlive the load call)."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise N.NativeError("%s runs on the HIP engine only; device must be a GPU (got %s)" % (type(self).__name__, device))
        self.device = torch.device("cuda", self.device.index if self.device.index is not None else 0)
        self.ctx = N.Context(self.device.index)
        keep = []

        def hp(a):
            a = _f32(a)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        return hp

    def _prep(self, x, flag):
        assert flag in self.allowed_flags
        x = x.to(self.device, torch.float32).contiguous()
        if flag == 0:
            assert x.dim() == 3 and x.shape[1] == 1, "wav input must be (B, 1, T)"
            return x, x.shape[0], x.shape[2]
        assert x.dim() == 3 and x.shape[2] == self._feat_width, "feature input must be (B, F, %d)" % self._feat_width
        return x, x.shape[0], x.shape[1]

    # ---- batches of unequal lengths (sg_xv_*_ragged): x (B, 1, T_max) padded, lengths (B,) int32 samples per utterance
    takes_lengths = False  # a model whose engine entries take lengths says True (xv_plda)
    _lengths_ok = None     # (tensor, its version, T_max, device copy, host copy) of the last lengths accepted
    min_length = 400       # one 25 ms window
    min_frames = 32        # the TDNN context (30 frames) and two frames for the pooled standard deviation

    def refuse_lengths(self, lengths):
        """A model (or a route through it) that cannot take ``lengths=`` must say so, never attack the padding."""
        if lengths is not None:
            raise ValueError("%s does not take lengths=: it handles batches of one length only (crop, or attack the utterances "
                             "one at a time)" % type(self).__name__)

    def _lengths_args(self, lengths, B, T, flag=0):
        """The checks of the *_ragged entry points, made here on the host from the tensor given (ValueError, before anything is
        drawn or launched) -> (device int32 tensor, host int32 array): what the kernels read and what the C entry validates
        again.  The pair is remembered per tensor (identity and in-place version), so a step loop pays one upload."""
        if not self.takes_lengths:
            self.refuse_lengths(lengths)
        if flag != 0:
            raise ValueError("lengths= goes with waveform input (flag 0) only")
        if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
            raise ValueError("lengths must be an int32 tensor of shape (%d,), one sample count per row of x" % B)
        ok = self._lengths_ok
        if ok is not None and ok[0] is lengths and ok[1] == lengths._version and ok[2] == T:
            return ok[3], ok[4]
        host = np.ascontiguousarray(lengths.detach().cpu().numpy(), dtype=np.int32)
        frames = N.load().sg_xv_num_frames
        for b, t in enumerate(host.tolist()):
            if t > T:
                raise ValueError("lengths[%d] = %d exceeds the padded length %d" % (b, t, T))
            if t < self.min_length:
                raise ValueError("lengths[%d] = %d is shorter than one 25 ms window (%d samples)" % (b, t, self.min_length))
            if frames(t) < self.min_frames:
                raise ValueError("lengths[%d] = %d gives %d frames, too few for the TDNN context (%d)" % (b, t, frames(t), self.min_frames))
        if int(host.max()) != T:
            raise ValueError("no utterance has the padded length %d: pad to the longest utterance (audio_io.pad_batch)" % T)
        dev = torch.from_numpy(host).to(self.device)
        self._lengths_ok = (lengths, lengths._version, T, dev, host)
        return dev, host

    def activation_shape(self, layer):
        """(rows, channels) per utterance of layer `layer`'s activation in the last pass"""
        rows, ch = C.c_int32(), C.c_int32()
        self.ctx.call(self._debug_activation, layer, None, 0, C.byref(rows), C.byref(ch), self._stream())
        return rows.value, ch.value

    def read_activation(self, layer, B):
        rows, ch = self.activation_shape(layer)
        out = torch.empty(B, rows, ch, device=self.device, dtype=torch.float32)
        self.ctx.call(self._debug_activation, layer, N._ptr(out), out.numel(), None, None, self._stream())
        return out

    def _loss_grad_args(self, x, y, loss_spec, flag, want_grad):
        """what every ``loss_grad`` starts with -> (x, y, B, T or F, (decisions, scores, loss, grad or None))"""
        x, B, TF = self._prep(x, flag)
        self.check_labels(y, loss_spec)
        y = y.to(self.device, torch.int64).contiguous()
        dec = torch.empty(B, device=self.device, dtype=torch.int64)
        scores = torch.empty(B, self.num_spks, device=self.device, dtype=torch.float32)
        loss = torch.empty(B, device=self.device, dtype=torch.float32)
        grad = torch.empty_like(x) if want_grad else None
        if hasattr(loss_spec, 'check'):
            loss_spec.check(B, self.num_spks)
        return x, y, B, TF, (dec, scores, loss, grad)

    # ---- the device-resident PGD loops ------------------------------------------------------------------------------
    fused_pass_seed = staticmethod(fused_pass_seed)

    def _pgd_dither(self, p):
        """hook: the front-end dither of one device loop call, into ``p.dither`` (none: the block stays zero)"""

    def _pgd_args(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size, eot_batch_size, trace):
        """the tensors and the parameter block the device loops share -> (x_adv, y, lower, upper, B, T, params, outputs)"""
        x, B, T = self._prep(x, 0)
        self.check_labels(y, loss_spec)  # once per call: the device loop runs max_iter steps on these labels
        x_adv = x.clone()
        y = y.to(self.device, torch.int64).contiguous()
        lower = lower.to(self.device, torch.float32).expand_as(x).contiguous()
        upper = upper.to(self.device, torch.float32).expand_as(x).contiguous()
        if hasattr(loss_spec, "check"):
            loss_spec.check(B, self.num_spks)  # ScoreVJP: one (B, S) table, shared by the EOT repeats of an utterance
        p = N.PgdParams()
        p.loss = loss_spec.native()
        p.step_size, p.max_iter, p.grad_sign = float(step_size), int(max_iter), int(grad_sign)
        p.eot_size, p.eot_batch_size = int(eot_size), int(eot_batch_size)
        self._pgd_dither(p)
        success = torch.empty(B, device=self.device, dtype=torch.uint8)
        dec = torch.empty(B, device=self.device, dtype=torch.int64)
        scores = torch.empty(B, self.num_spks, device=self.device, dtype=torch.float32)
        loss = torch.empty(B, device=self.device, dtype=torch.float32)
        ltr = torch.empty(max_iter + 1, B, device=self.device, dtype=torch.float32) if trace else None
        dtr = torch.empty(max_iter + 1, B, device=self.device, dtype=torch.int64) if trace else None
        return x_adv, y, lower, upper, B, T, p, (success, dec, scores, loss, ltr, dtr)

    @staticmethod
    def _checked_chain(chain, randomised_ok):
        """the host's refusals of a chain, asked before anything is drawn or cloned -> the chain as a list"""
        chain = list(chain)
        if not randomised_ok and any(getattr(d, 'randomised', False) for d in chain):
            raise ValueError("a randomised input-level defense in front of FeCo keeps the step loop")
        if not 1 <= len(chain) <= N.SG_WAV_CHAIN_MAX:
            raise ValueError("a chain of 1 .. %d input-level defenses runs on the device, got %d" % (N.SG_WAV_CHAIN_MAX, len(chain)))
        return chain

    def _wav_stages(self, chain):
        """the (checked) chain as a sg_wav_stage array.  Every randomised stage (AT) gets one base key, drawn in chain order
        like ``defended_model._fwd`` draws them; ``last_fused_defense_seeds`` keeps them (None for a deterministic stage)."""
        stages = (N.WavStage * len(chain))()
        keep, keys = [], []
        index_base, row_base, _ = self.row_keys()
        for i, d in enumerate(chain):
            st = d.stage()
            keep.append(st)  # (a filter's stage keeps its sections alive)
            key = None
            if getattr(d, 'randomised', False):
                key = self.defense_seed(d.seed, d.seed_tag)
                st.u.defense.seed, st.u.defense.index_base, st.u.defense.row_base = key, index_base, row_base
            keys.append(key)
            stages[i] = st
        self.last_fused_defense_seeds = keys
        return stages, keep

    def _pgd_loop(self, entry, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, eot_size, eot_batch_size, trace,
                  chain=None, feco=None, feco_slot=False, feco_level=None, lengths=None):
        """One device-resident PGD loop call: C entry `entry` over the common arguments, then the stage array and its length
        if a `chain` is given, then the FeCo block if `feco` is given (`feco_slot`: the entry takes that pointer anyway,
        NULL without a defense) and behind it the feature level FeCo sits at if `feco_level` is given (sg_xv_pgd_run_feco),
        then the outputs and the stream.  Keys are drawn in this order: the front-end's dither (``_pgd_dither``), the chain's
        randomised stages in chain order, FeCo's (``_feco_params``).  `lengths`: the entry takes the device and the host copy of
        a padded batch's sample counts in front of B (``_lengths_args``: checked before anything is drawn or cloned)."""
        if chain is not None:
            chain = self._checked_chain(chain, feco is None)
        if lengths is not None:
            lengths = self._lengths_args(lengths, x.shape[0], x.shape[-1])
        x_adv, y, lower, upper, B, T, p, outs = self._pgd_args(x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign,
                                                               eot_size, eot_batch_size, trace)
        extras = []
        if chain is not None:
            stages, keep = self._wav_stages(chain)
            extras += [stages, len(stages)]
        if feco is not None or feco_slot:
            extras.append(None if feco is None else C.byref(self._feco_params(feco, T)))
        if feco_level is not None:
            extras.append(int(feco_level))
        front = [] if lengths is None else [N._ptr(lengths[0]), lengths[1].ctypes.data_as(C.c_void_p)]
        self.ctx.call(entry, N._ptr(x_adv), N._ptr(y), N._ptr(lower), N._ptr(upper), *front, B, T, C.byref(p), *extras,
                      *[N._ptr(t) for t in outs], self._stream())
        return (x_adv,) + outs

    def check_health(self):
        """Raise NativeError if a kernel of an earlier launch flagged its own result as invalid (sg_health: a
        stream-K hand-off wait that timed out).  No synchronisation: call it once the results were awaited."""
        self.ctx.call("sg_health")

    def set_streamk(self, enable):
        """sg_set_streamk: False = every contraction as one block per tile (same bits; no need for all blocks of a launch to
        be resident at once -- the fallback on a GPU this process does not have to itself)."""
        self.ctx.call("sg_set_streamk", int(bool(enable)))
        self.streamk = bool(enable)

    def trace_stages(self, fn, max_records=4096):
        """Run fn() with the library's stage trace on (sg_trace_begin / sg_trace_end: a HIP-event pair around every launch
        of the pass sequences, on the launch stream) and return [(stage name, milliseconds)] in launch order.  Measurement
        aid (bench.py `roofline`); the events cost a few microseconds per launch, so trace a run of its own."""
        self.ctx.call("sg_trace_begin", int(max_records))
        try:
            fn()
        finally:
            tags = (C.c_int32 * max_records)()
            ms = (C.c_float * max_records)()
            n = C.c_int32()
            self.ctx.call("sg_trace_end", tags, ms, int(max_records), C.byref(n))
        k = min(n.value, max_records)
        return [(N.STAGE_NAMES.get(tags[i], str(tags[i])), float(ms[i])) for i in range(k)]

    def pgd_update(self, x, grad, lower, upper, step_size, grad_sign):
        """x <- min(max(x + step*sign(grad)*grad_sign, lower), upper) in place (attack/FGSM.py:65,68)."""
        self.ctx.call("sg_pgd_update", N._ptr(x), N._ptr(grad), N._ptr(lower), N._ptr(upper), x.numel(),
                      float(step_size), int(grad_sign), self._stream())
        return x

    def cw2_step(self, modifier, exp_avg, exp_avg_sq, x, input_cur, grad1, const, lr, step_t):
        """attack/CW2.py:72-82.  Updates modifier/Adam state in place when grad1 is given; returns the
        next (input_x, loss2)."""
        B, _, T = x.shape
        input_next = torch.empty_like(x)
        loss2 = torch.empty(B, device=x.device, dtype=torch.float32)
        self.ctx.call("sg_cw2_step", N._ptr(modifier), N._ptr(exp_avg), N._ptr(exp_avg_sq), N._ptr(x), N._ptr(input_cur),
                      N._ptr(grad1), N._ptr(const), B, T, float(lr), int(step_t), N._ptr(input_next), N._ptr(loss2),
                      self._stream())
        return input_next, loss2

    def nes_queries(self, x, half, with_clean, sigma, seed, pair_base, noise_in=None, want_noise=False, index_base=0):
        """adaptive_attack/NES.py:19-25 -> queries (n*(2*half+with_clean), 1, T) [, noise (n, half, 1, T)]."""
        n, _, T = x.shape
        Q = 2 * half + int(with_clean)
        queries = torch.empty(n * Q, 1, T, device=x.device, dtype=torch.float32)
        noise = torch.empty(n, half, 1, T, device=x.device, dtype=torch.float32) if want_noise else None
        self.ctx.call("sg_nes_queries", N._ptr(x), n, T, half, int(with_clean), float(sigma), C.c_uint64(seed), int(index_base),
                      int(pair_base), N._ptr(noise_in), N._ptr(queries), N._ptr(noise), self._stream())
        return queries, noise

    def nes_grad(self, loss, grad, n, T, half, with_clean, seed, pair_base, noise_in, accumulate, final_sigma, final_batches,
                 index_base=0):
        """adaptive_attack/NES.py:47-54; accumulates into `grad` (n,1,T)."""
        self.ctx.call("sg_nes_grad", N._ptr(loss), n, T, half, int(with_clean), C.c_uint64(seed), int(index_base), int(pair_base),
                      N._ptr(noise_in), int(accumulate), float(final_sigma), int(final_batches), N._ptr(grad), self._stream())
        return grad

    # ---- SirenAttack's swarm (csrc/k_pso.hip).  `st`: attack.SirenAttack.SwarmState, the chunk's state tensors, every utterance
    # in its slot; `rows`: the slots still attacked; x, lower, upper: (n, 1, T) of the whole chunk.
    @staticmethod
    def _i32(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.int32))

    def pso_init(self, st, x, lower, upper, rows, epoch, best_index, key, index_base=0, pos_in=None, vel_in=None):
        """attack/SirenAttack.py:66-86 -> the epoch's first queries (len(rows) * P, 1, T)"""
        n, P, T = st.loc.shape
        rows, best_index = self._i32(rows), None if best_index is None else self._i32(best_index)
        queries = torch.empty(len(rows) * P, 1, T, device=x.device, dtype=torch.float32)
        self.ctx.call("sg_pso_init", N._ptr(x), N._ptr(lower), N._ptr(upper), n, P, T, rows.ctypes.data_as(C.c_void_p), len(rows),
                      int(epoch), None if best_index is None else best_index.ctypes.data_as(C.c_void_p), C.c_uint64(key),
                      int(index_base), N._ptr(pos_in), N._ptr(vel_in), N._ptr(st.loc), N._ptr(st.vel), N._ptr(st.pbest_loc),
                      N._ptr(st.pbest), N._ptr(queries), self._stream())
        return queries

    def pso_select(self, st, loss, rows):
        """:115-132 on loss (len(rows), P); ``st.improved`` keeps who improved for ``pso_move``.  Returns host arrays
        (gbest of the rows, first-index argmin of their pbest, gbest_from): the iteration's one device-to-host read."""
        n, P, _ = st.loc.shape
        rows = self._i32(rows)
        st.improved = torch.empty(len(rows) * P, device=loss.device, dtype=torch.uint8)
        report = torch.empty(3, len(rows), device=loss.device, dtype=torch.float32)
        self.ctx.call("sg_pso_select", N._ptr(loss), n, P, rows.ctypes.data_as(C.c_void_p), len(rows), N._ptr(st.pbest),
                      N._ptr(st.gbest), N._ptr(st.improved), N._ptr(report), self._stream())
        report = report.cpu().numpy()
        return report[0].copy(), report[1].astype(np.int32), report[2].astype(np.int32)

    def pso_move(self, st, x, lower, upper, rows, gbest_from, cont, do_move, w, c1, c2, key, index_base=0, r1_in=None, r2_in=None):
        """:121, :131, :163-174 in one launch -> the next queries (rows that continue * P, 1, T), None when nothing moves"""
        n, P, T = st.loc.shape
        rows, gbest_from, cont = self._i32(rows), self._i32(gbest_from), self._i32(cont)
        n_cont = int(np.count_nonzero(cont)) if do_move else 0
        queries = torch.empty(n_cont * P, 1, T, device=x.device, dtype=torch.float32) if n_cont else None
        self.ctx.call("sg_pso_move", N._ptr(x), N._ptr(lower), N._ptr(upper), n, P, T, rows.ctypes.data_as(C.c_void_p), len(rows),
                      gbest_from.ctypes.data_as(C.c_void_p), cont.ctypes.data_as(C.c_void_p), int(bool(do_move)), float(w), float(c1),
                      float(c2), C.c_uint64(key), int(index_base), N._ptr(r1_in), N._ptr(r2_in), N._ptr(st.improved), N._ptr(st.loc),
                      N._ptr(st.vel), N._ptr(st.pbest_loc), N._ptr(st.gbest_loc), N._ptr(queries), self._stream())
        return queries

    def fakebob_step(self, x, grad, prev_grad, lr, lower, upper, momentum, grad_sign):
        """attack/FAKEBOB.py:93-104; grad and x are updated in place."""
        n, _, T = x.shape
        self.ctx.call("sg_fakebob_step", N._ptr(x), N._ptr(grad), N._ptr(prev_grad), N._ptr(lr), N._ptr(lower), N._ptr(upper),
                      n, T, float(momentum), float(1.0 - momentum), int(grad_sign), self._stream())
        return x, grad
