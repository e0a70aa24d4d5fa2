"""Time-domain input transformations on the native engine; mirrors reference defense/time_domain.py: quantisation ``QT``
(:10-44) and its bit-depth form ``BDR`` (:46-48), additive noise ``AT`` (:50-70), average smoothing ``AS`` (:72-97), median
smoothing ``MS`` (:100-127).

The reference's functions become objects whose constructors take the functions' keyword parameters (same names, same
defaults) and which expose the protocol ``defended_model`` chains by hand at input level 0, like ``FeCoDefense`` does at
the feature levels:

    out, saved = d.fwd(x)      # x: (T,), (B,T) or (B,1,T) on the HIP device, like the reference; out has x's shape
    gx = d.bwd(saved, g)       # d loss / d x from d loss / d out
    out = d(x)

Both directions are HIP kernels (csrc/k_time_domain.hip, C-ABI ``sg_wav_defense_forward`` / ``_backward``); the contracts
-- one fixed sequence of float32 operations per output value, whatever the batch -- are written in that file's header.
The gradients: QT / BDR the identity (the reference wraps them in BPDA, :44), AS its own adjoint, MS the scatter to the
selected sample that autograd performs for ``torch.median`` (ties resolved by window position), AT the exact derivative
including the dependence of the noise power on x (the reference does not BPDA-wrap it).
"""
import ctypes as C

import torch

from .. import _native as N
from ..metric.metric import _context
from ..model._engine_ops import REP_KEY_STRIDE

_MASK64 = 0xFFFFFFFFFFFFFFFF
_REPEAT_STRIDE = REP_KEY_STRIDE  # key offset of EOT repeat r (sg_dither)


class _WavDefense:
    batch_coupled = False  # every utterance of a call is transformed on its own (QT: see its docstring)
    kind = None

    def __init__(self, param, same_size=True):
        self.param, self.same_size = param, same_size  # same_size: accepted and unused, as in the reference

    @staticmethod
    def _rows(audio):
        """-> ((B,T) float32 contiguous view/copy on the device, the caller's shape); shapes as time_domain.py:13-21"""
        assert torch.is_tensor(audio)
        if not audio.is_cuda:
            raise N.NativeError("the time-domain defenses run on the HIP device only")
        shape = audio.shape
        if audio.dim() == 1:
            rows = audio.unsqueeze(0)
        elif audio.dim() == 2:
            rows = audio
        elif audio.dim() == 3 and shape[1] == 1:
            rows = audio.squeeze(1)
        else:
            raise NotImplementedError('Audio Shape Error')
        return rows.detach().to(torch.float32).contiguous(), shape

    def _spec(self, param):
        d = N.WavDefense()
        d.kind, d.param = N.SG_TD[self.kind], float(param)
        return d

    def stage(self):
        """This defense as one stage of the device-resident defended loop (sg_wav_stage; xv_plda.pgd_run_defended).  AT's key
        and row bookkeeping are filled in by the caller."""
        st = N.WavStage()
        st.tag = N.SG_WAV_STAGE_DEFENSE
        st.u.defense = self._spec(self._stage_param())
        return st

    def _stage_param(self):
        return self.param

    def _forward(self, spec, x, saved):
        out = torch.empty_like(x)
        _context(x.device).call("sg_wav_defense_forward", C.byref(spec), N._ptr(x), x.shape[0], x.shape[1], N._ptr(out),
                                N._ptr(saved), N.current_stream_ptr(x.device))
        return out

    def _backward(self, spec, x, g, saved, shape):
        g, _ = self._rows(g)
        if tuple(g.shape) != tuple(shape):
            raise ValueError("the cotangent must have the forward's shape")
        gx = torch.empty_like(g)
        _context(g.device).call("sg_wav_defense_backward", C.byref(spec), N._ptr(x), N._ptr(g), N._ptr(saved), g.shape[0],
                                g.shape[1], N._ptr(gx), N.current_stream_ptr(g.device))
        return gx

    def __call__(self, audio, **kw):
        return self.fwd(audio, **kw)[0]


class QT(_WavDefense):
    """Quantisation (:10-44): ``round(audio * s / q) * q / s`` with q = ``param`` and s = 32768 when the input is in the
    [-1, 1] float domain, 1 when it is int16-scaled.  Backward: the identity (BPDA).

    The scale decision is taken PER CALL, from the maximum and minimum of the whole batch, exactly as the reference does
    (:31) -- the one way in which the rows of a call are coupled (``batch_coupled`` stays False: inside an attack the
    iterate is clamped to [-1, 1], so the decision is the same however the batch is cut).  It is made on the device
    (``sg_input_scale``): no host synchronisation."""
    kind = "QT"

    def __init__(self, param=128, bits=16, same_size=True):
        super().__init__(param, same_size)
        self.bits = bits

    def _q(self):
        return self.param

    def _stage_param(self):
        return self._q()

    def fwd(self, audio):
        x, shape = self._rows(audio)
        scale = torch.empty(1, device=x.device, dtype=torch.float32)
        _context(x.device).call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), N.current_stream_ptr(x.device))
        return self._forward(self._spec(self._q()), x, scale).view(shape), None

    def bwd(self, saved, g):
        return g  # BPDA(QT_Non_Diff, identity), :44: nothing to launch


class BDR(QT):
    """Bit-depth reduction (:46-48): QT with q = 2 ** (bits - param)."""

    def __init__(self, param=8, bits=16, same_size=True):
        super().__init__(param, bits, same_size)

    def _q(self):
        return 2 ** (self.bits - self.param)


class _Windowed(_WavDefense):
    def _stage_param(self):
        return self._window()

    def _window(self):
        k = self.param
        if int(k) != k or int(k) % 2 != 1:
            raise ValueError("the window must be odd (the reference asserts / fails to reshape otherwise), got %r" % (k,))
        if not 1 <= int(k) <= 31:
            raise ValueError("windows of 1 .. 31 samples are built, got %r" % (k,))
        return int(k)


class AS(_Windowed):
    """Average smoothing (:72-97): conv1d with ``param`` taps of weight 1 / param, zero padding.  The operator is symmetric,
    so the backward is the forward applied to the cotangent (one kernel for both)."""
    kind = "AS"

    def __init__(self, param=3, same_size=True):
        super().__init__(param, same_size)

    def fwd(self, audio):
        x, shape = self._rows(audio)
        spec = self._spec(self._window())
        return self._forward(spec, x, None).view(shape), (spec, tuple(x.shape), shape)

    def bwd(self, saved, g):
        spec, rows, shape = saved
        return self._backward(spec, None, g, None, rows).view(shape)


class MS(_Windowed):
    """Median smoothing (:100-127) over ``param`` samples, zero padding.  The forward keeps, per output sample, which
    window element it selected (int8 offset); the backward hands each cotangent to that input sample -- what autograd does
    for ``torch.median`` -- as a gather in fixed order.  Equal values are ordered by their position in the window."""
    kind = "MS"

    def __init__(self, param=3, same_size=True):
        super().__init__(param, same_size)

    def fwd(self, audio):
        x, shape = self._rows(audio)
        spec = self._spec(self._window())
        sel = torch.empty(x.shape, device=x.device, dtype=torch.int8)
        return self._forward(spec, x, sel).view(shape), (spec, sel, shape)

    def bwd(self, saved, g):
        spec, sel, shape = saved
        return self._backward(spec, None, g, sel, sel.shape).view(shape)


class AT(_WavDefense):
    """Additive white noise at ``param`` dB signal-to-noise ratio per utterance (:50-70) -- a RANDOMISED defense, the case
    expectation-over-transformation attacks average over.

    The reference draws from torch's global generator; here the draws are a function of (key, global utterance, sample)
    only (Philox4x32-10, regenerated by the backward, never stored).  Called on its own the key is (seed, call number);
    inside ``defended_model`` it comes from the base model's noise bookkeeping (attack call, restart, call number inside
    the chunk) and ``row_keys`` names the global utterance and EOT repeat of every row, like the MFCC dither -- so the
    noise an utterance sees in repeat r of step i depends neither on the chunking nor on the rank that computes it.
    ``noise=`` (B,T) replaces the draws (parity tests).  The gradient is exact, the noise power's dependence on x
    included; for a silent utterance (zero power), where the reference's gradient is NaN, it is the cotangent itself."""
    kind = "AT"
    randomised = True
    seed_tag = 0x41546E7A  # 'ATnz': this defense's own key domain (FeCo's is 0x4665436F)

    def __init__(self, param=25, same_size=True, seed=0):
        super().__init__(param, same_size)
        self.seed = int(seed)
        self.calls = 0       # fwd calls so far: every call draws fresh noise
        self.index_base = 0  # global index of row 0 (set by sharded callers)

    def call_seed(self, call):
        """Generator key of fwd call number `call` (0-based)."""
        from ..model._engine_ops import mix64
        return mix64(self.seed ^ self.seed_tag, call)

    def fwd(self, audio, seed=None, row_keys=None, noise=None):
        x, shape = self._rows(audio)
        spec = self._spec(self.param)
        spec.seed = (self.call_seed(self.calls) if seed is None else int(seed)) & _MASK64
        self.calls += 1
        spec.index_base, spec.row_base, spec.rep_rows = row_keys if row_keys is not None else (self.index_base, 0, 0)
        if noise is not None:
            noise, _ = self._rows(noise)
            if noise.shape != x.shape:
                raise ValueError("noise must have the audio's shape")
            spec.noise_dev = noise.data_ptr()
        stats = torch.empty(3, x.shape[0], device=x.device, dtype=torch.float32)  # sigma, power, backward workspace
        return self._forward(spec, x, stats).view(shape), (spec, x, stats, noise, shape)

    def bwd(self, saved, g):
        spec, x, stats, noise, shape = saved  # (noise: kept alive for spec.noise_dev)
        return self._backward(spec, x, g, stats, x.shape).view(shape)
