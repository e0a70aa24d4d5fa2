"""Frequency-domain input transformations on the native engine; mirrors reference defense/frequency_domain.py: the
down-/up-sampling ``DS`` (:8-31), the Butterworth low-pass ``LPF`` (:33-70) and band-pass ``BPF`` (:72-112).

Like the time-domain classes, the reference's functions become objects whose constructors take the functions' keyword
parameters (same names, same defaults) and which expose the protocol ``defended_model`` chains at input level 0:

    out, saved = d.fwd(x)      # x: (T,), (B,T) or (B,1,T) on the HIP device; out has x's shape
    gx = d.bwd(saved, g)       # d loss / d x from d loss / d out
    out = d(x)

The filter is designed once per object on the host, in float64, by the reference's own recipe (``scipy.signal.buttord`` +
``butter``) -- but kept as second-order sections, and run on the device as that cascade in float32 (csrc/k_freq_domain.hip,
C-ABI ``sg_wav_filter_forward`` / ``_backward``: a parallel scan, one launch per direction, clamp and its mask included).
The reference casts the direct form (b, a) to float32 and filters on the host, one utterance after the other.  Where that
float32 direct form is stable the two agree to its coefficient rounding; for the default ``BPF`` it is NOT stable (largest
pole radius 0.985 in float64, 1.33 after the cast: the reference returns NaN), and this class computes the designed filter.
The gradient is exact: the anti-causal filter applied to the cotangent masked by the clamp.

``DS`` is two ``torchaudio.transforms.Resample`` calls of torchaudio 0.6.0 -- Kaldi's ``LinearResample``: a polyphase
evaluation of one Hann-windowed sinc.  torchaudio is not a dependency: ``ds_tables`` restates its table construction (torch
CPU float32 operations in its order, so the window starts and weights are the ones it would use), and the device runs down-
sampling, up-sampling and truncation as ONE launch per direction (csrc/k_resample.hip, C-ABI ``sg_wav_resample_forward`` /
``_backward``), the low-rate signal staying in LDS.  The reference neither clamps the result nor wraps it in BPDA: the
backward is the exact adjoint, in gather form.  Unpinned by a reference run (none can be made without torchaudio),
corroborated independently against ``scipy.signal.upfirdn``: DESIGN.md section 2.
"""
import ctypes as C
import math

import numpy as np
import torch
from scipy import signal

from .. import _native as N
from ..metric.metric import _context
from .time_domain import _WavDefense

MAX_SECTIONS = 16
LOWPASS_FILTER_WIDTH = 6   # torchaudio 0.6.0 kaldi.resample_waveform's default
DS_MAX_TABLE = 2048        # out_unit * W of a stage (sg_wav_resample_*'s table bound)
DS_MAX_UNIT = 1024
DS_TILE = 2048             # samples of the result one block owns, in whole units (csrc/k_resample.hip kRsTile)


class _Butterworth(_WavDefense):
    """``batch_coupled`` stays False: like QT's scale, the clip range is decided PER CALL from the maximum and minimum of the
    whole batch, as the reference does (:46-51); inside an attack the iterate is clamped to [-1, 1], so the decision is the
    same however the batch is cut.  It is made on the device (``sg_input_scale``): no host synchronisation."""
    btype = None

    def __init__(self, param, fs, wp, gpass, gstop, same_size, bits):
        super().__init__(param, same_size)
        self.fs, self.wp, self.gpass, self.gstop, self.bits = fs, wp, gpass, gstop, bits
        self.order, self.Wn, self.sos = self.design()
        self._filter = self._filter_spec(self.sos, N.SG_FD_CLIP_RANGE)

    def _edges(self):
        raise NotImplementedError

    def design(self):
        """-> (order, Wn, float64 (S,6) sos): frequency_domain.py:53-57 / :93-97 with output='sos'"""
        wp, ws = self._edges()
        order, Wn = signal.buttord(wp, ws, self.gpass, self.gstop, analog=False, fs=None)
        sos = np.ascontiguousarray(signal.butter(order, Wn, btype=self.btype, analog=False, output='sos'), np.float64)
        check_sos(sos)
        return int(order), Wn, sos

    def _filter_spec(self, sos, clip_mode, lo=0.0, hi=0.0):
        f = N.WavFilter()
        f.n_sections, f.sos = len(sos), sos.ctypes.data_as(C.POINTER(C.c_double))  # (self.sos keeps the array alive)
        f.clip_mode, f.bits, f.clip_lo, f.clip_hi = clip_mode, int(self.bits), lo, hi
        return f

    def stage(self):
        """This filter as one stage of the device-resident defended loop (sg_wav_stage).  The stage points at ``self.sos``: the
        object must outlive the call, which reads the sections on the host."""
        st = N.WavStage()
        st.tag = N.SG_WAV_STAGE_FILTER
        st.u.filter = self._filter
        st._keep = self.sos
        return st

    def fwd(self, audio):
        x, shape = self._rows(audio)
        ctx, s = _context(x.device), N.current_stream_ptr(x.device)
        scale = torch.empty(1, device=x.device, dtype=torch.float32)
        ctx.call("sg_input_scale", N._ptr(x), x.numel(), N._ptr(scale), s)
        out = torch.empty_like(x)
        mask = torch.empty(x.shape, device=x.device, dtype=torch.int8)
        ctx.call("sg_wav_filter_forward", C.byref(self._filter), N._ptr(x), x.shape[0], x.shape[1], N._ptr(scale), N._ptr(out),
                 N._ptr(mask), s)
        return out.view(shape), (mask, shape)

    def bwd(self, saved, g):
        mask, shape = saved
        g, _ = self._rows(g)
        if g.shape != mask.shape:
            raise ValueError("the cotangent must have the forward's shape")
        gx = torch.empty_like(g)
        _context(g.device).call("sg_wav_filter_backward", C.byref(self._filter), N._ptr(g), N._ptr(mask), g.shape[0], g.shape[1],
                                N._ptr(gx), N.current_stream_ptr(g.device))
        return gx.view(shape)


def check_sos(sos):
    """what sg_wav_filter_* refuse, said before any launch: 1 .. 16 finite sections, poles strictly inside the unit circle"""
    sos = np.asarray(sos, np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= len(sos) <= MAX_SECTIONS:
        raise ValueError("filters of 1 .. %d second-order sections are built, got shape %r" % (MAX_SECTIONS, sos.shape))
    if not np.isfinite(sos).all() or (sos[:, 3] == 0).any():
        raise ValueError("the design has a non-finite coefficient or a zero a0")
    for k, row in enumerate(sos):
        for a1, a2 in ((row[4] / row[3], row[5] / row[3]), (float(np.float32(row[4] / row[3])), float(np.float32(row[5] / row[3])))):
            if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
                raise ValueError("section %d of the design has a pole on or outside the unit circle" % k)


class LPF(_Butterworth):
    """Butterworth low-pass (:33-70): pass band up to ``wp`` Hz within ``gpass`` dB, stop band from ``param`` Hz at ``gstop`` dB
    down, then the clamp to [-1, 1] or to the ``bits``-bit integer range."""
    btype = "low"

    def __init__(self, param=8000, fs=16000, wp=4000, gpass=3, gstop=40, same_size=True, bits=16):
        super().__init__(param, fs, wp, gpass, gstop, same_size, bits)

    def _edges(self):
        return 2 * self.wp / self.fs, 2 * self.param / self.fs


class BPF(_Butterworth):
    """Butterworth band-pass (:72-112): pass band ``wp`` = [low, high] Hz, stop band ``param`` = [low, high] Hz."""
    btype = "bandpass"

    def __init__(self, param=[50, 5000], wp=[300, 4000], fs=16000, gpass=3, gstop=40, same_size=True, bits=16):
        super().__init__(list(param), fs, list(wp), gpass, gstop, same_size, bits)

    def _edges(self):
        return [2 * w / self.fs for w in self.wp], [2 * w / self.fs for w in self.param]


def _ds_first_f64(fi, fo, out_unit, w):
    """the window starts of ``ds_tables`` in float64 (the guard's second opinion)"""
    t = np.arange(out_unit, dtype=np.float64) / fo
    return np.ceil((t - w) * fi).astype(np.int64)


def ds_tables(fi, fo):
    """Polyphase tables of one ``Resample(fi -> fo)`` of torchaudio 0.6.0 (kaldi.resample_waveform, its
    ``_get_LR_indices_and_weights``, lowpass_filter_width 6) -> dict(in_unit, out_unit, W, first int32 (out_unit,), weight
    float32 (out_unit, W)).  Pure, host only.  The arithmetic is torch CPU float32, operation for operation in torchaudio's
    order -- float64 tables move the composite by 1.5e-7 .. 3e-6.  ``first`` is also computed in float64: a float32 product
    that lands on an integer the float64 one misses would select another window silently, so a disagreement raises."""
    fi, fo = int(fi), int(fo)
    if fi < 1 or fo < 1:
        raise ValueError("the sample rates must be positive, got %d -> %d" % (fi, fo))
    g = math.gcd(fi, fo)
    in_unit, out_unit = fi // g, fo // g
    cutoff = 0.99 * 0.5 * min(fi, fo)
    w = LOWPASS_FILTER_WIDTH / (2 * cutoff)
    t = torch.arange(0., out_unit) / fo
    min_t = t - w
    max_t = t + w
    first = torch.ceil(min_t * fi)
    last = torch.floor(max_t * fi)
    W = int((last - first + 1).max())
    idx = first.unsqueeze(1) + torch.arange(W).unsqueeze(0)
    delta = (idx / fi) - t.unsqueeze(1)
    weight = torch.zeros_like(delta)
    inside = delta.abs().lt(w)
    weight[inside] = 0.5 * (1 + torch.cos(2 * math.pi * cutoff / LOWPASS_FILTER_WIDTH * delta[inside]))
    zero = delta.eq(0.0)
    weight[~zero] *= torch.sin(2 * math.pi * cutoff * delta[~zero]) / (math.pi * delta[~zero])
    weight[zero] *= 2 * cutoff
    weight /= fi
    first = first.to(torch.int64).numpy()
    first64 = _ds_first_f64(fi, fo, out_unit, w)
    if not np.array_equal(first, first64):
        p = int(np.nonzero(first != first64)[0][0])
        raise ValueError("resampling %d -> %d: the float32 window start of phase %d (%d) is not the float64 one (%d)"
                         % (fi, fo, p, first[p], first64[p]))
    return dict(in_unit=in_unit, out_unit=out_unit, W=W, first=np.ascontiguousarray(first, np.int32),
                weight=np.ascontiguousarray(weight.numpy(), np.float32))


def ds_out_len(n, tab):
    """samples a stage returns for n: ceil(n out_unit / in_unit) (torchaudio's tick arithmetic, simplified)"""
    return -((-int(n) * tab["out_unit"]) // tab["in_unit"])


def check_ds_tables(tab):
    """what sg_wav_resample_* refuse about a stage's tables, said at construction"""
    if not (1 <= tab["in_unit"] <= DS_MAX_UNIT and 1 <= tab["out_unit"] <= DS_MAX_UNIT) or tab["out_unit"] * tab["W"] > DS_MAX_TABLE:
        raise ValueError("tables of up to %d entries with units up to %d are built, this ratio needs %d x %d taps on units %d -> %d"
                         % (DS_MAX_TABLE, DS_MAX_UNIT, tab["out_unit"], tab["W"], tab["in_unit"], tab["out_unit"]))
    if not np.isfinite(tab["weight"]).all() or tab["first"][0] > 0:
        raise ValueError("the tables hold a non-finite weight or a window that cannot reach its output")


class DS(_WavDefense):
    """Down-sampling to ``int(fs * param)`` Hz and up-sampling back (:8-31), truncated to the input's length when
    ``same_size``; otherwise the up-sampler's own length, as in the reference (odd lengths come back one sample longer).  No
    clamp: white noise of amplitude 1 comes out at up to 1.34.  Backward: the exact adjoint."""
    device_loop = False  # not yet a stage of the device-resident loops: FGSM._device_route keeps such a chain on the step loop

    def __init__(self, param=0.5, fs=16000, same_size=True):
        super().__init__(param, same_size)
        self.fs, self.new_freq = int(fs), int(fs * param)
        self.down, self.up = ds_tables(self.fs, self.new_freq), ds_tables(self.new_freq, self.fs)
        for tab in (self.down, self.up):
            check_ds_tables(tab)
        self._spec = N.WavResample()
        for st, tab in ((self._spec.down, self.down), (self._spec.up, self.up)):  # (self.down / .up keep the arrays alive)
            st.in_unit, st.out_unit, st.W = tab["in_unit"], tab["out_unit"], tab["W"]
            st.first = tab["first"].ctypes.data_as(C.POINTER(C.c_int32))
            st.weight = tab["weight"].ctypes.data_as(C.POINTER(C.c_float))
        self._spec.same_size = 1 if same_size else 0

    @property
    def tile(self):
        """output samples one block of the forward kernel owns"""
        return max(1, DS_TILE // self.up["out_unit"]) * self.up["out_unit"]

    def out_len(self, T):
        return int(T) if self.same_size else ds_out_len(ds_out_len(T, self.down), self.up)

    def stage(self):
        raise NotImplementedError("DS is not a stage of the device-resident loops")

    def fwd(self, audio):
        x, shape = self._rows(audio)
        n = self.out_len(x.shape[1])
        out = torch.empty(x.shape[0], n, device=x.device, dtype=torch.float32)
        _context(x.device).call("sg_wav_resample_forward", C.byref(self._spec), N._ptr(x), x.shape[0], x.shape[1], N._ptr(out), n,
                                N.current_stream_ptr(x.device))
        out_shape = tuple(shape[:-1]) + (n,)
        return out.view(out_shape), (tuple(x.shape), shape, out_shape)

    def bwd(self, saved, g):
        rows, shape, out_shape = saved
        if tuple(g.shape) != tuple(out_shape):
            raise ValueError("the cotangent must have the forward's shape")
        g, _ = self._rows(g)
        gx = torch.empty(rows, device=g.device, dtype=torch.float32)
        _context(g.device).call("sg_wav_resample_backward", C.byref(self._spec), N._ptr(g), rows[0], rows[1], g.shape[1], N._ptr(gx),
                                N.current_stream_ptr(g.device))
        return gx.view(shape)
