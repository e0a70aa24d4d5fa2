"""Frequency-domain input transformations on the native engine; mirrors reference defense/frequency_domain.py: the
Butterworth low-pass ``LPF`` (:33-70) and band-pass ``BPF`` (:72-112).  (``DS``, :8-31, is not built: DESIGN.md section 7.)

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
"""
import ctypes as C

import numpy as np
import torch
from scipy import signal

from .. import _native as N
from ..metric.metric import _context
from .time_domain import _WavDefense

MAX_SECTIONS = 16


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
