"""Perturbation metrics of the evaluation step; mirrors reference metric/metric.py:8-75.

L2 / L0 / L1 / Linf / SNR of a batch come from ONE native pass (C-ABI ``sg_wav_finalize``), with the
reference's ``preprocess`` rule (divide by 2^15 unless -1 <= max <= 1, metric.py:8-12) applied per utterance.
STOI of a batch is native too (C-ABI ``sg_wav_stoi``, csrc/k_stoi.hip): the published algorithm in float64 on the device, under
the same ``preprocess`` rule; its contract is DESIGN.md section 4 (unpinned by pystoi).  PESQ is a third-party package (pesq)
outside the accelerated path: it raises.
"""
import ctypes as C
import warnings

import numpy as np
import torch

from .. import _native as N

_ctx = {}


def _context(device):
    """One engine context per GPU.  An index-less ``cuda`` device means torch's CURRENT device (not GPU 0)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise N.NativeError("the HIP engine needs a GPU tensor/device (got %s)" % device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _ctx:
        _ctx[idx] = N.Context(idx)
    return _ctx[idx]


def _rows(x):
    x = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    x = x.to(torch.float32)
    return x.reshape(1, -1) if x.dim() <= 1 or (x.dim() == 2 and x.shape[0] == 1) else x.reshape(x.shape[0], -1)


def _device(a, device):
    """where a batch metric runs: ``device`` when given, else the adversarial rows' GPU, else torch's current GPU; NativeError for
    anything that is not a GPU, and when there is none (no CPU fallback)"""
    if device is not None:
        dev = torch.device(device)
    elif a.is_cuda:
        dev = a.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        raise N.NativeError("metrics run on the HIP device only, and there is none (no CPU fallback)")
    if dev.type != "cuda":
        raise N.NativeError("metrics run on the HIP device only (got %s)" % dev)
    return dev


def batch_metrics(benign, adver, device=None):
    """(N,1,T) or (1,T) pairs -> float64 array (N,5): L2, L0, L1, Linf, SNR (metric.py:70-75 order)."""
    b, a = _rows(benign), _rows(adver)
    if b.shape != a.shape:
        raise ValueError("benign and adversarial audio must have the same shape, got %s vs %s" % (tuple(b.shape), tuple(a.shape)))
    dev = _device(a, device)
    b, a = b.to(dev).contiguous(), a.to(dev).contiguous()
    out = torch.empty(a.shape[0], 5, device=dev, dtype=torch.float64)
    _context(dev).call("sg_wav_finalize", N._ptr(b), N._ptr(a), a.shape[0], a.shape[1], None, N._ptr(out),
                       N.current_stream_ptr(dev))
    return out.cpu().numpy()


STOI_FRAMES = 30        # frames of a segment: a row that keeps fewer than STOI_FRAMES + 1 frames has no segment
STOI_NOT_ENOUGH = 1e-5  # ... and gets pystoi's value for it


def _stoi_len_10k(T, fs):
    """samples at 10 kHz of T samples at fs; ValueError for an fs that is not built"""
    if fs == 10_000:
        return T
    if fs == 16_000:
        return -(-5 * T // 8)
    raise ValueError("STOI is built for fs = 10000 and fs = 16000, got %r" % (fs,))


def _stoi_rows(ctx, b, a, fs, stream):
    """the engine call on prepared rows -- (N,T) float32, contiguous, on the context's device: (values float64 (N,), kept frames
    int32 (N,)) on the host"""
    out = torch.empty(a.shape[0], device=a.device, dtype=torch.float64)
    frames = torch.empty(a.shape[0], device=a.device, dtype=torch.int32)
    ctx.call("sg_wav_stoi", N._ptr(b), N._ptr(a), a.shape[0], a.shape[1], int(fs), N._ptr(out), N._ptr(frames), stream)
    return out.cpu().numpy(), frames.cpu().numpy()


def batch_stoi(benign, adver, fs=16_000, device=None):
    """(N,1,T) or (1,T) pairs -> float64 array (N,): STOI of every pair (csrc/k_stoi.hip).

    A row that keeps fewer than 31 frames after the silent ones are dropped gets 1e-5, as from pystoi, and the call warns once."""
    b, a = _rows(benign), _rows(adver)
    if b.shape != a.shape:
        raise ValueError("benign and adversarial audio must have the same shape, got %s vs %s" % (tuple(b.shape), tuple(a.shape)))
    n10 = _stoi_len_10k(int(a.shape[1]), fs)
    if n10 <= 256:
        raise ValueError("the utterances are too short for STOI: %d samples at %d Hz are %d at 10 kHz, more than 256 are needed"
                         % (a.shape[1], fs, n10))
    dev = _device(a, device)
    d, k = _stoi_rows(_context(dev), b.to(dev).contiguous(), a.to(dev).contiguous(), fs, N.current_stream_ptr(dev))
    short = k - 1 < STOI_FRAMES
    if short.any():
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. "
                      "Returning 1e-5 for %d of %d utterances. Please check your wav files" % (int(short.sum()), d.shape[0]), RuntimeWarning)
        d[short] = STOI_NOT_ENOUGH
    return d


def _one(benign_xx, adver_xx, k):
    return float(batch_metrics(benign_xx, adver_xx)[0, k])


def L2(benign_xx, adver_xx, bits=16):
    return _one(benign_xx, adver_xx, 0)


def L0(benign_xx, adver_xx, bits=16):
    return _one(benign_xx, adver_xx, 1)


def L1(benign_xx, adver_xx, bits=16):
    return _one(benign_xx, adver_xx, 2)


def Linf(benign_xx, adver_xx, bits=16):
    return _one(benign_xx, adver_xx, 3)


def SNR(benign_xx, adver_xx, bits=16):
    return _one(benign_xx, adver_xx, 4)


def PESQ(benign_xx, adver_xx, bits=16):
    raise NotImplementedError("PESQ needs the third-party 'pesq' package (metric.py:44-48); not part of the native path")


def STOI(benign_xx, adver_xx, fs=16_000, bits=16, extended=False):
    """metric.py:50-54: STOI of one utterance pair, a float.  ``extended=True`` (ESTOI) is not built."""
    if extended:
        raise NotImplementedError("extended STOI (ESTOI) is not part of the native path")
    return float(batch_stoi(benign_xx, adver_xx, fs=fs)[0])


def get_all_metric(benign_xx, adver_xx, fs=16_000, bits=16):
    """[L2, L0, L1, Linf, SNR] of one utterance (metric.py:56-64 without the PESQ / STOI entries)."""
    return [float(v) for v in batch_metrics(benign_xx, adver_xx)[0]]


def get_all_metric_with_stoi(benign_xx, adver_xx, fs=16_000, bits=16):
    """[L2, L0, L1, Linf, SNR, STOI] of one utterance: metric.py:56-64 WITHOUT PESQ -- its slot (the sixth of the reference's
    seven) is absent, so STOI is entry 5 here and entry 6 there."""
    stoi = STOI(benign_xx, adver_xx, fs, bits)
    return get_all_metric(benign_xx, adver_xx, fs, bits) + [stoi]
