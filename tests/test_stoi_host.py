"""The host side of metric.batch_stoi / metric.STOI without a GPU: no device means NativeError (never a CPU fallback), refusals
come before the engine is asked, and the marshalling of the engine call -- pointers, shapes, dtypes, row order, the replacement of
short rows -- is checked on an engine double that reads the buffers it is handed and answers with the numpy restatement.  CPU only."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import stoi_cases as SC
import stoi_restate as R
from speakerguard_amd import _native
from speakerguard_amd.metric import metric


class StoiEngineDouble:
    """stands in for _native.Context: ``call("sg_wav_stoi", ...)`` on HOST pointers"""

    def __init__(self):
        self.calls = []

    def call(self, name, benign, adver, B, T, fs, out, frames, stream):
        assert name == "sg_wav_stoi"
        self.calls.append((B, T, fs, stream))
        b = np.ctypeslib.as_array(C.cast(benign, C.POINTER(C.c_float)), (B, T))
        a = np.ctypeslib.as_array(C.cast(adver, C.POINTER(C.c_float)), (B, T))
        d = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), (B,))
        k = np.ctypeslib.as_array(C.cast(frames, C.POINTER(C.c_int32)), (B,))
        for r in range(B):
            p = R.stoi_parts(b[r], a[r], fs)
            d[r], k[r] = (-7.0 if p["K"] - 1 < R.N else p["d"]), p["K"]  # (a short row's value must come from the host)


def test_no_gpu_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(1, 1, 8000)
    with pytest.raises(_native.NativeError):
        metric.batch_stoi(x, x)
    with pytest.raises(_native.NativeError):
        metric.STOI(x, x)
    with pytest.raises(_native.NativeError):
        metric.batch_stoi(x, x, device="cpu")
    with pytest.raises(_native.NativeError):
        metric.get_all_metric_with_stoi(x, x)


def test_refusals_come_first():
    x = torch.zeros(2, 1, 8000)
    with pytest.raises(ValueError, match="fs"):
        metric.batch_stoi(x, x, fs=8000)
    with pytest.raises(ValueError, match="short"):
        metric.batch_stoi(x[:, :, :409], x[:, :, :409])
    with pytest.raises(ValueError, match="short"):
        metric.batch_stoi(x[:, :, :256], x[:, :, :256], fs=10_000)
    with pytest.raises(ValueError, match="shape"):
        metric.batch_stoi(x, x[:, :, :7999])
    with pytest.raises(NotImplementedError):
        metric.STOI(x[:1], x[:1], extended=True)
    with pytest.raises(NotImplementedError):
        metric.PESQ(x[:1], x[:1])


def test_marshalling_on_the_engine_double():
    benign, adver = SC.case(3, 8000, "plain", "0dB")
    short_b, short_a = SC.case(3, 8000, "gap", "0dB")
    benign[1], adver[1] = short_b[1], short_a[1]  # row 1 keeps 8 frames
    eng = StoiEngineDouble()
    d, k = metric._stoi_rows(eng, torch.from_numpy(benign), torch.from_numpy(adver), 16_000, "stream")
    assert eng.calls == [(3, 8000, 16000, "stream")]
    assert d.dtype == np.float64 and d.shape == (3,) and k.dtype == np.int32 and k.shape == (3,)
    want = [R.stoi_parts(b, a) for b, a in zip(benign, adver)]
    assert k.tolist() == [p["K"] for p in want] == [38, 8, 38]
    assert d[0] == want[0]["d"] and d[2] == want[2]["d"] and d[1] == -7.0


def test_short_rows_are_replaced_and_warned_about(monkeypatch):
    benign, adver = SC.case(3, 8000, "plain", "eps")
    short_b, short_a = SC.case(3, 8000, "gap", "eps")
    benign[1], adver[1] = short_b[1], short_a[1]
    eng = StoiEngineDouble()
    # the device plumbing around the engine call, on the CPU: a "device" that is the host
    monkeypatch.setattr(metric, "_context", lambda dev: eng)
    monkeypatch.setattr(metric.N, "current_stream_ptr", lambda dev: None)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **kw: self, raising=True)
    b = torch.from_numpy(benign).unsqueeze(1)
    a = torch.from_numpy(adver).unsqueeze(1)
    with pytest.warns(RuntimeWarning, match="1 of 3") as rec:
        d = metric.batch_stoi(b, a, device="cuda:0")
    assert len(rec) == 1
    assert d[1] == 1e-5 and d[0] == R.stoi(benign[0], adver[0]) and d[2] == R.stoi(benign[2], adver[2])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        one = metric.batch_stoi(b[2], a[2], device="cuda:0")  # (1,T): one row
        assert one.shape == (1,) and one[0] == d[2]
        assert metric.batch_stoi(b[:1], a[:1], fs=10_000, device="cuda:0")[0] == R.stoi(benign[0], adver[0], fs=10000)
    assert [c[:3] for c in eng.calls] == [(3, 8000, 16000), (1, 8000, 16000), (1, 8000, 10000)]


def test_get_all_metric_keeps_its_five_entries():
    import inspect
    assert "PESQ" in inspect.getdoc(metric.get_all_metric_with_stoi)
    assert list(inspect.signature(metric.STOI).parameters) == ["benign_xx", "adver_xx", "fs", "bits", "extended"]
    assert list(inspect.signature(metric.batch_stoi).parameters) == ["benign", "adver", "fs", "device"]
    assert list(inspect.signature(metric.get_all_metric_with_stoi).parameters) == list(inspect.signature(metric.get_all_metric).parameters)


def test_the_tables_the_host_builds_are_the_restatement_s():
    """sg_stoi_debug_tables hands out the bytes sg_wav_stoi uploads.  The host's Kaiser window is its own power series for I0 and
    std::sin, the restatement's is numpy's (Chebyshev I0, np.sinc): a tap is two I0 values, a quotient, a sine, a quotient, the
    normalisation by a 581-term sum and two scalings on either side -- some 8 roundings each -- so the two may differ by 16 spacings of
    the largest tap (0.625: 16 * 2^-53 = 1.8e-15), far under the 1e-12 floor of the GPU parity test, and by nothing like a wrong tap.
    Window, twiddles and the clipping factor are one libm call and one rounding each: 2 spacings of 1."""
    lib = _native.load()
    n = lib.sg_stoi_debug_tables(None, 0)
    assert n == 8 * (616 + 256 + 2 * 448 + 2 * 72 + 2) + 4 * 32
    buf = (C.c_ubyte * n)()
    assert lib.sg_stoi_debug_tables(buf, n - 1) == n and not any(buf)  # too small: nothing is written
    assert lib.sg_stoi_debug_tables(buf, n) == n
    d = np.frombuffer(buf, dtype=np.float64, count=(n - 128) // 8)
    g, win = d[:615].reshape(5, 123), d[616:872]
    tw1, tw2, clip = d[872:1768].reshape(448, 2), d[1768:1912].reshape(72, 2), d[1912]
    edges = np.frombuffer(buf, dtype=np.int32, offset=n - 128)
    G = R.resample_branches()
    assert abs(G).max() == G[0, 58] and 0.62 < G[0, 58] < 0.63
    assert np.array_equal(g == 0, G == 0)  # the same taps lie outside the filter
    assert np.abs(g - G).max() <= 16 * 2.0 ** -53
    assert np.abs(win - R.window()).max() <= 2.0 ** -52
    i = np.arange(448)
    ang = 2 * np.pi * (i // 64 + 1) * (i % 64) / 512
    assert np.abs(tw1[:, 0] - np.cos(ang)).max() <= 2.0 ** -52 and np.abs(tw1[:, 1] + np.sin(ang)).max() <= 2.0 ** -52
    b, c = np.arange(72) // 9, np.arange(72) % 9
    ang = 2 * np.pi * b * c / 64
    assert np.abs(tw2[:, 0] - np.where(c < 8, np.cos(ang), 0)).max() <= 2.0 ** -52
    assert np.abs(tw2[:, 1] + np.where(c < 8, np.sin(ang), 0)).max() <= 2.0 ** -52
    assert abs(clip - (1 + 10 ** (-R.BETA / 20))) <= 2.0 ** -50  # (spacing at 6.6 is 2^-50)
    assert [(int(a), int(b)) for a, b in zip(edges[:15], edges[16:31])] == R.band_edges()
