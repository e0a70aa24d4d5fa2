"""The numpy restatement of the STOI contract (tests/stoi_restate.py) against code it does not share a line with -- scipy's polyphase
resampler and scipy's STFT -- and the properties of the value.  pystoi is not available: nothing here is pinned by it.  CPU only."""
import numpy as np
import pytest
import scipy.signal

import stoi_cases as SC
import stoi_restate as R
from speakerguard_amd import synth


def _utterances(B, T, seed):
    return synth.make_waveforms(B, T, seed=seed).reshape(B, T).astype(np.float32)


def _with_noise(b, snr_db, seed):
    n = np.random.RandomState(seed).standard_normal(b.shape)
    n *= np.sqrt((b.astype(np.float64) ** 2).mean() / (n ** 2).mean() / 10 ** (snr_db / 10))
    return (b + n).astype(np.float32)


@pytest.mark.parametrize("T", [4000, 8000, 16001, 20011])
def test_resampler_equals_scipy(T):
    x = np.concatenate([_utterances(1, T, seed=T)[0].astype(np.float64)[: T // 2], np.random.RandomState(T).uniform(-1, 1, T - T // 2)])
    want = scipy.signal.resample_poly(x, 5, 8, window=R.resample_window())
    for variant in (False, True):
        got = R.resample_16k(x, variant)
        assert got.shape == want.shape == (-(-5 * T // 8),)
        assert np.abs(got - want).max() <= 1e-12
    # the window itself: 581 taps, unit sum, symmetric; the branches hold 5 h, each tap once
    h, G = R.resample_window(), R.resample_branches()
    assert h.shape == (581,) and abs(h.sum() - 1) < 1e-15 and np.array_equal(h, h[::-1])
    assert np.count_nonzero(G) == np.count_nonzero(h) and abs(G.sum() - 5) < 1e-12


@pytest.mark.parametrize("T", [4000, 8000, 10001])
def test_frame_power_equals_scipy_stft(T):
    x = _utterances(1, T, seed=5)[0].astype(np.float64)
    w = R.window()
    _, _, Z = scipy.signal.stft(x, window=w, nperseg=256, noverlap=128, nfft=512, boundary=None, padded=False)
    want = np.abs(Z.T * w.sum()) ** 2  # (scipy divides the spectrum by the window's sum)
    n = len(range(0, T - 256, 128))
    assert Z.shape[1] >= n
    for variant in (False, True):
        got = R.frame_power(x, variant)
        assert got.shape == (n, 257)
        assert np.abs(got - want[:n]).max() <= 1e-12
    assert np.array_equal(w, np.hanning(258)[1:-1]) and w.shape == (256,)


def test_band_edges():
    e = R.band_edges()
    assert e == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
                 (109, 138), (138, 174), (174, 219)]
    assert len(e) == 15 and all(lo < hi for lo, hi in e) and all(a[1] <= b[0] for a, b in zip(e, e[1:]))
    f = np.arange(257) * 10000 / 512
    for i, (lo, hi) in enumerate(e):  # the centre frequency 150 * 2^(i/3) lies inside its band
        assert f[lo] <= 150 * 2 ** (i / 3) < f[hi]


def test_identity_and_gain():
    for b in _utterances(2, 16000, seed=7):
        assert abs(R.stoi(b, b) - 1) <= 1e-9
        a = _with_noise(b, 5, seed=8)
        d = R.stoi(b, a)
        assert 0 < d < 1
        assert abs(R.stoi(b, (a * np.float32(0.5)).astype(np.float32)) - d) <= 1e-9
        a16 = (a * np.float32(32768)).astype(np.float32)
        assert a16.max() > 1  # the input rule fires
        assert abs(R.stoi(b, a16) - d) <= 1e-9
        assert abs(R.stoi(b, a, variant=True) - d) <= 1e-12


def test_decreases_with_noise():
    for r, b in enumerate(_utterances(3, 16000, seed=9)):
        d = [R.stoi(b, _with_noise(b, snr, seed=10 + r)) for snr in (20, 10, 0, -10)]
        assert 1 > d[0] > d[1] > d[2] > d[3] > -1, d


def test_not_enough_frames():
    b = _utterances(1, 6400, seed=3)[0]  # 4000 samples at 10 kHz: 30 frames, M = 29
    p = R.stoi_parts(b, _with_noise(b, 10, seed=4))
    assert p["energies"].shape == (30,) and p["K"] == 30 and p["d"] == 1e-5
    b = _utterances(1, 6758, seed=3)[0]  # 4224 samples: 31 frames, one segment
    p = R.stoi_parts(b, _with_noise(b, 10, seed=4))
    assert p["energies"].shape == (31,) and p["K"] == 31 and p["d"] != 1e-5 and 0 < p["d"] < 1
    b = b.copy()
    b[2000:4000] = 0  # silence removes frames: below 31 again
    p = R.stoi_parts(b, b)
    assert p["K"] < 31 and p["d"] == 1e-5


def test_refusals():
    x = np.zeros(8000, np.float32)
    with pytest.raises(ValueError, match="fs"):
        R.stoi(x, x, fs=8000)
    with pytest.raises(ValueError, match="short"):
        R.stoi(x[:400], x[:400])
    with pytest.raises(ValueError, match="short"):
        R.stoi(x[:409], x[:409])  # 256 samples at 10 kHz
    with pytest.raises(ValueError, match="short"):
        R.stoi(x[:256], x[:256], fs=10000)
    with pytest.raises(ValueError, match="length"):
        R.stoi(x, x[:7999])
    assert R.stoi_parts(np.ones(410, np.float32), np.ones(410, np.float32))["d"] == 1e-5  # 257 samples: one frame


def test_silent_frames_are_removed_from_both_signals():
    b = _utterances(1, 16000, seed=6)[0]
    a = _with_noise(b, 10, seed=7)
    gap_b, gap_a = b.copy(), a.copy()
    gap_b[4800:11200] = 0
    gap_a[4800:11200] = 0
    p, q = R.stoi_parts(b, a), R.stoi_parts(gap_b, gap_a)
    assert p["K"] == 77 and 31 <= q["K"] < p["K"]
    x10 = R.to_10k(R.input_rule(gap_b), 16000)
    mask = R.silent_mask(q["energies"])
    assert R.remove_silent(x10, mask).shape == ((q["K"] - 1) * 128 + 256,)
    assert R.band_values(R.remove_silent(x10, mask)).shape == (15, q["K"] - 1)


def test_the_gpu_cases_keep_clear_of_the_threshold():
    """what tests/test_gpu_stoi.py asserts again on the device's side: chosen here, where seeds are cheap to change"""
    for c in SC.all_cases():
        benign, adver = SC.case(*c)
        for b in benign:
            assert R.threshold_margin(R.frame_energies(R.to_10k(R.input_rule(b), 16000))) > SC.MARGIN_DB, c
