"""STOI on the device (csrc/k_stoi.hip, metric.batch_stoi / metric.STOI) against the numpy restatement of its contract
(tests/stoi_restate.py): values and kept frames at every shape and layout, the "not enough frames" value, batch independence, the
range rule, the refusals, and a 10 kHz input.

Tolerance on the value: for every row delta = |restatement - variant| is the algorithm's own round-off at that input (the variant
reverses every reduction and uses a DFT by matrix), and the device must stay within max(16 delta, FLOOR): the factor allows for
another FFT factorisation and other reduction trees in the same float64 arithmetic.  FLOOR = 1e-12 was not raised: measured on the
MI355X over all rows, delta <= 1.4e-15 and |device - restatement| <= 3.4e-16 (profiles/stoi_parity_log.txt)."""
import warnings

import numpy as np
import pytest
import torch

import stoi_cases as SC
import stoi_restate as R
from conftest import log
from speakerguard_amd import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 1e-12


def _metric():
    from speakerguard_amd.metric import metric
    return metric


def device(benign, adver, fs=16000):
    """(values float64 (B,), kept frames int32 (B,)) of the C-ABI call itself: no host-side replacement of short rows"""
    from speakerguard_amd import _native as N
    m = _metric()
    b = torch.from_numpy(np.ascontiguousarray(benign, np.float32)).to(DEV)
    a = torch.from_numpy(np.ascontiguousarray(adver, np.float32)).to(DEV)
    return m._stoi_rows(m._context(DEV), b, a, fs, N.current_stream_ptr(DEV))


@pytest.fixture(scope="module")
def references():
    """{case: [(parts, delta)] per row}: the restatement and its distance to the variant, computed once"""
    out = {}
    for c in SC.all_cases():
        benign, adver = SC.case(*c)
        rows = []
        for b, a in zip(benign, adver):
            p = R.stoi_parts(b, a, 16000)
            rows.append((p, abs(p["d"] - R.stoi(b, a, 16000, variant=True))))
        out[c] = rows
    return out


def test_inputs_keep_clear_of_the_threshold(references):
    """the condition on the inputs: a flipped mask can never pass silently"""
    assert len(references) == len(SC.SHAPES) * len(SC.LAYOUTS) * len(SC.NOISES)
    for c, rows in references.items():
        for p, _ in rows:
            assert R.threshold_margin(p["energies"]) > SC.MARGIN_DB, c
    # T = 6758 as generated: 31 frames, none dropped, one segment
    for noise in SC.NOISES:
        for p, _ in references[(2, 6758, "plain", noise)]:
            assert p["energies"].shape[0] == 31 and p["K"] == 31


@pytest.mark.parametrize("B,T", SC.SHAPES)
def test_against_the_restatement(references, B, T):
    for layout in SC.LAYOUTS:
        for noise in SC.NOISES:
            benign, adver = SC.case(B, T, layout, noise)
            d, k = device(benign, adver)
            for r, (p, delta) in enumerate(references[(B, T, layout, noise)]):
                diff = abs(d[r] - p["d"])
                log("stoi parity B=%d T=%d %-5s %-3s row %d: K %d (restated %d)  d %.15f  delta %.3e  |gpu - restated| %.3e  bound %.3e"
                    % (B, T, layout, noise, r, k[r], p["K"], p["d"], delta, diff, max(16 * delta, FLOOR)))
            for r, (p, delta) in enumerate(references[(B, T, layout, noise)]):
                assert R.threshold_margin(p["energies"]) > SC.MARGIN_DB, (layout, noise, r)  # (else a flipped mask could pass)
                assert k[r] == p["K"], (layout, noise, r)
                assert abs(d[r] - p["d"]) <= max(16 * delta, FLOOR), (layout, noise, r)
                if p["K"] - 1 < R.N:
                    assert d[r] == R.NOT_ENOUGH


def test_not_enough_frames_warns_and_returns_the_constant():
    m = _metric()
    benign, adver = SC.case(2, 6400, "plain", "eps")
    assert all(R.stoi_parts(b, a)["K"] - 1 < R.N for b, a in zip(benign, adver))
    d, k = device(benign, adver)
    assert (d == 1e-5).all() and (k - 1 < 30).all()
    with pytest.warns(RuntimeWarning, match="Not enough"):
        out = m.batch_stoi(torch.from_numpy(benign).unsqueeze(1), torch.from_numpy(adver).unsqueeze(1))
    assert out.dtype == np.float64 and out.shape == (2,) and (out == 1e-5).all()
    with pytest.warns(RuntimeWarning):
        assert m.STOI(torch.from_numpy(benign[:1]), torch.from_numpy(adver[:1])) == 1e-5


def test_batch_independence():
    B, T = 64, 48000
    benign = synth.make_waveforms(B, T, seed=11).reshape(B, T).astype(np.float32)
    quiet, loud = SC.noisy(benign, "eps", 12), SC.noisy(benign, "0dB", 13)
    d, k = device(benign, quiet)
    d0, k0 = device(benign, loud)
    assert ((d > 0) & (d <= 1)).all() and (d > d0).all() and (k == k0).all() and (k - 1 >= 30).all()
    at = 0
    for n in (1, 7, 56):
        ds, ks = device(benign[at:at + n], quiet[at:at + n])
        assert np.array_equal(ds.view(np.uint64), d[at:at + n].view(np.uint64)) and np.array_equal(ks, k[at:at + n])
        at += n
    dr, kr = device(benign[::-1], quiet[::-1])
    assert np.array_equal(dr[::-1].view(np.uint64), d.view(np.uint64)) and np.array_equal(kr[::-1], k)
    log("stoi 64 x 48000: eps = 0.002 noise d in [%.6f, %.6f], 0 dB noise d in [%.6f, %.6f], kept frames %d .. %d of 233"
        % (d.min(), d.max(), d0.min(), d0.max(), k.min(), k.max()))


def test_range_rule():
    benign, adver = SC.case(3, 16000, "plain", "eps")
    d, k = device(benign, adver)
    d16, k16 = device(benign * 32768.0, adver * 32768.0)  # (exact in float32: a power of two)
    assert np.array_equal(d.view(np.uint64), d16.view(np.uint64)) and np.array_equal(k, k16)
    # ... per signal: only the degraded one at the int16 scale
    dm, km = device(benign, adver * 32768.0)
    assert np.array_equal(d.view(np.uint64), dm.view(np.uint64)) and np.array_equal(k, km)


def test_refusals():
    from speakerguard_amd import _native as N
    m = _metric()
    x = torch.zeros(2, 1, 8000)
    with pytest.raises(ValueError, match="fs"):
        m.batch_stoi(x, x, fs=8000)
    with pytest.raises(ValueError, match="short"):
        m.batch_stoi(torch.zeros(2, 1, 400), torch.zeros(2, 1, 400))
    with pytest.raises(ValueError, match="shape"):
        m.batch_stoi(x, torch.zeros(2, 1, 8001))
    with pytest.raises(NotImplementedError):
        m.STOI(x[:1], x[:1], extended=True)
    # ... and the entry point itself, before any launch
    for fs, T in ((8000, 8000), (16000, 400), (16000, 409), (10000, 256)):
        z = torch.zeros(2, T, device=DEV)
        with pytest.raises(N.NativeError):
            m._stoi_rows(m._context(DEV), z, z, fs, N.current_stream_ptr(DEV))


def test_a_10_khz_input_is_taken_as_it_is():
    benign, adver = SC.case(2, 10001, "plain", "0dB")
    d, k = device(benign, adver, fs=10000)
    for r in range(2):
        p = R.stoi_parts(benign[r], adver[r], 10000)
        delta = abs(p["d"] - R.stoi(benign[r], adver[r], 10000, variant=True))
        assert R.threshold_margin(p["energies"]) > SC.MARGIN_DB
        log("stoi parity fs=10000 T=10001 row %d: K %d (restated %d)  d %.15f  delta %.3e  |gpu - restated| %.3e" %
            (r, k[r], p["K"], p["d"], delta, abs(d[r] - p["d"])))
        assert k[r] == p["K"] and abs(d[r] - p["d"]) <= max(16 * delta, FLOOR)


def test_the_public_functions():
    m = _metric()
    benign, adver = SC.case(3, 16000, "plain", "eps")
    d, _ = device(benign, adver)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = m.batch_stoi(torch.from_numpy(benign).unsqueeze(1), torch.from_numpy(adver).unsqueeze(1).to(DEV))
        one = m.STOI(torch.from_numpy(benign[1:2]), torch.from_numpy(adver[1:2]))
        every = m.get_all_metric_with_stoi(torch.from_numpy(benign[1:2]), torch.from_numpy(adver[1:2]))
    assert np.array_equal(out, d) and isinstance(one, float) and one == d[1]
    assert every[:5] == m.get_all_metric(torch.from_numpy(benign[1:2]), torch.from_numpy(adver[1:2])) and every[5] == one and len(every) == 6
