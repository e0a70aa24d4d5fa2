"""speakerguard_amd.attack.Kenan's loop against the reference's own run (tests/golden/kenan_ref.npz, written by
tests/golden/make_golden_kenan.py): with the reference's float32 ``torch.fft`` gate injected and the generator's toy model, the
product's loop must reproduce the reference bit for bit -- audio, success flags, every iteration's factor and decision.
CPU only: the native gate is the GPU suite's business (tests/test_gpu_kenan.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import kenan_restate as kr
from conftest import GOLDEN, load_golden
from speakerguard_amd import _native
from speakerguard_amd.attack.Kenan import Kenan


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_kenan", os.path.join(GOLDEN, "make_golden_kenan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torch_gate(audio, factor):
    """_kenan_fft.py fft_compression :57-82, float32 on the CPU"""
    spec = torch.fft.rfft(audio, dim=2)
    spec[spec.abs() < factor.unsqueeze(1).unsqueeze(2)] = 0
    return torch.fft.irfft(spec, dim=2)


def torch_peak(audio):
    """_kenan_fft.py:198"""
    return torch.fft.fft(audio, dim=2).abs().max(dim=2)[0].view(-1)


@pytest.fixture(scope="module")
def golden():
    return load_golden("kenan_ref.npz")


def _adv(g, key):
    return g[key + "_adv"] if key + "_adv" in g else g[str(g[key + "_adv_is"])]


CASES = [(T, t, b) for T in (480, 16000) for t in (0, 1) for b in (1, 4)]


@pytest.mark.parametrize("T,targeted,bs", CASES)
def test_loop_reproduces_the_reference(golden, T, targeted, bs):
    g = golden
    key = "T%d_t%d_b%d" % (T, targeted, bs)
    model = _generator().ToyModel(g["W"])
    x = torch.from_numpy(g["x_%d" % T])
    atk = Kenan(model, atk_name='fft', max_iter=15, targeted=bool(targeted), verbose=0, batch_size=bs, gate=torch_gate,
                peak=torch_peak)
    adv, succ = atk.attack(x.clone(), torch.from_numpy(g[key + "_y"]))
    assert list(succ) == [bool(v) for v in g[key + "_succ"]]
    assert np.array_equal(atk.factor_history.numpy().view(np.uint32), g[key + "_factors"].view(np.uint32))
    assert np.array_equal(atk.decision_history.numpy(), g[key + "_decisions"])
    assert np.array_equal(adv.numpy().view(np.uint32), _adv(g, key).view(np.uint32))
    # a failed utterance comes back equal to its input; a succeeded one is the gate at its last successful factor (taken over the
    # utterance's own chunk: torch's CPU transform is not bit-stable across batch sizes, the native one is)
    last = atk.last_factors
    for lo in range(0, x.shape[0], bs):
        again = torch_gate(x[lo:lo + bs].clone(), last[lo:lo + bs])
        for i in range(lo, min(lo + bs, x.shape[0])):
            if not succ[i]:
                assert np.array_equal(adv[i].numpy().view(np.uint32), x[i].numpy().view(np.uint32)) and torch.isnan(last[i])
            else:
                assert torch.equal(adv[i], again[i - lo])


def test_fixture_holds_both_outcomes(golden):
    flags = np.concatenate([golden["T%d_t%d_b%d_succ" % c] for c in CASES])
    assert flags.any() and not flags.all()
    for t in (0, 1):  # ... in both modes
        f = np.concatenate([golden["T%d_t%d_b%d_succ" % c] for c in CASES if c[1] == t])
        assert f.any() and not f.all()


def test_ssa_is_not_built():
    with pytest.raises(NotImplementedError):
        Kenan(object(), atk_name='ssa')
    with pytest.raises(NotImplementedError):
        Kenan(object(), atk_name='dct')


def test_asserts_of_the_reference(golden):
    model = _generator().ToyModel(golden["W"])
    atk = Kenan(model, verbose=0, gate=torch_gate, peak=torch_peak)
    with pytest.raises(AssertionError, match="Mono"):
        atk.attack(torch.zeros(2, 2, 480), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="equal"):
        atk.attack(torch.zeros(2, 1, 480), torch.zeros(3, dtype=torch.int64))


def test_constructor_mirrors_the_reference():
    import inspect
    names = list(inspect.signature(Kenan.__init__).parameters)
    assert names[:10] == ["self", "model", "atk_name", "max_iter", "raster_width", "early_stop", "targeted", "verbose", "BITS",
                          "batch_size"]
    d = {k: v.default for k, v in inspect.signature(Kenan.__init__).parameters.items()}
    assert (d["atk_name"], d["max_iter"], d["raster_width"], d["early_stop"], d["targeted"], d["verbose"], d["BITS"],
            d["batch_size"]) == ('fft', 15, 100, False, False, 1, 16, 1)
    assert Kenan.chunk_coupling is None


def test_native_gate_refuses_a_cpu_tensor():
    with pytest.raises(_native.NativeError):
        Kenan(object(), verbose=0).attack(torch.zeros(1, 1, 480), torch.zeros(1, dtype=torch.int64))


# ---------------------------------------------------------------- the restatements the GPU suite judges the kernel with
@pytest.mark.parametrize("T,want", [(2, (1, 1, False, [])), (6, (3, 3, False, [3])), (10, (5, 5, False, [5])),
                                    (14, (7, 16, True, [4, 4])), (480, (240, 240, False, [4, 4, 3, 5])),
                                    (662, (331, 1024, True, [4] * 5)), (16000, (8000, 8000, False, [4, 4, 4, 5, 5, 5])),
                                    (48000, (24000, 24000, False, [4, 4, 4, 3, 5, 5, 5])),
                                    (52960, (26480, 65536, True, [4] * 8)), (1 << 22, (1 << 21, 1 << 21, False, [4] * 10 + [2]))])
def test_plan(T, want):
    p = kr.plan(T)
    assert (p["M"], p["N"], p["bluestein"], p["radix"]) == want
    assert int(np.prod(p["radix"], dtype=np.int64)) == p["N"] and (not p["bluestein"] or p["N"] >= 2 * p["M"] - 1 > p["N"] // 2)
    assert p["lds"] == (p["N"] <= 10224)


def test_plan_refuses():
    for T in (0, 1, 3, 481, -2, (1 << 22) + 2):
        with pytest.raises(ValueError):
            kr.plan(T)


@pytest.mark.parametrize("T", [2, 4, 6, 10, 14, 480, 662, 2000])
def test_route_is_the_transform(T):
    """the kernel's route in float64 is rfft / gate / irfft to rounding: the half-length trick, the passes, Bluestein"""
    rs = np.random.RandomState(T)
    x = 0.1 * rs.randn(T)
    X64 = kr.truth_spectrum(x)
    f = 0.3 * np.abs(X64).max()
    X, mag, keep, out = kr.network_gate(x, f, np.float64)
    scale = np.abs(X64).max()
    assert np.abs(X - X64).max() <= 1e-13 * scale
    assert np.array_equal(keep, ~(np.abs(X64) < f)) or np.abs(np.abs(X64) - f).min() < 1e-12 * scale
    assert np.abs(out - kr.truth_gate(x, keep)).max() <= 1e-13
    assert keep.any() and (T < 400 or not keep.all())  # (the gate cuts something, where there are enough bins for that)


def test_bisection_factors():
    f = kr.bisection_factors(np.float32(3.0), "SSSS")
    assert f.dtype == np.float32 and f.tolist() == [1.5, 0.75, 0.375, 0.1875]
    assert kr.bisection_factors(np.float32(256.0)).tolist() == [128.0, 64.0, 32.0, 16.0, 8.0, 4.0, 2.0, 3.0]
    assert kr.bisection_factors(np.float32(8.0), "FFS").tolist() == [4.0, 6.0, 7.0]
