"""The DS defense on the CPU: the restatement (tests/ds_restate.py) against scipy.signal.upfirdn -- the independent
corroboration DESIGN.md section 2 cites --, its lengths, adjoint, tones, the product's table builder and its guard, and the
a-priori bound of the float32 contract against the float64 truth."""
import numpy as np
import pytest
import torch
from scipy import signal

import ds_restate as R

FS = 16000
PARAMS = (0.5, 0.25, 0.3, 0.33, 0.7, 0.8)
LENGTHS = (1600, 1601, 4003)


def _x(B, T, seed=0, amp=1.0):
    return np.random.RandomState(seed).uniform(-amp, amp, (B, T))


def _upfirdn_stage(x, fi, fo):
    """the same resampler through zero-stuffing, one FIR and decimation: the filter sampled on the lcm(fi, fo) tick grid"""
    iu, ou = R.units(fi, fo)
    tick = fi * ou
    w = R.WIDTH / (2 * 0.99 * 0.5 * min(fi, fo))
    D = int(np.ceil(w * tick))
    c = -(-D // iu) * iu  # the filter's centre, on a multiple of the decimation step
    d = np.arange(-c, D + 1)
    h = R.kernel64(-d / tick, fi, fo)
    y = signal.upfirdn(h, x, up=ou, down=iu)
    n_out = R.out_len(len(x), fi, fo)
    y = y[c // iu:c // iu + n_out]
    return np.pad(y, (0, n_out - len(y)))


@pytest.mark.parametrize("param", PARAMS)
def test_restatement_against_upfirdn(param):
    new = int(FS * param)
    down, up = R.tables64(FS, new), R.tables64(new, FS)
    for T in LENGTHS:
        x = _x(1, T, seed=T)[0]
        low = _upfirdn_stage(x, FS, new)
        y = _upfirdn_stage(low, new, FS)
        mine_low, mine = R.stage64(x, down)[0], R.ds64(x, down, up, same_size=False)[0]
        assert len(low) == len(mine_low) == R.stage_len(T, down) and len(y) == len(mine) == R.out_len(len(low), new, FS)
        err = max(np.abs(low - mine_low).max(), np.abs(y - mine).max())
        assert err <= 1e-12, (param, T, err)


def test_output_lengths():
    down, up = R.class_tables(0.5)
    for T in (1, 2, 13, 25, 1601, 20011, 48000):
        n_low, n_up = R.out_len(T, FS, 8000), R.out_len(R.out_len(T, FS, 8000), 8000, FS)
        assert n_low == (T + 1) // 2 and n_up == 2 * n_low  # T -> ceil(T / 2) -> T, or T + 1 for odd T
        assert R.stage_len(T, down) == n_low and R.stage_len(n_low, up) == n_up
        x = _x(2, T, seed=1)
        assert R.ds32(x, down, up, same_size=False).shape == (2, n_up) and R.ds32(x, down, up).shape == (2, T)
    assert (R.out_len(48000, FS, 8000), R.out_len(20011, FS, 8000), R.out_len(10006, 8000, FS)) == (24000, 10006, 20012)
    for param in PARAMS:  # the tick arithmetic is a ceiling
        new = int(FS * param)
        for T in (1, 7, 1601, 4003):
            assert R.out_len(T, FS, new) == -((-T * new) // FS)


@pytest.mark.parametrize("param", (0.5, 0.33, 0.7))
def test_adjoint_and_autograd(param):
    down, up = R.class_tables(param)
    for T, same in ((257, True), (1601, True), (1601, False)):
        x = _x(2, T, seed=3)
        y = R.ds64(x, down, up, same)
        g = _x(2, y.shape[1], seed=4)
        gx = R.ds_adjoint64(g, down, up, T, same)
        lhs, rhs = float((y * g).sum()), float((x * gx).sum())
        assert abs(lhs - rhs) <= 1e-12 * float(np.abs(y).sum() + np.abs(gx).sum())
        xt = torch.from_numpy(x).requires_grad_(True)
        yt = R.ds_torch(xt, down, up, same)
        assert np.abs(yt.detach().numpy() - y).max() <= 1e-13
        ga, = torch.autograd.grad(yt, xt, torch.from_numpy(g))
        assert np.abs(ga.numpy() - gx).max() <= 1e-13 * max(1.0, np.abs(gx).max())
        # the float32 adjoint is the adjoint of the float32 forward's operator: same tables, same windows
        g32 = R.ds_adjoint32(g.astype(np.float32), down, up, T, same)
        assert (np.abs(g32 - R.ds_adjoint64(g.astype(np.float32), down, up, T, same)) <= R.backward_bound(g.astype(np.float32), down, up, T, same)).all()


def test_table_builder_shapes_values_and_guard(monkeypatch):
    from speakerguard_amd.defense import frequency_domain as FD
    shapes = {0.5: ((1, 25), (2, 13)), 0.33: ((33, 37), (100, 13))}
    for param in PARAMS:
        new = int(FS * param)
        for fi, fo in ((FS, new), (new, FS)):
            tab, t64 = FD.ds_tables(fi, fo), R.tables64(fi, fo)
            assert (tab["in_unit"], tab["out_unit"]) == R.units(fi, fo) and tab["weight"].shape == (tab["out_unit"], tab["W"])
            assert tab["first"].dtype == np.int32 and tab["weight"].dtype == np.float32
            assert np.array_equal(tab["first"], t64["first"]) and tab["W"] == t64["W"]
            # float32 rounding of the arguments: delta = idx / fi - t carries two roundings of numbers up to |idx / fi| + |t|
            # (absolute error e_d <= 2 u (|idx / fi| + |t|) + u |delta|), which moves a weight by |dh/d delta| e_d; the
            # filter's slope is below 2 pi cutoff . (2 cutoff / fi) + the window's pi cutoff / 3 . (2 cutoff / fi); the
            # remaining operations (cos, sin, one division, three products) add a few u relative to the peak 2 cutoff / fi
            cutoff = 0.99 * 0.5 * min(fi, fo)
            peak = 2 * cutoff / fi
            t = np.arange(tab["out_unit"]) / fo
            idx = tab["first"][:, None] + np.arange(tab["W"])[None]
            e_d = 2 * R.U * (np.abs(idx / fi) + t[:, None]) + R.U * np.abs(idx / fi - t[:, None])
            tol = (2 * np.pi * cutoff + np.pi * cutoff / 3) * peak * e_d + 8 * R.U * peak
            assert (np.abs(tab["weight"] - t64["weight"]) <= tol).all(), (fi, fo)
        if param in shapes:
            d, u = FD.ds_tables(FS, new), FD.ds_tables(new, FS)
            assert ((d["out_unit"], d["W"]), (u["out_unit"], u["W"])) == shapes[param]
    ds = FD.DS()
    assert (ds.param, ds.fs, ds.same_size, ds.new_freq, ds.batch_coupled, ds.device_loop) == (0.5, 16000, True, 8000, False, False)
    assert ds.out_len(20011) == 20011 and FD.DS(same_size=False).out_len(20011) == 20012 and ds.tile == 2048
    from speakerguard_amd import defense
    assert defense.DS is FD.DS
    # the guard: a float64 window start that disagrees with the float32 one
    real = FD._ds_first_f64
    monkeypatch.setattr(FD, "_ds_first_f64", lambda fi, fo, ou, w: real(fi, fo, ou, w) + (np.arange(ou) == ou - 1))
    with pytest.raises(ValueError, match="float64"):
        FD.ds_tables(8000, FS)
    monkeypatch.setattr(FD, "_ds_first_f64", real)
    with pytest.raises(ValueError, match="tables of up to"):
        FD.DS(0.335)  # 5360 Hz: 67 phases of 37 taps


def test_tones():
    down, up = R.class_tables(0.5)
    n = np.arange(8000)
    rms = lambda v: float(np.sqrt(np.mean(v[1000:-1000] ** 2)))  # noqa: E731  (away from the edges)
    for hz, lo, hi in ((1000, 0.99, 1.01), (6000, 0.0, 0.01)):
        x = np.sin(2 * np.pi * hz * n / FS)
        ratio = rms(R.ds64(x, down, up)[0]) / rms(x)
        assert lo <= ratio <= hi, (hz, ratio)


@pytest.mark.parametrize("param", PARAMS)
def test_float32_contract_within_the_apriori_bound(param):
    down, up = R.class_tables(param)
    d64, u64 = R.tables64(FS, int(FS * param)), R.tables64(int(FS * param), FS)
    for T in (13, 257, 1601):
        x = _x(2, T, seed=5, amp=0.5).astype(np.float32)
        for same in (True, False):
            y32, y64 = R.ds32(x, down, up, same), R.ds64(x, d64, u64, same)
            bound = R.forward_bound(x, down, up, same)
            assert y32.dtype == np.float32 and (np.abs(y32 - y64) <= bound).all(), (param, T, float(np.abs(y32 - y64).max()))
            assert bound.max() <= 2e-5  # (a bound that says something: the signal is O(1))
            g = _x(2, y32.shape[1], seed=6).astype(np.float32)
            gx32, gx64 = R.ds_adjoint32(g, down, up, T, same), R.ds_adjoint64(g, d64, u64, T, same)
            assert (np.abs(gx32 - gx64) <= R.backward_bound(g, down, up, T, same)).all(), (param, T)
