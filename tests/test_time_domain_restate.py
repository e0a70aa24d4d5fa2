"""The time-domain defenses' contracts (tests/time_domain_restate.py = csrc/k_time_domain.hip header, in numpy) against the
reference's own runs recorded in tests/golden/time_domain_ref.npz.  CPU only; tests/test_gpu_time_domain.py holds the
kernels to the same restatement."""
import inspect

import numpy as np
import pytest

import time_domain_restate as R
from conftest import load_golden

ULP = 2.0 ** -24  # relative half-spacing of float32: one rounding


@pytest.fixture(scope="module")
def ref():
    return load_golden("time_domain_ref.npz")


def cases(ref, *kinds):
    return [c for c in ref["meta"]["cases"] if c["kind"] in kinds]


def case_x(ref, c):
    return ref[c["x"]][:c["B"]]


def case_cot(ref, c):
    return ref[c["cot"]][:c["B"]]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def as_bound(k, x):
    """k fmaf roundings plus the rounding of w = float32(1/k), on sums of magnitude <= max|x|"""
    return (k + 2) * ULP * float(np.abs(x).max())


def as_f64(x, k):
    h = (k - 1) // 2
    xp = np.pad(x.astype(np.float64), ((0, 0), (h, h)))
    return sum(xp[:, j:j + x.shape[1]] for j in range(k)) / k


def at_f64(x, noise, snr, cot=None):
    """the reference formula (:63-69) and its exact gradient in float64"""
    x, noise = x.astype(np.float64), noise.astype(np.float64)
    T = x.shape[1]
    lin = 10.0 ** (snr / 10.0)
    sigma = np.sqrt(((x / np.sqrt(T)) ** 2).sum(1, keepdims=True) / lin)
    out = x + noise * sigma
    if cot is None:
        return out
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = cot + x / (T * lin * sigma) * (cot.astype(np.float64) * noise).sum(1, keepdims=True)
    return out, grad


def test_fixture_covers_the_issue_s_cases(ref):
    cs = ref["meta"]["cases"]
    assert {c["B"] for c in cs} == {1, 3} and {c["T"] for c in cs} >= {1, 2, 255, 256, 257, 4099}
    assert {c["param"] for c in cases(ref, "QT")} == {1, 3, 128, 256}
    for kind in ("AS", "MS"):
        assert {c["param"] for c in cases(ref, kind)} == {1, 3, 5, 17}
        assert any(c["T"] < c["param"] for c in cases(ref, kind))
    tags = {c["tag"] for c in cs}
    assert {"qt_q128_halfway", "qt_q3_int16scale", "ms_k5_ties", "at_snr25_silent"} <= tags


def test_qt_and_bdr_outputs_bit_equal(ref):
    for c in cases(ref, "QT", "BDR"):
        x = case_x(ref, c)
        ours = R.qt(x, c["param"]) if c["kind"] == "QT" else R.bdr(x, c["param"])
        assert np.array_equal(bits(ours), bits(ref[c["tag"] + "_out"])), c["tag"]
    assert R.qt_scale(ref["x_int16"]) == 1 and R.qt_scale(ref["x_float"]) == 32768
    # the half-way inputs really exercise round-half-to-even: both neighbours occur
    lv = np.rint(ref["x_half_q128"].astype(np.float64) * 32768 / 128)
    assert (lv % 2 == 0).all() and len(np.unique(lv)) == 129


def test_ms_outputs_bit_equal(ref):
    for c in cases(ref, "MS"):
        out, sel = R.median_smooth(case_x(ref, c), c["param"])
        assert np.array_equal(bits(out), bits(ref[c["tag"] + "_out"])), c["tag"]
        h = (c["param"] - 1) // 2
        assert sel.dtype == np.int8 and sel.min() >= -h and sel.max() <= h


def test_ms_gradient_without_ties(ref):
    n = 0
    for c in cases(ref, "MS"):
        if c["ties"]:
            continue
        k, x, g = c["param"], case_x(ref, c), case_cot(ref, c)
        h, T = (k - 1) // 2, c["T"]
        out, sel = R.median_smooth(x, k)
        src = np.arange(T)[None, :] + sel
        real = (src >= 0) & (src < T)  # (a selected pad zero is one of several equal pad entries: torch's pick among them is
        idx = ref[c["tag"] + "_idx"].astype(np.int64) - h  # arbitrary, and its cotangent is dropped either way)
        tsrc = np.arange(T)[None, :] + idx
        assert np.array_equal(real, (tsrc >= 0) & (tsrc < T)), c["tag"]
        assert np.array_equal(sel[real], idx[real]), c["tag"]
        gx = R.median_smooth_bwd(sel, g, k)
        # at most k addends per sample, torch adds them in its own order: 2 ulp of the largest addend
        tol = 2 * 2.0 ** -23 * float(np.abs(g).max())
        assert np.abs(gx.astype(np.float64) - ref[c["tag"] + "_grad"]).max() <= tol, c["tag"]
        n += 1
    assert n >= 12


def test_ms_gradient_with_ties_conserves_the_cotangent(ref):
    n = 0
    for c in cases(ref, "MS"):
        k, g = c["param"], case_cot(ref, c)
        out, sel = R.median_smooth(case_x(ref, c), k)
        gx = R.median_smooth_bwd(sel, g, k).astype(np.float64)
        kept = g.astype(np.float64).sum() - R.median_pad_mass(sel, g, k)
        assert abs(gx.sum() - kept) <= g.size * k * ULP * float(np.abs(g).max()), c["tag"]
        n += c["ties"]
    assert n == 3
    # the tie rule itself: among equal values the EARLIER window position ranks lower
    out, sel = R.median_smooth(np.array([[1, 1, 1, 5, 5]], np.float32), 3)
    assert sel.tolist() == [[0, 0, 0, 0, -1]] and out.tolist() == [[1, 1, 1, 5, 5]]  # last window: 5 5 pad -> the FIRST 5
    out, sel = R.median_smooth(np.array([[0, 0, 3]], np.float32), 5)  # window of t = 0: pad pad 0 0 3 -> rank 2 = first real 0
    assert sel[0, 0] == 0 and sel[0, 2] == 1  # (t = 2: 0 0 3 pad pad -> rank 2 of the four zeros = the first pad: dropped)


def test_as_both_directions_against_float64(ref):
    for c in cases(ref, "AS"):
        k, x, g = c["param"], case_x(ref, c), case_cot(ref, c)
        assert np.abs(R.avg_smooth(x, k) - as_f64(x, k)).max() <= as_bound(k, x), c["tag"]
        assert np.abs(R.avg_smooth(g, k) - as_f64(g, k)).max() <= as_bound(k, g), c["tag"]  # symmetric operator: gx = AS(g)
        # and the reference's float32 run sits inside the same bound around the same float64 values
        assert np.abs(ref[c["tag"] + "_out"] - as_f64(x, k)).max() <= as_bound(k, x), c["tag"]
        assert np.abs(ref[c["tag"] + "_grad"] - as_f64(g, k)).max() <= as_bound(k, g), c["tag"]


def test_fmaf_emulation_is_exact():
    """against exact rational arithmetic: the result is at least as close to a*b + c as both of its float32 neighbours"""
    from fractions import Fraction
    rs = np.random.RandomState(5)
    a, b, c = ((rs.randn(3000) * 10.0 ** rs.randint(-3, 4, 3000)).astype(np.float32) for _ in range(3))
    c[:500] = -(a[:500] * b[:500])  # heavy cancellation: the product's low half is all that is left
    got = R.fmaf(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        err = abs(Fraction(float(got[i])) - exact)
        for nb in (np.nextafter(got[i], np.float32(np.inf)), np.nextafter(got[i], np.float32(-np.inf))):
            assert err <= abs(Fraction(float(nb)) - exact), i


def test_at_both_directions_against_float64(ref):
    for c in cases(ref, "AT"):
        tag, x, g, noise, snr = c["tag"], case_x(ref, c), case_cot(ref, c), ref[c["tag"] + "_noise"], c["param"]
        out64, grad64 = at_f64(x, noise, snr, g)
        out, sigma, P = R.at_forward(x, noise, snr)
        gx = R.at_backward(x, noise, g, sigma, P, snr)
        live = P != 0
        # tolerance: twice what the reference's own float32 run shows against float64 on this case
        tol_out = 2 * np.abs(ref[tag + "_out"] - out64).max()
        tol_grad = 2 * np.abs(ref[tag + "_grad"][live] - grad64[live]).max()
        e_out, e_grad = np.abs(out - out64).max(), np.abs(gx[live] - grad64[live]).max()
        print("%s: out err %.3g (tol %.3g), grad err %.3g (tol %.3g)" % (tag, e_out, tol_out, e_grad, tol_grad))
        assert e_out <= tol_out, tag
        assert e_grad <= tol_grad, tag
        if not live.all():  # the silent utterance: the reference's gradient is NaN, ours is the cotangent itself
            assert not np.isfinite(ref[tag + "_grad"][~live]).any()
            assert np.isfinite(gx).all() and np.array_equal(gx[~live], g[~live]) and np.array_equal(out[~live], x[~live])


def test_at_noise_stream(ref):
    from oracle import philox
    T, seed = 700, 0x1234567890ABCDEF
    grid = {}
    for s in (seed, seed + 1):
        for utt in (0, 1, (1 << 32) + 1):
            for rep in (0, 1):
                key, u = R.at_row_key(s, utt, rep * 4, 4, 0)
                assert (key, u) == ((s + rep * R.REPEAT_STRIDE) & R.MASK64, utt)
                grid[(s, utt, rep)] = R.at_normal(key, u, T)
    vals = list(grid.values())
    for i in range(len(vals)):
        assert np.isfinite(vals[i]).all() and abs(vals[i].mean()) < 0.15 and abs(vals[i].std() - 1) < 0.1
        for j in range(i):
            assert abs(np.corrcoef(vals[i], vals[j])[0, 1]) < 0.15  # distinct (seed, utterance, repeat): distinct streams
    # rows of a call: row b of repeat r is utterance index_base + b under key seed + r * stride, however the call is cut
    whole = R.at_noise(seed, 40, 0, 3, 6, T)
    assert np.array_equal(whole[3:], R.at_noise(seed, 40, 3, 3, 3, T))
    assert np.array_equal(whole[3:], R.at_noise((seed + R.REPEAT_STRIDE) & R.MASK64, 40, 0, 0, 3, T))
    assert np.array_equal(whole[1:3], R.at_noise(seed, 41, 0, 0, 2, T))
    # the words are Philox4x32-10's for the documented counter, and the counter domain is not the dither's or the NES's
    k0, k1 = philox._key(seed)
    w0, w1, _, _ = philox.philox4x32_10(np.arange(T), R.AT_DOMAIN, 40, 0, k0, k1)
    bm = np.sqrt(np.float32(-2) * np.log(philox._uniform(w0))) * np.cos(np.float32(6.283185307179586) * philox._uniform(w1))
    assert np.array_equal(whole[0], bm.astype(np.float32))
    assert R.AT_DOMAIN > (1 << 31) // 160  # counter word 1 of the dither is a frame index: never this large
    assert not np.array_equal(whole[0][:400], philox.nes_normal(seed, 40, 0, 400))


def test_signatures_match_the_reference(ref):
    from speakerguard_amd import defense
    from speakerguard_amd.defense import time_domain as TD
    names = {"QT_Non_Diff": TD.QT, "BDR": TD.BDR, "AT": TD.AT, "AS": TD.AS, "MS": TD.MS}
    for fn, cls in names.items():
        want = [tuple(p) for p in ref["meta"]["signatures"][fn] if p[0] != "audio"]
        ps = [p for p in inspect.signature(cls.__init__).parameters.values() if p.name != "self"]
        got = [(p.name, p.default) for p in ps][:len(want)]
        assert got == want, (fn, got, want)
        assert all(p.default is not inspect.Parameter.empty for p in ps)
    assert [defense.QT, defense.BDR, defense.AT, defense.AS, defense.MS] == [TD.QT, TD.BDR, TD.AT, TD.AS, TD.MS]
    assert TD.AT.randomised and TD.AT.seed_tag != 0x4665436F and "seed" in inspect.signature(TD.AT.__init__).parameters
    assert not any(c.batch_coupled for c in names.values())
    for cls in (TD.AS, TD.MS):
        with pytest.raises(ValueError):
            cls(4)._window()
        with pytest.raises(ValueError):
            cls(33)._window()
    assert TD.BDR()._q() == 256 and TD.QT()._q() == 128
