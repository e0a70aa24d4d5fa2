"""The frequency-domain defenses' contract (tests/freq_domain_restate.py = csrc/k_freq_domain.hip header, in numpy) against
the float64 truth and the reference's own runs recorded in tests/golden/freq_domain_ref.npz.  CPU only;
tests/test_gpu_freq_domain.py holds the kernel to the same restatement, bit for bit."""
import inspect

import numpy as np
import pytest
from scipy import signal

import freq_domain_restate as R
from conftest import load_golden

# max |restatement - truth| / max |truth| per filter over the fixture, forward and adjoint (profiles/freq_domain_parity.txt).
# The tests assert FACTOR times it: room for inputs other than the fixture's, none for a wrong carry coefficient (1e-3 and up).
MEASURED = {"lpf8000": 7.48e-08, "lpf7000": 1.25e-07, "lpf5000": 5.01e-07, "bpf_a": 1.76e-06, "bpf_b": 5.27e-07,
            "bpf_c": 7.96e-07, "bpf_default": 3.92e-06}
FACTOR = 4


@pytest.fixture(scope="module")
def ref():
    return load_golden("freq_domain_ref.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case_x(ref, c):
    return ref[c["x"]][:c["B"], :c["T"]]


def case_cot(ref, c):
    return ref[c["cot"]][:c["B"], :c["T"]]


def truth(sos, x, lo, hi):
    """float64: (clamped output, mask, pre-clamp value) -- the generator's recipe"""
    v = signal.sosfilt(sos, np.asarray(x, np.float64), axis=1)
    return np.clip(v, lo, hi), (v >= lo) & (v <= hi), v


def truth_adjoint(sos, g, mask):
    gm = np.where(mask, np.asarray(g, np.float64), 0.0)
    return signal.sosfilt(sos, gm[:, ::-1], axis=1)[:, ::-1]


_CACHE = {}


def case_data(ref, c):
    """per case, computed once and shared (read only): the restatement's (out, mask, gx) and the truth's (out, mask, adjoint)"""
    if c["tag"] not in _CACHE:
        x, cot, sos = case_x(ref, c), case_cot(ref, c), ref[c["filter"] + "_sos"]
        out, mask, _ = R.forward(x, sos)
        t_out, t_mask, t_v = truth(sos, x, *c["clip"])
        _CACHE[c["tag"]] = dict(out=out, mask=mask, gx=R.backward(cot, mask, sos), t_out=t_out, t_mask=t_mask, t_v=t_v,
                                t_adj=truth_adjoint(sos, cot, t_mask))
    return _CACHE[c["tag"]]


def bound(c, arr):
    return FACTOR * MEASURED[c["filter"]] * float(np.abs(arr).max())


def test_fixture_covers_the_issue_s_cases(ref):
    m = ref["meta"]
    C, W, P = m["chunk"], m["wave"], m["pass"]
    assert (C, W, P) == (R.C, R.W, R.P)
    cs = m["cases"]
    assert {c["B"] for c in cs} == {1, 3}
    assert {c["T"] for c in cs} >= {1, 2, C - 1, C, C + 1, W - 1, W, W + 1, P - 1, P, P + 1, 2 * P + 3}
    f = m["filters"]
    assert [f[k]["order"] for k in ("lpf8000", "lpf7000", "lpf5000", "bpf_default")] == [1, 3, 12, 11]
    assert f["lpf8000"]["param"] == 8000 and f["bpf_default"]["param"] == [50, 5000] and f["bpf_default"]["wp"] == [300, 4000]
    assert [(f[k]["wp"], f[k]["param"]) for k in ("bpf_a", "bpf_b", "bpf_c")] == [
        ([300, 4000], [10, 7000]), ([1000, 4000], [100, 7000]), ([500, 3000], [50, 6000])]
    for c in cs:  # inputs: the int16 grid, amplitude <= 0.25 except for the clamp case
        x = case_x(ref, c)
        s = 1.0 if c["clip"][1] > 1 else 32768.0
        assert np.array_equal(np.round(x * s), x * s)
        assert np.abs(x * s).max() <= np.ceil((0.98 if c["tag"].startswith("clamp") else 0.25) * 32768)  # (the grid point next to 0.98)
        assert c["clamped"] == 0 or c["tag"].startswith("clamp")


def test_the_reference_s_default_bpf_does_not_work(ref):
    """the recorded finding: after the reference's float32 cast of (b, a) the default design's poles leave the unit circle"""
    f = ref["meta"]["filters"]["bpf_default"]
    assert f["direct_form_order"] == 22 and 1000 < f["max_abs_a"] < 1100
    assert abs(f["pole_radius_f64"] - 0.9853) < 1e-3 and abs(f["pole_radius_f32"] - 1.325) < 1e-2
    c = [c for c in ref["meta"]["cases"] if c["filter"] == "bpf_default"]
    assert len(c) == 1 and not c[0]["ref_finite"] and c[0]["ref_nonfinite"] > 0
    for k, g in ref["meta"]["filters"].items():  # every other recorded design survives the cast
        assert k == "bpf_default" or (g["pole_radius_f32"] < 0.95 and all(d["ref_finite"] for d in ref["meta"]["cases"] if d["filter"] == k))


def test_recorded_truth_is_the_recipe(ref):
    """the stored float64 truth equals sosfilt on the recorded sos (the long cases' truth is recomputed that way)"""
    n = 0
    for c in ref["meta"]["cases"]:
        if c["has_truth"]:
            d = case_data(ref, c)
            scale = np.abs(d["t_out"]).max()
            assert np.abs(ref[c["tag"] + "_truth"] - d["t_out"]).max() <= 1e-12 * scale, c["tag"]
            assert np.abs(ref[c["tag"] + "_truth_adj"] - d["t_adj"]).max() <= 1e-12 * np.abs(d["t_adj"]).max(), c["tag"]
            n += 1
    assert n >= 14


def test_restatement_against_float64_truth(ref):
    for c in ref["meta"]["cases"]:
        d = case_data(ref, c)
        e_out, e_adj = np.abs(d["out"] - d["t_out"]).max(), np.abs(d["gx"] - d["t_adj"]).max()
        print("%s: out err %.3g (bound %.3g), adjoint err %.3g (bound %.3g)" % (c["tag"], e_out, bound(c, d["t_out"]), e_adj,
                                                                                bound(c, d["t_adj"])))
        assert e_out <= bound(c, d["t_out"]), c["tag"]
        assert e_adj <= bound(c, d["t_adj"]), c["tag"]
        assert np.isfinite(d["out"]).all() and np.isfinite(d["gx"]).all()


def test_restatement_against_the_reference_where_it_is_finite(ref):
    """bound = ours against truth + the recorded distance of the reference's run from the truth (its coefficient rounding)"""
    n = 0
    for c in ref["meta"]["cases"]:
        if not c["ref_finite"]:
            continue
        d = case_data(ref, c)
        r_out, r_grad = ref[c["tag"] + "_out"], ref[c["tag"] + "_grad"]
        dist_out, dist_grad = np.abs(r_out - d["t_out"]).max(), np.abs(r_grad - d["t_adj"]).max()
        limit = 8.4e-5 * 4 if c["filter"] == "bpf_c" else 2e-6  # what the rounding of (b, a) can explain, no more
        assert dist_out <= limit * np.abs(d["t_out"]).max() and dist_grad <= limit * np.abs(d["t_adj"]).max(), c["tag"]
        assert np.abs(d["out"] - r_out).max() <= bound(c, d["t_out"]) + dist_out, c["tag"]
        assert np.abs(d["gx"] - r_grad).max() <= bound(c, d["t_adj"]) + dist_grad, c["tag"]
        n += 1
    assert n == len(ref["meta"]["cases"]) - 1


def test_clamp_case_mask(ref):
    c, = [c for c in ref["meta"]["cases"] if c["tag"].startswith("clamp")]
    d = case_data(ref, c)
    assert c["clamped"] > 10 and (d["mask"] == 0).sum() > 10
    near = np.minimum(np.abs(d["t_v"] - c["clip"][0]), np.abs(d["t_v"] - c["clip"][1])) <= bound(c, d["t_v"])
    assert near.mean() <= 0.01
    assert np.array_equal(d["mask"][~near] != 0, d["t_mask"][~near])
    assert np.abs(d["out"]).max() == 1.0 and np.array_equal(d["mask"] == 0, np.abs(R.forward(case_x(ref, c), ref["lpf5000_sos"])[2]) > 1)
    # clamped samples pass no gradient: the adjoint of the masked cotangent, not of the cotangent
    full = R.backward(case_cot(ref, c), np.ones_like(d["mask"]), ref["lpf5000_sos"])
    assert not np.array_equal(full, d["gx"])
    # the int16-scaled input takes the integer clip range, by the reference's rule
    i, = [c for c in ref["meta"]["cases"] if c["tag"].startswith("int16")]
    assert i["clip"] == [-32768.0, 32767.0] and tuple(R.clip_range(case_x(ref, i))) == (-32768.0, 32767.0)
    assert tuple(R.clip_range(case_x(ref, c))) == (-1.0, 1.0)


def test_generated_inputs_longer_than_two_passes(ref):
    """every filter across block passes (the fixture's other filters stop at 259 samples): same bounds"""
    rs = np.random.RandomState(5)
    T = 2 * R.P + 3
    x = (rs.randint(-8192, 8193, (2, T)) / 32768.0).astype(np.float32)
    g = rs.randn(2, T).astype(np.float32)
    for name in MEASURED:
        sos = ref[name + "_sos"]
        out, mask, _ = R.forward(x, sos)
        gx = R.backward(g, mask, sos)
        t_out, t_mask, _ = truth(sos, x, -1.0, 1.0)
        t_adj = truth_adjoint(sos, g, t_mask)
        c = dict(filter=name)
        assert mask.all() and np.abs(out - t_out).max() <= bound(c, t_out) and np.abs(gx - t_adj).max() <= bound(c, t_adj), name
        # rows do not depend on the batch, nor the forward on what follows
        assert np.array_equal(bits(R.forward(x[1:], sos)[0]), bits(out[1:]))
        assert np.array_equal(bits(R.forward(x[:, :R.P + 1], sos)[0]), bits(out[:, :R.P + 1]))


def test_signatures_and_design_match_the_reference(ref):
    from speakerguard_amd import defense
    from speakerguard_amd.defense import frequency_domain as FD
    assert [defense.LPF, defense.BPF] == [FD.LPF, FD.BPF]
    for name, cls in (("LPF", FD.LPF), ("BPF", FD.BPF)):
        want = {p[0]: p[1] for p in ref["meta"]["signatures"][name] if p[0] != "new"}
        ps = [p for p in inspect.signature(cls.__init__).parameters.values() if p.name != "self"]
        assert {p.name: p.default for p in ps} == want and ps[0].name == "param", name
        assert not cls.batch_coupled
    for name, f in ref["meta"]["filters"].items():
        d = getattr(FD, f["kind"])(param=f["param"], wp=f["wp"])
        assert d.order == f["order"] and np.allclose(np.atleast_1d(d.Wn), f["Wn"], rtol=1e-12, atol=0), name
        assert d.sos.dtype == np.float64 and d.sos.shape == (f["n_sections"], 6)
        assert np.allclose(d.sos, ref[name + "_sos"], rtol=1e-9, atol=1e-15), name
    assert FD.LPF().order == 1 and FD.BPF().order == 11 and FD.LPF(7000).order == 3 and FD.LPF(6000).order == 6


def test_designs_whose_poles_leave_the_unit_circle_are_refused(ref):
    from speakerguard_amd.defense import frequency_domain as FD
    ok = ref["lpf5000_sos"]
    FD.check_sos(ok)
    R.tables(ok)
    for a1, a2 in ((0.0, 1.0), (-2.0, 1.0), (0.0, -1.0), (0.5, 1.5), (-2.1, 1.05), (float("nan"), 0.5)):
        bad = ok.copy()
        bad[2, 4:] = a1, a2
        with pytest.raises(ValueError):
            FD.check_sos(bad)
        with pytest.raises(ValueError):
            R.tables(bad)
    with pytest.raises(ValueError):
        FD.check_sos(np.tile(ok, (3, 1)))  # 18 sections
