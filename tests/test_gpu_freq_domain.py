"""The frequency-domain defenses on the device (csrc/k_freq_domain.hip, defense.frequency_domain): every fixture case through
the C-ABI bit-equal to the restatement (tests/freq_domain_restate.py) and within the CPU bounds of truth and reference,
the backward and adjoint identities, batch independence, the default BPF the reference cannot run, refusals, and the
defenses inside defended_model under PGD."""
import ctypes as C

import numpy as np
import pytest
import torch

import freq_domain_restate as R
from conftest import load_golden, log
from test_freq_domain_restate import MEASURED, bits, bound, case_cot, case_data, case_x, truth, truth_adjoint
from test_gpu_time_domain import AN_T, XV_T, _models

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = float("inf")


@pytest.fixture(scope="module")
def ref():
    return load_golden("freq_domain_ref.npz")


def _ctx():
    from speakerguard_amd.metric.metric import _context
    return _context(DEV)


def _filter(sos, clip=None, bits_=16):
    from speakerguard_amd import _native as N
    sos = np.ascontiguousarray(sos, np.float64)
    f = N.WavFilter()
    f.n_sections, f.sos, f.bits = len(sos), sos.ctypes.data_as(C.POINTER(C.c_double)), bits_
    f.clip_mode = N.SG_FD_CLIP_RANGE if clip is None else N.SG_FD_CLIP_GIVEN
    f.clip_lo, f.clip_hi = (0.0, 0.0) if clip is None else clip
    return f, sos  # (sos: kept alive by the caller)


def fwd(sos, x, clip=None, raw=False, B=None, T=None):
    """x numpy (B,T) -> (out, mask) numpy through sg_wav_filter_forward (clip None: the reference's rule, after sg_input_scale)"""
    from speakerguard_amd import _native as N
    ctx, s = _ctx(), N.current_stream_ptr(DEV)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    scale = torch.empty(1, device=DEV)
    ctx.call("sg_input_scale", N._ptr(xd), xd.numel(), N._ptr(scale), s)
    out, mask = torch.full_like(xd, 7.0), torch.full(xd.shape, 5, dtype=torch.int8, device=DEV)
    f, keep = _filter(sos, clip)
    rc = ctx.lib.sg_wav_filter_forward(ctx.handle, C.byref(f), N._ptr(xd), xd.shape[0] if B is None else B,
                                       xd.shape[1] if T is None else T, N._ptr(scale), N._ptr(out), N._ptr(mask), s)
    torch.cuda.synchronize()
    if raw:
        return rc
    ctx.check(rc, "sg_wav_filter_forward")
    return out.cpu().numpy(), mask.cpu().numpy()


def bwd(sos, g, mask):
    from speakerguard_amd import _native as N
    gd = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(DEV)
    md = torch.from_numpy(np.ascontiguousarray(mask, np.int8)).to(DEV)
    gx = torch.full_like(gd, 7.0)
    f, keep = _filter(sos)
    _ctx().call("sg_wav_filter_backward", C.byref(f), N._ptr(gd), N._ptr(md), gd.shape[0], gd.shape[1], N._ptr(gx),
                N.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return gx.cpu().numpy()


# ---------------------------------------------------------------- the fixture through the C-ABI
def test_fixture_bit_equal_to_the_restatement_and_within_the_cpu_bounds(ref):
    for c in ref["meta"]["cases"]:
        tag, x, cot, sos, d = c["tag"], case_x(ref, c), case_cot(ref, c), ref[c["filter"] + "_sos"], case_data(ref, c)
        out, mask = fwd(sos, x)
        gx = bwd(sos, cot, mask)
        assert np.array_equal(bits(out), bits(d["out"])), tag
        assert np.array_equal(mask, d["mask"]), tag
        assert np.array_equal(bits(gx), bits(d["gx"])), tag
        e_out, e_adj = np.abs(out - d["t_out"]).max(), np.abs(gx - d["t_adj"]).max()
        log("freq %s: out err %.3g (bound %.3g), grad err %.3g (bound %.3g)" % (tag, e_out, bound(c, d["t_out"]), e_adj,
                                                                                bound(c, d["t_adj"])))
        assert e_out <= bound(c, d["t_out"]) and e_adj <= bound(c, d["t_adj"]), tag
        if c["ref_finite"]:
            r_out, r_grad = ref[tag + "_out"], ref[tag + "_grad"]
            assert np.abs(out - r_out).max() <= bound(c, d["t_out"]) + np.abs(r_out - d["t_out"]).max(), tag
            assert np.abs(gx - r_grad).max() <= bound(c, d["t_adj"]) + np.abs(r_grad - d["t_adj"]).max(), tag


def test_classes_shapes_and_clip_ranges(ref):
    from speakerguard_amd import _native as N
    from speakerguard_amd.defense import LPF
    c, = [c for c in ref["meta"]["cases"] if c["tag"] == "lpf5000_B3_T257"]
    x, cot, d = torch.from_numpy(case_x(ref, c)).to(DEV), torch.from_numpy(case_cot(ref, c)).to(DEV), case_data(ref, c)
    lpf = LPF(5000)
    for shape in ((257,), (3, 257), (3, 1, 257)):
        xi, gi = (x[0], cot[0]) if len(shape) == 1 else (x.view(shape), cot.view(shape))
        o, sv = lpf.fwd(xi)
        gx = lpf.bwd(sv, gi)
        rows = slice(0, 1) if len(shape) == 1 else slice(None)
        assert o.shape == shape and gx.shape == shape
        assert np.array_equal(bits(o.cpu().numpy().reshape(-1, 257)), bits(d["out"][rows]))
        assert np.array_equal(bits(gx.cpu().numpy().reshape(-1, 257)), bits(d["gx"][rows]))
        assert torch.equal(lpf(xi), o)
    for tag, cls_kw in (("clamp_lpf5000", dict(param=5000)), ("int16_lpf7000", dict(param=7000))):
        c, = [c for c in ref["meta"]["cases"] if c["tag"] == tag]
        d = case_data(ref, c)
        o, sv = LPF(**cls_kw).fwd(torch.from_numpy(case_x(ref, c)).to(DEV))
        assert np.array_equal(bits(o.cpu().numpy()), bits(d["out"])) and np.array_equal(sv[0].cpu().numpy(), d["mask"]), tag
    with pytest.raises(NotImplementedError):
        lpf(torch.zeros(2, 2, 300, device=DEV))
    with pytest.raises(N.NativeError):
        lpf(torch.zeros(2, 300))
    with pytest.raises(ValueError):
        lpf.bwd(lpf.fwd(x)[1], cot[:2])


# ---------------------------------------------------------------- identities
def test_backward_is_the_forward_on_the_reversed_row(ref):
    """bwd(g) == flip(H(flip(g . m))) bit for bit, H through the forward entry with a clip range that never binds"""
    c, = [c for c in ref["meta"]["cases"] if c["tag"] == "clamp_lpf5000"]
    rs = np.random.RandomState(3)
    for name, x in (("lpf5000", np.repeat(case_x(ref, c), 2, 0) * np.float32([[1], [0.5]])), ("bpf_default", None), ("bpf_a", None)):
        sos = ref[name + "_sos"]
        T = x.shape[1] if x is not None else R.P + R.W + 5
        x = x if x is not None else (rs.randn(2, T) * 0.4).astype(np.float32)
        g = rs.randn(2, T).astype(np.float32)
        out, mask = fwd(sos, x, clip=(-1.0, 1.0))
        assert name != "lpf5000" or ((mask[0] == 0).sum() > 10 and mask[1].all())
        gm = np.where(mask != 0, g, np.float32(0))
        h, hm = fwd(sos, gm[:, ::-1], clip=(-INF, INF))
        assert hm.all()
        assert np.array_equal(bits(bwd(sos, g, mask)), bits(h[:, ::-1])), name


def test_adjoint_identity(ref):
    """<H x, g> = <x, H^T g> in float64 accumulation: both sides carry the kernel's error against the exact operator once"""
    rs = np.random.RandomState(11)
    B, T = 3, R.P + 2 * R.W + 7
    x, g = rs.randn(B, T).astype(np.float32), rs.randn(B, T).astype(np.float32)
    ones = np.ones((B, T), np.int8)
    for name in MEASURED:
        sos = ref[name + "_sos"]
        hx, m = fwd(sos, x, clip=(-INF, INF))
        htg = bwd(sos, g, ones)
        assert m.all()
        t_hx, _, _ = truth(sos, x, -INF, INF)
        t_htg = truth_adjoint(sos, g, ones != 0)
        lhs, rhs = float((hx.astype(np.float64) * g).sum()), float((x.astype(np.float64) * htg).sum())
        c = dict(filter=name)
        tol = bound(c, t_hx) * float(np.abs(g).sum()) + bound(c, t_htg) * float(np.abs(x).sum())
        log("freq adjoint %s: |lhs - rhs| %.3g (tol %.3g, |lhs| %.3g)" % (name, abs(lhs - rhs), tol, abs(lhs)))
        assert abs(lhs - rhs) <= tol and tol < 1e-2 * float(np.abs(t_hx).max() * np.abs(g).sum()), name


def test_rows_do_not_depend_on_the_batch(ref):
    rs = np.random.RandomState(4)
    T = R.P + 3 * R.W + 2
    x = (rs.randn(3, T) * 0.2).astype(np.float32)
    g = rs.randn(3, T).astype(np.float32)
    for name in ("lpf5000", "bpf_default"):
        sos = ref[name + "_sos"]
        whole, mask = fwd(sos, x)
        gw = bwd(sos, g, mask)
        for lo, hi in ((0, 1), (1, 2), (2, 3), (0, 2)):  # B = 1 calls, and the call cut in two
            part, pm = fwd(sos, x[lo:hi])
            assert np.array_equal(bits(part), bits(whole[lo:hi])) and np.array_equal(pm, mask[lo:hi]), (name, lo, hi)
            assert np.array_equal(bits(bwd(sos, g[lo:hi], pm)), bits(gw[lo:hi])), (name, lo, hi)
        # the forward value at t does not depend on what follows
        assert np.array_equal(bits(fwd(sos, x[:, :R.P + 1])[0]), bits(whole[:, :R.P + 1])), name


def test_the_default_bpf_works(ref):
    """the case the reference cannot do: finite, and within the bound of the float64 truth"""
    from speakerguard_amd.defense import BPF
    c, = [c for c in ref["meta"]["cases"] if c["filter"] == "bpf_default"]
    assert not c["ref_finite"]
    x, cot, d = case_x(ref, c), case_cot(ref, c), case_data(ref, c)
    bpf = BPF()
    assert bpf.order == 11 and np.allclose(bpf.sos, ref["bpf_default_sos"], rtol=1e-9, atol=1e-15)
    out, sv = bpf.fwd(torch.from_numpy(x).to(DEV))
    gx = bpf.bwd(sv, torch.from_numpy(cot).to(DEV))
    out, gx = out.cpu().numpy(), gx.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(gx).all()
    assert np.abs(out - d["t_out"]).max() <= bound(c, d["t_out"]) and np.abs(gx - d["t_adj"]).max() <= bound(c, d["t_adj"])
    assert np.abs(d["t_out"]).max() > 0.05  # (a filter that passes the band, not one that returns zeros)


def test_refusals(ref):
    from speakerguard_amd import _native as N
    ok = ref["lpf5000_sos"]
    x = np.zeros((2, 300), np.float32)
    assert fwd(ok, x, raw=True) == 0
    assert fwd(np.tile(ok, (3, 1))[:17], x, raw=True) == 1
    for B, T in ((0, 300), (2, 0), (-1, 300)):
        assert fwd(ok, x, raw=True, B=B, T=T) == 1
    for a1, a2 in ((0.0, 1.0), (-2.0, 1.0), (0.5, 1.5), (float("nan"), 0.5), (INF, 0.0)):
        bad = ok.copy()
        bad[2, 4:] = a1, a2
        assert fwd(bad, x, raw=True) == 1, (a1, a2)
    ctx, s = _ctx(), N.current_stream_ptr(DEV)
    assert b"section 3 of 6" in ctx.lib.sg_last_error(ctx.handle)
    xd, md = torch.zeros(2, 300, device=DEV), torch.zeros(2, 300, dtype=torch.int8, device=DEV)
    sc = torch.ones(1, device=DEV)
    f, keep = _filter(ok)
    for args in ((None, 2, 300, N._ptr(sc), N._ptr(xd), N._ptr(md)), (N._ptr(xd), 2, 300, N._ptr(sc), None, N._ptr(md)),
                 (N._ptr(xd), 2, 300, N._ptr(sc), N._ptr(xd), None), (N._ptr(xd), 2, 300, None, N._ptr(xd), N._ptr(md))):
        assert ctx.lib.sg_wav_filter_forward(ctx.handle, C.byref(f), *args, s) == 1
    assert ctx.lib.sg_wav_filter_forward(ctx.handle, None, N._ptr(xd), 2, 300, N._ptr(sc), N._ptr(xd), N._ptr(md), s) == 1
    assert ctx.lib.sg_wav_filter_backward(ctx.handle, C.byref(f), N._ptr(xd), None, 2, 300, N._ptr(xd), s) == 1
    assert ctx.lib.sg_wav_filter_backward(ctx.handle, C.byref(f), None, N._ptr(md), 2, 300, N._ptr(xd), s) == 1
    f.sos = None
    assert ctx.lib.sg_wav_filter_forward(ctx.handle, C.byref(f), N._ptr(xd), 2, 300, N._ptr(sc), N._ptr(xd), N._ptr(md), s) == 1
    f, keep = _filter(ok)
    f.clip_mode = 7
    assert ctx.lib.sg_wav_filter_forward(ctx.handle, C.byref(f), N._ptr(xd), 2, 300, N._ptr(sc), N._ptr(xd), N._ptr(md), s) == 1
    f.n_sections = 0
    assert ctx.lib.sg_wav_filter_backward(ctx.handle, C.byref(f), N._ptr(xd), N._ptr(md), 2, 300, N._ptr(xd), s) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- through the product
@pytest.mark.parametrize("which", [0, 1], ids=["xv_plda", "audionet"])
def test_pgd_through_lpf_and_as_bpf_inside_defended_model(which):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense import AS, BPF, LPF
    from speakerguard_amd.model.defended_model import defended_model
    name, make, T = _models()[which]
    assert T == (XV_T, AN_T)[which]
    base = make()
    x = torch.from_numpy(synth.make_waveforms(3, T, seed=3)).to(DEV)
    ce = SEC4SR_CrossEntropy(reduction='none', task='CSI')
    kw = dict(task="CSI", epsilon=0.002, step_size=0.0004, max_iter=3, batch_size=3, verbose=0)
    for chain in ([LPF(5000)], [AS(3), BPF()]):
        dm = defended_model(base, [(0, d) for d in chain])
        y = dm.make_decision(x)[0]
        # the gradient is the hand-chained one, bit for bit
        h, saved = x, []
        for d in chain:
            h, sv = d.fwd(h)
            saved.append(sv)
        g = base.loss_grad(h, y, ce)[3]
        for d, sv in zip(reversed(chain), reversed(saved)):
            g = d.bwd(sv, g)
        got = dm.loss_grad(x, y, ce)[3]
        assert torch.equal(got, g) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        # PGD through the chain == the same attack cut into B = 1 calls
        adv = PGD(dm, **kw).attack(x, y)[0]
        assert float((adv - x).abs().max()) <= 0.002 + 1e-7 and not torch.equal(adv, x), name
        for b in range(3):
            one = PGD(dm, **dict(kw, batch_size=1)).attack(x[b:b + 1], y[b:b + 1])[0]
            assert torch.equal(one, adv[b:b + 1]), (name, b)
