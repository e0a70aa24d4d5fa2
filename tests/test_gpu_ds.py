"""The DS defense on the device (csrc/k_resample.hip, defense.frequency_domain.DS): both directions through the C-ABI bit-equal
to the float32 restatement (tests/ds_restate.py) and within its a-priori bound of the float64 truth, batch independence, shapes
and refusals, the adjoint identity, the gradient inside defended_model on both models, and the attacks on the step loop.

Inputs have amplitude <= 0.5: DS does not clamp, and white noise of amplitude 1 comes out at up to 1.34 -- past the 1 / 0.9
input-range bound of the models."""
import ctypes as C

import numpy as np
import pytest
import torch

import ds_restate as R
from conftest import log
from test_gpu_time_domain import AN_T, XV_T, _models

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARAMS = (0.5, 0.25, 0.3, 0.33, 0.7)
SHAPES = ((1, 1), (1, 2), (1, 13), (2, 25), (3, 257), (2, 1601), (5, 4003))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ctx():
    from speakerguard_amd.metric.metric import _context
    return _context(DEV)


def _ds(param=0.5, same_size=True):
    from speakerguard_amd.defense import DS
    return DS(param, same_size=same_size)


def fwd(ds, x, raw=False, B=None, T=None, N=None, spec=None):
    """x numpy (B,T) -> out numpy (B,N) through sg_wav_resample_forward"""
    from speakerguard_amd import _native as N_
    ctx, s = _ctx(), N_.current_stream_ptr(DEV)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    n = ds.out_len(xd.shape[1])
    out = torch.full((xd.shape[0], n), 7.0, device=DEV)
    rc = ctx.lib.sg_wav_resample_forward(ctx.handle, C.byref(ds._spec if spec is None else spec), N_._ptr(xd),
                                         xd.shape[0] if B is None else B, xd.shape[1] if T is None else T, N_._ptr(out),
                                         n if N is None else N, s)
    torch.cuda.synchronize()
    if raw:
        return rc
    ctx.check(rc, "sg_wav_resample_forward")
    return out.cpu().numpy()


def bwd(ds, g, T, spec=None):
    from speakerguard_amd import _native as N_
    gd = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(DEV)
    gx = torch.full((gd.shape[0], T), 7.0, device=DEV)
    _ctx().call("sg_wav_resample_backward", C.byref(ds._spec if spec is None else spec), N_._ptr(gd), gd.shape[0], T, gd.shape[1],
                N_._ptr(gx), N_.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return gx.cpu().numpy()


def _case(B, T, n_out, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.5, 0.5, (B, T)).astype(np.float32), rs.uniform(-1, 1, (B, n_out)).astype(np.float32)


# ---------------------------------------------------------------- bit equality and the truth bound
@pytest.mark.parametrize("param", PARAMS)
def test_bit_equal_to_the_restatement_and_within_the_bound_of_truth(param):
    down, up = R.class_tables(param)
    d64, u64 = R.tables64(down["fi"], down["fo"]), R.tables64(up["fi"], up["fo"])
    ds = {True: _ds(param), False: _ds(param, same_size=False)}
    assert ds[True].tile == max(1, 2048 // up["out_unit"]) * up["out_unit"]
    shapes = [(B, T, True) for B, T in SHAPES] + [(2, ds[True].tile + 1, True), (2, 25, False), (3, 257, False), (2, ds[True].tile + 1, False)]
    for B, T, same in shapes:
        d = ds[same]
        x, g = _case(B, T, d.out_len(T), seed=B * 100003 + T)
        out, gx = fwd(d, x), bwd(d, g, T)
        assert np.array_equal(bits(out), bits(R.ds32(x, down, up, same))), (param, B, T, same)
        assert np.array_equal(bits(gx), bits(R.ds_adjoint32(g, down, up, T, same))), (param, B, T, same)
        e_out, b_out = np.abs(out - R.ds64(x, d64, u64, same)), R.forward_bound(x, down, up, same)
        e_gx, b_gx = np.abs(gx - R.ds_adjoint64(g, d64, u64, T, same)), R.backward_bound(g, down, up, T, same)
        log("ds param %g B %d T %d same %d: out err %.3g (bound %.3g), grad err %.3g (bound %.3g)"
            % (param, B, T, same, e_out.max(), b_out.max(), e_gx.max(), b_gx.max()))
        assert (e_out <= b_out).all() and (e_gx <= b_gx).all(), (param, B, T, same)
        assert T < 13 or (np.abs(out).max() > 0.01 and np.abs(gx).max() > 0.01)  # (not a kernel that returns zeros)


# ---------------------------------------------------------------- independence, shapes, refusals
def test_rows_do_not_depend_on_the_batch():
    for param in (0.5, 0.33):
        d = _ds(param)
        T = d.tile + 37
        x, g = _case(3, T, T, seed=4)
        whole, gw = fwd(d, x), bwd(d, g, T)
        for lo, hi in ((0, 1), (1, 2), (2, 3), (0, 2)):
            assert np.array_equal(bits(fwd(d, x[lo:hi])), bits(whole[lo:hi])), (param, lo, hi)
            assert np.array_equal(bits(bwd(d, g[lo:hi], T)), bits(gw[lo:hi])), (param, lo, hi)


def test_shapes_lengths_and_refusals():
    from speakerguard_amd import _native as N_
    from speakerguard_amd.defense import DS
    down, up = R.class_tables(0.5)
    T = 257
    x, g = _case(3, T, T, seed=9)
    xd, gd = torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV)
    want, want_g = R.ds32(x, down, up), R.ds_adjoint32(g, down, up, T)
    d = DS()
    for shape in ((T,), (3, T), (3, 1, T)):
        xi, gi = (xd[0], gd[0]) if len(shape) == 1 else (xd.view(shape), gd.view(shape))
        rows = slice(0, 1) if len(shape) == 1 else slice(None)
        o, sv = d.fwd(xi)
        gx = d.bwd(sv, gi)
        assert o.shape == shape and gx.shape == shape
        assert np.array_equal(bits(o.cpu().numpy().reshape(-1, T)), bits(want[rows]))
        assert np.array_equal(bits(gx.cpu().numpy().reshape(-1, T)), bits(want_g[rows]))
        assert torch.equal(d(xi), o)
    # same_size=False: the up-sampler's own length, one more for odd T
    d2 = DS(same_size=False)
    o, sv = d2.fwd(xd.view(3, 1, T))
    assert o.shape == (3, 1, T + 1) and np.array_equal(bits(o.cpu().numpy()[:, 0]), bits(R.ds32(x, down, up, False)))
    assert torch.equal(o[..., :T], d(xd.view(3, 1, T)))
    g2 = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, (3, 1, T + 1)).astype(np.float32)).to(DEV)
    assert np.array_equal(bits(d2.bwd(sv, g2).cpu().numpy()[:, 0]), bits(R.ds_adjoint32(g2.cpu().numpy()[:, 0], down, up, T, False)))
    assert d2.fwd(xd[:, :256])[0].shape == (3, 256)
    # refusals
    with pytest.raises(N_.NativeError):
        d(torch.zeros(2, 300))
    with pytest.raises(NotImplementedError):
        d(torch.zeros(2, 2, 300, device=DEV))
    with pytest.raises(ValueError):
        d.bwd(d.fwd(xd)[1], gd[:2])
    with pytest.raises(ValueError):
        d2.bwd(sv, gd.view(3, 1, T))  # the cotangent of the untruncated output has T + 1 samples
    with pytest.raises(ValueError):
        DS(0.335)  # 67 phases of 37 taps: past the table bound, said at construction
    # ... and by the library, before any launch
    assert fwd(d, x, raw=True) == 0
    for B, T_, N in ((0, T, T), (3, 0, 0), (3, T, T + 1), (3, T + 1, T)):
        assert fwd(d, x, raw=True, B=B, T=T_, N=N) == 1, (B, T_, N)
    wide = N_.WavResample()
    C.memmove(C.byref(wide), C.byref(d._spec), C.sizeof(wide))
    first = np.zeros(100, np.int32) - 6
    weight = np.zeros((100, 21), np.float32)
    wide.up.in_unit, wide.up.out_unit, wide.up.W = 3, 100, 21
    wide.up.first, wide.up.weight = first.ctypes.data_as(C.POINTER(C.c_int32)), weight.ctypes.data_as(C.POINTER(C.c_float))
    assert fwd(d, x, raw=True, spec=wide) == 1
    ctx = _ctx()
    assert b"2048" in ctx.lib.sg_last_error(ctx.handle)
    weight = d.up["weight"].copy()
    weight[1, 3] = np.inf
    C.memmove(C.byref(wide), C.byref(d._spec), C.sizeof(wide))
    wide.up.weight = weight.ctypes.data_as(C.POINTER(C.c_float))
    assert fwd(d, x, raw=True, spec=wide) == 1
    assert ctx.lib.sg_wav_resample_forward(ctx.handle, C.byref(d._spec), None, 3, T, N_._ptr(xd), T, None) == 1
    assert ctx.lib.sg_wav_resample_backward(ctx.handle, C.byref(d._spec), N_._ptr(xd), 3, T, T, None, None) == 1
    assert ctx.lib.sg_wav_resample_backward(ctx.handle, None, N_._ptr(xd), 3, T, T, N_._ptr(gd), None) == 1
    torch.cuda.synchronize()


def test_tables_pushed_out_of_the_cache_come_back_the_same():
    """the context keeps the tables of 32 specs, keyed by content: 32 other specs (DS(0.5)'s tables with one weight's last bit
    flipped, another weight each time) push the original's out, freed behind the stream; rebuilt, they give the first call's bits"""
    from speakerguard_amd import _native as N_
    d = _ds(0.5)
    B, T = 2, 1000
    x, g = _case(B, T, T, seed=21)
    first = fwd(d, x), bwd(d, g, T)
    assert np.abs(first[0]).max() > 0.01 and np.abs(first[1]).max() > 0.01
    n_down = d.down["weight"].size
    assert n_down + d.up["weight"].size >= 32
    for k in range(32):
        down, up = np.ascontiguousarray(d.down["weight"], np.float32).copy(), np.ascontiguousarray(d.up["weight"], np.float32).copy()
        (down if k < n_down else up).reshape(-1).view(np.uint32)[k if k < n_down else k - n_down] ^= 1
        spec = N_.WavResample()
        C.memmove(C.byref(spec), C.byref(d._spec), C.sizeof(spec))
        spec.down.weight, spec.up.weight = (w.ctypes.data_as(C.POINTER(C.c_float)) for w in (down, up))
        fwd(d, x, spec=spec), bwd(d, g, T, spec=spec)
    again = fwd(d, x), bwd(d, g, T)
    assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(bits(again[1]), bits(first[1]))


# ---------------------------------------------------------------- the adjoint, from the device's outputs
@pytest.mark.parametrize("param", (0.5, 0.3, 0.33))
def test_adjoint_identity(param):
    """<DS x, g> = <x, DS^T g> accumulated in float64: each side carries the kernel's error against the float64-table
    operator -- which IS its own adjoint's transpose -- once, so the gap is within the two bounds weighted by |g| and |x|"""
    down, up = R.class_tables(param)
    d = _ds(param)
    for same in (True, False):
        d = _ds(param, same)
        T = d.tile + 301
        x, g = _case(2, T, d.out_len(T), seed=11)
        y, gx = fwd(d, x), bwd(d, g, T)
        lhs, rhs = float((y.astype(np.float64) * g).sum()), float((x.astype(np.float64) * gx).sum())
        tol = float((R.forward_bound(x, down, up, same) * np.abs(g)).sum() + (R.backward_bound(g, down, up, T, same) * np.abs(x)).sum())
        log("ds adjoint param %g same %d: |lhs - rhs| %.3g (tol %.3g, |lhs| %.3g)" % (param, same, abs(lhs - rhs), tol, abs(lhs)))
        assert abs(lhs - rhs) <= tol and tol < 1e-3 * float((np.abs(y).astype(np.float64) * np.abs(g)).sum())


# ---------------------------------------------------------------- through the product
def _waves(B, T, seed=3):
    from speakerguard_amd import synth
    x = synth.make_waveforms(B, T, seed=seed)
    return torch.from_numpy((x * np.float32(0.5 / max(0.5, float(np.abs(x).max())))).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("which", [0, 1], ids=["xv_plda", "audionet"])
def test_gradient_inside_defended_model(which):
    """d loss / d wav with DS in the chain.  (a) The bound LPF gets in this position (test_gpu_freq_domain.py): the defended
    model's gradient IS the hand-chained one, bit for bit.  (b) DS's own factor against autograd of its torch form (float64
    conv1d, the float64 formula's tables), on the cotangent the model hands it: within the a-priori bound of the contract."""
    from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
    from speakerguard_amd.defense import AS, DS
    from speakerguard_amd.model.defended_model import defended_model
    name, make, T = _models()[which]
    assert T == (XV_T, AN_T)[which]
    base = make()
    x = _waves(3, T)
    ce = SEC4SR_CrossEntropy(reduction='none', task='CSI')
    for chain in ([DS()], [DS(0.25), AS(3)]):
        dm = defended_model(base, [(0, d) for d in chain])
        y = dm.make_decision(x)[0]
        h, saved = x, []
        for d in chain:
            h, sv = d.fwd(h)
            saved.append(sv)
        assert float(h.abs().max()) <= 1 / 0.9
        g = base.loss_grad(h, y, ce)[3]
        for d, sv in zip(reversed(chain[1:]), reversed(saved[1:])):
            g = d.bwd(sv, g)
        g_ds = g  # the cotangent at DS's output
        g = chain[0].bwd(saved[0], g_ds)
        got = dm.loss_grad(x, y, ce)[3]
        assert torch.equal(got, g) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
        # autograd through the torch form
        down, up = R.class_tables(chain[0].param)
        d64, u64 = R.tables64(down["fi"], down["fo"]), R.tables64(up["fi"], up["fo"])
        xin = x.cpu().double().requires_grad_(True)
        yt = R.ds_torch(xin, d64, u64)
        gt, = torch.autograd.grad(yt, xin, g_ds.cpu().double())
        out_ds = chain[0](x)
        e_out = (out_ds.cpu().double() - yt.detach()).abs().numpy()[:, 0]
        e_g = (g.cpu().double() - gt).abs().numpy()[:, 0]
        b_out = R.forward_bound(x.cpu().numpy()[:, 0], down, up)
        b_g = R.backward_bound(g_ds.cpu().numpy()[:, 0], down, up, T)
        log("ds in %s, chain %s: out err %.3g (bound %.3g), grad err %.3g (bound %.3g, max |grad| %.3g)"
            % (name, "-".join(type(d).__name__ for d in chain), e_out.max(), b_out.max(), e_g.max(), b_g.max(), float(gt.abs().max())))
        assert (e_out <= b_out).all() and (e_g <= b_g).all(), name


@pytest.mark.parametrize("which", [0, 1], ids=["xv_plda", "audionet"])
def test_attacks_run_on_the_step_loop(which):
    from speakerguard_amd.attack.CWinf import CWinf
    from speakerguard_amd.attack.FGSM import FGSM
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense import DS
    from speakerguard_amd.model.defended_model import defended_model
    name, make, T = _models()[which]
    base = make()
    x = _waves(4, T)
    dm = defended_model(base, [(0, DS())])
    y = dm.make_decision(x)[0]
    eps, step = 0.002, 0.0004
    kw = dict(task="CSI", epsilon=eps, step_size=step, max_iter=5, batch_size=4, verbose=0)
    for cls in (PGD, CWinf):
        atk = cls(dm, **kw)
        assert atk._device_route(4) is None, (name, cls.__name__)
        adv = atk.attack(x, y)[0]
        assert float((adv - x).abs().max()) <= eps + 1e-7 and not torch.equal(adv, x), (name, cls.__name__)
        assert torch.equal(cls(dm, **kw).attack(x, y)[0], adv), (name, cls.__name__)
        # the same attack as a hand-written loop over loss_grad / pgd_update
        base.begin_attack()
        base.begin_batch(0, 1)
        xa = x.clone()
        lower, upper = torch.clamp(x - eps, min=-1).contiguous(), torch.clamp(x + eps, max=1).contiguous()
        for _ in range(5):
            g = dm.loss_grad(xa, y, atk.loss, want_grad=True)[3]
            base.pgd_update(xa, g.contiguous(), lower, upper, step, atk.grad_sign)
        assert torch.equal(xa, adv), (name, cls.__name__)
    for atk in (FGSM(dm, task="CSI", epsilon=eps, batch_size=4, verbose=0),
                PGD(dm, **dict(kw, max_iter=2, EOT_size=2, EOT_batch_size=2))):
        assert atk._device_route(4) is None
        adv = atk.attack(x, y)[0]
        assert float((adv - x).abs().max()) <= eps + 1e-7 and not torch.equal(adv, x), (name, type(atk).__name__)
        assert torch.equal(atk.attack(x, y)[0], adv), (name, type(atk).__name__)
