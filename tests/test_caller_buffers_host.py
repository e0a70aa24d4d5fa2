"""tests/caller_buffers.py on the CPU: the windows are where they claim to be, the judge rejects what it exists to reject, and
every entry point of the C-ABI that takes a caller's device buffer is placed in the GPU sweep (tests/test_gpu_caller_buffers.py)
or carries a reason why not.  No GPU: the "entry points" here are numpy functions that take raw addresses like the real ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import caller_buffers as cb
from conftest import ROOT
from speakerguard_amd import _native

K = (0, 1, 2, 3)


def filled(dtype, n=37):
    g = torch.Generator().manual_seed(n)
    if dtype.is_floating_point:
        return (torch.rand(n, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    hi = {torch.uint8: 255, torch.int16: 30000}.get(dtype, 2 ** 30)
    return torch.randint(0, hi, (n,), generator=g).to(dtype)


# ---------------------------------------------------------------- 1. window: residue, contiguity, content, guards
@pytest.mark.parametrize("k", K)
@pytest.mark.parametrize("dtype", cb.DTYPES, ids=lambda d: str(d).split(".")[1])
def test_window_residue_contiguity_content(dtype, k):
    t = filled(dtype).reshape(1, 37)
    w = cb.window(t, k)
    size = t.element_size()
    assert w.data_ptr() % 16 == (k * size) % 16 == cb.residue(dtype, k)
    if dtype == torch.float32:
        assert w.data_ptr() % 16 == 4 * k
    assert w.is_contiguous() and w.shape == t.shape and w.dtype == t.dtype
    assert cb.first_difference(t, w) is None
    buf, start, n, guard = w.cb_frame
    assert guard == 64 and n == 37 and start >= guard and buf.numel() >= start + n + guard
    assert w.data_ptr() == buf.data_ptr() + start * size
    want = cb.bits(torch.full((guard,), cb.poison_of(dtype), dtype=dtype))
    assert torch.equal(cb.bits(buf[start - guard:start]), want) and torch.equal(cb.bits(buf[start + n:start + n + guard]), want)
    assert cb.intact(w)
    if dtype.is_floating_point:
        assert float(buf[0]) == 2.0 ** 100 and np.isfinite(float(buf[0]))


@pytest.mark.parametrize("dtype", cb.DTYPES, ids=lambda d: str(d).split(".")[1])
def test_intact_is_bit_for_bit(dtype):
    """a guard element that changes in its last bit only, at either far end of a guard, is seen"""
    for where in ("first", "last"):
        for side in ("before", "after"):
            w = cb.window(filled(dtype), 1)
            buf, start, n, guard = w.cb_frame
            lo = start - guard if side == "before" else start + n
            i = lo if where == "first" else lo + guard - 1
            v = cb.bits(buf)
            v[i] = v[i] ^ 1
            assert not cb.intact(w) and side in cb.guard_report(w)


def test_judge_accepts_the_honest_call():
    for k in K:
        x = filled(torch.float32)
        w = cb.window(x, k)
        ok, why = cb.same({"y": x * 2}, {"y": w * 2}, [w])
        assert ok and why == "bit-equal, guards intact"


def test_judge_compares_bits_not_values():
    a, b = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    assert torch.equal(a, b)
    ok, why = cb.same({"y": a}, {"y": b}, [])
    assert not ok and "output y" in why and "first at 0" in why
    nan = torch.tensor([float("nan")])
    assert cb.same({"y": nan}, {"y": nan.clone()}, [])[0]


# ---------------------------------------------------------------- 2. the judge's power (style of test_truth_power.py)
def as_array(addr, n, ctype=C.c_float):
    return np.ctypeslib.as_array((ctype * n).from_address(addr))


def ep_scale(x_ptr, out_ptr, n):
    """the honest entry point: out = 2 x"""
    as_array(out_ptr, n)[:] = 2 * as_array(x_ptr, n)


def ep_writes_one_past(x_ptr, out_ptr, n):
    """a vector store that runs one element past a ragged row"""
    as_array(out_ptr, n + 1)[:] = np.concatenate([2 * as_array(x_ptr, n), [0.0]]).astype(np.float32)


def ep_writes_one_before(x_ptr, out_ptr, n):
    as_array(out_ptr - 4, n + 1)[:] = np.concatenate([[0.0], 2 * as_array(x_ptr, n)]).astype(np.float32)


def ep_aligned_only(x_ptr, out_ptr, n):
    """a 16-byte load whose address lost its low bits: right at k = 0 only"""
    as_array(out_ptr, n)[:] = 2 * as_array(x_ptr & ~15, n)


def red_max(x_ptr, out_ptr, n):
    as_array(out_ptr, 1)[0] = as_array(x_ptr, n).max()


def red_max_overread(x_ptr, out_ptr, n):
    """a max that reads one element past the row: the guard's 2^100 wins (a NaN would have been dropped)"""
    as_array(out_ptr, 1)[0] = np.fmax.reduce(as_array(x_ptr, n + 1))


def red_sum(x_ptr, out_ptr, n):
    as_array(out_ptr, 1)[0] = as_array(x_ptr, n).sum(dtype=np.float32)


def red_sum_underread(x_ptr, out_ptr, n):
    """a sum that starts one element before the row"""
    as_array(out_ptr, 1)[0] = as_array(x_ptr - 4, n + 1)[1:].sum(dtype=np.float32) + as_array(x_ptr - 4, 1)[0]


def judged(ep, honest, k, n_out=None):
    """the GPU sweep's procedure on a fake entry point: expected from fresh tensors, got on windows -> the judge's verdict"""
    x = filled(torch.float32, 37)
    n = x.numel()
    exp = torch.zeros(n if n_out is None else n_out)
    honest(x.data_ptr(), exp.data_ptr(), n)
    wx, wo = cb.window(x, k), cb.window(torch.zeros_like(exp), k)
    ep(wx.data_ptr(), wo.data_ptr(), n)
    return cb.same({"out": exp}, {"out": wo}, [("x", wx), ("out", wo)])


@pytest.mark.parametrize("k", K)
def test_judge_passes_the_honest_entry_points(k):
    assert judged(ep_scale, ep_scale, k)[0]
    assert judged(red_max, red_max, k, 1)[0]
    assert judged(red_sum, red_sum, k, 1)[0]


@pytest.mark.parametrize("k", K)
def test_judge_rejects_a_write_past_the_window(k):
    ok, why = judged(ep_writes_one_past, ep_scale, k)
    assert not ok and "out" in why and "1 element(s) past its end" in why, why


@pytest.mark.parametrize("k", K)
def test_judge_rejects_a_write_before_the_window(k):
    ok, why = judged(ep_writes_one_before, ep_scale, k)
    assert not ok and "out" in why and "1 element(s) before its start" in why, why


@pytest.mark.parametrize("k", K)
def test_judge_rejects_a_result_that_folds_the_guard_in(k):
    ok, why = judged(red_max_overread, red_max, k, 1)
    assert not ok and "output out" in why, why
    ok, why = judged(red_sum_underread, red_sum, k, 1)
    assert not ok and "output out" in why, why


def test_a_nan_poison_would_have_hidden_the_overread():
    """why the poison is finite: fmax drops a NaN, and the over-reading max would pass"""
    x = filled(torch.float32, 37)
    padded = np.concatenate([x.numpy(), [np.nan]]).astype(np.float32)
    assert np.fmax.reduce(padded) == x.numpy().max()


def test_judge_rejects_right_at_k0_only():
    assert judged(ep_aligned_only, ep_scale, 0)[0]
    for k in (1, 2, 3):
        ok, why = judged(ep_aligned_only, ep_scale, k)
        assert not ok and "output out" in why, (k, why)


# ---------------------------------------------------------------- Relocated, on a fake context
def test_relocated_moves_every_buffer_and_restores_the_binding(monkeypatch):
    seen = []

    def fake_call(self, name, *args):
        x, out = args[0].value, args[1].value
        seen.append((x % 16, out % 16))
        ep_scale(x, out, 37)

    monkeypatch.setattr(_native.Context, "call", fake_call)
    ctx = _native.Context.__new__(_native.Context)
    ctx.handle = None
    x = filled(torch.float32)
    for k, want in ((2, (8, 8)), ("mixed", (4, 8))):
        out = torch.zeros(37)
        with cb.Relocated(k, host_too=True) as r:
            ctx.call("sg_fake", _native._ptr(x), _native._ptr(out))
            assert _native._ptr(None) is None
        assert seen[-1] == want and r.entries == {"sg_fake": 2} and len(r.windows) == 2
        assert cb.same({"out": 2 * x}, {"out": out}, r.windows)[0]
        assert _native.Context.call is fake_call
    assert _native._ptr(x).value == x.data_ptr()


# ---------------------------------------------------------------- 3. every entry point of the ABI is placed
def header_params(name):
    text = open(os.path.join(ROOT, "include", "speakerguard_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def prototype(name):
    """(argtypes of the binding, parameters of the header's declaration) of an export"""
    return getattr(_native.load(), name).argtypes, header_params(name)


def caller_pointer_count(name):
    """c_void_p arguments of the binding's prototype, less the context handle and the stream"""
    argtypes, params = prototype(name)
    n = sum(1 for a in argtypes if a is C.c_void_p)
    return n - int(params[0] in ("sg_ctx* ctx", "const sg_ctx* ctx")) - int(params[-1] == "void* stream")


def entries_with_caller_buffers():
    return {name for name in _native.EXPORTS if caller_pointer_count(name) > 0}


def test_the_derivation_reads_the_prototypes():
    assert caller_pointer_count("sg_sync") == 0 and caller_pointer_count("sg_health") == 0
    assert caller_pointer_count("sg_pgd_update") == 4 and caller_pointer_count("sg_input_scale") == 2
    assert caller_pointer_count("sg_xv_time_layer") == 0  # (typed host pointers)
    assert caller_pointer_count("sg_stoi_debug_tables") == 1 and caller_pointer_count("sg_iv_load") == 1


def test_every_entry_with_a_caller_buffer_is_swept_or_excused():
    import test_gpu_caller_buffers as sweep
    swept, excused = set(sweep.SWEPT), set(sweep.NOT_SWEPT)
    assert not swept & excused
    have = entries_with_caller_buffers()
    assert have - (swept | excused) == set(), "entry points nobody placed: add a case to the sweep (or a reason to NOT_SWEPT)"
    assert (swept | excused) - have == set(), "placed, but the binding shows no caller's buffer"
    assert len(swept) >= 60
    for name, reason in sweep.NOT_SWEPT.items():
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason, name
        assert re.search(r"_(load|set_enroll)$|^sg_(trace|debug|stoi_debug)_|_debug_", name), \
            "%s is not a debug, trace, load or enrol call: it belongs in the sweep" % name
        assert "host" in reason, "NOT_SWEPT holds calls that take host pointers only (%s)" % name


def test_an_entry_added_later_fails_until_placed(monkeypatch):
    """the assertion above, made to bite: the binding gains an export with a device buffer that nobody placed, and the test
    above must fail naming it; one without a caller's buffer passes untouched"""
    import sys
    real = prototype
    vp, i32 = C.c_void_p, C.c_int32
    fakes = {"sg_new_kernel": ([vp, vp, i32, vp], ["sg_ctx* ctx", "float* x_dev", "int32_t n", "void* stream"]),
             "sg_new_knob": ([vp, i32], ["sg_ctx* ctx", "int32_t mode"])}
    monkeypatch.setattr(sys.modules[__name__], "prototype", lambda name: fakes[name] if name in fakes else real(name))
    monkeypatch.setattr(_native, "EXPORTS", _native.EXPORTS + ("sg_new_knob",))
    test_every_entry_with_a_caller_buffer_is_swept_or_excused()
    monkeypatch.setattr(_native, "EXPORTS", _native.EXPORTS + ("sg_new_kernel",))
    with pytest.raises(AssertionError, match="nobody placed") as err:
        test_every_entry_with_a_caller_buffer_is_swept_or_excused()
    assert "sg_new_kernel" in str(err.value)
