"""Batches of unequal lengths through the x-vector engine (``lengths=``; sg_xv_forward_ragged, sg_xv_loss_grad_ragged,
sg_xv_pgd_run_ragged).

The yardstick is the engine's own uniform path, which the rest of the suite pins against the oracle: utterance b run ALONE at
its own length through ``loss_grad`` / ``PGD.attack``.  The relation asserted is bit equality, not a tolerance -- a row of the
padded batch sees the frames, the CMVN window, the pooling order and the zero taps that it sees alone, and every contraction
output is one fmaf chain whatever its place in the batch ("Batches of unequal lengths").  Padding content
must not matter, and what the backward leaves behind an utterance's own frames must be exact zeros.

Shapes: the lengths put both CMVN branches (F <= 300 / sliding), both pooling branches (F5 <= 384 / above) and a right
reflection that lands mid-row into ONE launch; 9999 is no multiple of 4 or 160.  The four-sample overlap-add needs
B * T_max >= 768000 samples, hence the 12 rows of that test.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS5 = (16000, 9999, 51200, 8000, 67200)  # frames 100, 62, 320, 50, 420
LENGTHS12 = (67200, 9999, 9998, 66001, 16000, 33333, 67200, 8000, 48000, 66001, 9999, 51200)
CONTEXT = (4, 12, 30, 30, 30)  # frames an utterance has lost behind tdnn1 .. tdnn5


def frames(t):
    return (t + 80) // 160


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(xv_weights, dev):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=dev, dither=0.0)


def make_batch(lengths, seed, dev, fill=0.0):
    """utterance b = synth.make_waveforms(1, T_b, seed + b); -> x (B, 1, T_max) with `fill` in the padding, lengths, labels"""
    from speakerguard_amd import synth
    from speakerguard_amd.audio_io import pad_batch
    waves = [torch.from_numpy(synth.make_waveforms(1, t, seed=seed + b))[0] for b, t in enumerate(lengths)]
    x, lens = pad_batch(waves)
    assert lens.dtype == torch.int32 and lens.tolist() == list(lengths) and x.shape == (len(lengths), 1, max(lengths))
    if fill:
        for b, t in enumerate(lengths):
            x[b, 0, t:] = fill
    y = (torch.arange(len(lengths)) * 3) % 10
    return x.to(dev), lens, y.to(dev)


def spec_of(name):
    from speakerguard_amd.attack.utils import resolve_loss
    return resolve_loss(loss_name=name, clip_max=False)[0]


_SOLO = {}


def solo(model, x, lens, y, loss_name, key):
    """utterance b alone at its own length through the uniform path, once per (batch, loss): [(dec, scores, loss, grad)]"""
    if (key, loss_name) not in _SOLO:
        spec = spec_of(loss_name)
        _SOLO[key, loss_name] = [tuple(t.clone() for t in model.loss_grad(x[b:b + 1, :, :t_b].contiguous(), y[b:b + 1], spec))
                                 for b, t_b in enumerate(lens.tolist())]
    return _SOLO[key, loss_name]


def assert_rows_equal_solo(out, ref, lens):
    dec, scores, loss, grad = out
    for b, t_b in enumerate(lens.tolist()):
        d1, s1, l1, g1 = ref[b]
        assert torch.equal(dec[b:b + 1], d1) and torch.equal(scores[b:b + 1], s1) and torch.equal(loss[b:b + 1], l1), b
        assert torch.equal(grad[b, :, :t_b], g1[0]), (b, t_b, float((grad[b, :, :t_b] - g1[0]).abs().max()))
        assert grad[b, :, :t_b].abs().max() > 0, b
        assert not grad[b, :, t_b:].any(), (b, "gradient in the padding")


# ------------------------------------------------------------------------------ 1. loss_grad
@pytest.mark.parametrize("loss_name", ["Entropy", "Margin"])
def test_loss_grad_rows_equal_the_solo_runs_and_padding_does_not_matter(model, dev, loss_name):
    x, lens, y = make_batch(LENGTHS5, 40, dev)
    out = [t.clone() for t in model.loss_grad(x, y, spec_of(loss_name), lengths=lens)]
    assert_rows_equal_solo(out, solo(model, x, lens, y, loss_name, "five"), lens)
    xf, _, _ = make_batch(LENGTHS5, 40, dev, fill=0.9)
    assert float(xf[1, 0, -1]) == pytest.approx(0.9)
    again = model.loss_grad(xf, y, spec_of(loss_name), lengths=lens)
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    # make_decision / score take the same route
    dec, scores = model.make_decision(xf, lengths=lens)
    assert torch.equal(dec, out[0]) and torch.equal(scores, out[1]) and torch.equal(model.score(xf, lengths=lens), scores)


# ------------------------------------------------------------------------------ 2. what the pass leaves in its buffers
def test_backward_buffers_hold_zeros_behind_every_utterance(model, dev):
    x, lens, y = make_batch(LENGTHS5, 40, dev, fill=0.9)
    spec = spec_of("Entropy")
    model.loss_grad(x, y, spec, lengths=lens)
    B, Fmax = len(LENGTHS5), frames(max(LENGTHS5))
    act5 = model.read_activation(5, B)
    assert act5.shape == (B, Fmax - 30, 1536)
    for l in range(1, 6):
        d = model.read_gradient("dact%d" % l)
        assert d.shape[:2] == (B, Fmax - CONTEXT[l - 1])
        for b, t_b in enumerate(LENGTHS5):
            own = frames(t_b) - CONTEXT[l - 1]
            assert not d[b, own:].any(), (l, b)
            assert d[b, :own].abs().max() > 0, (l, b)
    raw = model.read_gradient("dfeats_raw")
    assert raw.shape == (B, Fmax, 30)
    for b, t_b in enumerate(LENGTHS5):
        assert not raw[b, frames(t_b):].any(), b
        assert raw[b, :frames(t_b)].abs().max() > 0, b
    for b, t_b in enumerate(LENGTHS5):  # (the solo passes overwrite the workspace: the batch's buffers were read above)
        model.loss_grad(x[b:b + 1, :, :t_b].contiguous(), y[b:b + 1], spec)
        own = frames(t_b) - 30
        assert torch.equal(act5[b, :own], model.read_activation(5, 1)[0]), b


# ------------------------------------------------------------------------------ 3. the four-sample overlap-add
def test_four_sample_overlap_add_with_quads_across_the_end_of_an_utterance(model, dev):
    from speakerguard_amd.attack.PGD import PGD
    x, lens, y = make_batch(LENGTHS12, 60, dev)
    assert x.shape[0] * x.shape[2] >= 768000 and x.shape[2] % 4 == 0 and x.data_ptr() % 16 == 0
    for loss_name in ("Entropy", "Margin"):
        out = [t.clone() for t in model.loss_grad(x, y, spec_of(loss_name), lengths=lens)]
        assert out[3].data_ptr() % 16 == 0
        assert_rows_equal_solo(out, solo(model, x, lens, y, loss_name, "twelve"), lens)
        xf, _, _ = make_batch(LENGTHS12, 60, dev, fill=0.9)
        for a, b in zip(out, model.loss_grad(xf, y, spec_of(loss_name), lengths=lens)):
            assert torch.equal(a, b)
    # one step of the device loop: the update fused into that kernel
    kw = dict(epsilon=0.002, step_size=0.0004, max_iter=1, verbose=0)
    atk = PGD(model, batch_size=12, **kw)
    assert atk._device_route(12) == ("pgd_run", ())
    adv, succ = atk.attack(xf, y, lengths=lens)
    one = PGD(model, batch_size=1, **kw)
    for b, t_b in enumerate(lens.tolist()):
        a1, s1 = one.attack(x[b:b + 1, :, :t_b].contiguous(), y[b:b + 1])
        assert torch.equal(adv[b, :, :t_b], a1[0]) and succ[b] == s1[0], b
        assert not adv[b, :, t_b:].any(), b
    assert (adv - x).abs().max() > 0


# ------------------------------------------------------------------------------ 4. dither
def test_dither_is_keyed_by_utterance_frame_and_sample(xv_weights, dev):
    from speakerguard_amd.model.xv_plda import xv_plda
    m = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=7)
    lengths = (24000, 9999, 16123, 30000)
    x, lens, y = make_batch(lengths, 80, dev, fill=0.9)
    spec, key = spec_of("Entropy"), 0x1234ABCD
    m.begin_batch(index_base=0)
    out = [t.clone() for t in m.loss_grad(x, y, spec, lengths=lens, dither_seed=key)]
    ref = []
    for b, t_b in enumerate(lengths):
        m.begin_batch(index_base=b)
        ref.append(tuple(t.clone() for t in m.loss_grad(x[b:b + 1, :, :t_b].contiguous(), y[b:b + 1], spec, dither_seed=key)))
    assert_rows_equal_solo(out, ref, lens)
    m.begin_batch(index_base=0)
    other = m.loss_grad(x, y, spec, lengths=lens, dither_seed=key + 1)
    assert not torch.equal(other[3], out[3])  # (the dither is on)


# ------------------------------------------------------------------------------ 5. PGD
LENGTHS6 = (16000, 9999, 24000, 8000, 20001, 12345)


def test_pgd3_device_loop_step_loop_and_solo_attacks_agree(model, dev, monkeypatch):
    from speakerguard_amd.attack.PGD import PGD
    x, lens, y = make_batch(LENGTHS6, 90, dev, fill=0.9)
    kw = dict(epsilon=0.002, step_size=0.0004, max_iter=3, verbose=0)
    atk = PGD(model, batch_size=6, **kw)
    assert atk._device_route(6) == ("pgd_run", ())
    adv_dev, succ_dev = atk.attack(x, y, lengths=lens)
    stepper = PGD(model, batch_size=6, **kw)
    monkeypatch.setattr(stepper, "_device_route", lambda n: None)
    adv_step, succ_step = stepper.attack(x, y, lengths=lens)
    assert torch.equal(adv_dev, adv_step) and succ_dev == succ_step
    one = PGD(model, batch_size=1, **kw)
    for b, t_b in enumerate(LENGTHS6):
        a1, s1 = one.attack(x[b:b + 1, :, :t_b].contiguous(), y[b:b + 1])
        assert torch.equal(adv_dev[b, :, :t_b], a1[0]) and succ_dev[b] == s1[0], b
        assert not adv_dev[b, :, t_b:].any(), b
        assert (adv_dev[b, :, :t_b] - x[b, :, :t_b]).abs().max() > 0, b
    # chunks: each is cut to its own longest utterance and padded back; same rows
    adv_c, succ_c = PGD(model, batch_size=4, **kw).attack(x, y, lengths=lens)
    assert torch.equal(adv_c, adv_dev) and succ_c == succ_dev


def test_pgd_eot_over_dither_device_loop_equals_the_replayed_steps(xv_weights, dev):
    """EOT_size 2 in one batch of 2 B rows, dither on: the device loop keys the dither of step `it`, repeat `r` by
    ``fused_pass_seed(base, it, r)``; the step loop's calls replayed with those keys -- one ``loss_grad`` of the repeated rows and
    the repeated lengths per step, repeat r keyed by the kernel's own stride -- give the same audio bit for bit."""
    from speakerguard_amd.model.xv_plda import xv_plda
    m = xv_plda.from_weights(xv_weights, device=dev, dither=1.0, dither_seed=3)
    x, lens, y = make_batch(LENGTHS6, 90, dev)
    B, spec, iters = len(LENGTHS6), spec_of("Entropy"), 3
    keep = (torch.arange(x.shape[2]).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1).to(dev)
    zero = torch.zeros((), device=dev)
    lower = torch.where(keep, torch.clamp(x - 0.002, min=-1), zero)
    upper = torch.where(keep, torch.clamp(x + 0.002, max=1), zero)
    m.begin_batch(index_base=0)
    xa, success, dec, scores, loss, _, _ = m.pgd_run(x, y, lower, upper, spec, 0.0004, iters, 1, eot_size=2, eot_batch_size=2, lengths=lens)
    base = m.last_fused_seed
    xb, y2, lens2 = x.clone(), y.repeat(2), lens.repeat(2)
    for it in range(iters):
        m._rep_rows = B
        try:
            _, _, _, g = m.loss_grad(xb.repeat(2, 1, 1), y2, spec, lengths=lens2, dither_seed=m.fused_pass_seed(base, it, 0))
        finally:
            m._rep_rows = 0
        g = g.view(2, B, 1, -1)
        assert not torch.equal(g[0], g[1])
        m.pgd_update(xb, (g[0] + g[1]).contiguous(), lower, upper, 0.0004, 1)
    d2, s2, l2, _ = m.loss_grad(xb, y, spec, want_grad=False, lengths=lens, dither_seed=m.fused_pass_seed(base, iters, 0))
    assert torch.equal(xa, xb) and torch.equal(dec, d2) and torch.equal(scores, s2) and torch.equal(loss, l2)
    assert not torch.where(keep, zero, xa).any() and (xa - x).abs().max() > 0
    assert success.bool().tolist() == (dec != y).tolist()


# ------------------------------------------------------------------------------ 6. refusals
def refused(model, fn, exc, *words):
    """fn() raises `exc` naming `words`, and the pass sequences launched nothing"""
    caught = []

    def run():
        with pytest.raises(exc) as e:
            fn()
        caught.append(str(e.value))
    assert model.trace_stages(run) == [], "a refused call launched something"
    model.check_health()
    for w in words:
        assert w in caught[0], (w, caught[0])


def test_refusals_come_before_any_launch(model, xv_weights, dev):
    from speakerguard_amd import _native as N, synth
    from speakerguard_amd.attack.CW2 import CW2
    from speakerguard_amd.attack.PGD import PGD
    from speakerguard_amd.defense.time_domain import QT
    from speakerguard_amd.model.defended_model import defended_model
    lengths = (16000, 9999, 8000)
    x, lens, y = make_batch(lengths, 100, dev)
    spec = spec_of("Entropy")
    model.loss_grad(x, y, spec, lengths=lens)  # (tables and workspace exist: a refusal below has nothing to set up)

    def i32(*v):
        return torch.tensor(v, dtype=torch.int32)
    for call in (lambda l: model.loss_grad(x, y, spec, lengths=l), lambda l: model.make_decision(x, lengths=l),
                 lambda l: model.pgd_run(x, y, x - 0.002, x + 0.002, spec, 0.0004, 2, 1, lengths=l)):
        refused(model, lambda: call(i32(16001, 9999, 8000)), ValueError, "lengths[0] = 16001", "exceeds")
        refused(model, lambda: call(i32(16000, 399, 8000)), ValueError, "lengths[1] = 399", "25 ms window")
        refused(model, lambda: call(i32(16000, 9999, 5000)), ValueError, "lengths[2] = 5000", "31 frames", "TDNN context")
        refused(model, lambda: call(i32(15999, 9999, 8000)), ValueError, "no utterance has the padded length 16000")
        refused(model, lambda: call(i32(16000, 9999)), ValueError, "int32 tensor of shape (3,)")
        refused(model, lambda: call(torch.tensor(lengths, dtype=torch.int64)), ValueError, "int32 tensor of shape (3,)")
    refused(model, lambda: model.loss_grad(model.compute_feat(x, flag=1), y, spec, flag=1, lengths=lens), ValueError, "flag 0")
    # the C entries check the host copy themselves (a caller that is not this wrapper)
    out = [torch.empty(3, device=dev, dtype=torch.int64), torch.empty(3, 10, device=dev), torch.empty(3, device=dev), torch.empty_like(x)]
    nat, dz = spec.native(), model._dither(seed=1)
    for bad, words in (((16001, 9999, 8000), ("lengths[0] = 16001 exceeds T_max = 16000",)), ((16000, 399, 8000), ("shorter than one 25 ms window",)),
                       ((16000, 5000, 8000), ("31 frames, too few for the TDNN context",)), ((15999, 9999, 8000), ("no utterance has T_max = 16000",))):
        host = np.asarray(bad, np.int32)
        devl = torch.from_numpy(host).to(dev)
        refused(model, lambda: model.ctx.call("sg_xv_loss_grad_ragged", N._ptr(x), N._ptr(devl), host.ctypes.data_as(C.c_void_p), N._ptr(y), 3,
                                              16000, C.byref(nat), C.byref(dz), *[N._ptr(t) for t in out], model._stream()),
                N.NativeError, *words)
    refused(model, lambda: model.ctx.call("sg_xv_forward_ragged", N._ptr(x), N._ptr(lens.to(dev)), None, 3, 16000, C.byref(dz), None, None, None,
                                          None, model._stream()), N.NativeError, "lengths_host")
    # models and attacks that cannot take lengths say so by name
    defended = defended_model(model, defense=[(0, QT(param=512))])
    refused(model, lambda: defended.make_decision(x, lengths=lens), ValueError, "defended_model")
    refused(model, lambda: defended.loss_grad(x, y, spec, lengths=lens), ValueError, "defended_model")
    refused(model, lambda: PGD(defended, max_iter=2, verbose=0).attack(x, y, lengths=lens), ValueError, "defended_model")
    refused(model, lambda: CW2(model, verbose=0).attack(x, y, lengths=lens), ValueError, "CW2")
    assert torch.equal(defended_model(model).make_decision(x, lengths=lens)[0], model.make_decision(x, lengths=lens)[0])
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.iv_plda import iv_plda
    iv = iv_plda.from_weights(synth.make_iv_weights(), device=dev, dither=0.0, white_box=True)
    yi = y % 4
    for fn in (lambda: iv.make_decision(x, lengths=lens), lambda: iv.loss_grad(x, yi, spec, lengths=lens),
               lambda: PGD(iv, max_iter=1, verbose=0).attack(x, yi, lengths=lens)):
        with pytest.raises(ValueError, match="iv_plda"):
            fn()
    an = audionet_csine.from_weights(synth.make_audionet_state_dict(num_class=10), device=dev)
    for fn in (lambda: an.make_decision(x, lengths=lens), lambda: an.loss_grad(x, y, spec, lengths=lens),
               lambda: PGD(an, max_iter=1, verbose=0).attack(x, y, lengths=lens)):
        with pytest.raises(ValueError, match="audionet_csine"):
            fn()
    # the model still works after all of it
    assert torch.equal(model.loss_grad(x, y, spec, lengths=lens)[3], model.loss_grad(x, y, spec, lengths=lens.clone())[3])


# ------------------------------------------------------------------------------ 7. uniform lengths
def test_equal_lengths_are_the_call_without_lengths(model, dev):
    from speakerguard_amd import synth
    from speakerguard_amd.attack.PGD import PGD
    x = torch.from_numpy(synth.make_waveforms(4, 16123, seed=120)).to(dev)
    y = (torch.arange(4) % 10).to(dev)
    lens = torch.full((4,), 16123, dtype=torch.int32)
    for loss_name in ("Entropy", "Margin"):
        for a, b in zip(model.loss_grad(x, y, spec_of(loss_name), lengths=lens), model.loss_grad(x, y, spec_of(loss_name))):
            assert torch.equal(a, b)
    for a, b in zip(model.make_decision(x, lengths=lens), model.make_decision(x)):
        assert torch.equal(a, b)
    kw = dict(epsilon=0.002, step_size=0.0004, max_iter=2, batch_size=4, verbose=0)
    a1, s1 = PGD(model, **kw).attack(x, y, lengths=lens)
    a2, s2 = PGD(model, **kw).attack(x, y)
    assert torch.equal(a1, a2) and s1 == s2
