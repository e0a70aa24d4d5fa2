"""The implicit-GEMM convolution kernels in isolation (C-ABI sg_conv1d_rows) against the numpy oracle.

Every launch strategy (one block per tile, 16 x 16 blocks, stream-K with the b32-fed 8-wave kernel, with the 8-wave and the
16-wave quad-fed kernels and with the wave-specialised kinds -- which of them a TDNN layer gets depends on its shape and the
batch: conv_plan, csrc/sg_internal.h) must give BIT-IDENTICAL results -- that is what makes a batch shard
reproduce the unsharded batch exactly -- and all must agree with the float64 oracle to fp32 accumulation error.
"""
import numpy as np
import pytest
import torch

from oracle.conv_rows import conv1d_rows, conv1d_torch_layout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from speakerguard_amd import _native as N
    return N.Context()


def _run(ctx, a, w, B, Ta, Tc, taps, step, base, epi, kernel, bias=None, mask=None):
    from speakerguard_amd import _native as N
    dev = torch.device("cuda:0")
    Kc, n = a.shape[1], w.shape[1]
    ta, tw = torch.from_numpy(a).to(dev), torch.from_numpy(w).to(dev)
    tb = torch.from_numpy(bias).to(dev) if bias is not None else None
    tm = torch.from_numpy(mask).to(dev) if mask is not None else None
    out = torch.full((B * Tc, n), float("nan"), device=dev)
    ctx.call("sg_conv1d_rows", N._ptr(ta), N._ptr(tw), N._ptr(out), N._ptr(tb) if tb is not None else None,
             N._ptr(tm) if tm is not None else None, B, Ta, Tc, Kc, n, taps, step, base, epi, kernel,
             N.current_stream_ptr(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(seed, B, Ta, Tc, Kc, n, taps):
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((B * Ta, Kc)).astype(np.float32)
    w = (rng.standard_normal((taps * Kc, n)) / np.sqrt(taps * Kc)).astype(np.float32)
    return a, w


# (B, Ta, Tc, Kc, N, taps, step, base): the two big ones qualify for stream-K (>= 512 tiles of 128x128)
SHAPES = [
    pytest.param((64, 270, 266, 192, 512, 3, 2, 0), id="fwd_streamk_dil2"),
    pytest.param((64, 266, 270, 192, 512, 3, -2, 0), id="dgrad_streamk_edges"),
    # medium / small batches: fewer 256-row tiles than CUs -> stream-K with one 8-wave 128x128 block per CU (B = 32)
    # or one 4-wave 64x128 block per CU (B = 16)
    pytest.param((32, 270, 266, 192, 512, 3, 2, 0), id="fwd_streamk_mid_128row"),
    pytest.param((32, 266, 270, 192, 512, 3, -2, 0), id="dgrad_streamk_mid_128row"),
    pytest.param((16, 270, 266, 192, 512, 3, 2, 0), id="fwd_streamk_small_64row"),
    pytest.param((16, 266, 270, 192, 512, 3, -2, 0), id="dgrad_streamk_small_64row"),
    pytest.param((8, 270, 266, 192, 512, 3, 2, 0), id="fwd_streamk_tiny_32row"),
    pytest.param((8, 266, 270, 192, 512, 3, -2, 0), id="dgrad_streamk_tiny_32row"),
    pytest.param((3, 50, 46, 64, 128, 5, 1, 0), id="fwd_small_ragged_tile"),
    pytest.param((2, 40, 46, 96, 256, 3, -3, 0), id="dgrad_small"),
    pytest.param((5, 33, 33, 32, 128, 3, 1, -1), id="same_padding_tap_base"),
]


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_rows_matches_oracle_and_all_kernels_agree(ctx, shape):
    B, Ta, Tc, Kc, n, taps, step, base = shape
    a, w = _case(7, B, Ta, Tc, Kc, n, taps)
    want = conv1d_rows(a, w, B, Ta, Tc, taps, step, base)
    outs = [_run(ctx, a, w, B, Ta, Tc, taps, step, base, 0, k) for k in (0, 1, 2, 3, 4, 5)]
    scale = np.abs(want).max()
    for k, o in enumerate(outs):
        assert np.isfinite(o).all(), "kernel %d left rows unwritten" % k
        err = np.abs(o - want).max() / scale
        assert err < 2e-5, "kernel %d: rel err %.3e" % (k, err)  # fp32 accumulation over K <= 576
    assert np.array_equal(outs[0], outs[1]), "quad-fed stream-K differs from the tile launch"
    assert np.array_equal(outs[2], outs[1]), "b32-fed stream-K differs from the tile launch"
    assert np.array_equal(outs[3], outs[1]), "8-wave quad-fed stream-K differs from the tile launch"
    assert np.array_equal(outs[4], outs[1]), "quad-fed tile launch differs from the b32-fed tile launch"
    # v_mfma_f32_16x16x4_f32 fed the k values in the order the 32x32x2 kernels consume them: the same fmaf chain
    assert np.array_equal(outs[5], outs[1]), "16 x 16 blocks (small-batch kernel) differ from the tile launch"
    # round 3: the wave-specialised stream-K kernels (computing waves + four staging waves, three LDS stages), forced on
    # every shape that qualifies (enough tiles for 256 workers, a range >= one tile's chunks)
    chunks = taps * (Kc // 32)
    for k, rows in ((6, 128), (7, 64), (8, 32), (9, 256), (10, 128)):
        tiles = -(-(B * Tc) // rows) * (n // 128)
        if chunks >= 16 and tiles >= 256 and -(-tiles * chunks // 256) >= chunks:
            o = _run(ctx, a, w, B, Ta, Tc, taps, step, base, 0, k)
            assert np.array_equal(o, outs[1]), "wave-specialised stream-K with %d-row tiles differs from the tile launch" % rows
    # and all of them ARE the documented arithmetic: one float32 fmaf chain per output in the kernels' k order, restated
    # in C on the CPU (oracle/conv_chain.c) -- bit for bit, signs of zeros included
    from oracle.conv_chain import conv_chain
    chain = conv_chain(a, w, B, Ta, Tc, taps, step, base)
    assert np.array_equal(outs[1].view(np.uint32), chain.view(np.uint32)), "device result is not the restated fmaf chain"


@pytest.mark.parametrize("B", [8, 16, 32, 64])
@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_real_tdnn3_shape_is_the_restated_fmaf_chain(ctx, B, direction):
    """The contraction of the real tdnn3 layer (xvecTDNN.py:24-26: 512 -> 512 channels, 7 taps, dilation 3: K = 3584, 112
    chunks) at the per-GPU shard sizes of a batch of 64 over 8 / 4 / 2 / 1 GPUs, through the launcher's own choice of
    kernel (deep stream-K with 32- / 64- / 128-row tiles, 16-wave stream-K at 64): bit for bit the C restatement
    oracle/conv_chain.c, forward and data gradient (hardware-zero-filled taps at the utterance edges)."""
    from oracle.conv_chain import conv_chain
    Kc, n, taps = 512, 512, 7
    Ta, Tc, step = (288, 270, 3) if direction == "fwd" else (270, 288, -3)
    base = 0  # dgrad: output row t (an input frame) collects the d(out) rows t - 3 j that exist, as run_tdnn_backward does
    a, w = _case(100 + B, B, Ta, Tc, Kc, n, taps)
    got = _run(ctx, a, w, B, Ta, Tc, taps, step, base, 0, 0)
    chain = conv_chain(a, w, B, Ta, Tc, taps, step, base)
    assert np.array_equal(got.view(np.uint32), chain.view(np.uint32))


@pytest.mark.parametrize("B,F", [(64, 300), (8, 300), (3, 125), (1, 100), (5, 208)])
def test_real_tdnn1_forward_shape_is_the_restated_fmaf_chain(ctx, B, F):
    """tdnn1 forward at its real shape (xvecTDNN.py:16-17: 30 -> 512 channels, 5 taps: K = 5 x 32, bias + ReLU epilogue):
    through the launcher's choice (kernel 0) it must be, bit for bit, the C restatement oracle/conv_chain.c and the generic
    one-block-per-tile launch (kernel 1), for full batches, a row count that is no multiple of 32 and short utterances.
    (Round 5 ran this test against a weight-stationary kernel of its own for the layer, which passed it and was dropped for
    not being faster: profiles/r05_experiments.txt.)"""
    from oracle.conv_chain import conv_chain
    Kc, n, taps = 32, 512, 5
    Ta, Tc = F, F - 4
    a, w = _case(300 + B, B, Ta, Tc, Kc, n, taps)
    bias = np.random.RandomState(B).standard_normal(n).astype(np.float32)
    got = _run(ctx, a, w, B, Ta, Tc, taps, 1, 0, 1, 0, bias=bias)
    tiles = _run(ctx, a, w, B, Ta, Tc, taps, 1, 0, 1, 1, bias=bias)
    chain = conv_chain(a, w, B, Ta, Tc, taps, 1, 0, bias=bias)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), tiles.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), chain.view(np.uint32))


def test_streamk_slabs_reused_back_to_back(ctx):
    """the stream-K hand-off parks accumulators in slabs that every launch of a context reuses, published by
    write-through (sc1) stores and a relaxed flag -- a stale line would not raise the health word.  Many launches in a
    row on the same context, a different input every time and the kinds interleaved (16-wave, 8-wave, deep 128 / 64 /
    32 rows: all park into the same slab addresses): every result must equal the one-block-per-tile launch."""
    B, Ta, Tc, Kc, n, taps, step = 64, 270, 266, 192, 512, 3, 2
    rng = np.random.RandomState(17)
    w = (rng.standard_normal((taps * Kc, n)) / 24).astype(np.float32)
    for it in range(12):
        a = rng.standard_normal((B * Ta, Kc)).astype(np.float32)
        ref = _run(ctx, a, w, B, Ta, Tc, taps, step, 0, 0, 4)
        for k in (0, 3, 6, 7, 8, 9, 10, 0):
            assert np.array_equal(_run(ctx, a, w, B, Ta, Tc, taps, step, 0, 0, k), ref), (it, k)


def test_conv_rows_epilogues(ctx):
    B, Ta, Tc, Kc, n, taps, step = 64, 270, 266, 192, 512, 3, 2
    a, w = _case(11, B, Ta, Tc, Kc, n, taps)
    rng = np.random.RandomState(3)
    bias = rng.standard_normal(n).astype(np.float32)
    mask = (rng.standard_normal((B * Tc, n)) > 0).astype(np.float32) * rng.rand(B * Tc, n).astype(np.float32)
    for epi, kw in ((1, dict(bias=bias)), (2, dict(mask=mask))):
        want = conv1d_rows(a, w, B, Ta, Tc, taps, step, 0, **kw)
        o0 = _run(ctx, a, w, B, Ta, Tc, taps, step, 0, epi, 0, **kw)
        o1 = _run(ctx, a, w, B, Ta, Tc, taps, step, 0, epi, 1, **kw)
        o4 = _run(ctx, a, w, B, Ta, Tc, taps, step, 0, epi, 4, **kw)
        assert np.abs(o0 - want).max() / np.abs(want).max() < 2e-5
        assert np.array_equal(o0, o1) and np.array_equal(o4, o1)
        o5 = _run(ctx, a, w, B, Ta, Tc, taps, step, 0, epi, 5, **kw)
        from oracle.conv_chain import conv_chain
        chain = conv_chain(a, w, B, Ta, Tc, taps, step, 0, **kw)
        assert np.array_equal(o5, o1) and np.array_equal(o1.view(np.uint32), chain.view(np.uint32))


def test_conv_rows_is_torch_conv1d(ctx):
    """The row formulation equals torch.nn.functional.conv1d (CPU, float64) on the reference's layout."""
    rng = np.random.RandomState(5)
    x = rng.standard_normal((4, 64, 60)).astype(np.float32)
    wt = (rng.standard_normal((128, 64, 3)) / 14).astype(np.float32)
    ref = torch.nn.functional.conv1d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), dilation=3).numpy()
    assert np.abs(conv1d_torch_layout(x, wt, 3) - ref).max() < 1e-12
    a = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(4 * 60, 64)
    w = np.ascontiguousarray(wt.transpose(2, 1, 0)).reshape(3 * 64, 128)
    got = _run(ctx, a, w, 4, 60, 54, 3, 3, 0, 0, 0).reshape(4, 54, 128).transpose(0, 2, 1)
    assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-5


def test_conv_rows_rejects_bad_shapes(ctx):
    from speakerguard_amd import _native as N
    dev = torch.device("cuda:0")
    t = torch.zeros(64, 64, device=dev)
    with pytest.raises(N.NativeError):
        ctx.call("sg_conv1d_rows", N._ptr(t), N._ptr(t), N._ptr(t), None, None, 1, 64, 64, 48, 128, 1, 1, 0, 0, 0,
                 N.current_stream_ptr(dev))


def test_lost_streamk_handoff_is_reported_not_silent():
    """a hand-off wait that times out used to continue silently with a stale slab.  With the hand-off
    flags of ONE launch suppressed (the library's fault-injection hook sg_debug_lose_handoffs; until round 4 an environment
    switch of the shipped library) the waiting workers give up after a short bound, raise the context's health word, and
    sg_sync / the next pass fail; sg_set_streamk(ctx, 0) -- the documented remedy on a shared GPU -- gives the same bits."""
    from speakerguard_amd import _native as N
    DEV = torch.device("cuda:0")
    ctx = N.Context()
    B, Ta, Tc, Kc, n, taps = 64, 270, 266, 192, 512, 3
    torch.manual_seed(3)
    a = torch.randn(B * Ta, Kc, device=DEV)
    w = torch.randn(taps * Kc, n, device=DEV) / 24

    def run():
        out = torch.empty(B * Tc, n, device=DEV)
        ctx.call("sg_conv1d_rows", N._ptr(a), N._ptr(w), N._ptr(out), None, None, B, Ta, Tc, Kc, n, taps, 2, 0, 0, 0,
                 N.current_stream_ptr(DEV))
        return out

    ctx.call("sg_health")  # clean before
    good = run()
    ctx.call("sg_sync", N.current_stream_ptr(DEV))
    ctx.call("sg_debug_lose_handoffs", 1)
    run()
    with pytest.raises(N.NativeError, match="hand-off"):
        ctx.call("sg_sync", N.current_stream_ptr(DEV))
    ctx.call("sg_health")  # the word is cleared once reported
    again = run()          # the hook covered one launch only
    ctx.call("sg_sync", N.current_stream_ptr(DEV))
    assert torch.equal(again, good)
    ctx.call("sg_set_streamk", 0)
    ctx.call("sg_debug_lose_handoffs", 1)  # nothing to lose: one block per tile
    tiles = run()
    ctx.call("sg_sync", N.current_stream_ptr(DEV))
    assert torch.equal(tiles, good)
    ctx.close()


def test_whole_model_is_bit_identical_with_and_without_streamk(tmp_path):
    """Odd (batch, length) shapes -- ragged last tiles, utterances shorter than a tile, batches that pick the 32- / 64- /
    128- / 256-row wave-specialised kinds and the 16x16 small-batch kernel -- through the WHOLE x-vector pass (scores and
    d loss / d waveform): the launcher's own choice of kernels against the one-block-per-tile launches (SG_STREAMK=0, its own
    process because the knob is read once), bit for bit."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    code = r"""
import sys, numpy as np, torch
from speakerguard_amd import synth
from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
from speakerguard_amd.model.xv_plda import xv_plda
dev = torch.device("cuda:0")
m = xv_plda.from_weights(synth.make_xv_weights(), device=dev, dither=0.0)
out = {}
for B, T in ((9, 48000), (17, 33000), (31, 48000), (33, 20000), (48, 48000), (96, 12000), (12, 100000), (5, 48000), (64, 48000)):
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=B + T)).to(dev)
    y = (torch.arange(B) % 10).to(dev)
    dec, sc, ls, g = m.loss_grad(x, y, SEC4SR_CrossEntropy())
    out["s_%d_%d" % (B, T)] = sc.cpu().numpy()
    out["g_%d_%d" % (B, T)] = g.cpu().numpy()
np.savez(sys.argv[1], **out)
"""
    files = []
    for tag, env in (("auto", {}), ("tiles", {"SG_STREAMK": "0"})):
        f = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        files.append(np.load(f))
    a, b = files
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 18
    for k in a.files:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
