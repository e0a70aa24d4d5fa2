"""Every x-vector contraction at the shape the product launches it, pinned to the float32 fmaf chain bit for bit.

The determinism contract (DESIGN.md "Tolerances"): whatever kernel the launcher picks -- 16 x 16 blocks, plain quad-fed
tiles, stream-K with 32- / 64- / 128- / 256-row tiles -- an output element is ONE fmaf chain in the documented k order,
restated in oracle/conv_chain.c.  The choice depends on M, N, the chunk count and the CU count, so it flips layer by layer
and batch by batch; tests/test_gpu_conv.py pins it at tdnn3 (B = 8..64), tdnn1 forward and a synthetic shape.  Here:

(a) forward, in situ: the model's own pass (its host-packed weights, workspace strides and launcher choice) on CMVN-level
    features, every layer's activation read back and compared, over every element, with the chain applied to the previous
    layer's readback and the numpy restatement of the loader's fold (tests/xv_fold.py; proved against the float64 model
    in tests/test_layer_chain_power.py).  Pad channels 1500..1535 of tdnn5 included: exactly +0.
(b) data gradients of tdnn2 / tdnn3 / tdnn4 / tdnn5, isolated at the real shapes through sg_conv1d_rows with the
    launcher's choice (kernel 0) and the ReLU-mask epilogue: equal to the chain and to the one-block-per-tile launch
    (kernel 1), over every element.
(c) the split-K launches, which have no single chain: fc1 forward (48 slabs summed in the tail) and, through it,
    statistics pooling -- the engine's tdnn_emb against a float64 pool + folded fc1 of the engine's own tdnn5 readback,
    with the same computation in float32 torch on the CPU as the yardstick (tests/truth.py constants).

The grid is chosen from the launcher's branch points at 256 CUs (launch_conv_gemm / launch_streamk in k_conv_gemm.hip):
3 s at B = 1, 2, 4, 5, 7, 8, 16, 32, 64 reaches the 16 x 16 blocks, plain quad tiles and kinds 7, 6, 5 and 8 on the N = 512
layers, and 16 x 16 (B = 1), plain tiles (2), kind 7 (4), kind 6 (8) and kind 5 (>= 16) on N = 1536; plus ragged and long
utterances.  Every output element of every case is compared.

The backward half in situ -- tdnn1's data gradient (split-K per tap into slabs the CMVN backward sums), fc1 backward
(split-K into slabs the pooling backward sums), the data gradients as the step launches them, pooling's backward, the CMVN
adjoint and the tail's gradient -- is pinned stage by stage in tests/test_gpu_backward_stages.py, on a readback of the
backward workspace (sg_xv_debug_gradient).
"""
import numpy as np
import pytest
import torch

import truth
import xv_fold
from conftest import log
from oracle.conv_chain import conv_chain

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T3 = 48000
GRID = [(B, T3) for B in (1, 2, 4, 5, 7, 8, 16, 32, 64)] + [(9, 52960), (5, 16123), (2, 192000), (3, 16000)]
SMALL_AND_RAGGED = [(B, T) for B, T in GRID if T != T3 or B < 8]  # tdnn3's data gradient: B = 8..64 is in test_gpu_conv.py


def _id(B, T):
    return "B%d_T%d" % (B, T)


@pytest.fixture(scope="module")
def hip(xv_weights):
    from speakerguard_amd.model.xv_plda import xv_plda
    return xv_plda.from_weights(xv_weights, device=DEV, dither=0.0)


@pytest.fixture(scope="module")
def ora(xv_weights):
    from oracle.xv_plda import XvPlda
    return XvPlda(xv_weights)


@pytest.fixture(scope="module")
def fd(xv_weights):
    return xv_fold.fold(xv_weights["state_dict"])


@pytest.fixture(scope="module")
def ctx():
    from speakerguard_amd import _native as N
    return N.Context()


_FEATS = {}
_PASS = {}  # the latest (B, T) only: the tdnn5 output of 64 x 3 s is 106 MB


def _feats(ora, B, T):
    """CMVN-level features (B, F, 30) of seeded waveforms, from the oracle's front-end."""
    if (B, T) not in _FEATS:
        from speakerguard_amd import synth
        x = torch.from_numpy(synth.make_waveforms(B, T, seed=1000 + B + T))
        with torch.no_grad():
            _FEATS[(B, T)] = ora.compute_feat(x, flag=2).contiguous()
        assert _FEATS[(B, T)].shape == (B, xv_fold.num_frames(T), 30)
    return _FEATS[(B, T)]


def _engine_pass(hip, ora, B, T):
    """The model's own forward on the features of (B, T): [padded features, act1 .. act5] as (B * F_l, C_pad) rows, and
    tdnn_emb (B, 512)."""
    if (B, T) not in _PASS:
        _PASS.clear()
        feats = _feats(ora, B, T)
        F = feats.shape[1]
        fl = xv_fold.layer_frames(F)
        x = feats.to(DEV)
        hip.make_decision(x, flag=2)
        acts = [xv_fold.pad_features(feats.numpy())]
        for l in range(1, 6):
            a = hip.read_activation(l, B).cpu().numpy()
            assert a.shape == (B, fl[l - 1], xv_fold.COUT_PAD[l - 1]), (l, a.shape)
            acts.append(a.reshape(B * fl[l - 1], -1))
        temb = hip._forward(x, 2, want_tdnn=True)[3].cpu().numpy()
        again = hip.read_activation(5, B).cpu().numpy().reshape(acts[5].shape)
        xv_fold.assert_same_bits(again, acts[5], fl[4], "tdnn5 of a second pass on the same features, B=%d T=%d" % (B, T))
        _PASS[(B, T)] = dict(F=F, fl=fl, acts=acts, temb=temb)
    return _PASS[(B, T)]


# ------------------------------------------------------------------------------------------------- (a) forward, in situ
@pytest.mark.parametrize("B,T,layer", [pytest.param(B, T, l, id="%s_tdnn%d" % (_id(B, T), l)) for B, T in GRID for l in range(1, 6)])
def test_forward_layer_in_situ_is_the_restated_fmaf_chain(hip, ora, fd, B, T, layer):
    p = _engine_pass(hip, ora, B, T)
    l = layer - 1
    Ta = p["F"] if l == 0 else p["fl"][l - 1]
    Tc = p["fl"][l]
    got = p["acts"][layer]
    want = conv_chain(p["acts"][l], fd.wf[l], B, Ta, Tc, xv_fold.TAPS[l], xv_fold.DIL[l], 0, bias=fd.bias[l])
    xv_fold.assert_same_bits(got, want, Tc, "tdnn%d forward in situ, B=%d T=%d (M=%d N=%d chunks=%d)"
                             % (layer, B, T, B * Tc, xv_fold.COUT_PAD[l], xv_fold.TAPS[l] * xv_fold.CIN_PAD[l] // 32))
    pad = got[:, xv_fold.COUT[l]:]
    assert not pad.view(np.uint32).any(), "pad channels of tdnn%d are not exactly +0" % layer


# ------------------------------------------------------------------------------------ (b) data gradients, real shapes
def _conv_rows(ctx, a, w, B, Ta, Tc, taps, step, mask, kernel):
    from speakerguard_amd import _native as N
    Kc, n = a.shape[1], w.shape[1]
    ta, tw, tm = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (a, w, mask))
    out = torch.full((B * Tc, n), float("nan"), device=DEV)
    ctx.call("sg_conv1d_rows", N._ptr(ta), N._ptr(tw), N._ptr(out), None, N._ptr(tm), B, Ta, Tc, Kc, n, taps, step, 0, 2,
             kernel, N.current_stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dgrad_case(ctx, fd, layer, B, T, mask, seed):
    """d(out) of layer `layer` (seeded normal rows, pad channels included) -> d(in) under `mask` (B * F_{l-1}, C_in)."""
    l = layer - 1
    fl = xv_fold.layer_frames(xv_fold.num_frames(T))
    Ta, Tc = fl[l], fl[l - 1]
    Kc, taps, step = xv_fold.COUT_PAD[l], xv_fold.TAPS[l], -xv_fold.DIL[l]
    a = np.random.RandomState(seed).standard_normal((B * Ta, Kc)).astype(np.float32)
    w = fd.wb[l]
    assert mask.shape == (B * Tc, xv_fold.CIN_PAD[l])
    what = "tdnn%d data gradient, B=%d T=%d (M=%d N=%d chunks=%d)" % (layer, B, T, B * Tc, w.shape[1], taps * Kc // 32)
    got = _conv_rows(ctx, a, w, B, Ta, Tc, taps, step, mask, 0)
    tiles = _conv_rows(ctx, a, w, B, Ta, Tc, taps, step, mask, 1)
    want = conv_chain(a, w, B, Ta, Tc, taps, step, 0, mask=mask)
    xv_fold.assert_same_bits(got, want, Tc, what + ", launcher's choice vs chain")
    xv_fold.assert_same_bits(tiles, want, Tc, what + ", one block per tile vs chain")
    xv_fold.assert_same_bits(got, tiles, Tc, what + ", launcher's choice vs one block per tile")


@pytest.mark.parametrize("B,T,layer", [pytest.param(B, T, l, id="%s_tdnn%d" % (_id(B, T), l)) for B, T in GRID for l in (2, 4, 5)])
def test_data_gradient_at_the_real_shape_is_the_restated_fmaf_chain(hip, ora, fd, ctx, B, T, layer):
    """tdnn2 (5 taps, step -2, 80 chunks), tdnn4 (16 chunks: the stream-K qualification edge) and tdnn5 (Kc = 1536, 48
    chunks), with the folded transposed weights; the mask is the ReLU output of the layer below from the model's own pass."""
    mask = _engine_pass(hip, ora, B, T)["acts"][layer - 1]
    assert 0.05 < (mask > 0).mean() < 0.95, "a ReLU pattern that masks nothing or everything tests nothing"
    _dgrad_case(ctx, fd, layer, B, T, mask, 4000 + 10 * B + layer)


@pytest.mark.parametrize("B,T", [pytest.param(B, T, id=_id(B, T)) for B, T in SMALL_AND_RAGGED])
def test_tdnn3_data_gradient_small_and_ragged_is_the_restated_fmaf_chain(fd, ctx, B, T):
    """tdnn3 (7 taps, step -3, 112 chunks) below the batches of tests/test_gpu_conv.py and at the ragged shapes; a seeded
    half-dense mask with values in (0, 1)."""
    Tc = xv_fold.layer_frames(xv_fold.num_frames(T))[1]
    rng = np.random.RandomState(5000 + B + T)
    mask = ((rng.standard_normal((B * Tc, 512)) > 0) * rng.uniform(0.01, 0.99, (B * Tc, 512))).astype(np.float32)
    _dgrad_case(ctx, fd, 3, B, T, mask, 6000 + B)


# ----------------------------------------------------------------------------------- (c) pooling + split-K fc1 forward
@pytest.mark.parametrize("B,T", [pytest.param(B, T, id=_id(B, T)) for B, T in GRID])
def test_pool_and_split_k_fc1_against_float64_on_the_engines_own_tdnn5(hip, ora, fd, B, T):
    """tdnn_emb of sg_xv_forward against mean / unbiased deviation over the frames and the folded fc1, evaluated in float64
    on the engine's own tdnn5 readback (so nothing upstream enters).  Yardstick: the same computation in float32 torch on
    the CPU.  Per utterance: max |engine - fp64| <= C x (the yardstick's max error on that utterance) + FLOOR_SCORE x
    max |fp64| of that utterance (truth.POLICY)."""
    p = _engine_pass(hip, ora, B, T)
    F5 = p["fl"][4]
    a32 = torch.from_numpy(p["acts"][5]).view(B, F5, xv_fold.POOL_C)
    w32, b32 = torch.from_numpy(fd.fc1_w), torch.from_numpy(fd.fc1_b)

    def emb(a, w, b):
        return torch.cat((a.mean(1), a.std(1)), 1).matmul(w) + b
    e64 = emb(a32.double(), w32.double(), b32.double()).numpy()
    yard = np.abs(emb(a32, w32, b32).double().numpy() - e64).max(1)
    eng = np.abs(p["temb"].astype(np.float64) - e64).max(1)
    bound = truth.POLICY["C"] * yard + truth.POLICY["FLOOR_SCORE"] * np.abs(e64).max(1)
    log("pool + fc1 forward B=%d T=%d: engine / fp32 torch vs fp64 on the engine's tdnn5, max over utterances %.3e / %.3e "
        "(max |emb| %.2f); worst engine error over its bound %.2f"
        % (B, T, eng.max(), yard.max(), np.abs(e64).max(), (eng / bound).max()))
    assert np.isfinite(p["temb"]).all()
    bad = np.flatnonzero(~(eng <= bound))
    assert bad.size == 0, [(int(u), float(eng[u]), float(yard[u]), float(bound[u])) for u in bad[:8]]
