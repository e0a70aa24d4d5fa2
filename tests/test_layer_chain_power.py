"""The tools of tests/test_gpu_layers.py, proved on the CPU before the engine is judged by them.

Fold check: the five TDNN layers as float32 fmaf chains (oracle/conv_chain.c) over the numpy restatement of the loader's
BatchNorm fold (tests/xv_fold.py) reproduce the ReLU outputs of the float64 model (oracle.xv_plda.XvPlda.tdnn_layers) to
fp32 accumulation error -- without the engine, so a wrong fold (a BatchNorm applied to the wrong layer, a bias term lost, a
transposed tap) cannot hide behind an engine that makes the same mistake.

Comparison helper: ``xv_fold.bit_mismatch`` accepts equal arrays and rejects one ulp, a swapped sign of zero, two rows
swapped across a 32-row tile boundary and an unwritten row, naming the coordinates.
"""
import copy

import numpy as np
import pytest
import torch

import xv_fold
from conftest import log
from oracle.conv_chain import conv_chain

EPS32 = float(np.finfo(np.float32).eps)
B, T = 3, 16000


@pytest.fixture(scope="module")
def weights():
    from speakerguard_amd import synth
    return synth.make_xv_weights(seed=0, D=200, n_spk=10)


@pytest.fixture(scope="module")
def fd(weights):
    return xv_fold.fold(weights["state_dict"])


def test_layout_and_padding_of_the_fold(weights, fd):
    """wf and wb are each other's transposes per tap, the pad rows / columns and pad biases are +0, and tdnn1 (no
    BatchNorm in front of it) is the checkpoint's weight unchanged."""
    sd = weights["state_dict"]
    for l in range(xv_fold.LAYERS):
        k, cip, cop = xv_fold.TAPS[l], xv_fold.CIN_PAD[l], xv_fold.COUT_PAD[l]
        f = fd.wf[l].reshape(k, cip, cop)
        b = fd.wb[l].reshape(k, cop, cip)
        assert np.array_equal(f.view(np.uint32), b.transpose(0, 2, 1).view(np.uint32))
        assert not f[:, xv_fold.CIN[l]:, :].view(np.uint32).any() and not f[:, :, xv_fold.COUT[l]:].view(np.uint32).any()
        assert not fd.bias[l][xv_fold.COUT[l]:].view(np.uint32).any()
    w1 = np.asarray(sd["tdnn1.weight"], np.float32)  # (co, ci, j)
    assert np.array_equal(fd.wf[0].reshape(5, 32, 512)[:, :30, :], w1.transpose(2, 1, 0))
    assert np.array_equal(fd.bias[0], np.asarray(sd["tdnn1.bias"], np.float32))
    assert xv_fold.layer_frames(300) == [296, 288, 270, 270, 270] and xv_fold.num_frames(48000) == 300


def test_folded_chain_is_the_float64_model_to_fp32_accumulation_error(weights, fd):
    """CMVN-level features of 3 x 1 s from the oracle's front-end through the five folded layers as fmaf chains, against
    the float64 model's ReLU outputs.

    The bound, per layer, on max |chain - fp64| / max |fp64|: a sequential float32 sum of K products carries a rounding
    error that grows like a random walk, sqrt(K) units of eps32 / 2 against the size of the partial sums (the worst case,
    K eps32 / 2, is never met by data without a common sign); the weights were rounded once (half an ulp each, another
    random walk below the first); the error a layer inherits passes through at about its own relative size, because the
    BatchNorm folded into the weights keeps the activations at unit scale.  So layer l is allowed sum_{i <= l}
    sqrt(K_i) eps32 with K = taps x input channels = 150, 2560, 3584, 512, 512: 1.5e-6, 7.5e-6, 1.5e-5, 1.7e-5, 2.0e-5.
    A fold that is wrong anywhere is off by the BatchNorm's scale or shift, orders of magnitude above it.  The fp32
    model's own error is logged next to the chain's."""
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    om = XvPlda(weights)
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=11))
    with torch.no_grad():
        feats = om.compute_feat(x, flag=2)
        F = feats.shape[1]
        assert F == xv_fold.num_frames(T)
        a32 = [a for a, _ in om.tdnn_layers(feats.transpose(1, 2))]
        a64 = [a for a, _ in copy.deepcopy(om).double().tdnn_layers(feats.double().transpose(1, 2))]
    chain = xv_fold.chain_forward(fd, xv_fold.pad_features(feats.numpy()), B, F, conv_chain)
    allowed = 0.0
    for l, Fl in enumerate(xv_fold.layer_frames(F)):
        allowed += np.sqrt(xv_fold.TAPS[l] * xv_fold.CIN[l]) * EPS32
        want = a64[l].numpy().transpose(0, 2, 1)  # (B, F_l, C)
        got = chain[l].reshape(B, Fl, xv_fold.COUT_PAD[l])
        assert want.shape == (B, Fl, xv_fold.COUT[l])
        assert not got[:, :, xv_fold.COUT[l]:].view(np.uint32).any(), "pad channels of layer %d are not +0" % (l + 1)
        scale = np.abs(want).max()
        err = np.abs(got[:, :, :xv_fold.COUT[l]] - want).max() / scale
        err32 = np.abs(a32[l].numpy().transpose(0, 2, 1) - want).max() / scale
        log("fold check tdnn%d (3 x 1 s): folded fmaf chain vs fp64 model %.3e of max |act| (allowed %.3e); fp32 model %.3e"
            % (l + 1, err, allowed, err32))
        assert err <= allowed, "layer %d: %.3e > %.3e" % (l + 1, err, allowed)


def test_folded_fc1_is_the_float64_model(weights, fd):
    """Statistics pooling + the folded fc1 over the chain's tdnn5 output, in float64, against the float64 model's
    tdnn_embedding: the bound of the test above at the last layer plus sqrt(3000) eps32 for the fc1 weights' own rounding,
    relative to the largest embedding entry."""
    from oracle.xv_plda import XvPlda
    from speakerguard_amd import synth
    om = XvPlda(weights)
    x = torch.from_numpy(synth.make_waveforms(B, T, seed=11))
    with torch.no_grad():
        feats = om.compute_feat(x, flag=2)
        want = copy.deepcopy(om).double().tdnn_embedding(feats.double().transpose(1, 2)).numpy()
    F = feats.shape[1]
    act5 = xv_fold.chain_forward(fd, xv_fold.pad_features(feats.numpy()), B, F, conv_chain)[4]
    a = act5.reshape(B, -1, xv_fold.POOL_C).astype(np.float64)
    stats = np.concatenate((a.mean(1), a.std(1, ddof=1)), 1)
    got = stats @ fd.fc1_w.astype(np.float64) + fd.fc1_b.astype(np.float64)
    allowed = (sum(np.sqrt(xv_fold.TAPS[l] * xv_fold.CIN[l]) for l in range(5)) + np.sqrt(3000.0)) * EPS32
    err = np.abs(got - want).max() / np.abs(want).max()
    log("fold check fc1 (3 x 1 s): fp64 pool + folded fc1 on the chain's tdnn5 vs fp64 model %.3e of max |emb| (allowed %.3e)"
        % (err, allowed))
    assert err <= allowed


# ------------------------------------------------------------------------------------------------ comparison helper
FRAMES, CH = 68, 256


def _case():
    rng = np.random.RandomState(2)
    a = np.maximum(rng.standard_normal((3 * FRAMES, CH)), 0).astype(np.float32)  # a ReLU output: half of it +0
    return a, a.copy()


def test_bit_mismatch_accepts_equal_arrays():
    a, b = _case()
    a[5, 7] = b[5, 7] = np.nan  # the same bits are the same bits
    a[9, 1] = b[9, 1] = -0.0
    assert xv_fold.bit_mismatch(a, b, FRAMES, "tdnn2 B=3") is None
    xv_fold.assert_same_bits(a, b, FRAMES)


def test_bit_mismatch_rejects_one_ulp():
    a, b = _case()
    r, c = 2 * FRAMES + 13, 200
    b[r, c] = 0.75
    a[r, c] = np.nextafter(np.float32(0.75), np.float32(1))
    msg = xv_fold.bit_mismatch(a, b, FRAMES, "tdnn4 B=3")
    assert msg is not None and msg.startswith("tdnn4 B=3: 1 of %d elements differ in 1 rows" % a.size), msg
    assert "utterance 2 frame 13 channel 200" in msg and "0x3f400001" in msg and "0x3f400000" in msg, msg
    with pytest.raises(AssertionError, match="utterance 2 frame 13 channel 200"):
        xv_fold.assert_same_bits(a, b, FRAMES, "tdnn4 B=3")


def test_bit_mismatch_rejects_a_swapped_sign_of_zero():
    a, b = _case()
    r, c = FRAMES + 1, 3
    b[r, c] = 0.0
    a[r, c] = -0.0
    assert np.array_equal(a, b), "the values are equal: only the bits tell"
    msg = xv_fold.bit_mismatch(a, b, FRAMES)
    assert msg is not None and "utterance 1 frame 1 channel 3" in msg and "0x80000000" in msg and "0x00000000" in msg, msg


def test_bit_mismatch_rejects_rows_swapped_at_a_32_row_boundary():
    a, b = _case()
    a[[31, 32]] = a[[32, 31]]
    msg = xv_fold.bit_mismatch(a, b, FRAMES)
    assert msg is not None and "in 2 rows (first row 31, last row 32)" in msg and "utterance 0 frame 31" in msg, msg


def test_bit_mismatch_rejects_an_unwritten_row():
    a, b = _case()
    a[3 * FRAMES - 1] = np.nan  # the last row of the last utterance: a ragged tile nobody wrote
    msg = xv_fold.bit_mismatch(a, b, FRAMES)
    assert msg is not None and "%d of %d elements differ in 1 rows" % (CH, a.size) in msg, msg
    assert "utterance 2 frame %d channel 0" % (FRAMES - 1) in msg and "0x7fc00000" in msg, msg


def test_bit_mismatch_rejects_another_shape():
    a, b = _case()
    assert "shape" in xv_fold.bit_mismatch(a[:-1], b, FRAMES)
