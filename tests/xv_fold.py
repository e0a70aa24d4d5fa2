"""The x-vector loader's BatchNorm fold, restated in numpy, and the bitwise comparison the layer tests judge with.
TEST INFRASTRUCTURE (a plain module, not a conftest).

``sg_xv_load`` (speakerguard_amd/csrc/sg_api.hip, the loop over kLayers) folds the eval-mode BatchNorm that follows every
ReLU into the NEXT layer's weights and bias, pads the channels and stores every weight twice: K-major for the forward
contraction and transposed for the data gradient.  ``fold`` reproduces that arithmetic operation by operation -- float64
products, ``r = 1 / sqrt(double(var) + double(float32(eps)))``, the bias accumulated sequentially in the loader's (ci, j)
order (vectorised over the output channel only, which is the loop the loader runs outermost: every channel still sees its
own terms in the loader's order), one final cast to float32 -- so that

    act[l] == conv_chain(act[l - 1], wf[l], bias=bias[l])          (oracle/conv_chain.c, bit for bit)

can be asserted on the engine's own activations (tests/test_gpu_layers.py).  tests/test_layer_chain_power.py proves the
restatement against the float64 model without the engine, and proves that ``bit_mismatch`` rejects planted defects.
"""
from dataclasses import dataclass

import numpy as np

# restated from speakerguard_amd/csrc/sg_internal.h (kLayers, kCin, kCout, kCinPad, kCoutPad, kTaps, kDil, kPoolC, kStats, kEmb)
LAYERS = 5
NAMES = ("tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5")
CIN = (30, 512, 512, 512, 512)
COUT = (512, 512, 512, 512, 1500)
CIN_PAD = (32, 512, 512, 512, 512)
COUT_PAD = (512, 512, 512, 512, 1536)
TAPS = (5, 5, 7, 1, 1)
DIL = (1, 2, 3, 1, 1)
POOL_C = 1536
STATS = 2 * POOL_C
EMB = 512
BN_EPS = np.float32(1e-5)  # sg_xv_weights.bn_eps is a float: the loader widens the ROUNDED 1e-5


def num_frames(T):
    """MFCC frames of a T-sample waveform (10 ms shift, snip_edges off: sg_internal.h num_frames)."""
    return (T + 80) // 160


def layer_frames(F):
    """Output frames of tdnn1..5 for F input frames (sg_api.hip layer_frames)."""
    out, f = [], F
    for l in range(LAYERS):
        f -= (TAPS[l] - 1) * DIL[l]
        out.append(f)
    return out


@dataclass
class Fold:
    wf: list      # [l] (taps * cin_pad, cout_pad) float32: wf[(j * cin_pad + ci) * cout_pad + co]
    wb: list      # [l] (taps * cout_pad, cin_pad) float32: wb[(j * cout_pad + co) * cin_pad + ci]
    bias: list    # [l] (cout_pad,) float32, folded
    fc1_w: np.ndarray  # (STATS, EMB) float32: rows [0, 1500) the means, [POOL_C, POOL_C + 1500) the deviations
    fc1_b: np.ndarray  # (EMB,) float32, folded


def fold(state_dict, eps=BN_EPS):
    sd = {k: np.asarray(v) for k, v in state_dict.items()}
    eps = float(np.float32(eps))
    wf, wb, bias = [], [], []
    r_prev = m_prev = None
    for l, name in enumerate(NAMES):
        cin, cout, k, cip, cop = CIN[l], COUT[l], TAPS[l], CIN_PAD[l], COUT_PAD[l]
        w32 = np.ascontiguousarray(sd[name + ".weight"], np.float32)
        assert w32.shape == (cout, cin, k), (name, w32.shape)
        v = w32.astype(np.float64)  # (co, ci, j)
        bacc = np.ascontiguousarray(sd[name + ".bias"], np.float32).astype(np.float64)
        if l > 0:
            for ci in range(cin):
                for j in range(k):
                    bacc -= v[:, ci, j] * m_prev[ci] * r_prev[ci]  # (v * m) * r, as the loader's expression associates
            v = v * r_prev[None, :, None]
        f = np.zeros((k, cip, cop), np.float32)
        f[:, :cin, :cout] = v.transpose(2, 1, 0).astype(np.float32)
        b = np.zeros((k, cop, cip), np.float32)
        b[:, :cout, :cin] = v.transpose(2, 0, 1).astype(np.float32)
        bb = np.zeros(cop, np.float32)
        bb[:cout] = bacc.astype(np.float32)
        wf.append(f.reshape(k * cip, cop))
        wb.append(b.reshape(k * cop, cip))
        bias.append(bb)
        var = np.ascontiguousarray(sd["bn_" + name + ".running_var"], np.float32).astype(np.float64)
        r_prev = 1.0 / np.sqrt(var + eps)
        m_prev = np.ascontiguousarray(sd["bn_" + name + ".running_mean"], np.float32).astype(np.float64)
    # fc1 over stats = [mean | std] of the bn5 output: mean_y = (mean_a - m) r, std_y = std_a r
    c5 = COUT[4]
    fw32 = np.ascontiguousarray(sd["fc1.weight"], np.float32)
    assert fw32.shape == (EMB, 2 * c5), fw32.shape
    w64 = fw32.astype(np.float64)
    wm, wsd = w64[:, :c5], w64[:, c5:]
    fb = np.ascontiguousarray(sd["fc1.bias"], np.float32).astype(np.float64)
    for c in range(c5):
        fb -= wm[:, c] * m_prev[c] * r_prev[c]
    fc1_w = np.zeros((STATS, EMB), np.float32)
    fc1_w[:c5] = (wm * r_prev[None, :]).T.astype(np.float32)
    fc1_w[POOL_C:POOL_C + c5] = (wsd * r_prev[None, :]).T.astype(np.float32)
    return Fold(wf, wb, bias, fc1_w, fb.astype(np.float32))


def pad_features(feats):
    """(B, F, 30) CMVN features -> (B * F, 32) rows, the pad columns +0: what the forward stages for tdnn1."""
    feats = np.asarray(feats, np.float32)
    B, F, C = feats.shape
    out = np.zeros((B * F, CIN_PAD[0]), np.float32)
    out[:, :C] = feats.reshape(B * F, C)
    return out


def chain_forward(fd, a, B, F, conv_chain):
    """The five folded layers as fmaf chains: a (B * F, 32) -> [ReLU output of tdnn1..5, (B * F_l, cout_pad)]."""
    outs, Ta = [], F
    for l, Tc in enumerate(layer_frames(F)):
        a = conv_chain(a, fd.wf[l], B, Ta, Tc, TAPS[l], DIL[l], 0, bias=fd.bias[l])
        outs.append(a)
        Ta = Tc
    return outs


# ------------------------------------------------------------------------------------------------------- comparison
def bit_mismatch(got, want, frames, what=""):
    """None if `got` and `want` -- (B * frames, C) float32 -- hold the same bits in every element (signs of zeros and NaN
    payloads included); else one line naming the first differing element (utterance, frame, channel, both bit patterns),
    how many differ and how many rows they touch.  `what`: the case's name (layer, batch, kernel) for the message."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    assert got.ndim == 2 and got.shape[0] % frames == 0, (got.shape, frames)
    g, w = got.view(np.uint32), want.view(np.uint32)
    if np.array_equal(g, w):
        return None
    diff = g != w
    rows = np.flatnonzero(diff.any(1))
    r = int(rows[0])
    c = int(np.flatnonzero(diff[r])[0])
    return ("%s: %d of %d elements differ in %d rows (first row %d, last row %d); first: utterance %d frame %d channel %d: "
            "got 0x%08x (%r), expected 0x%08x (%r)" % (what, int(diff.sum()), diff.size, rows.size, r, int(rows[-1]),
                                                       r // frames, r % frames, c, int(g[r, c]), float(got[r, c]),
                                                       int(w[r, c]), float(want[r, c])))


def assert_same_bits(got, want, frames, what=""):
    msg = bit_mismatch(got, want, frames, what)
    assert msg is None, msg
