"""The AudioNet loader's BatchNorm fold, restated in numpy.  TEST INFRASTRUCTURE (a plain module, not a conftest).

``sg_an_load`` (speakerguard_amd/csrc/sg_api_audionet.hip) folds the eval-mode BatchNorm that follows every convolution
(and precedes the ReLU) into that convolution's weights and bias and stores every weight twice: ``wf`` K-major for the
forward contraction and ``wb`` transposed for the data gradient.  ``fold`` reproduces the loader's arithmetic operation by
operation, with each cast where the loader has it:

* ``eps``: the float field ``bn_eps`` (1e-5 rounded to float32), widened;
* conv1 + conv1.1 (one channel): ``sc = g / sqrt(var + eps)`` in float64, ``w25[i] = float32(w[i] * sc)`` laid out
  [mel offset][time offset], ``pre_bias = float32((b - mean) * sc + beta)`` with the subtraction in float64 (the loader
  widens the mean first);
* conv2 .. conv8: ``sc = g / sqrt(float64(var) + eps)``, ``v = float32(w * sc)`` written to ``wf[(j cin + ci) cout + co]``
  and ``wb[(j cout + co) cin + ci]``, ``bias = float32((b - mean) * sc + beta)`` where ``b - mean`` is a float32
  subtraction (both operands are floats in the loader) and the rest float64.

so that the engine's own activations can be held against ``conv_chain(previous, wf[l], bias=bias[l])`` bit for bit
(tests/test_gpu_an_stages.py).  tests/test_an_stages_power.py proves the restatement against the float64 model without
the engine.
"""
from dataclasses import dataclass

import numpy as np

# restated from speakerguard_amd/csrc/sg_internal.h (kAnConv, kAnCin, kAnCout, kAnPad, kAnPool, kAnMel)
CONVS = 7
NAMES = ("conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8")
CIN = (32, 64, 128, 128, 128, 128, 64)
COUT = (64, 128, 128, 128, 128, 64, 32)
PAD = (1, 1, 1, 1, 1, 1, 0)
POOL = (True, False, False, True, False, True, False)
MEL = 32
BN_EPS = np.float32(1e-5)


def layer_frames(F):
    """(Tin, Tout) -- frames entering / leaving conv2 .. conv8 before pooling -- or None where the stack refuses F
    (sg_internal.h an_layer_frames)."""
    tin, tout, t = [], [], F
    for l in range(CONVS):
        tin.append(t)
        tout.append(t + 2 * PAD[l] - 2)
        if tout[l] < 1:
            return None
        t = tout[l] // 2 if POOL[l] else tout[l]
        if t < 1:
            return None
    return (tin, tout) if tin[-1] >= 3 else None


@dataclass
class Fold:
    w25: np.ndarray      # (25,) float32 [mel offset][time offset]
    pre_bias: np.float32
    wf: list             # [l] (3 * cin, cout) float32
    wb: list             # [l] (3 * cout, cin) float32
    bias: list           # [l] (cout,) float32
    fc_w: np.ndarray     # (S, 32) float32, the checkpoint's
    fc_b: np.ndarray     # (S,) float32


def _f32(sd, key):
    return np.ascontiguousarray(np.asarray(sd[key]), np.float32)


def fold(state_dict, eps=BN_EPS):
    sd = state_dict
    eps = float(np.float32(eps))
    g, beta, mean, var = (float(_f32(sd, "conv1.1." + k).reshape(-1)[0]) for k in ("weight", "bias", "running_mean", "running_var"))
    sc = g / np.sqrt(var + eps)
    w1 = _f32(sd, "conv1.0.weight")
    assert w1.shape == (1, 1, 5, 5), w1.shape  # (out, in, mel, time)
    w25 = (w1.reshape(25).astype(np.float64) * sc).astype(np.float32)
    pre_bias = np.float32((float(_f32(sd, "conv1.0.bias").reshape(-1)[0]) - mean) * sc + beta)
    wf, wb, bias = [], [], []
    for l, name in enumerate(NAMES):
        cin, cout = CIN[l], COUT[l]
        w = _f32(sd, name + ".0.weight")
        assert w.shape == (cout, cin, 3), (name, w.shape)
        sc = _f32(sd, name + ".1.weight").astype(np.float64) / np.sqrt(_f32(sd, name + ".1.running_var").astype(np.float64) + eps)
        diff = _f32(sd, name + ".0.bias") - _f32(sd, name + ".1.running_mean")  # float32 - float32, as the loader's operands are
        assert diff.dtype == np.float32
        bias.append((diff.astype(np.float64) * sc + _f32(sd, name + ".1.bias").astype(np.float64)).astype(np.float32))
        v = (w.astype(np.float64) * sc[:, None, None]).astype(np.float32)  # (co, ci, j)
        wf.append(np.ascontiguousarray(v.transpose(2, 1, 0)).reshape(3 * cin, cout))
        wb.append(np.ascontiguousarray(v.transpose(2, 0, 1)).reshape(3 * cout, cin))
    return Fold(w25, pre_bias, wf, wb, bias, _f32(sd, "fc.weight"), _f32(sd, "fc.bias"))
