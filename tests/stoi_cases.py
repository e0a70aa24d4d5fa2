"""The inputs of the STOI parity tests (tests/test_gpu_stoi.py on the device, tests/test_stoi_restate.py for the condition they
must meet), generated from seeds: synth.make_waveforms utterances plus seeded noise.  Test infrastructure."""
import numpy as np

from speakerguard_amd import synth

SHAPES = ((1, 8000), (3, 16000), (2, 16001), (5, 20011), (2, 6758))  # T = 6758: 4224 samples at 10 kHz, exactly 31 frames
LAYOUTS = ("plain", "gap", "edges")
NOISES = ("eps", "0dB")
EPSILON = 0.002
GAP = 6400                  # 0.4 s of exact zeros in the middle
LEAD, TRAIL = 1600, 800     # ... or at the two ends
MARGIN_DB = 1e-6            # every frame energy lies further than this from its row's threshold


def noisy(benign, kind, seed):
    """benign (B,T) float32 -> adver (B,T) float32"""
    rs = np.random.RandomState(seed)
    if kind == "eps":
        return (benign + rs.uniform(-EPSILON, EPSILON, benign.shape).astype(np.float32)).astype(np.float32)
    n = rs.standard_normal(benign.shape)
    gain = np.sqrt((benign.astype(np.float64) ** 2).mean(axis=1, keepdims=True) / (n ** 2).mean(axis=1, keepdims=True))
    return (benign + gain * n).astype(np.float32)


def case(B, T, layout, noise):
    """(benign, adver) float32 (B,T)"""
    seed = 1000 * B + T
    benign = synth.make_waveforms(B, T, seed=seed).reshape(B, T).astype(np.float32)
    adver = noisy(benign, noise, seed + 1 + NOISES.index(noise))
    if layout == "gap":
        lo = max(0, (T - GAP) // 2)
        benign[:, lo:lo + GAP] = 0
        adver[:, lo:lo + GAP] = 0
    elif layout == "edges":
        for a in (benign, adver):
            a[:, :LEAD] = 0
            a[:, T - TRAIL:] = 0
    return benign, adver


def all_cases():
    return [(B, T, layout, noise) for B, T in SHAPES for layout in LAYOUTS for noise in NOISES]
