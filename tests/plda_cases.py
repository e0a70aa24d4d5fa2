"""The back-end corner cases both speaker models are run at (test_gpu_xv.py, test_gpu_ivector.py; checked on the CPU by
test_plda_cases_cpu.py): D = 150 (the x-vector kernel pads its rows to 152) and enrolled counts S = 1, 27 / 28 (S D = 4050 /
4200: the x-vector tail keeps the table in LDS up to 4096 floats) and 64 / 65 (the loss: one wave up to 64 classes, the block
above).  One model per system holds 65 speakers; a case enrols the first S of them.  Inputs: 3 x 1 s, dither 0."""
import numpy as np

from speakerguard_amd import synth

D, S_MAX, S_CASES = 150, 65, (1, 27, 28, 64, 65)
B, T = 3, 16000
XV_SEED, IV_SEED, WAV_SEED = 3, 2, 77  # (test_plda_cases_cpu.py: at these, no row of any case sits inside its tie margin)


def xv_weights():
    return synth.make_xv_weights(seed=XV_SEED, D=D, n_spk=S_MAX, calibrated=False)


def iv_weights():
    return synth.make_iv_weights(seed=IV_SEED, C=16, R=24, D=D, n_spk=S_MAX)


def waveforms():
    return synth.make_waveforms(B, T, seed=WAV_SEED)


def llr(emb, enroll, psi, dtype=np.float64):
    """PLDA log-likelihood ratios (rows, S) of embeddings (rows, D) against enroll (S, D) in `dtype` arithmetic: plda.py:140-190"""
    emb, enroll, psi = (np.asarray(a, dtype) for a in (emb, enroll, psi))
    var = 1.0 + psi / (psi + 1.0)
    log2pi = np.log(dtype(2 * 3.1415926)) * dtype(emb.shape[1])
    given = -0.5 * (np.log(var).sum() + log2pi + ((emb[:, None, :] - psi / (psi + 1.0) * enroll[None]) ** 2 / var).sum(2))
    without = -0.5 * (np.log(psi + 1.0).sum() + log2pi + (emb ** 2 / (psi + 1.0)).sum(1))
    return given - without[:, None]


def xv_score_bound(truth, yard):
    """the score rule of tests/truth.py (POLICY), per row: C * (the float32 side's largest error in the batch) + FLOOR_SCORE * max|s64|"""
    from truth import POLICY
    return POLICY["C"] * np.abs(yard - truth).max() + POLICY["FLOOR_SCORE"] * np.abs(truth).max(1)


def iv_score_bound(truth, yard):
    """the rule of test_gpu_ivector.judge, one bound for the batch: max(4 err_ref, 2^-20 max|q|)"""
    from test_gpu_ivector import FLOOR
    return np.full(truth.shape[0], max(4.0 * np.abs(yard - truth).max(), FLOOR * np.abs(truth).max()))


def top_two_margin(truth):
    """per row: best score minus the runner-up (inf with one speaker)"""
    if truth.shape[1] == 1:
        return np.full(truth.shape[0], np.inf)
    top = np.sort(truth, axis=1)
    return top[:, -1] - top[:, -2]


def subset(S):
    """a permuted subset of the S enrolled speakers (at least one)"""
    idx = np.random.RandomState(S).permutation(S)
    return idx[:max(1, (S + 1) // 2)]
