"""The floor cases of tests/frontend_adjoint.py (``FLOOR_CASES``: digital silence at both log floors) proved on the CPU, without
the engine: the condition their inputs meet, and the power of the judgements tests/test_gpu_frontend_floor.py applies to them.

Both front ends take a logarithm behind a floor -- the MFCC twice, ``log(max(., eps32))`` on the 30 mel energies and on the frame
energy that becomes c0; AudioNet once, ``10 log10(max(., 1e-16))`` on its 32 mel energies -- and both adjoints gate on it.  The
oracle writes the floor as ``torch.clamp``, whose adjoint is 0 below the floor, so the float64 vector-Jacobian product of the
oracle stays an exact truth at such inputs PROVIDED no pre-log value sits near the floor, where float32 and float64 could
land on different sides of it.

The condition (``test_inputs_keep_clear_of_the_floor``; every case, row, frame and bin, nothing left out, no tolerance): each
pre-log value of the float64 oracle is either exactly 0 or at least 2**10 x the floor, and the float32 oracle is exactly 0 in
exactly the same places.  A case that broke it would get its boundary moved by a sample, the move recorded in the case
table of tests/frontend_adjoint.py; none needed one.  Measured here: the smallest nonzero value is 1.2e5 x the floor (AudioNet
(2, 4096) one-hot ``gap``), 4.6e8 x for the MFCC; a case holds 4 .. 277 silent frames.  Two alignments are known to break the
condition and are kept out of the layouts: for the MFCC, leading silence whose first nonzero sample is sample 399 of a frame
(index = 119 mod 160), where the povey window is 0 and only the DC-removal residue is left; for AudioNet, trailing silence
that begins 10, 12 or 14 samples into a frame's last hop, where what is left under the window's tail is near 1e-16.

A second condition, found when the GPU module first ran on another machine than the one these cases were drawn up on
(``test_truths_do_not_depend_on_the_cpu_that_built_the_mel_bank``): the oracle's float32 mel bank comes out of ``torch.log`` and
differs between CPUs in its last bits.  A frame left with a few samples of speech under the povey window's last taps turns
that into 6.6e-4 of the row's RMS on one 160-sample block of the float64 VJP -- the truth itself, before any engine.  The
truth under either bank has to agree to FLOOR_UTT / FLOOR_BLOCK; one boundary was moved for it (row 4 of (16, 48000) ``edges``, by
8 samples: ``frontend_adjoint.FLOOR_MOVES``).  The engine's result for that row was the same bits on both machines.

Out of scope, and why: tonal, band-limited and constant-but-nonzero audio.  There a bin's pre-log value is not 0 but the
reference's own float32 round-off -- the residue of DC removal, the noise floor of its FFT -- and which side of the floor it
falls on is decided by that round-off.  No kernel can be right or wrong about it: a different, equally valid float32
evaluation order moves the bin across the floor, and the gradient from 0 to c / 1e-7.  The one constant that IS in scope is
``plateau`` (x-vector): +1.0 is 32768 on the int16 scale and 32768 x 400 / 400 is exact, so DC removal leaves exact zeros.

Planted defects (float64 models ``xv_candidate`` / ``an_candidate`` / ``forward_candidate`` through ``xv_forward_frames`` /
``an_forward_frames``), each caught on EVERY floor case of its front end, none passing silently:
  * floor_ungated -- the backward divides by the mel energy, and by the frame energy, without the gate: 0 / 0 or c / 0 on a
    silent frame, a non-finite gradient; ``judge`` rejects it ("finite").
  * floor_value -- the forward floors at 1e-10 instead of the reference's constant: a silent frame's c0 is -23.03 for -15.94,
    its log-mel -100 dB for -160 dB; the forward bounds of the suite (rtol 1e-4, atol 5e-3; atol 8e-4) reject it.
  * floor_none -- no floor: -inf features; the finiteness check of the forward rejects it.

What these inputs provably CANNOT tell apart -- so that nobody reads more into them than they carry:
  * the gate ``v > floor ? g / v : 0`` from a clamped denominator ``g / max(v, floor)``.  On a silent frame the spectrum and
    the samples are exactly 0, so d v / d frame is exactly 0 and the product is 0 either way; on every other frame v is far
    above the floor and the two coincide (``test_what_exact_silence_cannot_tell_apart``: the same float64 bits).  Likewise
    ``>`` from ``>=`` in the gate, and any floor constant in the BACKWARD between 0 and 2**10 x the floor.
  * a wrong floor constant from the ADJOINT's side, as long as no pre-log value lies between the two constants: the MFCC's
    gradient under floor_value (1e-10 < eps32) is the same float64 bits (asserted there too); only the forward comparison
    sees it.  (AudioNet's 1e-10 lies above its 1e-16, and a few bins of a frame that holds a sliver of speech under the
    window's tail -- down to 1.2e5 x 1e-16 -- fall between them: there the gradient differs too.)
  * anything about bins NEAR the floor: by the condition there are none.
"""
import numpy as np
import pytest
import torch

import frontend_adjoint as fa
from oracle import kaldi_mfcc as km

MARGIN = 2.0 ** 10


@pytest.mark.parametrize("c", fa.FLOOR_CASES, ids=fa.case_id)
def test_inputs_keep_clear_of_the_floor(c):
    rep = fa.floor_report(c)
    (e64, m64), (e32, m32) = rep["f64"], rep["f32"]
    lowest = np.inf
    for name, v64, v32 in (("mel energy", m64, m32), ("frame energy", e64, e32)):
        if v64 is None:
            continue
        assert v64.dtype == np.float64 and v32.dtype == np.float32 and v64.shape == v32.shape
        assert np.isfinite(v64).all() and np.isfinite(v32).all() and (v64 >= 0).all() and (v32 >= 0).all()
        near = (v64 != 0) & (v64 < MARGIN * rep["floor"])
        assert not near.any(), "%s: %d values within 2**10 of the floor, at (row, frame[, bin]) %s" % (name, near.sum(), np.argwhere(near)[:4].tolist())
        assert np.array_equal(v64 == 0, v32 == 0), "%s: float32 and float64 disagree on %d exact zeros" % (name, ((v64 == 0) != (v32 == 0)).sum())
        lowest = min(lowest, v64[v64 != 0].min() / rep["floor"])
    zeros = int((m64 == 0).sum()) + (0 if e64 is None else int((e64 == 0).sum()))
    print("%s: %d silent frames, %d exact zeros before the logarithms, the smallest nonzero value %.2e x the floor" % (
        fa.case_id(c), len(rep["silent"]), zeros, lowest))
    assert rep["silent"], "no frame takes the floor"
    # a frame is silent in every bin or in none: no bin of a speech frame is exactly 0
    assert zeros == len(rep["silent"]) * (m64.shape[2] + (e64 is not None))


@pytest.mark.parametrize("c", [c for c in fa.FLOOR_CASES if c.kind == "dense" and c.B == 2], ids=fa.case_id)
def test_the_logarithm_of_the_reported_values_is_the_oracle(c):
    """``floor_report`` restates the oracle up to its clamp: the clamp and logarithm of what it reports is the oracle's output
    bit for bit, in float32 and in float64 (so 'exactly 0 in the float32 oracle' is said of the oracle itself)"""
    rep = fa.floor_report(c)
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        energy, mel = (None if v is None else torch.from_numpy(v) for v in rep[name])
        want = torch.from_numpy(fa.forward_oracle(c, dtype))
        assert want.dtype == dtype
        if c.model == "an":
            assert torch.equal(10 * torch.clamp(mel, fa.AN_FLOOR).log10(), want)
        else:
            k = {n: v.to(dtype) for n, v in km.constants().items()}
            for r in range(c.B):
                feats = (torch.clamp(mel[r], min=km.EPSILON).log().matmul(k["dct"]) * k["lifter"].unsqueeze(0))[:, :want.shape[2]]
                assert torch.equal(feats[:, 1:], want[r, :, 1:]) and torch.equal(torch.clamp(energy[r], min=km.EPSILON).log(), want[r, :, 0])


def test_plateau_and_window0_put_raw_content_on_silent_frames():
    """the two layouts whose silent frames are not made of zero samples: the frame's raw samples are nonzero, every pre-log value 0"""
    c = fa.Case("xv", 2, 5200, "dense", "plateau")
    x, silent = fa.inputs(c)["x"], fa.floor_report(c)["silent"]
    idx = fa.xv_frame_index(c.T)
    assert len(silent) == 20 and all((x[r, 0, idx[f]] == 1.0).all() for r, f in silent)
    for T in (4096, 16001):
        c = fa.Case("an", 2, T, "dense", "window0")
        x, silent = fa.inputs(c)["x"], fa.floor_report(c)["silent"]
        w = torch.hann_window(fa.AN_WIN, dtype=torch.float64).numpy()
        assert w[0] == 0.0 and w[-1] > 1e-5
        for r in range(2):
            raw = fa.an_frames(x[r, 0], 1.0).numpy()
            lit = [f for f in range(raw.shape[0]) if (r, f) in silent and raw[f].any()]
            assert len(lit) == 1 and np.flatnonzero(raw[lit[0]]).tolist() == [0], (T, r, lit)  # column 0 alone, where the window is 0


# ------------------------------------------------------------------------------------------------------ the truths
@pytest.mark.parametrize("c", fa.FLOOR_CASES, ids=fa.case_id)
def test_truths_are_finite_and_judge_accepts_the_float32_yardstick(c):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    assert np.isfinite(yard).all() and np.isfinite(g64).all()
    fails, line, _ = fa.judge(yard, yard, g64)
    print(fa.case_id(c), line)
    assert not fails, (fails[:6], line)
    assert np.array_equal(yard == 0, g64 == 0), "float32 and float64 disagree on which samples are exactly zero"
    assert (g64 == 0).sum() > 0 and np.abs(g64).max() > 0
    if c.variant == "all":
        assert not g64[0].any() and not i["x"][0].any() and g64[1].any()
    if c.kind == "onehot":  # a one-hot on a silent frame: the whole row's truth is exactly zero, and judge covers every sample
        silent = {f for _, f in fa.floor_report(c)["silent"]}
        lit = [int(np.argwhere(i["cot"][r])[0][0]) for r in range(len(g64))]
        assert sum(f in silent for f in lit) == 3 * len(lit) // 5 and sum(f not in silent for f in lit) == 2 * len(lit) // 5
        for r, f in enumerate(lit):
            assert bool(g64[r].any()) == (f not in silent), (r, f)


@pytest.mark.parametrize("c", [c for c in fa.FLOOR_CASES if c.model != "an"], ids=fa.case_id)
def test_truths_do_not_depend_on_the_cpu_that_built_the_mel_bank(c):
    """The oracle builds its 30 x 256 mel bank in float32 from ``torch.log``, whose last bit differs between CPUs:
    tests/golden/kaldi_mel_bank_second_cpu.npy is the bank a second machine built (34 weights differ from the first's, by at
    most 2.8e-6).  Speech does not feel it (1e-6 of a row).  A frame that holds a few samples of speech under the window's last
    taps does: its gradient on its silent samples is the remainder of a near-total cancellation across the spectrum.  The
    float64 VJP is a truth only where it is the same under either bank: required here to FLOOR_UTT per row and FLOOR_BLOCK per
    160-sample block, half of the smallest bound ``judge`` can apply (C max(yard, FLOOR) with C = 2), so that the engine keeps
    at least the room the policy gives round-off.  Measured: at most 1.4e-5 / 1.2e-4 against 3.1e-5 / 2.4e-4, after the one
    move recorded in ``frontend_adjoint.FLOOR_MOVES`` (6.6e-4 before it).  (AudioNet's mel basis is float64 numpy, rounded once.)"""
    import os
    import truth
    other = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kaldi_mel_bank_second_cpu.npy"), allow_pickle=False)
    consts = km.constants()
    here = consts["mel"]
    assert other.shape == tuple(here.shape) and other.dtype == np.float32 and np.abs(other - here.numpy()).max() < 4e-6
    i = fa.inputs(c)
    x, cot = (i["x"][:1], fa.cot30(c, i["cot"])[:i["n"]]) if i["shared"] else (i["x"], fa.cot30(c, i["cot"]))
    g = []
    try:
        for bank in (here, torch.from_numpy(other.copy())):
            consts["mel"] = bank
            g.append(fa.xv_vjp(x, cot, shared=i["shared"]))
    finally:
        consts["mel"] = here
    utt, block = truth.utt_error(g[1], g[0]), truth.block_error(g[1], g[0], fa.HOP)
    live = np.abs(g[0]).max(1) > 0  # (a one-hot on a silent frame: both are exactly zero)
    assert np.array_equal(g[0] == 0, g[1] == 0)
    print("%s: the truth under the second CPU's mel bank, per row %.2e, per block %.2e" % (fa.case_id(c), utt[live].max(), block[live].max()))
    assert (utt[live] <= truth.POLICY["FLOOR_UTT"]).all() and (block[live] <= truth.POLICY["FLOOR_BLOCK"]).all(), (utt, block)


def _candidate(c, defect=None):
    i = fa.inputs(c)
    if c.model == "an":
        return fa.an_candidate(i["x"], i["cot"], frame_defect=defect)
    V = 4 if c.T % 4 == 0 and i["x"].shape[0] * c.T >= fa.QUAD_MIN else 1
    return fa.xv_candidate(i["x"], fa.cot30(c, i["cot"]), None, V, frame_defect=defect)


@pytest.mark.parametrize("c", fa.FLOOR_CASES, ids=fa.case_id)
def test_float64_models_equal_the_float64_truth_on_the_floor_cases(c):
    yard, g64 = fa.truths(c)
    got = _candidate(c)
    norm = np.maximum(np.linalg.norm(g64, axis=1), 1e-300)
    assert float((np.linalg.norm(got - g64, axis=1) / norm).max()) < 1e-9
    assert np.array_equal(got == 0, g64 == 0)
    assert not fa.judge(got, yard, g64)[0]
    assert fa.forward_fails(fa.forward_candidate(c), fa.forward_oracle(c, torch.float64), c.model) is None


# ------------------------------------------------------------------------------------------------------ the planted defects
@pytest.mark.parametrize("c", fa.FLOOR_CASES, ids=fa.case_id)
def test_judge_rejects_the_ungated_backward(c):
    yard, g64 = fa.truths(c)
    got = _candidate(c, "floor_ungated")
    fails, line, _ = fa.judge(got, yard, g64)
    print("floor_ungated on %s: %d non-finite samples; %s" % (fa.case_id(c), (~np.isfinite(got)).sum(), line))
    assert not np.isfinite(got).all() and any(f[0] == "finite" for f in fails), line


@pytest.mark.parametrize("defect", ("floor_value", "floor_none"))
@pytest.mark.parametrize("c", fa.FLOOR_CASES, ids=fa.case_id)
def test_forward_bounds_reject_a_wrong_or_missing_floor(c, defect):
    want = fa.forward_oracle(c, torch.float64)  # (the candidate is a float64 model)
    what = fa.forward_fails(fa.forward_candidate(c, defect), want, c.model)
    print("%s on %s: %s" % (defect, fa.case_id(c), what))
    assert what is not None and ("non-finite" in what) == (defect == "floor_none")
    if defect == "floor_value" and c.model != "an":  # the MFCC adjoint cannot see this constant: the same gradient, bit for bit
        assert np.array_equal(_candidate(c, defect), _candidate(c, "floor_as_is"))


@pytest.mark.parametrize("c", [c for c in fa.FLOOR_CASES if c.B == 2], ids=fa.case_id)
def test_what_exact_silence_cannot_tell_apart(c):
    """the gate replaced by a clamped denominator: the same float64 bits on every case (module docstring)"""
    assert np.array_equal(_candidate(c, "floor_clamped"), _candidate(c, "floor_as_is"))
    assert not np.array_equal(_candidate(c, "floor_as_is"), np.zeros_like(fa.truths(c)[1]))
