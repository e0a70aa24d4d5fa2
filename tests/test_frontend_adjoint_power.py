"""tests/frontend_adjoint.py proved on the CPU, without the engine: the index arithmetic of both front-end adjoints as the
kernels write it, the float64 model of the engine built from it, and the power of the judgement.

* Index audit.  The restated frame maps stay inside [0, T) and equal the oracle's framing (``kaldi_mfcc.get_strided`` for every
  T in 400 .. 6000; torch's reflect padding for every T in 1024 .. 2000 and the lengths the GPU module runs).  On
  integer-valued frames every restated overlap-add -- frames_to_wave_kernel<1> and <4>, an_frames_to_wave_kernel,
  an_frames_to_wave4_kernel, the runs of an_logmel_bwd_ola_kernel for every number of runs the planner may cut, with
  an_edge_to_wave_kernel over an_ola_ranges -- equals the transposed framing EXACTLY, never gathers outside a frame, and the
  edge kernel reads only frames the fused kernel wrote.  Each planted index defect breaks that equality.
* The float64 model of the engine (restated framing, autograd of the restated per-frame forward, restated overlap-add) equals
  the float64 VJP of the oracle to 1e-9 of the utterance norm, in every form.
* The judge accepts the float32 yardstick on every case of the GPU module, and rejects each planted defect on a listed case.

Planted defects and the judged error on the listed case that rejects them (per row / worst 160-sample block, against bounds
of 6.1e-5 / 4.9e-4), measured here.  MFCC on (2, 5199) dense unless named: right reflection dropped 1.1e-2 / 9.0e-2; left
reflection off by one 4.1e-2 / 2.3e-1; last frame not gathered 1.8e-1 / 9.2e-1; DC-removal mean dropped 3.0e-2 / 6.8e-2; energy path
into c0 dropped 2.7e-3 / 5.9e-3; lifter missing on column 29: 1.5e-1 / 3.5e-1, on column 1 (one-hot family) 6.1e-1 / 3.4; dither
ignored in the backward ((2, 5041) with noise) 4.9e-1 / 9.9e-1; four-sample interior path one quad early at the left edge
((152, 5056) one-hot) 9.6e-2 / 5.4e-1, one quad late at the right edge 1.2e-1 / 6.9e-1 (dense: 5.7e-4 / 3.2e-3).  Log-mel on (2, 3681)
dense unless named: right reflection dropped 1.5e-1 / 7.0e-1; left reflection off by one 1.5e-1 / 6.7e-1; reflection about Lp
instead of Lp - 1: 1.8e-1 / 8.5e-1; last frame not gathered 3.2e-1 / 3.0; interior path one block early ((2, 4096)) 1.0e-1 / 6.5e-1;
pre-emphasis t == 0 term wrong 4.9e-2 / 2.4e-1; t == T - 1 term dropped 2.3e-2 / 1.4.

What the judgement does NOT reject, and what catches it instead:
  * MFCC, the pre-emphasis n == 0 term dropped: nothing can see it.  ``if (n == 0) g -= 0.97f * sw[0]`` multiplies the povey
    window's first tap, which is exactly 0 (so is its last): the term is identically zero in any arithmetic
    (test_the_mfcc_pre_emphasis_n0_term_is_identically_zero).
  * MFCC, the interior path one quad early, on a DENSE cotangent: the four samples lose columns 0 .. 3 of frame 0, where the povey
    window is below 2e-3 and only the energy and DC terms remain -- 3.0e-5 / 1.7e-4 on the first four rows of (152, 5056), half the
    bound.  The case that catches it is the one-hot family at the four-sample shapes (column 0, the energy path, of frame 0 and
    of frame F - 1 has no window): the figures above; the integer audit catches it at every T % 4 == 0.
  * log-mel, a halo of 4 frames instead of 5 at a run cut: what is lost is ONE term per cut, column 799 of frame fa - 5, where the
    periodic Hann window is 1.5e-5 -- 2.4e-7 / 1.5e-6 at (2, 16000) in 12 runs, 0.004 of the bound and below float32 round-off of
    the utterance.  What catches it: the integer audit here (the restated runs equal the transposed framing with a halo of 5
    or 6, not 4), and a bitwise comparison of the fused form with the separate pair (21 of 32000 float32 samples differ) --
    tests/test_gpu_audionet.py, and the in-situ case of tests/test_gpu_frontend_adjoint.py, both sides of which are also
    judged against float64.
"""
import numpy as np
import pytest
import torch

import frontend_adjoint as fa
from oracle import audionet as oan
from oracle import kaldi_mfcc as km

AN_LISTED = sorted({T for _, T in fa.AN_SHAPES} | {3680 + 1, 16000})


def _int_frames(F, W, seed):
    return np.random.RandomState(seed).randint(-8, 9, size=(F, W)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ index audit
def test_mfcc_index_audit_every_length_400_to_6000():
    seen = {d: 0 for d in ("no_right", "left_off_by_one", "no_last_frame", "interior_early", "interior_late_edge")}
    for T in range(400, 6001):
        idx = fa.xv_frame_index(T)
        assert idx.min() >= 0 and idx.max() < T, T
        assert np.array_equal(idx, km.get_strided(torch.arange(T)).numpy()), "frame map differs from get_strided at T=%d" % T
        df = _int_frames(idx.shape[0], fa.XV_WIN, T)
        want = fa.xv_scatter(df, T)
        forms = (1, 4) if T % 4 == 0 else (1,)
        for V in forms:
            assert np.array_equal(fa.xv_gather(df, T, V), want), "overlap-add V=%d differs from the transposed framing at T=%d" % (V, T)
        if T % 97 == 0 or T in (400, 5040, 5056, 6000):  # (the defects: a sample of lengths is enough to show each one breaks)
            for d in seen:
                V = 4 if d.startswith("interior") else 1
                if V == 4 and T % 4:
                    continue
                seen[d] += not np.array_equal(fa.xv_gather(df, T, V, d), want)
    assert all(seen.values()), seen


def _an_torch_index(T):
    Lp = T - 1
    padded = torch.nn.functional.pad(torch.arange(Lp, dtype=torch.float64)[None, None], (fa.AN_FFT // 2, fa.AN_FFT // 2), mode="reflect")[0, 0]
    off = (fa.AN_FFT - fa.AN_WIN) // 2
    pos = np.arange(fa.an_num_frames(T))[:, None] * fa.AN_HOP + off + np.arange(fa.AN_WIN)[None, :]
    return padded.numpy()[pos].astype(np.int64)


def _an_audit(T, seen):
    idx = fa.an_frame_index(T)
    F = idx.shape[0]
    assert idx.min() >= 0 and idx.max() < T - 1, T
    assert np.array_equal(idx, _an_torch_index(T)), "frame map differs from torch.stft's reflect padding at T=%d" % T
    df = _int_frames(F, fa.AN_WIN, T)
    dpre = fa.an_scatter(df, T)
    want = fa._an_pair(dpre, T)
    same = lambda got: np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert same(fa.an_form_one(df, T)), "one-position form differs at T=%d" % T
    if T % 4 == 0:
        assert same(fa.an_form_quad(df, T)), "four-position form differs at T=%d" % T
        seen["interior_early"] += not same(fa.an_form_quad(df, T, "interior_early"))
    runs = sorted(set(range(1, max(F // 8, 1) + 1)) | {fa.an_ola_slices(B, F, f32) for B in (2, 3, 5) for f32 in (True, False)})
    for S in runs:
        assert same(fa.an_form_ola(df, T, S)), "fused overlap-add in %d runs differs at T=%d" % (S, T)
        if S > 1:
            seen["halo_4"] += not same(fa.an_form_ola(df, T, S, halo=4))
            assert same(fa.an_form_ola(df, T, S, halo=6)), "a longer halo must not change the sums (T=%d, S=%d)" % (T, S)
    for d in ("no_right", "left_off_by_one", "about_Lp", "no_last_frame"):
        seen[d] += not same(fa.an_form_one(df, T, d))


def test_logmel_index_audit_every_length_1024_to_2000_and_the_listed_lengths():
    seen = {d: 0 for d in ("no_right", "left_off_by_one", "about_Lp", "no_last_frame", "interior_early", "halo_4")}
    for T in list(range(1024, 2001)) + AN_LISTED:
        _an_audit(T, seen)
    assert all(seen.values()), seen
    assert fa.an_ola_slices(3, fa.an_num_frames(16000)) == 12  # the in-situ GPU case cuts 12 runs: the halo is exercised
    assert fa.an_ola_ranges(3684, fa.an_num_frames(3684))[0] <= 3683 and fa.an_num_frames(3680) == 23


# ------------------------------------------------------------------------------------------------------ the float64 model
def _rel(a, b):
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def test_restated_forwards_are_the_oracles():
    from speakerguard_amd import synth
    x = torch.from_numpy(synth.make_waveforms(1, 5041, seed=3)).double()[0, 0]
    xs = x * 32768.0
    a, b = fa.xv_forward_frames(xs[torch.as_tensor(fa.xv_frame_index(5041))]), km.mfcc(xs)
    assert torch.equal(a, b)
    pre = x[1:] - oan.PREEMPH * x[:-1]
    a = fa.an_forward_frames(pre[torch.as_tensor(fa.an_frame_index(5041))])
    b = oan.preprocess(x[None])[0].t()
    assert a.shape == b.shape and float((a - b).abs().max()) < 1e-9  # dB, values of -60 .. 20


@pytest.mark.parametrize("c,V", [(fa.Case("xv", 2, 5041, "dense", None), 1), (fa.Case("xv", 2, 5041, "dense", "noise"), 1),
                                 (fa.Case("xv", 2, 5041, "dense", "int16"), 1), (fa.Case("xv", 2, 5200, "onehot", None), 4),
                                 (fa.Case("iv", 2, 400, "dense", None), 1), (fa.Case("iv", 2, 401, "onehot", None), 1)],
                         ids=lambda v: fa.case_id(v) if isinstance(v, fa.Case) else "V%d" % v)
def test_mfcc_float64_model_equals_the_float64_truth(c, V):
    i, (_, g64) = fa.inputs(c), fa.truths(c)
    got = fa.xv_candidate(i["x"], fa.cot30(c, i["cot"]), i["noise"], V)
    assert _rel(got, g64) < 1e-9
    assert np.array_equal(got == 0, g64 == 0)


@pytest.mark.parametrize("form,T,S", [("one", 3681, 1), ("quad", 4096, 1), ("ola", 4096, 3), ("ola", 3684, 1), ("ola", 16000, 12)])
@pytest.mark.parametrize("kind", ("dense", "onehot"))
def test_logmel_float64_model_equals_the_float64_truth(form, T, S, kind):
    c = fa.Case("an", 2, T, kind, None)
    i, (_, g64) = fa.inputs(c), fa.truths(c)
    got = fa.an_candidate(i["x"][:3], i["cot"][:3], form, S)
    assert _rel(got, g64[:3]) < 1e-9


# ------------------------------------------------------------------------------------------------------ the judgement
@pytest.mark.parametrize("c", fa.XV_CASES + fa.IV_CASES + fa.AN_CASES, ids=fa.case_id)
def test_judge_accepts_the_float32_yardstick(c):
    yard, g64 = fa.truths(c)
    fails, line, _ = fa.judge(yard, yard, g64)
    print(fa.case_id(c), line)
    assert not fails, (fails[:6], line)
    assert np.array_equal(yard == 0, g64 == 0), "float32 and float64 disagree on which samples are exactly zero"
    assert np.abs(g64).max() > 0


XV_DENSE, XV_HOT = fa.Case("xv", 2, 5199, "dense", None), fa.Case("xv", 2, 5199, "onehot", None)
XV_QUAD_DENSE, XV_QUAD_HOT = fa.Case("xv", 152, 5056, "dense", None), fa.Case("xv", 152, 5056, "onehot", None)
XV_NOISE = fa.Case("xv", 2, 5041, "dense", "noise")
AN_DENSE, AN_QUAD, AN_RUNS = fa.Case("an", 2, 3681, "dense", None), fa.Case("an", 2, 4096, "dense", None), fa.Case("an", 2, 16000, "dense", None)
XV_DEFECTS = [  # (name, case, candidate keywords, rows judged)
    ("right reflection dropped", XV_DENSE, dict(gather_defect="no_right"), 2),
    ("left reflection off by one", XV_DENSE, dict(gather_defect="left_off_by_one"), 2),
    ("last frame not gathered", XV_DENSE, dict(gather_defect="no_last_frame"), 2),
    ("interior path one quad early, one-hot", XV_QUAD_HOT, dict(V=4, gather_defect="interior_early"), 15),
    ("interior path one quad late at the right edge, one-hot", XV_QUAD_HOT, dict(V=4, gather_defect="interior_late_edge"), 15),
    ("interior path one quad late at the right edge, dense", XV_QUAD_DENSE, dict(V=4, gather_defect="interior_late_edge"), 4),
    ("DC-removal mean dropped", XV_DENSE, dict(frame_defect="no_dc_mean"), 2),
    ("energy path into c0 dropped", XV_DENSE, dict(frame_defect="no_energy"), 2),
    ("lifter missing on column 1", XV_HOT, dict(frame_defect="lifter_1"), 15),
    ("lifter missing on column 29", XV_DENSE, dict(frame_defect="lifter_29"), 2),
    ("dither ignored in the backward", XV_NOISE, dict(backward_noise=False), 2),
]
AN_DEFECTS = [
    ("right reflection dropped", AN_DENSE, dict(gather_defect="no_right"), 2),
    ("left reflection off by one", AN_DENSE, dict(gather_defect="left_off_by_one"), 2),
    ("reflection about Lp instead of Lp - 1", AN_DENSE, dict(gather_defect="about_Lp"), 2),
    ("last frame not gathered", AN_DENSE, dict(gather_defect="no_last_frame"), 2),
    ("interior path one block early", AN_QUAD, dict(form="quad", gather_defect="interior_early"), 2),
    ("pre-emphasis t == 0 term wrong", AN_DENSE, dict(dx_defect="t0"), 2),
    ("pre-emphasis t == T - 1 term dropped", AN_DENSE, dict(dx_defect="tlast"), 2),
]


def _judge_candidate(c, kw, rows, model):
    i, (yard, g64) = fa.inputs(c), fa.truths(c)
    x, cot = i["x"][:rows], fa.cot30(c, i["cot"][:rows])
    if model == "xv":
        got = fa.xv_candidate(x, cot, None if i["noise"] is None else i["noise"][:rows], **kw)
    else:
        got = fa.an_candidate(x, cot, **kw)
    return fa.judge(got, yard[:rows], g64[:rows])


@pytest.mark.parametrize("name,c,kw,rows", XV_DEFECTS, ids=[d[0] for d in XV_DEFECTS])
def test_judge_rejects_each_planted_mfcc_defect(name, c, kw, rows):
    fails, line, _ = _judge_candidate(c, kw, rows, "xv")
    print("MFCC, %s on %s: %s" % (name, fa.case_id(c), line))
    assert fails, line
    clean = {k: v for k, v in kw.items() if k == "V"}
    assert not _judge_candidate(c, clean, rows, "xv")[0], "the model without the defect is not accepted"


@pytest.mark.parametrize("name,c,kw,rows", AN_DEFECTS, ids=[d[0] for d in AN_DEFECTS])
def test_judge_rejects_each_planted_logmel_defect(name, c, kw, rows):
    fails, line, _ = _judge_candidate(c, kw, rows, "an")
    print("log-mel, %s on %s: %s" % (name, fa.case_id(c), line))
    assert fails, line
    clean = {k: v for k, v in kw.items() if k == "form"}
    assert not _judge_candidate(c, clean, rows, "an")[0], "the model without the defect is not accepted"


def test_the_mfcc_pre_emphasis_n0_term_is_identically_zero():
    """``if (n == 0) g -= 0.97f * sw[0]`` multiplies the povey window's first tap, which is exactly 0 (as is its last, so no
    end term of the pre-emphasis adjoint reaches a sample): dropping it changes nothing, in any arithmetic"""
    w = km.povey_window()
    assert float(w[0]) == 0.0 and float(w[-1]) == 0.0
    i = fa.inputs(XV_DENSE)
    a, b = (fa.xv_candidate(i["x"], i["cot"], frame_defect=d) for d in (None, "no_preemph_n0"))
    assert np.array_equal(a, b)


def test_the_defects_a_dense_cotangent_cannot_see_and_what_catches_them():
    """a halo of 4 frames: the measured size of the module docstring; caught by the integer audit above and by a bitwise
    comparison of the fused form with the separate pair"""
    fails, line, ratio = _judge_candidate(XV_QUAD_DENSE, dict(V=4, gather_defect="interior_early"), 4, "xv")
    print("MFCC, interior path one quad early on %s, 4 rows: %s" % (fa.case_id(XV_QUAD_DENSE), line))
    assert not fails, "the dense cotangent now sees this defect: move it to XV_DEFECTS"
    fails, line, ratio = _judge_candidate(AN_RUNS, dict(form="ola", S=12, halo=4), 2, "an")
    print("log-mel, halo of 4 frames on %s in 12 runs: %s" % (fa.case_id(AN_RUNS), line))
    assert not fails and ratio < 0.01
    i = fa.inputs(AN_RUNS)
    five, four = (fa.an_candidate(i["x"], i["cot"], "ola", 12, h) for h in (5, 4))
    differ = five.astype(np.float32) != four.astype(np.float32)
    print("log-mel, halo of 4 frames: %d of %d float32 samples differ (a bitwise comparison of the two forms sees them)"
          % (differ.sum(), differ.size))
    assert differ.any()
