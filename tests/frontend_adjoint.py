"""The two front-end adjoints -- d loss / d raw MFCC -> d loss / d wav (mfcc_bwd_kernel, frames_to_wave_kernel<1|4>,
k_mfcc.hip) and d loss / d log-mel -> d loss / d wav (an_logmel_bwd_kernel, an_frames_to_wave_kernel, an_frames_to_wave4_kernel,
an_logmel_bwd_ola_kernel + an_edge_to_wave_kernel, k_audionet.hip) -- restated for tests/test_gpu_frontend_adjoint.py.  TEST
INFRASTRUCTURE (a plain module, not a conftest); proved on the CPU, without the engine, by tests/test_frontend_adjoint_power.py.

Both stages are linear in the cotangent, so a float64 vector-Jacobian product of the oracle's front end (oracle/kaldi_mfcc.py
``mfcc_batch``, oracle/audionet.py ``preprocess``, each behind the oracle's own input-range rule) is an exact truth for ANY
cotangent, a one-hot one that lights a single edge frame included.  Here:

* truths and yardstick -- ``xv_vjp`` / ``an_vjp``: torch.autograd of the oracle in float64 (truth) and float32 (yardstick);
  ``shared=True`` evaluates one waveform once and takes one VJP per cotangent row (a family of one-hots is one engine call).
* cotangents -- ``dense`` (seeded normals) and ``one_hot_rows`` (one row per (frame, column)).
* cases -- ``XV_CASES`` / ``IV_CASES`` / ``AN_CASES``: every (shape, cotangent) the GPU module runs, built by ``inputs`` and
  judged against ``truths`` (cached: computed once, shared by every test that needs them, never modified).
* numpy restatements of the index arithmetic as the kernels write it -- ``xv_frame_index`` (load_frame), ``xv_gather``
  (frames_to_wave_kernel<V>, the V = 4 interior predicate included), ``an_frame_index`` (an_load_frame / an_reflect),
  ``an_form_one`` / ``an_form_quad`` / ``an_form_ola`` (the three overlap-add forms: one position per thread, four with the
  block-wide interior predicate, runs with a 5-frame halo + the edge kernel over ``an_ola_ranges``), ``an_dx`` (the
  pre-emphasis adjoint with its end terms) -- and of the per-frame forwards (``xv_forward_frames``, ``an_forward_frames``), so
  that ``xv_candidate`` / ``an_candidate`` are a float64 model of the engine in which a defect can be planted by name.
* ``judge(got, yard, g64)`` -- the per-utterance rule of tests/truth.py (POLICY's C, FLOOR_UTT, FLOOR_BLOCK, TAU, unchanged; the
  rule ``xv_backward.judge`` applies) over 160-sample blocks, plus: where the float64 truth is exactly 0 the judged value is
  exactly 0 (a frame with a zero cotangent contributes zeros in exact arithmetic).  Every element of every row is judged.
* the floors -- ``FLOOR_CASES``: digital silence written over the utterances (``FLOOR_LAYOUTS``, ``apply_layout``) so that both
  logarithms take their floor, forward and backward; ``floor_report`` (what the oracle's floors see, in float64 and float32, and
  the silent frames), ``forward_oracle`` / ``forward_candidate`` / ``forward_fails`` (the forward under the suite's own bounds)
  and the slips ``floored_log`` plants by name (FLOOR_SLIPS); run by tests/test_gpu_frontend_floor.py, proved on the CPU by
  tests/test_frontend_floor_power.py, which also states the condition on these inputs under which the VJP stays a truth.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import truth
from oracle import audionet as oan
from oracle import kaldi_mfcc as km
from oracle.xv_plda import check_input_range as xv_input_range

HOP = truth.HOP
XV_WIN, XV_SHIFT, XV_PAD, XV_CEPS, IV_CEPS = 400, 160, 120, 30, 24  # kWin, kShift, kWin / 2 - kShift / 2, kCep
AN_WIN, AN_HOP, AN_FFT, AN_MEL = 800, 160, 1024, 32                 # kAnWin, kAnHop, kAnFft, kAnMel
AN_QUAD_BLOCK, AN_HALO, AN_CUS = 1024, 5, 256                      # kAnF2wPerBlock, the halo of a run cut, kAnCus
QUAD_MIN = 16 * 48000  # launch_frames_to_wave: four samples per thread once B T reaches this (and T % 4 == 0)


# ---------------------------------------------------------------------------------------------------------------- truths
def _rows(t):
    return t.detach().double().numpy().reshape(t.shape[0], -1)


def _vjp(forward, x, cot, dtype, shared):
    x = torch.as_tensor(np.asarray(x, np.float32))
    cot = torch.as_tensor(np.asarray(cot, np.float32)).to(dtype)
    leaf = x.to(dtype).clone().requires_grad_(True)
    feats = forward(leaf)
    if not shared:
        assert feats.shape == cot.shape, (feats.shape, cot.shape)
        return _rows(torch.autograd.grad(feats, leaf, cot)[0])
    assert x.shape[0] == 1 and feats.shape[1:] == cot.shape[1:], (x.shape, feats.shape, cot.shape)
    return np.concatenate([_rows(torch.autograd.grad(feats, leaf, cot[r:r + 1], retain_graph=True)[0]) for r in range(cot.shape[0])])


def xv_vjp(x, cot, dtype=torch.float64, noise=None, shared=False):
    """x (B, 1, T) float32 as the engine receives it, cot (B, F, 30) -> d <cot, mfcc(x)> / d x, (B, T) float64, by autograd of
    oracle.kaldi_mfcc.mfcc_batch behind the oracle's range rule (oracle.xv_plda.check_input_range) in `dtype`.
    noise: explicit dither (B, F, 400), added to the strided int16-scale frames.  shared: x is (1, 1, T), one VJP per row."""
    nz = None if noise is None else torch.as_tensor(np.asarray(noise, np.float32)).to(dtype)
    return _vjp(lambda w: km.mfcc_batch(xv_input_range(w, "origin"), nz), x, cot, dtype, shared)


def an_vjp(x, cot, dtype=torch.float64, shared=False):
    """x (B, 1, T), cot (B, F, 32) -> (B, T) float64: autograd of oracle.audionet.preprocess behind its range rule"""
    return _vjp(lambda w: oan.preprocess(oan.check_input_range(w, "scale").squeeze(1)).transpose(1, 2), x, cot, dtype, shared)


# ---------------------------------------------------------------------------------------------------------------- cotangents
def dense(B, F, D, seed):
    return np.random.RandomState(seed).standard_normal((B, F, D)).astype(np.float32)


def one_hot_rows(F, D, frames, cols, rows=None):
    """(rows, F, D): row r is 1 at combo r % n of the n distinct (frame, column) pairs, 0 elsewhere -> (cot, n)"""
    combos = [(f, c) for f in sorted({int(f) for f in frames}) for c in cols]
    assert all(0 <= f < F and 0 <= c < D for f, c in combos), (F, D, combos)
    rows = len(combos) if rows is None else rows
    out = np.zeros((rows, F, D), np.float32)
    for r in range(rows):
        f, c = combos[r % len(combos)]
        out[r, f, c] = 1.0
    return out, len(combos)


def xv_num_frames(T):
    return (T + XV_SHIFT // 2) // XV_SHIFT


def an_num_frames(T):
    return (T - 1) // AN_HOP + 1


# ---------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "model B T kind variant")  # model xv | iv | an; kind dense | onehot; variant None | int16 | noise | a layout
XV_LENGTHS = (5040, 5041, 5119, 5199, 5200, 16123)  # both sides of a frame-count step, right reflection of 41 .. 200 samples
# (16 | 15, 48000): the two sides of B T >= 16 x 48000; (152, 5056): four samples per thread with both edges inside a 32-frame
# utterance and 4864 frames > 512 blocks x 8 waves (the grid-stride loop iterates); (150, 5121): as large, T % 4 != 0
XV_SHAPES = tuple((2, T) for T in XV_LENGTHS) + ((16, 48000), (15, 48000), (152, 5056), (150, 5121))
XV_SHORT = (400, 401, 479, 480, 559, 560, 719, 720)
AN_SHAPES = tuple((2, T) for T in (3681, 3684, 3840, 3841, 4096, 16000, 16001)) + ((5, 4096),)
XV_ONE_HOT_COLS, AN_ONE_HOT_BINS = (0, 1, 29), (0, 31)  # column 0: the energy path
XV_CASES = tuple(Case("xv", B, T, k, None) for B, T in XV_SHAPES for k in ("dense", "onehot")) + (
    Case("xv", 2, 5041, "dense", "int16"), Case("xv", 2, 5041, "dense", "noise"))
IV_CASES = tuple(Case("iv", 2, T, k, None) for T in XV_SHORT for k in ("dense", "onehot"))
AN_CASES = tuple(Case("an", B, T, k, None) for B, T in AN_SHAPES for k in ("dense", "onehot"))

# ---- digital silence: spans of exact zeros written over the utterance after it is generated, so that both log floors are
# taken, forward and backward (tests/test_frontend_floor_power.py states the condition these inputs meet, tests/
# test_gpu_frontend_floor.py runs them).  A layout is a list of (start, stop, value) spans of row 0; row r moves every
# boundary that is not an end of the utterance by ROW_SHIFT r samples, so the rows sit at different frame phases.
ROW_SHIFT = 53
FLOOR_LAYOUTS = {  # T -> spans; None as a bound: that end of the utterance
    "gap": lambda T: [(T // 3, T // 3 + 2000, 0.0)],
    "lead": lambda T: [(None, 1500, 0.0)],
    "trail": lambda T: [(T - 1500, None, 0.0)],
    "edges": lambda T: [(None, 1500, 0.0), (T - 1700, None, 0.0)],  # the zero-padded utterance: both reflections inside silence
    "all": lambda T: [],  # row 0 entirely zero, row 1 untouched speech (the batch's range rule still says "scale")
    # x-vector only: a hard clip at PGD's upper clamp.  32768 x 400 / 400 is exact in float32 and float64, so DC removal leaves
    # exact zeros: raw samples nonzero, every floor taken.  (AudioNet has no DC removal; its windowed constant leaks ~1e-16.)
    "plateau": lambda T: [(2000, 4000, 1.0)],
    # AudioNet only: the last nonzero sample of the PRE-EMPHASISED signal (index s - 1 when x[s:] is zero) is column 0 of
    # frame f, s = 160 f - 399, where the periodic Hann window is exactly 0: that frame's raw content is nonzero, its windowed
    # content exactly zero.  (Only column 0 can do this -- the window's last tap is 1.5e-5 --, so the frame is the one where
    # speech stops; read backwards in time, where it starts.)  Rows move by one hop, not by ROW_SHIFT: the alignment is the case.
    "window0": lambda T: [(160 * ((T - 1500 + 399) // 160) - 399, None, 0.0)],
    "lead480": lambda T: [(None, 480, 0.0)],  # the i-vector route at T = 720: frames 0 and 1 silent, frame 2 partial
}
XV_FLOOR_LAYOUTS = ("gap", "lead", "trail", "edges", "all", "plateau")
AN_FLOOR_LAYOUTS = ("gap", "lead", "trail", "edges", "all", "window0")
# Boundaries moved off the table above, {case: {row: samples}}.  None was needed for the condition on the pre-log values
# (test_inputs_keep_clear_of_the_floor).  One for the condition that the truth does not depend on the CPU that built the
# oracle's float32 mel bank (test_truths_do_not_depend_on_the_cpu_that_built_the_mel_bank): row 4 of (16, 48000) ``edges`` led
# with 1712 zeros, which leaves frame 9 eight samples of speech under the last eight taps of the povey window (<= 0.0072); its
# gradient on the 392 silent samples is what is left of a near-total cancellation across the spectrum, and two CPUs' mel banks
# (they differ in 34 weights by at most 2.8e-6) move the float64 VJP there by 6.6e-4 of the row's RMS -- more than the bound.
# Eight samples later the frame is silent.
FLOOR_MOVES = {Case("xv", 16, 48000, "dense", "edges"): {4: 8}}
XV_FLOOR_CASES = tuple(Case("xv", 2, T, "dense", v) for T in (5200, 16123) for v in XV_FLOOR_LAYOUTS) + tuple(
    Case("xv", 2, T, "onehot", "gap") for T in (5200, 16123)) + (Case("xv", 16, 48000, "dense", "edges"),)
IV_FLOOR_CASES = (Case("iv", 2, 720, "dense", "lead480"),)
AN_FLOOR_CASES = tuple(Case("an", 2, T, "dense", v) for T in (4096, 16001) for v in AN_FLOOR_LAYOUTS) + tuple(
    Case("an", 2, T, "onehot", "gap") for T in (4096, 16001))
FLOOR_CASES = XV_FLOOR_CASES + IV_FLOOR_CASES + AN_FLOOR_CASES


def apply_layout(x, layout, rows=None, moves=None):
    """x (R, 1, T) float32, overwritten in place with `layout`'s spans; row r is shifted as batch row rows[r] (default r),
    plus moves[row] samples (FLOOR_MOVES)"""
    R, _, T = x.shape
    rows = range(R) if rows is None else rows
    for r, k in enumerate(rows):
        if layout == "all":
            if k == 0:
                x[r] = 0.0
            continue
        shift = (AN_HOP if layout == "window0" else ROW_SHIFT) * k + (moves or {}).get(k, 0)
        for a, b, value in FLOOR_LAYOUTS[layout](T):
            a, b = 0 if a is None else a + shift, T if b is None else b + shift
            assert 0 <= a < b <= T, (layout, T, k, a, b)
            x[r, 0, a:b] = value
    return x


def is_floor_case(c):
    return c.variant in FLOOR_LAYOUTS


def case_id(c):
    return "%s_B%d_T%d_%s%s" % (c.model, c.B, c.T, c.kind, "_" + c.variant if c.variant else "")


def xv_one_hot_frames(F):
    return (0, 1, F // 2, F - 2, F - 1)


def an_one_hot_frames(F):
    return (0, 5, 6, F - 6, F - 5, F - 1)  # the boundaries of what the edge kernel owns


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> dict(x (R, 1, T) float32 as the engine gets it, cot (R, F, D) float32, noise (R, F, 400) or None, shared, n): a
    one-hot family shares ONE waveform over its R rows (R = B where the launcher's choice depends on B T, else the n combos)"""
    from speakerguard_amd import synth
    F = an_num_frames(c.T) if c.model == "an" else xv_num_frames(c.T)
    D = {"xv": XV_CEPS, "iv": IV_CEPS, "an": AN_MEL}[c.model]
    seed = 7000 + c.B + c.T
    noise = None
    if is_floor_case(c):
        if c.kind == "dense":
            x = apply_layout(synth.make_waveforms(c.B, c.T, seed=seed), c.variant, moves=FLOOR_MOVES.get(c))
            return dict(x=x, cot=dense(c.B, F, D, seed + 1), noise=None, shared=False, n=c.B)
        x = apply_layout(synth.make_waveforms(1, c.T, seed=seed), c.variant)
        silent = sorted(f for _, f in silent_frames(c.model, x))
        assert silent and silent == list(range(silent[0], silent[-1] + 1)) and 0 < silent[0] and silent[-1] < F - 1, silent
        # the last speech frame before the silence, its first, a middle and its last frame, the first speech frame after it
        frames = (silent[0] - 1, silent[0], silent[len(silent) // 2], silent[-1], silent[-1] + 1)
        cot, n = one_hot_rows(F, D, frames, AN_ONE_HOT_BINS if c.model == "an" else XV_ONE_HOT_COLS)
        return dict(x=np.repeat(x, cot.shape[0], 0), cot=cot, noise=None, shared=True, n=n)
    if c.kind == "dense":
        x = synth.make_waveforms(c.B, c.T, seed=seed)
        cot, n, shared = dense(c.B, F, D, seed + 1), c.B, False
    else:
        frames, cols = (an_one_hot_frames(F), AN_ONE_HOT_BINS) if c.model == "an" else (
            xv_one_hot_frames(F), tuple(min(k, D - 1) for k in XV_ONE_HOT_COLS))  # (the i-vector route: its last column, 23)
        rows = c.B if c.B * c.T >= 15 * 48000 else None
        cot, n = one_hot_rows(F, D, frames, cols, rows)
        x = np.repeat(synth.make_waveforms(1, c.T, seed=seed), cot.shape[0], 0)
        shared = True
    if c.variant == "int16":
        x = (x * np.float32(32768.0)).astype(np.float32)
    if c.variant == "noise":  # RMS a quarter of the int16-scale signal's: dropped or misplaced noise is an order-one change
        rms = float(np.sqrt(np.mean((x.astype(np.float64) * 32768.0) ** 2)))
        noise = (0.25 * rms * np.random.RandomState(seed + 2).standard_normal((x.shape[0], F, XV_WIN))).astype(np.float32)
    return dict(x=x, cot=cot, noise=noise, shared=shared, n=n)


def cot30(c, cot):
    """the cotangent as the MFCC sees it: the i-vector route's 24 columns padded with zeros into the 30"""
    if c.model != "iv":
        return cot
    out = np.zeros(cot.shape[:2] + (XV_CEPS,), np.float32)
    out[:, :, :IV_CEPS] = cot
    return out


@functools.lru_cache(maxsize=None)
def truths(c):
    """-> (yard (R, T), g64 (R, T)) float64, read-only: the float32 and the float64 VJP of the oracle at inputs(c)"""
    i = inputs(c)
    n, R = i["n"], i["cot"].shape[0]
    out = []
    for dtype in (torch.float32, torch.float64):
        if c.model == "an":
            g = an_vjp(i["x"][:1], i["cot"][:n], dtype, True) if i["shared"] else an_vjp(i["x"], i["cot"], dtype)
        elif i["shared"]:
            g = xv_vjp(i["x"][:1], cot30(c, i["cot"][:n]), dtype, None, True)
        else:
            g = xv_vjp(i["x"], cot30(c, i["cot"]), dtype, i["noise"])
        g = g[np.arange(R) % n] if i["shared"] else g
        g.setflags(write=False)
        out.append(g)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- the floors
XV_FLOOR, AN_FLOOR = float(km.EPSILON), oan.EPSILON  # kEps of k_mfcc.hip (float32 eps), 1e-16f of k_audionet.hip


def oracle_pre_log(model, x, dtype=torch.float64):
    """what the oracle's floors see at x (R, 1, T) float32 as the engine receives it, in `dtype` -> (frame energies (R, F) or
    None for AudioNet, mel energies (R, F, D)).  The oracle's own lines up to its clamp: oracle.kaldi_mfcc.mfcc's framing
    (get_strided) and per-frame arithmetic (xv_forward_frames, bit-equal to it), oracle.audionet.preprocess's torch.stft;
    tests/test_frontend_floor_power.py checks that the logarithm of these IS the oracle's output, bit for bit."""
    w = torch.as_tensor(np.asarray(x, np.float32)).to(dtype)
    if model == "an":
        wav = oan.check_input_range(w, "scale").squeeze(1)
        wav = wav[:, 1:] - oan.PREEMPH * wav[:, :-1]
        spec = torch.stft(wav, n_fft=oan.N_FFT, hop_length=oan.HOP, win_length=oan.WIN, window=torch.hann_window(oan.WIN, dtype=dtype),
                          center=True, pad_mode="reflect", return_complex=True)
        mag = spec.real.pow(2) + spec.imag.pow(2)
        mel = torch.matmul(mag.transpose(2, 1), torch.from_numpy(oan.mel_basis()).t().to(dtype))
        return None, mel.numpy()
    w = xv_input_range(w, "origin")
    pairs = [xv_forward_frames(km.get_strided(w[r, 0]), pre_log=True) for r in range(w.shape[0])]
    return np.stack([e.numpy() for e, _ in pairs]), np.stack([m.numpy() for _, m in pairs])


def silent_frames(model, x):
    """{(row, frame)} whose every pre-log value is exactly 0 in the float64 oracle"""
    energy, mel = oracle_pre_log(model, x)
    dead = (mel == 0).all(2) if energy is None else (mel == 0).all(2) & (energy == 0)
    return {(int(r), int(f)) for r, f in zip(*np.nonzero(dead))}


@functools.lru_cache(maxsize=None)
def floor_report(c):
    """-> dict(f64=(energy, mel), f32=(energy, mel), silent={(row, frame)}, floor): ``oracle_pre_log`` of the distinct waveforms
    of inputs(c) (one for a one-hot family) in float64 and float32, the silent frames of the float64 one, the floor's value"""
    i = inputs(c)
    x = i["x"][:1] if i["shared"] else i["x"]
    return dict(f64=oracle_pre_log(c.model, x), f32=oracle_pre_log(c.model, x, torch.float32), silent=silent_frames(c.model, x),
                floor=AN_FLOOR if c.model == "an" else XV_FLOOR)


def forward_oracle(c, dtype=torch.float32):
    """the oracle's features at inputs(c), (R, F, D) in `dtype` (the i-vector route: the first 24 columns), as the forward
    tests of the suite compute them: oracle.kaldi_mfcc.mfcc_batch / oracle.audionet.preprocess behind the range rule"""
    x = torch.as_tensor(inputs(c)["x"]).to(dtype)
    if c.model == "an":
        return oan.preprocess(oan.check_input_range(x, "scale").squeeze(1)).transpose(1, 2).numpy()
    return km.mfcc_batch(xv_input_range(x, "origin")).numpy()[:, :, :IV_CEPS if c.model == "iv" else XV_CEPS]


def forward_candidate(c, defect=None):
    """the engine's forward modelled in float64 (restated framing, restated per-frame forward), with a floor defect planted"""
    x = inputs(c)["x"]
    x = x.reshape(len(x), -1)
    out = []
    for r in range(1 if inputs(c)["shared"] else x.shape[0]):
        if c.model == "an":
            out.append(an_forward_frames(an_frames(x[r], input_scale(x, "scale")), defect).numpy())
        else:
            xs = torch.as_tensor(x[r].astype(np.float64)) * input_scale(x, "origin")
            out.append(xv_forward_frames(xs[torch.as_tensor(xv_frame_index(x.shape[1]))], defect).numpy())
    out = np.stack(out)[:, :, :IV_CEPS if c.model == "iv" else None]
    return np.repeat(out, len(x), 0) if inputs(c)["shared"] else out


def forward_fails(got, want, model):
    """the suite's own forward bounds, unchanged: rtol 1e-4, atol 5e-3 (test_mfcc_matches_oracle); atol 8e-4 (the log-mel test)
    -> a description of the failure, or None"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.isfinite(got).all():
        return "%d non-finite features" % (~np.isfinite(got)).sum()
    rtol, atol = (0.0, 8e-4) if model == "an" else (1e-4, 5e-3)
    bad = np.abs(got - want) > atol + rtol * np.abs(want)
    return "%d features off, the worst by %.3e" % (bad.sum(), np.abs(got - want).max()) if bad.any() else None


# ---------------------------------------------------------------------------------------------------------------- judgement
def judge(got, yard, g64, hop=HOP):
    """-> (violations [(metric, row, value, bound)], one line of judged / yard / bound, the largest judged error over its
    bound).  Per row: utt_error <= C max(yard's, FLOOR_UTT); block_error over `hop` samples <= C max(yard's, FLOOR_BLOCK); no
    decided sign wrong; exactly 0 wherever g64 is exactly 0."""
    P = truth.POLICY
    R = np.asarray(g64).shape[0]
    got, yard, g64 = (np.asarray(a, np.float64).reshape(R, -1) for a in (got, yard, g64))
    assert got.shape == yard.shape == g64.shape, (got.shape, yard.shape, g64.shape)
    fails, worst = [], {}
    if not np.isfinite(got).all():
        fails.append(("finite", -1, float((~np.isfinite(got)).sum()), 0))
        got = np.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30)
    for name, fn, floor in (("utt", truth.utt_error, P["FLOOR_UTT"]),
                            ("block", lambda a, b: truth.block_error(a, b, hop), P["FLOOR_BLOCK"])):
        j, y = fn(got, g64), fn(yard, g64)
        bound = P["C"] * np.maximum(y, floor)
        worst[name] = (float(j.max()), float(y.max()), float(bound.min()), float((j / bound).max()))
        fails += [(name, int(u), float(j[u]), float(bound[u])) for u in np.flatnonzero(~(j <= bound))]
    signs = truth.decided_sign(got, g64)
    fails += [("decided_sign", int(u), int(signs[u]), 0) for u in np.flatnonzero(signs != 0)]
    nonzero = ((g64 == 0) & (got != 0)).sum(1)
    fails += [("exact_zero", int(u), int(nonzero[u]), 0) for u in np.flatnonzero(nonzero)]
    line = ("utt judged %.2e yard %.2e bound >= %.2e (worst %.2f of it), block judged %.2e yard %.2e bound >= %.2e (worst %.2f "
            "of it), decided signs %d, nonzero at an exact zero %d of %d" % (worst["utt"] + worst["block"] + (
                int(signs.sum()), int(nonzero.sum()), int((g64 == 0).sum()))))
    return fails, line, max(worst["utt"][3], worst["block"][3])


# ---------------------------------------------------------------------------------------------------------------- MFCC, restated
def xv_frame_index(T):
    """load_frame: (F, 400) index of the waveform sample frame f reads at n (reflected at both ends, snip_edges=False)"""
    p = np.arange(xv_num_frames(T))[:, None] * XV_SHIFT - XV_PAD + np.arange(XV_WIN)[None, :]
    return np.where(p < 0, -p - 1, np.where(p >= T, 2 * T - 1 - p, p))


def _xv_add_pos(df, p, on, last):
    """add_pos of frames_to_wave_kernel over an array of padded-signal positions (where `on`); frames flo .. min(fhi, last)"""
    q = p + XV_PAD
    assert (q[on] >= 0).all()
    fhi = np.minimum(q // XV_SHIFT, last)
    flo = np.where(q > XV_WIN - 1, (q - (XV_WIN - 1) + XV_SHIFT - 1) // XV_SHIFT, 0)
    assert not (on & (flo + 3 <= fhi)).any()  # at most three frames cover a position
    g = np.zeros(p.shape)
    for k in range(3):
        f = flo + k
        ok = on & (f <= fhi)
        col = q - f * XV_SHIFT
        assert (f[ok] >= 0).all() and (col[ok] >= 0).all() and (col[ok] < XV_WIN).all(), "gather outside a frame"
        g[ok] += df[f[ok], col[ok]]
    return g


def xv_gather(df, T, V=1, defect=None):
    """frames_to_wave_kernel<V>: df (F, 400) per-frame sample gradients -> (T,) overlap-add through both reflections.
    defect: None | no_right | left_off_by_one | no_last_frame | interior_early (one quad, the left edge) | interior_late_edge
    (one quad, the right edge)"""
    df = np.asarray(df, np.float64)
    F = df.shape[0]
    assert F == xv_num_frames(T) and df.shape[1] == XV_WIN
    last = F - 2 if defect == "no_last_frame" else F - 1
    n = np.arange(T)
    last_q = (F - 1) * XV_SHIFT - XV_PAD + XV_WIN - 1
    pr = 2 * T - 1 - n
    every = np.ones(T, bool)
    g = _xv_add_pos(df, n, every, last)
    g = g + _xv_add_pos(df, -n if defect == "left_off_by_one" else -n - 1, n < XV_PAD, last)
    if defect != "no_right":
        g = g + _xv_add_pos(df, pr, pr <= last_q, last)
    if V == 1:
        return g
    assert V == 4 and T % 4 == 0
    n0 = n - n % 4
    lo = XV_PAD - 4 if defect == "interior_early" else XV_PAD
    slack = 4 if defect == "interior_late_edge" else 0
    interior = (n0 >= lo) & (2 * T - 1 - (n0 + 3) > last_q - slack) & (n0 + 3 < T)
    q = n0 + XV_PAD  # the quad's first position decides the frames of all four
    fhi = np.minimum(q // XV_SHIFT, last)
    flo = np.where(q > XV_WIN - 1, (q - (XV_WIN - 1) + XV_SHIFT - 1) // XV_SHIFT, 0)
    gi = np.zeros(T)
    for k in range(3):
        f = flo + k
        ok = interior & (f <= fhi)
        col = q - f * XV_SHIFT + n % 4
        assert (col[ok] >= 0).all() and (col[ok] < XV_WIN).all() and (col[ok] % 4 == n[ok] % 4).all(), "quad load outside a frame"
        gi[ok] += df[f[ok], col[ok]]
    assert not (interior & (flo + 3 <= fhi)).any()
    return np.where(interior, gi, g)


def xv_scatter(df, T):
    """the transpose of the framing, by the index map: the sum every gather has to equal"""
    return np.bincount(xv_frame_index(T).ravel(), weights=np.asarray(df, np.float64).ravel(), minlength=T)


FLOOR_DEFECTS = ("floor_ungated", "floor_value", "floor_none")  # each must be caught on a floor case
# floor_clamped: what exact silence cannot tell from the gate; floor_as_is: no slip, through the same natural-log expressions
FLOOR_SLIPS = FLOOR_DEFECTS + ("floor_clamped", "floor_as_is")
WRONG_FLOOR = 1e-10  # what floor_value floors at, in both front ends


class _UngatedLog(torch.autograd.Function):
    """log(max(v, floor)) whose backward divides by v itself (the adjoint without its ``v > floor ? . / v : 0`` gate) or, with
    `clamped`, by max(v, floor) (the gate replaced by a clamped denominator)"""
    @staticmethod
    def forward(ctx, v, floor, clamped):
        ctx.save_for_backward(v)
        ctx.floor = floor if clamped else None
        return torch.clamp(v, min=floor).log()

    @staticmethod
    def backward(ctx, g):
        v = ctx.saved_tensors[0]
        return g / (v if ctx.floor is None else torch.clamp(v, min=ctx.floor)), None, None


def floored_log(v, floor, defect=None):
    """log(max(v, floor)) as both oracles write it (torch.clamp: the adjoint is 0 below the floor), or with a planted slip:
    floor_ungated (the backward divides by v without the gate: 0 / 0 or c / 0 on a silent frame), floor_value (the forward
    floors at WRONG_FLOOR), floor_none (no floor at all: log 0), floor_clamped (the backward divides by max(v, floor))"""
    if defect in ("floor_ungated", "floor_clamped"):
        return _UngatedLog.apply(v, floor, defect == "floor_clamped")
    if defect == "floor_none":
        return v.log()
    return torch.clamp(v, min=WRONG_FLOOR if defect == "floor_value" else floor).log()


def xv_forward_frames(frames, defect=None, pre_log=False):
    """oracle.kaldi_mfcc.mfcc after the framing, on (F, 400) strided frames (dither added): equal to it when defect is None.
    A defect alters what the BACKWARD of this forward computes, as the named slip in mfcc_bwd_kernel would:
    no_dc_mean (the DC-removal mean dropped), no_energy (the energy path into c0 dropped), no_preemph_n0 (the n == 0 term of
    the pre-emphasis adjoint dropped), lifter_1 / lifter_29 (the lifter missing on that column); or one of FLOOR_DEFECTS at
    both logarithms (``floored_log``, FLOOR_SLIPS).  pre_log: -> (frame energies (F,), mel energies (F, 30)), what the two floors see"""
    c = {k: v.to(frames.dtype) for k, v in km.constants().items()}
    mean = frames.mean(dim=1, keepdim=True)
    frames = frames - (mean.detach() if defect == "no_dc_mean" else mean)
    floor_defect = defect if defect in FLOOR_SLIPS else None
    raw_energy = frames.pow(2).sum(1)
    energy = floored_log(raw_energy, km.EPSILON, floor_defect)
    if defect == "no_energy":
        energy = energy.detach()
    first = frames[:, :1].detach() if defect == "no_preemph_n0" else frames[:, :1]
    frames = frames - km.PREEMPH * torch.cat((first, frames[:, :-1]), dim=1)
    frames = torch.nn.functional.pad(frames * c["window"].unsqueeze(0), (0, km.PADDED_WINDOW_SIZE - km.WINDOW_SIZE))
    spec = torch.fft.rfft(frames, dim=1)
    power = spec.real.pow(2) + spec.imag.pow(2)
    mel = torch.nn.functional.pad(c["mel"], (0, 1))
    mel_energies = (power.unsqueeze(1) * mel.unsqueeze(0)).sum(dim=2)
    if pre_log:
        return raw_energy, mel_energies
    mel_energies = floored_log(mel_energies, km.EPSILON, floor_defect)
    feature = mel_energies.matmul(c["dct"])
    lifter = c["lifter"].clone()
    if defect in ("lifter_1", "lifter_29"):
        lifter[int(defect.split("_")[1])] = 1.0
    feature = feature * lifter.unsqueeze(0)
    return torch.cat((energy.unsqueeze(1), feature[:, 1:]), dim=1)


def input_scale(x, target):
    """the range rule both oracles share: the factor that takes the batch to `target` ('origin': int16 scale, 'scale': +-1)"""
    x = np.asarray(x)
    is_scale = 0.9 * x.max() <= 1 and 0.9 * x.min() >= -1
    if target == "origin":
        return 32768.0 if is_scale else 1.0
    return 1.0 if is_scale else 1.0 / 32768.0


def xv_dframes(x, cot, noise=None, defect=None, scale=None):
    """one row: x (T,), cot (F, 30) -> ((F, 400) float64 d <cot, mfcc> / d strided frame, the input scale): what
    mfcc_bwd_kernel writes before its `* scale`"""
    scale = input_scale(x, "origin") if scale is None else scale
    xs = torch.as_tensor(np.asarray(x, np.float64)) * scale
    frames = xs[torch.as_tensor(xv_frame_index(xs.shape[0]))]
    if noise is not None:
        frames = frames + torch.as_tensor(np.asarray(noise, np.float64))
    frames = frames.clone().requires_grad_(True)
    feats = xv_forward_frames(frames, defect)
    return torch.autograd.grad(feats, frames, torch.as_tensor(np.asarray(cot, np.float64)))[0].numpy(), scale


def xv_candidate(x, cot, noise=None, V=1, frame_defect=None, gather_defect=None, backward_noise=True):
    """the engine modelled in float64, one row: framing by the restated index map, the per-frame adjoint by autograd of the
    restated per-frame forward, the restated overlap-add, the input scale.  backward_noise=False: the dither ignored in the
    backward (the forward recomputed without it).  x (R, 1, T), cot (R, F, 30) -> (R, T)"""
    x = np.asarray(x).reshape(len(x), -1)
    scale = input_scale(x, "origin")
    out = []
    for r in range(x.shape[0]):
        nz = None if noise is None or not backward_noise else noise[r]
        df, _ = xv_dframes(x[r], cot[r], nz, frame_defect, scale)
        out.append(scale * xv_gather(df, x.shape[1], V, gather_defect))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- log-mel, restated
def an_frame_index(T):
    """an_load_frame / an_reflect: (F, 800) index of the pre-emphasised sample (length Lp = T - 1) frame f reads at n; torch.stft
    centre=True reflects about 0 and about Lp - 1"""
    Lp = T - 1
    p = np.arange(an_num_frames(T))[:, None] * AN_HOP - AN_WIN // 2 + np.arange(AN_WIN)[None, :]
    return np.where(p < 0, -p, np.where(p >= Lp, 2 * (Lp - 1) - p, p))


def _an_at_pos(df, p, on, last):
    """an_at_pos over an array of signal positions: the ascending sum over the frames that cover p, 0 outside [pmin, pmax]"""
    F = df.shape[0]
    pmax = (F - 1) * AN_HOP + AN_WIN // 2 - 1
    on = on & (p >= -AN_WIN // 2) & (p <= pmax)
    q = p + AN_WIN // 2
    fhi = np.minimum(q // AN_HOP, last)
    flo = np.where(q > AN_WIN - 1, (q - (AN_WIN - 1) + AN_HOP - 1) // AN_HOP, 0)
    assert not (on & (flo + 5 <= fhi)).any()  # at most five frames cover a position
    g = np.zeros(p.shape)
    for k in range(5):
        f = flo + k
        ok = on & (f <= fhi)
        col = q - f * AN_HOP
        assert (f[ok] >= 0).all() and (col[ok] >= 0).all() and (col[ok] < AN_WIN).all(), "gather outside a frame"
        g[ok] += df[f[ok], col[ok]]
    return g


def an_dpre(df, T, s, defect=None):
    """an_dpre at the positions s (all in [0, Lp)): the position itself and what the reflect padding folds onto it.
    defect: None | no_right | left_off_by_one | about_Lp (the right reflection about Lp instead of Lp - 1) | no_last_frame"""
    Lp = T - 1
    s = np.asarray(s)
    assert ((s >= 0) & (s <= Lp - 1)).all()
    last = df.shape[0] - (2 if defect == "no_last_frame" else 1)
    every = np.ones(s.shape, bool)
    g = _an_at_pos(df, s, every, last)
    g = g + _an_at_pos(df, -s - 1 if defect == "left_off_by_one" else -s, s >= 1, last)
    if defect != "no_right":
        g = g + _an_at_pos(df, (2 * Lp if defect == "about_Lp" else 2 * (Lp - 1)) - s, s <= Lp - 2, last)
    return g


def _an_pair(dpre, T):
    """(dp0, dpm1) of length T from d pre (Lp,): what an_dx takes as d pre[t] (0 past the end) and d pre[t - 1] (0 at t = 0)"""
    return np.append(dpre, 0.0), np.append(0.0, dpre)


def an_form_one(df, T, defect=None):
    """an_frames_to_wave_kernel (and an_edge_to_wave_kernel's expressions): every position by an_dpre"""
    return _an_pair(an_dpre(np.asarray(df, np.float64), T, np.arange(T - 1), defect), T)


def an_form_quad(df, T, defect=None):
    """an_frames_to_wave4_kernel: blocks of 1024 positions; an interior block sums frames k - 4 .. k of its quad's first
    position with no reflection term, any other block takes an_dpre.  defect: interior_early (a block counts as interior when
    its left neighbour is, by the right-hand conditions) or one of an_dpre's"""
    df = np.asarray(df, np.float64)
    F, Lp = df.shape[0], T - 1
    assert T % 4 == 0
    pmax = (F - 1) * AN_HOP + AN_WIN // 2 - 1
    nb = -(-T // AN_QUAD_BLOCK)
    s = np.arange(nb * AN_QUAD_BLOCK)
    t0 = s - s % AN_QUAD_BLOCK
    s_last = t0 + AN_QUAD_BLOCK - 1 - (AN_QUAD_BLOCK if defect == "interior_early" else 0)
    interior = (t0 - 1 >= AN_WIN // 2 + 1) & (s_last <= Lp - 1) & (2 * (Lp - 1) - s_last > pmax)
    s0 = s - s % 4
    q = s0 + AN_WIN // 2
    k, r = q // AN_HOP, q % AN_HOP
    gi = np.zeros(s.shape)
    for d in range(5):
        f = k - 4 + d
        ok = interior & (f <= F - 1)
        col = r + AN_HOP * (4 - d) + s % 4
        assert (f[ok] >= 0).all() and (col[ok] < AN_WIN).all(), "quad load outside a frame"
        gi[ok] += df[f[ok], col[ok]]
    edge = ~interior & (s <= Lp - 1)
    dp = np.where(interior, gi, 0.0)
    dp[edge] = an_dpre(df, T, s[edge], None if defect == "interior_early" else defect)
    dp0 = dp[:T].copy()
    dpm1 = np.append(0.0, dp0[:-1])
    first = np.flatnonzero(interior[:T] & (s[:T] == t0[:T]))  # dp[3] of an interior block: an_at_pos(t0 - 1), no reflections
    dpm1[first] = _an_at_pos(df, first - 1, np.ones(first.shape, bool), F - 1)
    return dp0, dpm1


def an_ola_ranges(T, F):
    """an_ola_ranges: (t_lo, t_hi, edge_lo, edge_hi) -- the fused kernel writes d x[t_lo .. t_hi], the edge kernel the rest from
    frames [0, edge_lo) and [edge_hi, F)"""
    Lp, pmax = T - 1, (F - 1) * AN_HOP + AN_WIN // 2 - 1
    t_lo = AN_WIN // 2 + 2
    t_hi = min(2 * (Lp - 1) - pmax, F * AN_HOP - AN_WIN // 2) - 1
    t_hi = min(t_hi, Lp - 1)
    if t_hi < t_lo:
        return T, T - 1, F, F
    q = t_hi + AN_WIN // 2
    return t_lo, t_hi, (t_lo - 1 + AN_WIN // 2) // AN_HOP + 1, ((q - (AN_WIN - 1) + AN_HOP - 1) // AN_HOP if q > AN_WIN - 1 else 0)


def an_ola_slices(B, F, fft32=True, cus=AN_CUS):
    """an_ola_slices: the runs per utterance the planner cuts, over resident waves x (frames per run + 5 halo frames)"""
    slots = cus * (12 if fft32 else 8)
    best, best_cost = 1, -1
    for sl in range(1, max(F // 8, 1) + 1):
        cost = -(-B * sl // slots) * (-(-F // sl) + (AN_HALO if sl > 1 else 0))
        if best_cost < 0 or cost < best_cost:
            best, best_cost = sl, cost
    return best


def an_form_ola(df, T, S, halo=AN_HALO):
    """an_logmel_bwd_ola_kernel + an_edge_to_wave_kernel: each of S runs [fa, fb) walks its frames from fa - halo in ascending
    order over a circular 800-position accumulator (a position's first frame stores, the next four add), finishes one hop per
    frame and carries d pre of the position before it; the edge kernel takes t < t_lo and t > t_hi from the edge frames only"""
    df = np.asarray(df, np.float64)
    F, Lp = df.shape[0], T - 1
    t_lo, t_hi, edge_lo, edge_hi = an_ola_ranges(T, F)
    dp0, dpm1 = np.full(T, np.nan), np.full(T, np.nan)
    j = np.arange(AN_WIN)
    for r in range(S if t_hi >= t_lo else 0):
        fa, fb = F * r // S, F * (r + 1) // S
        fs = max(fa - halo, 0)
        acc, carry, ph = np.zeros(AN_WIN), 0.0, AN_HOP * (fs % 5)
        for f in range(fs, fb):
            pos = (ph + j) % AN_WIN
            acc[pos] = np.where((f == fs) | (j >= AN_WIN - AN_HOP), 0.0 + df[f], acc[pos] + df[f])
            if f >= fa:
                hop = acc[ph:ph + AN_HOP].copy()
                tt = AN_HOP * f + np.arange(AN_HOP) - AN_WIN // 2
                ok = (tt >= t_lo) & (tt <= t_hi)
                assert np.isnan(dp0[tt[ok]]).all(), "a position written twice"
                dp0[tt[ok]], dpm1[tt[ok]] = hop[ok], np.append(carry, hop[:-1])[ok]
                carry = hop[-1]
            elif f == fa - 1:
                carry = acc[ph + AN_HOP - 1]
            ph = 0 if ph + AN_HOP >= AN_WIN else ph + AN_HOP
    own = np.zeros(T, bool)
    own[t_lo:t_hi + 1] = True
    assert not np.isnan(dp0[own]).any() and np.isnan(dp0[~own]).all(), "the runs do not tile [t_lo, t_hi]"
    dfe = df.copy()
    dfe[edge_lo:edge_hi] = np.nan  # the frames the fused kernel keeps out of HBM: the edge kernel must not read them
    t = np.flatnonzero(~own)
    dp0[t] = np.where(t <= Lp - 1, an_dpre(dfe, T, np.minimum(t, Lp - 1)), 0.0)
    dpm1[t] = np.where(t >= 1, an_dpre(dfe, T, np.maximum(t - 1, 0)), 0.0)
    assert np.isfinite(dp0).all() and np.isfinite(dpm1).all(), "the edge kernel reads a frame that was not written"
    return dp0, dpm1


def an_scatter(df, T):
    """the transpose of the framing, by the index map -> d pre (Lp,)"""
    return np.bincount(an_frame_index(T).ravel(), weights=np.asarray(df, np.float64).ravel(), minlength=T - 1)


def an_dx(dp0, dpm1, scale=1.0, defect=None):
    """an_dx: d x[t] = ([t >= 1] d pre[t - 1] - 0.97 [t <= Lp - 1] d pre[t]) scale.  defect: t0 (the t == 0 term taken as if
    t >= 1 failed for it too: no -0.97 d pre[0]) | tlast (the t == T - 1 term dropped)"""
    T = dp0.shape[0]
    t = np.arange(T)
    a = np.where(t >= 1, dpm1, 0.0)
    b = np.where(t <= T - 2, dp0, 0.0)
    if defect == "t0":
        b[0] = 0.0
    if defect == "tlast":
        a[T - 1] = 0.0
    return (a - 0.97 * b) * scale


def an_forward_frames(frames, defect=None, pre_log=False):
    """oracle.audionet.preprocess after pre-emphasis and framing: (F, 800) -> (F, 32) log-mel (the 800-tap window centred in
    the 1024-point transform, as torch.stft places it).  defect: one of FLOOR_DEFECTS; pre_log: -> the mel energies (F, 32)"""
    w = torch.hann_window(AN_WIN, dtype=frames.dtype)
    pad = (AN_FFT - AN_WIN) // 2
    spec = torch.fft.rfft(torch.nn.functional.pad(frames * w, (pad, pad)), dim=1)
    mag = spec.real.pow(2) + spec.imag.pow(2)
    mel = torch.as_tensor(oan.mel_basis()).to(frames.dtype)
    energies = mag.matmul(mel.t())
    if pre_log:
        return energies
    if defect is None:
        return 10 * torch.clamp(energies, oan.EPSILON).log10()
    return (10 / np.log(10.0)) * floored_log(energies, oan.EPSILON, defect)


def an_frames(x, scale, dtype=torch.float64):
    """one row: x (T,) -> (F, 800) frames of the pre-emphasised signal by the restated index map"""
    xs = torch.as_tensor(np.asarray(x, np.float32)).to(dtype) * scale
    pre = xs[1:] - oan.PREEMPH * xs[:-1]
    return pre[torch.as_tensor(an_frame_index(xs.shape[0]))]


def an_dframes(x, cot, scale=None, defect=None):
    """one row: x (T,), cot (F, 32) -> ((F, 800) float64 d <cot, log-mel> / d frame of the pre-emphasised signal, the scale)"""
    scale = input_scale(x, "scale") if scale is None else scale
    xs = torch.as_tensor(np.asarray(x, np.float64)) * scale
    pre = xs[1:] - oan.PREEMPH * xs[:-1]
    frames = pre[torch.as_tensor(an_frame_index(xs.shape[0]))].clone().requires_grad_(True)
    return torch.autograd.grad(an_forward_frames(frames, defect), frames, torch.as_tensor(np.asarray(cot, np.float64)))[0].numpy(), scale


def an_candidate(x, cot, form="one", S=1, halo=AN_HALO, gather_defect=None, dx_defect=None, frame_defect=None):
    """the engine modelled in float64: x (R, 1, T), cot (R, F, 32) -> (R, T); form one | quad | ola; frame_defect: one of
    FLOOR_DEFECTS in the per-frame forward"""
    x = np.asarray(x).reshape(len(x), -1)
    scale, T = input_scale(x, "scale"), x.shape[1]
    out = []
    for r in range(x.shape[0]):
        df, _ = an_dframes(x[r], cot[r], scale, frame_defect)
        dp0, dpm1 = (an_form_one(df, T, gather_defect) if form == "one" else
                     an_form_quad(df, T, gather_defect) if form == "quad" else an_form_ola(df, T, S, halo))
        out.append(an_dx(dp0, dpm1, scale, dx_defect))
    return np.stack(out)
