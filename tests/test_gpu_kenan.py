"""The spectrum gate on the device (csrc/k_spectrum.hip) and the Kenan FFT attack on it (speakerguard_amd/attack/Kenan.py).

Spectrum, mask and output are judged against float64 (tests/kenan_restate.py truth_*), with the REFERENCE's own float32
transform (CPU ``torch.fft``) on the same input as the yardstick: E_ref is the largest deviation of ``torch.fft.rfft`` (float32)
from float64 over the case's input (all its utterances: at a handful of bins a single row's deviation can be zero by luck), and the native spectrum may deviate at most 4 x E_ref on smooth lengths and 8 x on
Bluestein lengths (both sides are O(eps log N) networks that differ in radix order; Bluestein runs three such networks).  A
bin is undecided when its float64 magnitude is within that margin of the factor; on every other bin the mask is exact.  The
gate's output is judged the same way against the reference's float32 gate under the native mask.  Measured ratios are logged.
The eight factors of a case are the first eight of a bisection from peak / 2 (kenan_restate.bisection_factors): six successes halve
the factor down into the bulk of the noise bins, a failure at peak / 128 and a success after it bisect upwards.  With them the
inputs leave at most 0.05 % of an utterance's bins undecided, which the test asserts (at T = 52960 a straight halving to peak / 256
lands on the mode of the noise bins' magnitudes and leaves 23 of 26481 undecided at that length's margin, 14 are allowed).

Shapes: every radix (2, 4, 3, 5), the smallest Bluestein lengths (T = 14: M = 7; T = 662: M = 331), both sides of the switch
from LDS to the workspace (16000 / 48000 smooth, 662 / 52960 Bluestein) and both workload lengths."""
import math

import numpy as np
import pytest
import torch

import kenan_restate as kr
from conftest import log

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = ((1, 2), (1, 4), (2, 6), (3, 10), (2, 14), (3, 480), (2, 662), (2, 16000), (2, 48000), (2, 52960))
CASES = [(B, T, "noise") for B, T in SHAPES] + [(2, 16000, "tone")]
IDS = ["%dx%d-%s" % c for c in CASES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(B, T, kind):
    from speakerguard_amd import synth
    x = synth.make_tone_waveforms(B, T) if kind == "tone" else synth.make_waveforms(B, T, seed=11)
    return np.ascontiguousarray(x[:, 0], np.float32)


def _margin_factor(T):
    return 8.0 if kr.plan(T)["bluestein"] else 4.0


_REF = {}


def _reference(B, T, kind):
    """computed once per case, shared by its tests, never changed: input, float64 spectrum, the reference's float32 spectrum,
    E_ref, the native spectrum and peak"""
    key = (B, T, kind)
    if key not in _REF:
        from speakerguard_amd.attack.Kenan import wav_spectrum
        x = _inputs(B, T, kind)
        X64 = kr.truth_spectrum(x)
        Xref = torch.fft.rfft(torch.from_numpy(x), dim=1).numpy()
        e_ref = np.abs(Xref.astype(np.complex128) - X64).max(keepdims=True)
        spec, peak = wav_spectrum(torch.from_numpy(x).to(DEV).unsqueeze(1))
        torch.cuda.synchronize()
        _REF[key] = dict(x=x, X64=X64, Xref=Xref, e_ref=e_ref, spec=spec[:, 0].cpu().numpy(), peak=peak.cpu().numpy())
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("B,T,kind", CASES, ids=IDS)
def test_spectrum_and_peak(B, T, kind):
    r = _reference(B, T, kind)
    dev = np.abs(r["spec"].astype(np.complex128) - r["X64"]).max()
    mf, e_ref = _margin_factor(T), float(r["e_ref"].max())
    log("kenan spectrum %s B=%d T=%d: E_ref %.3e native %.3e ratio %.2f (margin %g)" %
        (kind, B, T, e_ref, dev, dev / max(e_ref, 1e-300), mf))
    assert dev <= mf * e_ref, (dev, e_ref)
    # the peak: the maximum of the native spectrum's own float32 magnitudes, bit for bit
    # (the square root through float64: correctly rounded, which a vectorised float32 sqrt of the host need not be)
    re, im = r["spec"].real.astype(np.float32), r["spec"].imag.astype(np.float32)
    mag = np.sqrt((re * re + im * im).astype(np.float64)).astype(np.float32)
    assert np.array_equal(bits(mag.max(axis=1)), bits(r["peak"]))
    # DC and Nyquist are real
    assert (r["spec"].imag[:, 0] == 0).all() and (r["spec"].imag[:, -1] == 0).all()


@pytest.mark.parametrize("B,T,kind", CASES, ids=IDS)
def test_gate_mask_and_output(B, T, kind):
    from speakerguard_amd.attack.Kenan import wav_spectrum_gate
    r = _reference(B, T, kind)
    x, X64, mf = r["x"], r["X64"], _margin_factor(T)
    mag64 = np.abs(X64)
    nb = T // 2 + 1
    allowed = math.ceil(0.0005 * nb)
    factors = np.stack([kr.bisection_factors(p) for p in r["peak"]], 1)  # (8, B): six successes, a failure, a success
    xd = torch.from_numpy(x.copy()).to(DEV).unsqueeze(1)
    worst_und, worst_ratio = 0, 0.0
    for j in range(8):
        f = factors[j]
        out, keep, kept = wav_spectrum_gate(xd, torch.from_numpy(f), want_keep=True)
        torch.cuda.synchronize()
        out, keep, kept = out[:, 0].cpu().numpy(), keep.cpu().numpy().astype(bool), kept.cpu().numpy()
        assert np.array_equal(kept, keep.sum(1))
        margin = mf * float(r["e_ref"].max())
        undecided = np.abs(mag64 - f[:, None].astype(np.float64)) <= margin
        worst_und = max(worst_und, int(undecided.sum(1).max()))
        assert (undecided.sum(1) <= allowed).all(), "the inputs must leave at most %d undecided bins" % allowed
        want = ~(mag64 < f[:, None].astype(np.float64))
        assert np.array_equal(keep[~undecided], want[~undecided])
        # the output under the native mask: float64 truth, the reference's float32 gate as the yardstick
        truth = kr.truth_gate(x, keep)
        spec = torch.from_numpy(r["Xref"].copy())
        spec[torch.from_numpy(~keep)] = 0
        ref = torch.fft.irfft(spec, n=T, dim=1).numpy()
        d_ref = np.abs(ref.astype(np.float64) - truth).max()
        d_nat = np.abs(out.astype(np.float64) - truth).max()
        worst_ratio = max(worst_ratio, d_nat / max(d_ref, 1e-300) if d_nat > 0 else 0.0)
        assert d_nat <= mf * d_ref, (j, d_nat, d_ref)
    log("kenan gate %s B=%d T=%d: undecided bins at most %d of %d (allowed %d), output deviation at most %.2f x the reference's "
        "(margin %g)" % (kind, B, T, worst_und, nb, allowed, worst_ratio, mf))


@pytest.mark.parametrize("B,T", [(2, 6), (3, 10), (2, 14), (3, 480), (2, 662), (2, 16000)])
def test_kernel_equals_its_float32_restatement(B, T):
    """tests/kenan_restate.py network_gate in float32 IS the kernel's arithmetic: spectrum, peak, mask, count and gated output
    equal it value for value (compared as numbers: a zero of either sign is a zero), at three of the eight factors"""
    from speakerguard_amd.attack.Kenan import wav_spectrum_gate
    r = _reference(B, T, "noise")
    xd = torch.from_numpy(r["x"].copy()).to(DEV).unsqueeze(1)
    factors = np.stack([kr.bisection_factors(p) for p in r["peak"]], 1)
    for b in range(B):
        X, mag, _, _ = kr.network_gate(r["x"][b], None, np.float32)
        assert X.dtype == np.complex64 and np.array_equal(X, r["spec"][b]) and mag.max() == r["peak"][b]
    for j in (1, 5, 7):
        out, keep, kept = wav_spectrum_gate(xd, torch.from_numpy(factors[j]), want_keep=True)
        out, keep, kept = out[:, 0].cpu().numpy(), keep.cpu().numpy().astype(bool), kept.cpu().numpy()
        for b in range(B):
            _, _, k, o = kr.network_gate(r["x"][b], factors[j][b], np.float32)
            assert np.array_equal(k, keep[b]) and int(k.sum()) == int(kept[b])
            assert o.dtype == np.float32 and np.array_equal(o, out[b]), (T, j, b, float(np.abs(o - out[b]).max()))


@pytest.mark.parametrize("T", [16000, 48000, 662, 52960], ids=["lds", "workspace", "bluestein-lds", "bluestein-workspace"])
def test_row_of_a_batch_equals_the_row_alone(T):
    from speakerguard_amd.attack.Kenan import wav_spectrum, wav_spectrum_gate
    r = _reference(2, T, "noise")
    xd = torch.from_numpy(r["x"].copy()).to(DEV).unsqueeze(1)
    f = torch.from_numpy(r["peak"] / np.float32(8))
    out, keep, kept = wav_spectrum_gate(xd, f, want_keep=True)
    for b in range(2):
        s1, p1 = wav_spectrum(xd[b:b + 1])
        o1, k1, c1 = wav_spectrum_gate(xd[b:b + 1], f[b:b + 1], want_keep=True)
        assert np.array_equal(bits(torch.view_as_real(s1)[0, 0].cpu().numpy()), bits(np.stack([r["spec"][b].real, r["spec"][b].imag], -1)))
        assert np.array_equal(bits(p1.cpu().numpy()), bits(r["peak"][b:b + 1]))
        assert torch.equal(o1[0], out[b]) and torch.equal(k1[0], keep[b]) and int(c1[0]) == int(kept[b])
    assert 0 < int(kept[0]) < T // 2 + 1


@pytest.mark.parametrize("T", [480, 662], ids=["smooth", "bluestein"])
def test_tables_pushed_out_of_the_cache_come_back_the_same(T):
    """the context keeps the tables of 16 lengths: 16 other lengths push T's out, freed behind the stream; rebuilt, they give
    the first call's bits"""
    from speakerguard_amd.attack.Kenan import wav_spectrum
    xd = torch.from_numpy(_inputs(2, T, "noise")).to(DEV).unsqueeze(1)
    spec, peak = wav_spectrum(xd)
    first = torch.view_as_real(spec).cpu().numpy(), peak.cpu().numpy()
    assert first[1].min() > 0
    for other in range(100, 161, 4):
        wav_spectrum(xd[:, :, :other].contiguous())
    spec, peak = wav_spectrum(xd)
    assert np.array_equal(bits(torch.view_as_real(spec).cpu().numpy()), bits(first[0]))
    assert np.array_equal(bits(peak.cpu().numpy()), bits(first[1]))


def test_factor_edge_cases():
    """a NaN, a negative and a zero factor keep everything; a factor above the peak keeps nothing; the comparison is strict"""
    from speakerguard_amd.attack.Kenan import wav_spectrum_gate
    r = _reference(3, 480, "noise")
    xd = torch.from_numpy(r["x"].copy()).to(DEV).unsqueeze(1)
    # (the truth of a gate that keeps everything is x itself; the yardstick is the reference's own round trip, margin as above)
    d_ref = np.abs(torch.fft.irfft(torch.from_numpy(r["Xref"].copy()), n=480, dim=1).numpy().astype(np.float64) - r["x"]).max()
    for f in (float("nan"), -1.0, 0.0):
        out, keep, kept = wav_spectrum_gate(xd, torch.full((3,), f), want_keep=True)
        assert bool(keep.all()) and kept.tolist() == [241] * 3
        assert np.abs(out[:, 0].cpu().numpy().astype(np.float64) - r["x"]).max() <= 4 * d_ref
    out, keep, kept = wav_spectrum_gate(xd, torch.from_numpy(r["peak"] * np.float32(1.5)), want_keep=True)
    assert not bool(keep.any()) and kept.tolist() == [0] * 3 and not bool(out.any())
    out, keep, kept = wav_spectrum_gate(xd, torch.from_numpy(r["peak"].copy()), want_keep=True)  # the peak bin equals the factor: it stays
    assert (kept.cpu().numpy() >= 1).all()


def test_refusals_leave_the_outputs_untouched():
    from speakerguard_amd import _native as N
    from speakerguard_amd.metric.metric import _context
    ctx, s = _context(DEV), N.current_stream_ptr(DEV)
    x = torch.zeros((2, 480), device=DEV)
    f = torch.ones((2,), device=DEV)
    out = torch.full((2, 482), 7.0, device=DEV)
    spec = torch.full((2, 242, 2), 7.0, device=DEV)
    peak = torch.full((2,), 7.0, device=DEV)
    keep = torch.full((2, 242), 7, dtype=torch.uint8, device=DEV)
    kept = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    P = N._ptr
    lib, h = ctx.lib, ctx.handle
    rcs = [lib.sg_wav_spectrum(None, P(x), 2, 480, P(spec), P(peak), s),
           lib.sg_wav_spectrum(h, None, 2, 480, P(spec), P(peak), s),
           lib.sg_wav_spectrum(h, P(x), 2, 480, None, None, s),
           lib.sg_wav_spectrum_gate(None, P(x), 2, 480, P(f), P(out), P(keep), P(kept), s),
           lib.sg_wav_spectrum_gate(h, None, 2, 480, P(f), P(out), P(keep), P(kept), s),
           lib.sg_wav_spectrum_gate(h, P(x), 2, 480, None, P(out), P(keep), P(kept), s),
           lib.sg_wav_spectrum_gate(h, P(x), 2, 480, P(f), None, P(keep), P(kept), s),
           lib.sg_wav_spectrum_gate(h, P(x), 2, 480, P(f), P(x), P(keep), P(kept), s)]
    for B, T in ((0, 480), (-1, 480), (2, 481), (2, 1), (2, 0), (2, -2), (1, (1 << 22) + 2)):
        rcs.append(lib.sg_wav_spectrum(h, P(x), B, T, P(spec), P(peak), s))
        rcs.append(lib.sg_wav_spectrum_gate(h, P(x), B, T, P(f), P(out), P(keep), P(kept), s))
    torch.cuda.synchronize()
    assert rcs == [1] * len(rcs)  # SG_ERR_ARG
    assert bool((out == 7).all()) and bool((spec == 7).all()) and bool((peak == 7).all()) and bool((keep == 7).all()) and \
        bool((kept == 7).all())
    with pytest.raises(N.NativeError):
        from speakerguard_amd.attack.Kenan import wav_spectrum_gate
        wav_spectrum_gate(torch.zeros((1, 1, 481), device=DEV), torch.ones(1))


# ---------------------------------------------------------------- the attack, end to end
# xv_plda at T = 5120 (M = 2560, smooth), AudioNet at T = 3682 (M = 7 * 263: Bluestein)
E2E = (("xv_plda", 0, 5120), ("audionet", 1, 3682))


def cpu_gate(audio, factor):
    """the reference's float32 gate (_kenan_fft.py:57-82) on the CPU, for a device tensor"""
    a = audio.detach().cpu()
    spec = torch.fft.rfft(a, dim=2)
    spec[spec.abs() < factor.detach().cpu().unsqueeze(1).unsqueeze(2)] = 0
    return torch.fft.irfft(spec, dim=2).to(audio.device)


def reference_loop(model, x, y, targeted, max_iter):
    """_kenan_fft.py:180-245 restated on the test's side, utterance by utterance as the reference writes it: the float32 CPU gate,
    the native model, and -- as the issue sets it -- the starting factor from the peak of sg_wav_spectrum.  Shares no line with
    speakerguard_amd/attack/Kenan.py.  -> (succ, factors (iters, n), decisions (iters, n))"""
    from speakerguard_amd.attack.Kenan import wav_spectrum
    n = x.shape[0]
    labels = y.cpu().tolist()
    lo = torch.tensor([0.] * n)
    hi = wav_spectrum(x, want_spec=False)[1].cpu().view(-1)
    f = hi / 2
    succ, factors, decisions = [False] * n, [], []
    for _ in range(max_iter):
        dec = model.make_decision(cpu_gate(x.clone(), f))[0].cpu().tolist()
        factors.append(f.clone())
        decisions.append(torch.tensor(dec))
        for p in range(n):
            if (labels[p] != dec[p] and not targeted) or (labels[p] == dec[p] and targeted):
                hi[p] = f[p]
                f[p] = ((lo[p] + hi[p]) / 2).abs()
                succ[p] = True
            else:
                lo[p] = f[p]
                f[p] = ((lo[p] + hi[p]) / 2).abs()
    return succ, torch.stack(factors), torch.stack(decisions)


def _e2e_inputs(T):
    """four utterances of clipped white noise, 0.05 .. 0.3 N(0,1) (SURVEY.md section 8(d)'s input).  White on purpose: the gate
    at peak / 2 leaves a harmonic utterance of ``synth.make_waveforms`` ONE bin, a pure tone whose other mel bands hold rounding
    noise only, and both models' decisions on such audio flip under a 1e-7 change of the samples (measured: score gap 0.78, the
    native and the CPU gate 1.5e-7 apart, decisions 8 and 3) -- no loop comparison across two float32 transforms survives that.
    A flat spectrum keeps a tenth of its bins at peak / 2."""
    rs = np.random.RandomState(0)
    return np.clip(np.array([a * rs.randn(1, T) for a in (0.05, 0.1, 0.2, 0.3)]), -0.95, 0.95).astype(np.float32)


_RUNS = {}


def _runs(which):
    """every run of one model, made once: (model, x, {mode: (y, plain bs 1, bs 4, the test-side CPU-gate loop, sharded)})"""
    if which not in _RUNS:
        from speakerguard_amd.attack.Kenan import Kenan
        from speakerguard_amd.shard import ShardedAttack
        from test_gpu_time_domain import _models
        name, make, _ = _models()[which]
        T = E2E[which][2]
        model = make()
        x = torch.from_numpy(_e2e_inputs(T)).to(DEV)
        own = model.make_decision(x)[0]
        n_spk = model.make_decision(x)[1].shape[1]
        res = {}
        for targeted in (False, True):
            y = (own + 1) % n_spk if targeted else own.clone()

            def run(atk, sharded=False):
                adv, succ = (ShardedAttack(atk) if sharded else atk).attack(x, y)
                return dict(adv=adv, succ=list(succ), last=atk.last_factors.clone(), factors=atk.factor_history.clone(),
                            decisions=atk.decision_history.clone())
            kw = dict(max_iter=8, targeted=targeted, verbose=0)
            res[targeted] = dict(y=y, b1=run(Kenan(model, batch_size=1, **kw)), b4=run(Kenan(model, batch_size=4, **kw)),
                                 cpu=reference_loop(model, x, y, targeted, 8),
                                 shard=run(Kenan(model, batch_size=4, **kw), sharded=True))
        _RUNS[which] = (model, x, res)
    return _RUNS[which]


@pytest.mark.parametrize("name,which,T", E2E, ids=[e[0] for e in E2E])
def test_attack_end_to_end(name, which, T):
    from speakerguard_amd.attack.Kenan import wav_spectrum_gate
    model, x, res = _runs(which)
    outcomes = set()
    for targeted, r in res.items():
        b1, b4 = r["b1"], r["b4"]
        y = r["y"].cpu().tolist()
        log("kenan attack %s targeted=%d: success %s last factors %s" % (name, targeted, b4["succ"], b4["last"].tolist()))
        outcomes.update(b4["succ"])
        dec = model.make_decision(b4["adv"])[0].cpu().tolist()
        regate = wav_spectrum_gate(x, torch.nan_to_num(b4["last"], nan=0.0))
        for i, s in enumerate(b4["succ"]):
            if s:  # re-decided as a success, and the native gate of x at the recorded factor
                assert (dec[i] == y[i]) == targeted
                assert torch.equal(b4["adv"][i], regate[i])
            else:
                assert torch.equal(b4["adv"][i], x[i]) and math.isnan(float(b4["last"][i]))
        # batch size 4 = batch size 1 = a world-1 ShardedAttack run, bit for bit
        for other in (b1, r["shard"]):
            assert other["succ"] == b4["succ"] and torch.equal(other["adv"], b4["adv"])
            assert np.array_equal(bits(other["factors"].numpy()), bits(b4["factors"].numpy()))
            assert torch.equal(other["decisions"], b4["decisions"])
            assert np.array_equal(bits(other["last"].numpy()), bits(b4["last"].numpy()))
        # the test's own restatement of the loop on the reference's float32 CPU gate, through the same native model
        ref_succ, ref_factors, ref_decisions = r["cpu"]
        assert ref_succ == b4["succ"]
        assert np.array_equal(bits(ref_factors.numpy()), bits(b4["factors"].numpy()))
        assert torch.equal(ref_decisions, b4["decisions"])
    assert outcomes == {True, False}, "both outcomes must occur over the two modes"


def test_attack_through_query_sharded_model():
    from speakerguard_amd.attack.Kenan import Kenan
    from speakerguard_amd.shard import QueryShardedModel
    model, x, res = _runs(0)
    r = res[False]
    atk = Kenan(QueryShardedModel(model), max_iter=8, verbose=0, batch_size=4)
    adv, succ = atk.attack(x, r["y"])
    assert list(succ) == r["b4"]["succ"] and torch.equal(adv, r["b4"]["adv"])
