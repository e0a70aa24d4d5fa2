"""GMM / i-vector / PLDA system, everything that needs no GPU: the restatement (tests/iv_restate.py) against the reference's
recorded outputs at every stage, the Kaldi-text parsers, the packing the kernels read, the C struct's layout, the raises."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import iv_restate as R
from conftest import ROOT, load_golden
from speakerguard_amd import _native, synth
from speakerguard_amd.model import iv_plda as M

MODELS = {"a": dict(seed=0, C=16, R=24, D=10, n_spk=4), "b": dict(seed=1, C=80, R=100, D=24, n_spk=5),
          "c": dict(seed=2, C=272, R=262, D=24, n_spk=5)}
CASES = ((2, 5), (13, 5), (100, 3), (331, 1))
# model C = 256 + 16 components, 256 + 6 i-vector entries: the smallest sizes at which every 256-wide loop of the kernels takes
# a second, partial pass (tests/golden/make_golden_ivector.py); each model carries its own cases
CASES_OF = {"a": CASES, "b": CASES, "c": ((13, 3), (100, 2))}
FILES = {"a": "iv_ref.npz", "b": "iv_ref_b.npz", "c": "iv_ref_c.npz"}
GRAD_FILES = {"a": "iv_grad_ref.npz", "b": "iv_grad_ref_b.npz", "c": "iv_grad_ref_c.npz"}
MODEL_CASES = [(F, B, tag) for tag in "abc" for F, B in CASES_OF[tag]]
MODEL_CASE_IDS = ["%d-%d-%s" % mc for mc in MODEL_CASES]  # (the ids of the two stacked parametrisations A and B had)
KEYS = ("gconsts", "means_invcovars", "invcovars", "extractor", "sigma_inv", "ivector_offset", "emb_mean", "lda", "plda_mean",
        "plda_transform", "plda_psi", "enroll")
# float32 unit roundoff times 64: sqrt(2700) ~ 52 rounding steps of the longest sum, random-walk growth, relative to the largest
# entry of the quantity (the measured distances of the reference's float32 outputs from float64 are 2e-8 .. 1.5e-6)
REF_REL = 64 * 2.0 ** -24


def checksum(w):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(w[k]).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for tag, name in FILES.items():
        g = load_golden(name)
        w = synth.make_iv_weights(**MODELS[tag])
        assert checksum(w) == g["meta"][tag]["weights_sha256"], "synth.make_iv_weights moved: regenerate tests/golden/iv_ref*.npz"
        out[tag] = (w, g, R.IvRestated(w))
    return out


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("F,B", CASES)
def test_front_end_restated(fixtures, F, B):
    g = fixtures["a"][1]
    delta = R.add_delta(g["raw_%d" % F])
    assert g["raw_%d" % F].shape == (B, F, 24)
    assert rel(g["delta_%d" % F], delta) <= REF_REL
    assert rel(g["cmvn_%d" % F], R.cmvn(delta)) <= REF_REL


@pytest.mark.parametrize("F,B,tag", MODEL_CASES, ids=MODEL_CASE_IDS)
def test_chain_restated(fixtures, tag, F, B):
    w, g, truth = fixtures[tag]
    t = truth.chain(g["x_%d" % F])
    for k in ("zeroth", "first", "ivector", "emb", "scores"):
        assert rel(g["%s_%d" % (k, F)], t[k]) <= REF_REL, k
    assert np.array_equal(t["decisions"], g["decisions_%d" % F])
    raw = fixtures["a"][1]["raw_%d" % F][:B]  # (model C: the first rows of the shared raw inputs)
    t1 = truth.chain(R.cmvn(R.add_delta(raw)))
    assert rel(g["raw_scores_%d" % F], t1["scores"]) <= REF_REL
    assert np.array_equal(t1["decisions"], g["raw_decisions_%d" % F])


def test_generator_recorded_its_asserts(fixtures):
    for tag in ("a", "b", "c"):
        info = fixtures[tag][1]["meta"][tag]
        assert [tuple(c) for c in fixtures[tag][1]["meta"]["cases"]] == list(CASES_OF[tag])
        assert min(min(v) for k, v in info["cond_L"].items() if int(k) >= 100) >= 100.0
        assert all(5.0 / MODELS[tag]["C"] < v < 0.85 for v in info["top_posterior"].values())
        assert info["min_gap_over_err"] > 100.0


def test_parsers_round_trip(tmp_path):
    w = synth.make_iv_weights(seed=3, C=5, R=7, D=4, n_spk=2)
    paths = synth.write_iv_model_dir(str(tmp_path), w)
    ubm, ie = M.parse_fgmm_file(paths["fgmm_file"]), M.parse_ie_file(paths["extractor_file"])
    for k in ("gconsts", "gmm_weights", "means_invcovars", "invcovars"):
        assert np.array_equal(ubm[k], w[k]), k
    for k in ("extractor", "sigma_inv"):
        assert np.array_equal(ie[k], w[k]), k
    assert ie["ivector_offset"] == w["ivector_offset"]
    assert ubm["invcovars"].dtype == np.float32 and np.array_equal(ubm["invcovars"], ubm["invcovars"].transpose(0, 2, 1))


def test_parsers_refuse_a_short_triangle(tmp_path):
    w = synth.make_iv_weights(seed=3, C=2, R=3, D=2, n_spk=1)
    paths = synth.write_iv_model_dir(str(tmp_path), w)
    lines = open(paths["fgmm_file"]).read().split("\n")
    at = [i for i, l in enumerate(lines) if "<INV_COVARS>" in l][0]
    del lines[at + 3]  # a component loses a row: every later row has the wrong length
    open(paths["fgmm_file"], "w").write("\n".join(lines))
    with pytest.raises(ValueError):
        M.parse_fgmm_file(paths["fgmm_file"])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_packing_equals_the_direct_form(fixtures, tag):
    w, g, truth = fixtures[tag]
    x = g["x_13"].reshape(-1, 72)
    W = R.pack_w(w["means_invcovars"], w["invcovars"])
    assert W.shape == (MODELS[tag]["C"], 2700) and R.zpos(71, 71) == 2699 and R.zpos(0, 0) == 72
    ll = R.make_z(x) @ W.T + w["gconsts"].astype(np.float64)
    assert rel(ll, truth.loglik(x)) < 1e-12
    V, U = R.pack_vu(w["extractor"], w["sigma_inv"])
    n, f, _ = truth.stats(g["x_13"][1])
    L, lin = truth.system(n, f)
    assert rel(np.eye(L.shape[0]) + np.einsum("c,crs->rs", n, U), L) < 1e-12
    assert rel(np.einsum("crd,cd->r", V, f), lin) < 1e-12
    assert np.abs(U - U.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(U).max()  # only the upper triangle is kept


def test_delta_scales():
    s1, s2 = R.delta_scales()
    assert np.allclose(s1, np.arange(-3, 4) / 28.0, rtol=1e-6)
    assert np.allclose(s2, np.convolve(np.arange(-3, 4) / 28.0, np.arange(-3, 4) / 28.0), rtol=1e-5, atol=1e-9)


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "speakerguard_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(sg_iv_weights), offsetof(sg_iv_weights, gconsts),\n'
                   '           offsetof(sg_iv_weights, emb_mean), offsetof(sg_iv_weights, threshold));\n    return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, o1, o2, o3 = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    T = _native.IvWeights
    assert (ctypes.sizeof(T), T.gconsts.offset, T.emb_mean.offset, T.threshold.offset) == (size, o1, o2, o3)


def test_gradient_paths_raise():
    """forward only: everything that needs d loss / d x says that the gradient is not built"""
    m = object.__new__(M.iv_plda)
    for call in (lambda: m.loss_grad(None, None, None, want_grad=True), lambda: m.loss_grad(None, None, None),
                 lambda: m.pgd_run(None), lambda: m.pgd_run_defended(None), lambda: m.pgd_run_feco(None)):
        with pytest.raises(NotImplementedError, match="gradient is not built"):
            call()
    assert M.iv_plda.allowed_flags == [0, 1, 2, 3]


def test_model_refuses_cpu_device():
    w = synth.make_iv_weights(**MODELS["a"])
    with pytest.raises(_native.NativeError):
        M.iv_plda.from_weights(w, device="cpu")


def test_existing_synth_checksums_unmoved():
    """make_iv_weights draws from its own RandomState: the x-vector generator's numbers stay where they were"""
    from conftest import weights_checksum
    a = weights_checksum(synth.make_xv_weights(seed=0, D=200, n_spk=10))
    synth.make_iv_weights(seed=0, C=4, R=5, D=3, n_spk=2)
    assert weights_checksum(synth.make_xv_weights(seed=0, D=200, n_spk=10)) == a
