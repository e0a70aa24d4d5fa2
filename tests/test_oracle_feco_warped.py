"""The warped k-means restatement (tests/feco_warped_restate.py: the kernel's determinism contract) against the REFERENCE's own
warped_kmeans (tests/golden/feco_warped_ref.npz, made by tests/golden/make_golden_feco_warped.py), and the C-ABI's export.
CPU only."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import feco_warped_restate as R
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "feco_warped_ref.npz"))
    return z, json.loads(str(z["meta"]))


def _cases(ref):
    z, meta = ref
    assert len(meta["cases"]) >= 8 and all(m >= meta["margin_floor"] for m in meta["min_rel_margin"].values())
    return z, meta["cases"]


def test_restatement_reproduces_the_reference(ref):
    z, cases = _cases(ref)
    seen = set()
    for tag in cases:
        x, k, init, delta = z[tag + "_feat"], int(z[tag + "_k"]), str(z[tag + "_init"]), float(z[tag + "_delta"])
        seen.add((x.shape[0], x.shape[1], init, delta != 0))
        # random init: the reference's draw comes from numpy's global generator; the fixture recorded it and it is replayed
        r = R.warped(x, k, init, delta, boundaries=None if init == "ts" else z[tag + "_init_bnd"])
        np.testing.assert_array_equal(r["init_bnd"], z[tag + "_init_bnd"], err_msg=tag)
        np.testing.assert_array_equal(r["bnd"], z[tag + "_bnd"], err_msg=tag)
        np.testing.assert_allclose(r["means"], z[tag + "_out"], rtol=0, atol=1e-5 * np.abs(x).max(), err_msg=tag)
        feat = torch.from_numpy(x.copy()).requires_grad_(True)
        y = R.torch_with_quirk(feat, r)
        assert torch.equal(y.detach(), torch.from_numpy(r["means"]))
        (y * torch.from_numpy(z[tag + "_cot"])).sum().backward()
        np.testing.assert_allclose(feat.grad.numpy(), z[tag + "_dfeat"], rtol=0, atol=1e-6, err_msg=tag)
        # the quirk is real: the forward means moved away from the initial ones the gradient belongs to
        if tag == "mfcc300_ts":
            assert np.abs(r["means"] - R.init_segments(x, r["init_bnd"])[0]).max() > 1e-3
    assert {F for F, _, _, _ in seen} >= {60, 300, 1200} and {D for _, D, _, _ in seen} >= {30, 32}
    assert any(s[3] for s in seen) and {s[2] for s in seen} == {"ts", "random"}


def test_degenerate_ts_init_is_detected(ref):
    z, _ = ref
    x, k = z["degenerate_feat"], int(z["degenerate_k"])
    b = R.ts_boundaries(x, k)
    np.testing.assert_array_equal(b, z["degenerate_ts_bnd"])
    assert list(b[:4]) == [0, 39, 22, 23] and not R.valid(b, x.shape[0])
    with pytest.raises(R.Degenerate):
        R.warped(x, k, "ts")


def test_random_boundaries_are_a_keyed_sorted_draw():
    b = R.random_boundaries(1234, 5, 300, 150)
    assert b[0] == 0 and len(b) == 150 and np.all(np.diff(b) > 0) and b[-1] <= 299 and b[1] >= 1
    assert np.array_equal(b, R.random_boundaries(1234, 5, 300, 150))
    assert not np.array_equal(b, R.random_boundaries(1234, 6, 300, 150))
    assert not np.array_equal(b, R.random_boundaries(1235, 5, 300, 150))
    assert np.array_equal(R.random_boundaries(7, 0, 40, 40), np.arange(40))  # k = F: every frame


def test_butterfly_is_the_pairwise_tree():
    v = np.random.RandomState(0).randn(5, 64).astype(np.float32)
    t = v.copy()
    while t.shape[-1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    np.testing.assert_array_equal(R.bfly(v), t[:, 0])
    np.testing.assert_array_equal(R.bfly(v[:, :30]), R.bfly(np.concatenate([v[:, :30], np.zeros((5, 2), np.float32)], 1)))


def test_library_exports_sg_feco_warped():
    from speakerguard_amd import _native
    assert "sg_feco_warped" in _native.EXPORTS
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "sg_feco_warped")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speakerguard_hip.h")).read(), flags=re.S)
    m = re.search(r"int sg_feco_warped\((.*?)\);", hdr, re.S)
    assert m, "sg_feco_warped is not declared"
    assert len(m.group(1).split(",")) == 17
    lib = _native.load()
    assert len(lib.sg_feco_warped.argtypes) == 17 and lib.sg_feco_warped.argtypes[7] is ctypes.c_double


def test_defense_refuses_bad_arguments_without_a_gpu():
    from speakerguard_amd.defense.feature_level import WarpedFeCoDefense, FeCoDefense
    with pytest.raises(ValueError):
        WarpedFeCoDefense(0.5, 'L2')
    with pytest.raises(ValueError):
        WarpedFeCoDefense(0.5, 'ts', delta=1.5)
    d = WarpedFeCoDefense(0.5, 'random')
    assert d.init == 'random' and d.batch_coupled is False and not isinstance(d, FeCoDefense)
    assert WarpedFeCoDefense(0.5, 'ts').init == 'ts'
