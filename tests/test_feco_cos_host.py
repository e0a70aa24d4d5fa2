"""FeCo with the cosine distance (``FeCoDefense(other_param='cos')``), the parts that need no GPU: the constructor, the
routing (a cosine FeCo never reaches a device loop: they cluster with L2) and the contract's restatement
(tests/feco_cos_restate.py) against float64 Lloyd iterations on real features."""
import numpy as np
import pytest
import torch

import feco_cos_restate as R
from oracle import audionet as oan
from oracle import feco as ofeco
from oracle import kaldi_mfcc
from speakerguard_amd import _native as N
from speakerguard_amd import synth
from speakerguard_amd.attack.CWinf import CWinf
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.defense import AS
from speakerguard_amd.defense.feature_level import FeCoDefense
from speakerguard_amd.model.audionet_csine import audionet_csine
from speakerguard_amd.model.defended_model import defended_model
from speakerguard_amd.model.xv_plda import xv_plda
from test_device_route import BASES
from test_xv_feco_route import _XvFecoBase


def test_the_cosine_distance_constructs():
    d = FeCoDefense(0.5, other_param='cos')
    assert d.other_param == 'cos' and FeCoDefense(0.5).other_param == 'L2'
    assert d.param == 0.5 and d.init == 'even' and d.max_iter == 10
    assert FeCoDefense(0.2, other_param='cos', init='random', seed=3).init == 'random'


@pytest.mark.parametrize("name", ['cosine', 'L1', 'l2', 'COS', None])
def test_other_distances_keep_raising(name):
    with pytest.raises(NotImplementedError):
        FeCoDefense(0.5, other_param=name)


def test_the_library_names_the_new_entry():
    assert "sg_feco_kmeans_compress_metric" in N.EXPORTS
    assert (N.SG_FECO_L2, N.SG_FECO_COS) == (0, 1)


FLAG_NAMES = ("fuse_defended", "fuse_input_defenses", "fuse_randomised_input_defenses", "fuse_randomised_feco")
FLAG_CELLS = [(name, v) for name in FLAG_NAMES for v in (False, True)] + [(None, None)]


def _bases():
    return {"xv-like": lambda: _XvFecoBase(0.0), "an-like": BASES["an-like"]}


@pytest.mark.parametrize("base", ["xv-like", "an-like"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("chain", [False, True], ids=["no-chain", "chain"])
def test_cosine_feco_never_takes_a_device_loop(base, level, chain):
    """... while the same configuration with L2 does wherever the base offers its loop: the cell is not dead"""
    took_l2 = False
    for init in ("even", "random"):
        for attack in (PGD, CWinf):
            for flag, value in FLAG_CELLS:
                for n in (1, 2, 64):
                    routes = {}
                    for dist in ("cos", "L2"):
                        defense = ([(0, AS(3))] if chain else []) + [(level, FeCoDefense(0.5, other_param=dist, init=init))]
                        atk = attack(defended_model(_bases()[base](), defense), verbose=0)
                        if flag is not None:
                            setattr(atk, flag, value)
                        routes[dist] = atk._device_route(n)
                    assert routes["cos"] is None, (init, attack.__name__, flag, value, n)
                    took_l2 = took_l2 or routes["L2"] is not None
    expect_l2 = {("xv-like", 1, False), ("xv-like", 2, False), ("an-like", 1, False), ("an-like", 1, True)}
    assert took_l2 == ((base, level, chain) in expect_l2)


@pytest.mark.parametrize("cls", [xv_plda, audionet_csine])
def test_feco_params_refuses_the_cosine_distance(cls):
    class Model:  # `_feco_params` must refuse before it touches the model or the library
        pass
    with pytest.raises(N.NativeError, match="L2"):
        cls._feco_params(Model(), FeCoDefense(0.5, other_param='cos'), 32000)


# ---- the restatement against float64 ------------------------------------------------------------------------------------------
WAVES = [(32000, 72), (48000, 5)]
_FEATS = {}


def _features(T, seed):
    """[('mfcc', (4, F, 30)), ('logmel', (4, F, 32))] float32 of four synthetic utterances"""
    if (T, seed) not in _FEATS:
        x = torch.from_numpy(synth.make_waveforms(4, T, seed=seed))
        mfcc = kaldi_mfcc.mfcc_batch(x * 32768.0).numpy().astype(np.float32)
        logmel = oan.preprocess(x.reshape(4, -1)).transpose(1, 2).contiguous().numpy().astype(np.float32)
        _FEATS[(T, seed)] = [("mfcc", mfcc), ("logmel", logmel)]
    return _FEATS[(T, seed)]


@pytest.mark.parametrize("T,seed", WAVES)
@pytest.mark.parametrize("ratio", [0.5, 0.2])
def test_restatement_agrees_with_float64_lloyd(T, seed, ratio):
    differs_from_l2 = 0
    for name, feats in _features(T, seed):
        assert feats.shape[2] % 2 == 0
        for u in range(feats.shape[0]):
            x = feats[u]
            F = x.shape[0]
            k = int(F * ratio)
            for init_seed in (None, 9):
                frames = R.init_frames(F, k, init_seed, u)
                st = {}
                ids = R.kmeans_ids(x, k, 10, frames, stats=st)
                ref = R.lloyd_f64(x, k, 10, frames)
                what = (name, u, ratio, init_seed, st)
                assert np.array_equal(ids, ref), what
                # (what keeps the float64 run comparable: nothing degenerate; up to 10 assignment steps occur)
                assert st['zero_norm'] == 0 and st['empty'] == 0 and 2 <= st['steps'] <= 10, what
                assert ids.min() >= 0 and ids.max() < k
                out, counts = R.compress(x, ids, k)
                assert np.isfinite(out).all() and counts.sum() == F
                differs_from_l2 += int((ids != ofeco.kmeans_ids(x, k, 10, frames)).sum())
    assert differs_from_l2 > 0  # over the batch: single utterances may cluster alike under both distances


def test_restatement_degenerate_rows():
    """a zero initial centroid scores 0 and stays put while empty; identical frames tie and the lower index wins"""
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((40, 30)) * 6).astype(np.float32)
    x[:5] = 0
    x[21] = x[20]
    st = {}
    ids = R.kmeans_ids(x, 20, 10, stats=st)
    assert st['zero_norm'] > 0 and st['ties'] > 0
    assert ids[20] == ids[21] and (ids[:5] == ids[0]).all()
    rows, n = R.unit_rows(x[:6], 32)
    assert (rows[:5] == 0).all() and n[5] > 0 and np.isfinite(rows).all()
