"""The wide k-means contract (tests/feco_wide_restate.py, csrc/k_feco_wide.hip header) on the CPU: on real iv_plda delta and
CMVN features the float32 chain over 128 lanes gives the ids of plain float64 Lloyd iterations, and running the chain over
72 lanes changes no id; on degenerate rows, where float64 has nothing to say, the contract's own rules hold."""
import numpy as np
import pytest

import feco_wide_restate as R

WAVES = [(32000, 72), (48000, 5)]
_FEATS = {}


def _features(T, seed):
    if (T, seed) not in _FEATS:
        _FEATS[(T, seed)] = R.iv_features(T, seed)
    return _FEATS[(T, seed)]


@pytest.mark.parametrize("T,seed", WAVES)
@pytest.mark.parametrize("ratio", [0.5, 0.2])
def test_restatement_agrees_with_float64_lloyd(T, seed, ratio):
    cells = 0
    for name, feats in _features(T, seed):
        assert feats.shape[2] == 72
        for u in range(feats.shape[0]):
            x = feats[u]
            F = x.shape[0]
            k = int(F * ratio)
            for init_seed in (None, 9):
                frames = R.init_frames(F, k, init_seed, u)
                st = {}
                ids = R.kmeans_ids(x, k, 10, frames, stats=st)
                what = (name, u, ratio, init_seed, st)
                assert np.array_equal(ids, R.lloyd_f64(x, k, 10, frames)), what
                assert st['ties'] == 0 and st['empty'] == 0 and 2 <= st['steps'] <= 10, what
                assert np.array_equal(ids, R.kmeans_ids(x, k, 10, frames, lanes=72)), what  # 72 lanes == 128 lanes
                assert ids.min() >= 0 and ids.max() < k
                out, counts = R.compress(x, ids, k)
                assert np.isfinite(out).all() and counts.sum() == F
                cells += 1
    assert cells == 16  # x 4 parameter cells: the 64 cells


def test_duplicates_tie_to_the_lowest_index_and_empty_clusters_keep_their_centroid():
    x, k = R.degenerate_rows()["duplicates"]
    st = {}
    ids = R.kmeans_ids(x, k, 10, stats=st)
    assert st['ties'] > 0 and st['empty'] > 0
    assert np.array_equal(ids[:20], ids[20:40]) and np.array_equal(ids[:20], ids[60:])  # copies of a row cluster alike
    # the even start (frames 2 j) puts centroids j, j + 10, j + 20, j + 30 on copies of one row: in step 1 they score alike
    # and the lowest index wins (st['ties']); 20 distinct rows can fill 20 of the 40 clusters at the most
    assert len(set(ids.tolist())) <= 20
    assert np.array_equal(ids, R.kmeans_ids(x, k, 10, lanes=72))
    out, counts = R.compress(x, ids, k)
    assert (counts == 0).sum() >= 20 and np.array_equal(out[counts == 0], x[:k][counts == 0])  # the `force` fallback


def test_offset_rows_need_the_centring():
    x, k = R.degenerate_rows()["offset"]
    ids = R.kmeans_ids(x, k, 10)
    assert np.array_equal(ids, R.lloyd_f64(x, k, 10))
    assert np.array_equal(ids, R.kmeans_ids(x, k, 10, lanes=72))
    # without the centring the expanded distance loses the frames' differences in the rounding of |c|^2 ~ 72 x 300^2
    xp = np.zeros((x.shape[0], 128), np.float32)
    xp[:, :72] = x
    c = x[R.init_frames(x.shape[0], k)]
    cp = np.zeros((k, 128), np.float32)
    cp[:, :72] = c
    raw = np.argmax(R.scores(xp, cp, R.half_norms(c, 128)), axis=1)
    assert not np.array_equal(raw, np.argmin(((x[:, None, :].astype(np.float64) - c[None].astype(np.float64)) ** 2).sum(2), axis=1))


def test_one_cluster_and_one_cluster_per_frame():
    x, k = R.degenerate_rows()["k1"]
    st = {}
    assert (R.kmeans_ids(x, k, 10, stats=st) == 0).all() and st['steps'] == 2
    x, k = R.degenerate_rows()["kF"]
    st = {}
    assert np.array_equal(R.kmeans_ids(x, k, 10, stats=st), np.arange(k)) and st['steps'] == 2
    out, counts = R.compress(x, np.arange(k), k)
    assert np.array_equal(out, x) and (counts == 1).all()


def test_scores_take_any_multiple_of_eight():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 80)).astype(np.float32)
    c = rng.standard_normal((3, 80)).astype(np.float32)
    h = rng.standard_normal(3).astype(np.float32)
    s80 = R.scores(x, c, h)
    s128 = R.scores(np.pad(x, ((0, 0), (0, 48))), np.pad(c, ((0, 0), (0, 48))), h)
    assert np.array_equal(s80, s128)
    assert np.allclose(s80, x.astype(np.float64) @ c.T.astype(np.float64) + h, rtol=1e-5, atol=1e-5)
