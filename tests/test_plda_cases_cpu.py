"""The back-end corner cases of tests/plda_cases.py, judged on the CPU: with the oracles' embeddings of the cases' inputs, at
least 90 % of the rows of each system's cases have a float64 top-two margin above the score rule's bound -- so that the GPU
tests' decision assertion (decisions equal the float64 arg-max outside the margin) covers them."""
import numpy as np
import pytest
import torch

import plda_cases as P


def _xv_emb():
    from oracle.xv_plda import XvPlda
    w = P.xv_weights()
    with torch.no_grad():
        emb = XvPlda(w).embedding(torch.from_numpy(P.waveforms()))
    return w, emb.double().numpy()


def _iv_emb():
    import iv_restate as R
    w = P.iv_weights()
    o = R.IvOracleModel(w)
    return w, o.r.chain(R.cmvn(R.add_delta(o.features(torch.from_numpy(P.waveforms())))))["emb"]


@pytest.mark.parametrize("name,emb_of,bound_of", [("xv", _xv_emb, P.xv_score_bound), ("iv", _iv_emb, P.iv_score_bound)])
def test_the_cases_sit_outside_their_tie_margins(name, emb_of, bound_of):
    w, emb = emb_of()
    assert emb.shape == (P.B, P.D) and w["enroll"].shape == (P.S_MAX, P.D)
    outside = []
    for S in P.S_CASES:
        truth = P.llr(emb, w["enroll"][:S], w["plda_psi"])
        yard = P.llr(emb.astype(np.float32), w["enroll"][:S], w["plda_psi"], np.float32).astype(np.float64)
        margin, bound = P.top_two_margin(truth), bound_of(truth, yard)
        print("%s S=%d: margins %s, bound %s" % (name, S, margin, bound))
        outside += list(margin > bound)
    assert np.mean(outside) >= 0.9, outside
