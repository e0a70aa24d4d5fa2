"""Host-side attack logic (speakerguard_amd.attack.*, adaptive_attack.*) against the fixtures the
REFERENCE attack classes produced on the toy model (tests/golden/attack_toy.npz).  The engine is a
CPU test double (tests/engine_doubles.py), so this pins chunking, EOT averaging, majority vote,
random restarts, CW2's Adam / binary search / bookkeeping and FAKEBOB's NES + plateau-LR logic
without a GPU.  Also pins the file parsers and the torch-side loss formulas."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from engine_doubles import AutogradEngine
from oracle import attacks as oatk
from speakerguard_amd.attack.CW2 import CW2
from speakerguard_amd.attack.CWinf import CWinf
from speakerguard_amd.attack.FAKEBOB import FAKEBOB
from speakerguard_amd.attack.FGSM import FGSM
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy, SEC4SR_MarginLoss, resolve_loss, resolve_prediction
from toy_model import ToyModel


@pytest.mark.parametrize("tag,thr,task", [("csi", None, "CSI"), ("osi", 1.5, "OSI")])
def test_attacks_match_reference_trajectories(tag, thr, task, capsys):
    g = load_golden("attack_toy.npz")
    x = torch.from_numpy(g["x"])
    toy = ToyModel(threshold=thr).eval()
    for p in toy.parameters():
        p.requires_grad_(False)
    model = AutogradEngine(toy)

    def check(name, atk, exact=True):
        torch.manual_seed(123)
        np.random.seed(123)
        y = torch.from_numpy(g["%s_%s_y" % (tag, name)])
        adv, success = atk.attack(x.clone(), y)
        assert list(success) == g["%s_%s_success" % (tag, name)].tolist(), name
        np.testing.assert_allclose(adv.numpy(), g["%s_%s_adv" % (tag, name)], rtol=0, atol=1e-6 if exact else 2e-4,
                                   err_msg=name)

    check("fgsm", FGSM(model, task=task, epsilon=0.01, batch_size=4, verbose=0))
    check("pgd", PGD(model, task=task, epsilon=0.01, step_size=0.002, max_iter=8, batch_size=3, verbose=0))
    check("pgd_t", PGD(model, task=task, epsilon=0.01, step_size=0.002, max_iter=8, batch_size=2, targeted=True, verbose=0))
    check("pgd_eot", PGD(model, task=task, epsilon=0.01, step_size=0.002, max_iter=4, batch_size=4,
                         EOT_size=4, EOT_batch_size=2, verbose=0))
    check("pgd_rand", PGD(model, task=task, epsilon=0.01, step_size=0.002, max_iter=4, batch_size=4,
                          num_random_init=3, verbose=0))
    check("cwinf", CWinf(model, task=task, epsilon=0.01, step_size=0.002, max_iter=8, batch_size=4, verbose=0))
    check("cw2", CW2(model, task=task, initial_const=0.5, binary_search_steps=4, max_iter=30, stop_early=True,
                     stop_early_iter=10, lr=5e-3, batch_size=4, verbose=0), exact=False)
    check("cw2_t", CW2(model, task=task, initial_const=0.5, binary_search_steps=3, max_iter=25, stop_early=False,
                       lr=5e-3, batch_size=2, targeted=True, confidence=0.1, verbose=0), exact=False)
    fb = dict(task=task, epsilon=0.02, max_iter=30, max_lr=0.004, min_lr=1e-4, samples_per_draw=16,
              samples_per_draw_batch_size=8, sigma=0.01, stop_early=True, stop_early_iter=10, verbose=0)
    if thr is not None:
        fb["threshold"] = thr
    # the reference draws NES noise with torch.randn from the global RNG (seeded by check()); the
    # product takes it through noise_fn so that the same stream is consumed in the same order
    rn = lambda shape: torch.randn(shape)
    check("fakebob", FAKEBOB(model, batch_size=1, noise_fn=rn, **fb))
    check("fakebob_t", FAKEBOB(model, batch_size=1, targeted=True, confidence=0.05, noise_fn=rn, **fb))


def test_estimate_threshold_matches_reference():
    """Product FAKEBOB.estimate_threshold vs the reference's own run (tests/golden/estimate_threshold.npz)."""
    import json
    from conftest import load_golden
    g = load_golden("estimate_threshold.npz")
    x = torch.from_numpy(g["x"])
    kw = json.loads(g["meta"]["kw"])
    rn = lambda shape: torch.randn(shape)
    for name in ("single", "batch_quirk", "accepted", "negative"):
        model = AutogradEngine(ToyModel(threshold=float(g[name + "_model_threshold"])).eval())
        atk = FAKEBOB(model, noise_fn=rn, **kw)
        torch.manual_seed(321)
        np.random.seed(321)
        est = atk.estimate_threshold(x[g[name + "_idx"].tolist()].clone(), step=g["meta"]["step"])
        want = float(g[name + "_estimate"])
        if np.isnan(want):
            assert est is None and atk.threshold is None
        else:
            assert abs(est - want) < 1e-5, (name, est, want)
    assert FAKEBOB(model, task="CSI", verbose=0).estimate_threshold(x) is None  # FAKEBOB.py:281-283


def test_attack_asserts_follow_reference():
    model = AutogradEngine(ToyModel().eval())
    atk = PGD(model, verbose=0)
    x = torch.zeros(2, 1, 800)
    with pytest.raises(AssertionError):
        atk.attack(x + 1.0, torch.zeros(2, dtype=torch.long))  # x.max() must be < 1 (PGD.py:44)
    with pytest.raises(AssertionError):
        atk.attack(torch.zeros(2, 2, 800), torch.zeros(2, dtype=torch.long))  # mono only (:46)
    with pytest.raises(AssertionError):
        atk.attack(x, torch.zeros(3, dtype=torch.long))  # len(y) == N (:47)
    with pytest.raises(AssertionError):
        PGD(model, EOT_size=3, EOT_batch_size=2, verbose=0)  # divisibility (:27)
    with pytest.raises(NotImplementedError):
        FAKEBOB(model, task="OSI", verbose=0).attack(x, torch.zeros(2, dtype=torch.long))  # FAKEBOB.py:178-180


def test_loss_objects_match_oracle_formulas():
    rs = np.random.RandomState(3)
    scores = torch.from_numpy(rs.randn(6, 5).astype(np.float32) * 3)
    y = torch.tensor([0, 4, -1, 2, -1, 1])
    np.testing.assert_allclose(SEC4SR_CrossEntropy()(scores, y).numpy(), oatk.cross_entropy_loss(scores, y).numpy(), atol=1e-5)
    for task in ("CSI", "OSI"):
        for targeted in (False, True):
            for clip in (False, True):
                a = SEC4SR_MarginLoss(targeted, 0.3, task, 0.7, clip)(scores, y)
                b = oatk.margin_loss(scores, y, targeted, 0.3, task, 0.7, clip)
                np.testing.assert_allclose(a.numpy(), b.numpy(), atol=1e-5, err_msg="%s %s %s" % (task, targeted, clip))
    ysv = torch.tensor([0, -1, 0, -1, 0, 0])
    for targeted in (False, True):
        a = SEC4SR_MarginLoss(targeted, 0.3, "SV", 0.7, False)(scores[:, :1], ysv)
        b = oatk.margin_loss(scores[:, :1], ysv, targeted, 0.3, "SV", 0.7, False)
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=1e-5)
    # grad_sign rule, attack/utils.py:114
    assert resolve_loss("Entropy", False)[1] == 1 and resolve_loss("Entropy", True)[1] == -1
    assert resolve_loss("Margin", False)[1] == -1 and resolve_loss("Margin", True)[1] == -1
    with pytest.warns(UserWarning):
        assert isinstance(resolve_loss("Entropy", False, task="OSI", threshold=0.)[0], SEC4SR_MarginLoss)
    assert resolve_prediction([[1, 2, 2], [3, 1, 1, 3], [-1]]).tolist() == [2, 3, -1]  # first-seen wins ties


def test_model_file_parsers_roundtrip(tmp_path, xv_weights):
    from speakerguard_amd import synth
    from speakerguard_amd.model import xv_plda as m
    paths = synth.write_xv_model_dir(str(tmp_path), xv_weights)
    np.testing.assert_allclose(m.parse_mean_file(paths["mean_file"]), xv_weights["emb_mean"], rtol=1e-6)
    np.testing.assert_allclose(m.parse_transform_mat_file(paths["transform_mat_file"]), xv_weights["lda"], rtol=1e-6, atol=1e-9)
    mean, tr, psi = m.parse_plda_file(paths["plda_file"])
    np.testing.assert_allclose(mean, xv_weights["plda_mean"], rtol=1e-6)
    np.testing.assert_allclose(tr, xv_weights["plda_transform"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(psi, xv_weights["plda_psi"], rtol=1e-6)
    ids, zm, zs, enroll = m.parse_enroll_model_file(paths["model_file"])
    assert ids[0] == "spk00" and len(ids) == 10
    np.testing.assert_allclose(enroll, xv_weights["enroll"])


def test_label_check_runs_once_per_label_tensor(monkeypatch):
    """EngineOps.check_labels remembers the label tensor it accepted: a loop that passes the same tensor (CW2, the EOT
    wrapper's cached repeat, the sharded proxy's cached slice) pays one check and one copy to the host, an in-place change
    is checked again, and a ScoreVJP call in between (no labels) leaves the memo alone."""
    import types
    from speakerguard_amd import _native as N
    from speakerguard_amd.adaptive_attack.EOT import EOT
    from speakerguard_amd.attack import utils as U
    from speakerguard_amd.model._engine_ops import EngineOps
    from speakerguard_amd.shard import QueryShardedModel
    calls = []
    real = U.check_labels
    monkeypatch.setattr(U, "check_labels", lambda y, S, spec: (calls.append(1), real(y, S, spec)))

    class Model(EngineOps):
        num_spks = 10

    m, ce = Model(), U.SEC4SR_CrossEntropy()
    vjp = types.SimpleNamespace(loss_id=N.SG_LOSS_LINEAR, task="CSI")
    y = torch.tensor([0, 9, -1, 3])
    for _ in range(3):
        m.check_labels(y, ce)
        m.check_labels(y, vjp)
    assert len(calls) == 1
    y[1] = 10
    with pytest.raises(ValueError, match="label 10 of row 1 "):
        m.check_labels(y, ce)
    y[1] = 9
    m.check_labels(y, ce)
    m.check_labels(y.clone(), ce)  # another tensor: checked
    assert len(calls) == 4
    eot = EOT(m, ce, 2, 2)
    assert eot._labels(y, 2) is eot._labels(y, 2) and eot._labels(y, 2).tolist() == y.repeat(2).tolist()
    ns = types.SimpleNamespace(_y_slice=None)
    a = QueryShardedModel._labels_slice(ns, y, 1, 3)
    assert QueryShardedModel._labels_slice(ns, y, 1, 3) is a and a.tolist() == [9, -1]
    y[2] = 4  # in place: a view shares the version counter, so the model sees the change
    assert QueryShardedModel._labels_slice(ns, y, 1, 3) is not a
