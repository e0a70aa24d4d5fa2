"""What the public methods that ``xv_plda`` and ``iv_plda`` share (model/_plda_model.py) hand to the C ABI, without a GPU: the
models are built with ``cls.__new__`` on the CPU and the recording stand-in for the engine context of test_loop_marshalling.

One fixed script of public calls per model; after every call the record is the list of (C entry, plain arguments) it made
and the dither draw counter ``_draw``.  ``tests/native/plda_host_calls.expected`` holds the records captured ONCE by running
``python tests/test_plda_model_host.py`` (it rewrites the table) on the commit before the shared base class existed, when
each model carried its own copy of these methods: the script uses public methods only, so it runs on both trees.
"""
import json
import os

import numpy as np
import pytest
import torch

from speakerguard_amd.attack.utils import resolve_loss
from speakerguard_amd.model.iv_plda import iv_plda
from speakerguard_amd.model.xv_plda import xv_plda
from test_loop_marshalling import _Recorder

EXPECTED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "plda_host_calls.expected")
B, T, S, D, R, CN = 3, 5043, 5, 7, 6, 4
MODELS = {"xv": xv_plda, "iv": iv_plda}


def _model(cls):
    m = cls.__new__(cls)
    m.device, m.ctx = torch.device("cpu"), _Recorder()
    m._stream = lambda: "stream"
    m.dither, m.dither_seed, m.threshold = 1.0, 9, -np.inf
    m.dim, m.num_spks, m._has_enroll = D, S, False
    m.enroll_embs = torch.zeros(1, D)
    if cls is iv_plda:
        m.ivector_dim, m.num_gaussians, m._white_box = R, CN, False
    m.begin_attack()
    m.begin_batch(40, 1)
    return m


def _table(n):
    return (np.arange(n * D, dtype=np.float32).reshape(n, D) - 3.0) / 8


def script(name):
    """[(label, thunk)] on one fresh model, in order; a thunk returns nothing that is compared"""
    m = _model(MODELS[name])
    x = torch.zeros(B, 1, T)
    y = torch.arange(B) % S
    sub = torch.from_numpy(_table(2))
    loss, _ = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    steps = [
        ("forward without enrolled speakers", lambda: pytest.raises(AssertionError, m.forward, x)),
        ("set_enroll(table)", lambda: m.set_enroll(_table(S))),
        ("set_enroll(threshold only)", lambda: m.set_enroll(threshold=1.25)),
        ("set_enroll(table, threshold)", lambda: m.set_enroll(torch.from_numpy(_table(S - 1)), 0.5)),
        ("set_enroll()", lambda: m.set_enroll()),
        ("forward", lambda: m.forward(x)),
        ("__call__(return_emb, dither_seed)", lambda: m(x, return_emb=True, dither_seed=77)),
        ("forward(enroll_embs)", lambda: m.forward(x, enroll_embs=sub)),
        ("score", lambda: m.score(x)),
        ("score(enroll_embs numpy)", lambda: m.score(x, enroll_embs=_table(3))),
        ("make_decision", lambda: m.make_decision(x)),
        ("make_decision(enroll_embs)", lambda: m.make_decision(x, enroll_embs=sub)),
        ("embedding", lambda: m.embedding(x)),
    ]
    steps += [("compute_feat(flag=%d)" % f, lambda f=f: m.compute_feat(x, flag=f)) for f in m.allowed_flags[1:]]
    if name == "xv":
        steps.append(("frontend_forward", lambda: m.frontend_forward(x)))
        steps.append(("frontend_forward(dither_seed)", lambda: m.frontend_forward(x, dither_seed=5)))
        steps.append(("next_dither_seed", lambda: m.next_dither_seed()))
    steps.append(("loss_grad(want_grad=False)", lambda: m.loss_grad(x, y, loss, want_grad=False)))
    return m, steps


def record(name, monkeypatch):
    # the per-call override marks its table as in use on the current GPU stream: no such thing on the CPU
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, stream: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    m, steps = script(name)
    out = []
    for label, thunk in steps:
        m.ctx.calls = []
        thunk()
        out.append({"call": label, "entries": [[entry, args] for entry, args in m.ctx.calls], "_draw": m._draw,
                    "num_spks": m.num_spks, "threshold": float(m.threshold), "_has_enroll": bool(m._has_enroll)})
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_what_the_shared_methods_hand_to_the_engine(name, monkeypatch):
    with open(EXPECTED_PATH) as f:
        want = json.load(f)[name]
    got = json.loads(json.dumps(record(name, monkeypatch)))  # (tuples -> lists, like the table)
    assert [g["call"] for g in got] == [w["call"] for w in want]
    for g, w in zip(got, want):
        assert g == w, g["call"]


def test_the_models_share_no_method_body():
    """every method the two models have in common is the SAME function object (the base's) or differs in its code"""
    for attr in set(vars(xv_plda)) & set(vars(iv_plda)):
        a, b = vars(xv_plda)[attr], vars(iv_plda)[attr]
        if callable(a) and callable(b) and hasattr(a, "__code__") and hasattr(b, "__code__"):
            assert a.__code__.co_code != b.__code__.co_code or a.__code__.co_consts != b.__code__.co_consts, attr


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    table = {name: record(name, mp) for name in sorted(MODELS)}
    mp.undo()
    with open(EXPECTED_PATH, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
