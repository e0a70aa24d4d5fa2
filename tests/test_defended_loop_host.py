"""Host side of the device-resident defended PGD loop (sg_xv_pgd_run_defended), without a GPU: which defended models
``FGSM.attack_batch`` hands to ``base.pgd_run_defended`` and which keep the step loop, and that header and ctypes mirror agree
on the new call and its stage struct."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from speakerguard_amd import _native
from speakerguard_amd.adaptive_attack.BPDA import BPDA
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.defense import AS, LPF, QT
from speakerguard_amd.defense.feature_level import FeCoDefense
from speakerguard_amd.model.defended_model import defended_model

B, T, S = 3, 64, 4


class _StepBase:
    """the least a base model needs for attack_batch's step loop: records its calls, computes nothing of interest"""
    allowed_flags = [0, 1, 2]
    threshold = 0.0

    def __init__(self):
        self.calls = []

    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, **kw):
        self.calls.append("loss_grad")
        n = x.shape[0]
        return torch.zeros(n, dtype=torch.int64), torch.zeros(n, S), torch.zeros(n), (torch.ones_like(x) if want_grad else None)

    def make_decision(self, x, flag=0, enroll_embs=None):
        self.calls.append("make_decision")
        return torch.zeros(x.shape[0], dtype=torch.int64), torch.zeros(x.shape[0], S)

    def score(self, x, flag=0, enroll_embs=None):
        return self.make_decision(x, flag)[1]

    def pgd_update(self, x, grad, lower, upper, step_size, grad_sign):
        self.calls.append("pgd_update")
        return x

    def frontend_forward(self, x):
        return torch.zeros(x.shape[0], 5, 30), None

    def frontend_backward(self, saved, g):
        return torch.ones(g.shape[0], 1, T)

    def comput_feat_from_feat(self, feats, ori_flag=1, des_flag=2):
        return feats

    def cmvn_backward(self, g):
        return g


class _FusedBase(_StepBase):
    def pgd_run_defended(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, chain, eot_size=1,
                         eot_batch_size=1, trace=False):
        self.calls.append(("pgd_run_defended", tuple(type(d).__name__ for d in chain), x.shape[0], eot_size, eot_batch_size, trace))
        n = x.shape[0]
        ltr = torch.zeros(max_iter + 1, n) if trace else None
        dtr = torch.zeros(max_iter + 1, n, dtype=torch.int64) if trace else None
        return (x.clone(), torch.ones(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64), torch.zeros(n, S), torch.zeros(n),
                ltr, dtr)


def _on_cpu(d):
    """the defense object as the route sees it (its type, its level), with a CPU body for the step loop it may fall back to:
    the real bodies are device kernels"""
    d.fwd = lambda x, **kw: (x, None)
    d.bwd = lambda saved, g: g
    return d


def _attack(base, defense, order='sequential', batch_size=2, **attrs):
    x = torch.zeros(B, 1, T)
    y = torch.zeros(B, dtype=torch.int64)
    atk = PGD(defended_model(base, defense, order=order), max_iter=2, batch_size=batch_size, EOT_size=2, EOT_batch_size=2, verbose=0)
    for k, v in attrs.items():
        setattr(atk, k, v)
    return atk.attack(x, y)


@pytest.mark.parametrize("chain", [[AS(3)], [QT(), LPF(5000)]], ids=["AS", "QT-LPF"])
def test_native_input_chains_take_the_device_loop(chain):
    base = _FusedBase()
    adv, success = _attack(base, [(0, d) for d in chain])
    fused = [c for c in base.calls if isinstance(c, tuple)]
    # two batches (2 + 1 utterances): exactly one call each, the chain in order, the EOT sizes handed on
    assert fused == [("pgd_run_defended", tuple(type(d).__name__ for d in chain), n, 2, 2, False) for n in (2, 1)]
    assert "loss_grad" not in base.calls and "pgd_update" not in base.calls
    assert adv.shape == (B, 1, T) and success == [True] * B


def _fallbacks():
    return {
        "bpda": (_FusedBase, [(0, BPDA(lambda a: a))], {}),
        "feature-level-mixed-in": (_FusedBase, [(0, _on_cpu(AS(3))), (1, _on_cpu(FeCoDefense(0.5)))], {}),
        "flag-off": (_FusedBase, [(0, _on_cpu(AS(3)))], {"fuse_input_defenses": False}),
        "base-without-the-call": (_StepBase, [(0, _on_cpu(AS(3)))], {}),
    }


@pytest.mark.parametrize("case", sorted(_fallbacks()))
def test_everything_else_keeps_the_step_loop(case):
    make, defense, attrs = _fallbacks()[case]
    base = make()
    _attack(base, defense, **attrs)
    assert not [c for c in base.calls if isinstance(c, tuple)], base.calls
    assert base.calls.count("loss_grad") == 2 * 3 and base.calls.count("pgd_update") == 2 * 2  # 2 batches x (2 steps + final pass)


def _step_loop(atk):
    """the route is the step loop whatever the batch size"""
    return atk._device_route(1) is None and atk._device_route(2) is None


def test_average_order_keeps_the_step_loop():
    """'average' has no device loop: the route must not take it (the step loop then needs a native base, so the attack is
    not run here: the routing decision is asked directly)"""
    base = _FusedBase()
    seq = PGD(defended_model(base, [(0, AS(3))]), verbose=0)
    avg = PGD(defended_model(base, [(0, AS(3))], order='average'), verbose=0)
    name, (chain,) = seq._device_route(B)
    assert name == "pgd_run_defended" and [type(d).__name__ for d in chain] == ["AS"]
    assert _step_loop(avg)
    # and the other refusals at the same level
    assert _step_loop(PGD(defended_model(base, [(0, AS(3)), (1, FeCoDefense(0.5))]), verbose=0))
    assert _step_loop(PGD(defended_model(base, [(0, BPDA(AS(3)))]), verbose=0))
    assert _step_loop(PGD(defended_model(_StepBase(), [(0, AS(3))]), verbose=0))
    assert _step_loop(PGD(defended_model(base, [(0, AS(3))] * 9), verbose=0))  # past the cap
    assert PGD.fuse_input_defenses is True
    # a randomised stage keeps the step loop (and its noise keys) unless the device loop's schedule is asked for
    from speakerguard_amd.defense import AT
    at = PGD(defended_model(base, [(0, AS(3)), (0, AT(25))]), verbose=0)
    assert PGD.fuse_randomised_input_defenses is False and _step_loop(at)
    at.fuse_randomised_input_defenses = True
    name, (chain,) = at._device_route(B)
    assert name == "pgd_run_defended" and [type(d).__name__ for d in chain] == ["AS", "AT"]


# ---------------------------------------------------------------- header and ctypes mirror (tests/test_abi.py's method)
def _header():
    text = open(os.path.join(ROOT, "include", "speakerguard_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_call_and_the_binding_lists_it():
    names = set(re.findall(r"\b(sg_[a-z0-9_]+)\s*\(", _header()))
    assert {"sg_xv_pgd_run_defended", "sg_wav_rep_sum_update"} <= names
    assert {"sg_xv_pgd_run_defended", "sg_wav_rep_sum_update"} <= set(_native.EXPORTS)
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "sg_xv_pgd_run_defended") and hasattr(lib, "sg_wav_rep_sum_update")
    assert int(re.search(r"#define\s+SG_WAV_CHAIN_MAX\s+(\d+)", _header()).group(1)) == _native.SG_WAV_CHAIN_MAX
    for tag in (64, 65, 66):
        assert tag in _native.STAGE_NAMES and re.search(r"#define\s+SG_STAGE_DEF_\w+\s+%d\b" % tag, _header())


def test_stage_struct_layout_matches_header(tmp_path):
    """sizeof and member offsets of sg_wav_stage (and of the two structs it holds) as gcc lays the header out"""
    fields = [("sg_wav_stage", "tag"), ("sg_wav_stage", "u"), ("sg_wav_stage", "u.defense"), ("sg_wav_stage", "u.filter")]
    src = tmp_path / "stage.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "speakerguard_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(sg_wav_stage), sizeof(sg_wav_defense), sizeof(sg_wav_filter));\n' +
                   "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "stage"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:3] == [ctypes.sizeof(_native.WavStage), ctypes.sizeof(_native.WavDefense), ctypes.sizeof(_native.WavFilter)]
    u = _native.WavStage.u
    assert out[3:] == [_native.WavStage.tag.offset, u.offset, u.offset + _native._WavStageU.defense.offset,
                       u.offset + _native._WavStageU.filter.offset]


def test_stage_methods_fill_the_struct():
    st = AS(5).stage()
    assert st.tag == _native.SG_WAV_STAGE_DEFENSE and st.u.defense.kind == _native.SG_TD["AS"] and st.u.defense.param == 5.0
    from speakerguard_amd.defense import BDR
    st = BDR(8).stage()
    assert st.u.defense.kind == _native.SG_TD["QT"] and st.u.defense.param == 256.0
    f = LPF(5000)
    st = f.stage()
    assert st.tag == _native.SG_WAV_STAGE_FILTER and st.u.filter.n_sections == len(f.sos)
    assert ctypes.addressof(st.u.filter.sos.contents) == f.sos.ctypes.data
    with pytest.raises(ValueError):
        AS(4).stage()
