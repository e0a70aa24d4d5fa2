"""Host side of AudioNet's device-resident defended PGD loops (sg_an_pgd_run_defended), without a GPU: which defended models
``FGSM.attack_batch`` hands to ``base.pgd_run_defended`` / ``base.pgd_run_defended_feco`` and which keep the step loop, and that
header, library and ctypes mirror agree on the new call.  The doubles and the header reader are test_defended_loop_host's,
with AudioNet's input levels (``allowed_flags = [0, 1]``)."""
import ctypes
import re

import pytest
import torch

from speakerguard_amd import _native
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.defense import AS, AT, BDR, LPF, MS, QT
from speakerguard_amd.defense.feature_level import FeCoDefense, WarpedFeCoDefense
from speakerguard_amd.model.defended_model import defended_model
from test_abi import declared_argtypes
from test_defended_loop_host import B, S, T, _FusedBase, _header, _on_cpu, _step_loop, _StepBase


class _AnStepBase(_StepBase):
    allowed_flags = [0, 1]


class _AnChainBase(_FusedBase):
    """offers the input-chain loop only, like xv_plda"""
    allowed_flags = [0, 1]


class _AnBase(_AnChainBase):
    """offers both loops, like audionet_csine"""

    def pgd_run_defended_feco(self, x, y, lower, upper, loss_spec, step_size, max_iter, grad_sign, chain, feco, eot_size=1,
                              eot_batch_size=1, trace=False):
        self.calls.append(("pgd_run_defended_feco", tuple(type(d).__name__ for d in chain), type(feco).__name__, x.shape[0],
                           eot_size, eot_batch_size, trace))
        n = x.shape[0]
        return (x.clone(), torch.ones(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64), torch.zeros(n, S), torch.zeros(n),
                None, None)


def _attack(base, defense, order='sequential', batch_size=2, n=B, **attrs):
    x = torch.zeros(n, 1, T)
    y = torch.zeros(n, dtype=torch.int64)
    atk = PGD(defended_model(base, defense, order=order), max_iter=2, batch_size=batch_size, EOT_size=2, EOT_batch_size=2, verbose=0)
    for k, v in attrs.items():
        setattr(atk, k, v)
    return atk.attack(x, y)


def _fused(base):
    return [c for c in base.calls if isinstance(c, tuple)]


@pytest.mark.parametrize("chain", [[AS(3)], [QT(), LPF(5000)], [MS(5), AS(31), BDR()]], ids=["AS", "QT-LPF", "MS-AS-BDR"])
def test_native_input_chains_take_the_device_loop(chain):
    base = _AnBase()
    adv, success = _attack(base, [(0, d) for d in chain])
    # two batches (2 + 1 utterances): exactly one call each, the chain in order, the EOT sizes handed on
    assert _fused(base) == [("pgd_run_defended", tuple(type(d).__name__ for d in chain), n, 2, 2, False) for n in (2, 1)]
    assert "loss_grad" not in base.calls and "pgd_update" not in base.calls
    assert adv.shape == (B, 1, T) and success == [True] * B


def test_chain_in_front_of_feco_takes_its_own_loop():
    base = _AnBase()
    adv, success = _attack(base, [(0, AS(3)), (1, FeCoDefense(0.5))], batch_size=2, n=4)
    # two batches of 2 utterances: one call each, chain and defense handed on
    assert _fused(base) == [("pgd_run_defended_feco", ("AS",), "FeCoDefense", 2, 2, 2, False)] * 2
    assert "loss_grad" not in base.calls and "pgd_update" not in base.calls
    assert adv.shape == (4, 1, T) and success == [True] * 4
    # the input-chain route does not claim the mixed model, the FeCo-only route neither
    atk = PGD(defended_model(base, [(0, AS(3)), (1, FeCoDefense(0.5))]), verbose=0)
    name, (chain, feco) = atk._device_route(2)
    assert name == "pgd_run_defended_feco" and [type(d).__name__ for d in chain] == ["AS"] and isinstance(feco, FeCoDefense)


def _feco_fallbacks():
    feco = lambda: _on_cpu(FeCoDefense(0.5))  # noqa: E731
    as3 = lambda: _on_cpu(AS(3))  # noqa: E731
    return {
        # name: (base, defense, order, utterances, batch size, attributes)
        "batch-of-1": (_AnBase, [(0, as3()), (1, feco())], 'sequential', 2, 1, {}),
        "at-in-the-chain": (_AnBase, [(0, as3()), (0, _on_cpu(AT(25))), (1, feco())], 'sequential', 2, 2,
                            {"fuse_randomised_input_defenses": True}),
        "warped-feco": (_AnBase, [(0, as3()), (1, _on_cpu(WarpedFeCoDefense(0.5)))], 'sequential', 2, 2, {}),
        "second-feature-level-defense": (_AnBase, [(0, as3()), (1, feco()), (1, feco())], 'sequential', 2, 2, {}),
        "fuse_defended-off": (_AnBase, [(0, as3()), (1, feco())], 'sequential', 2, 2, {"fuse_defended": False}),
        "fuse_input_defenses-off": (_AnBase, [(0, as3()), (1, feco())], 'sequential', 2, 2, {"fuse_input_defenses": False}),
        "base-without-the-method": (_AnChainBase, [(0, as3()), (1, feco())], 'sequential', 2, 2, {}),
    }


@pytest.mark.parametrize("case", sorted(_feco_fallbacks()))
def test_everything_else_in_front_of_feco_keeps_the_step_loop(case):
    make, defense, order, n, batch_size, attrs = _feco_fallbacks()[case]
    base = make()
    _attack(base, defense, order=order, batch_size=batch_size, n=n, **attrs)
    assert not _fused(base), base.calls
    batches = n // batch_size
    assert base.calls.count("loss_grad") == batches * 3 and base.calls.count("pgd_update") == batches * 2  # 2 steps + final pass


def test_average_order_keeps_the_step_loop():
    """'average' has no device loop (its step loop needs a native base, so the routing decision is asked directly)"""
    base = _AnBase()
    defense = [(0, AS(3)), (1, FeCoDefense(0.5))]
    name, (chain, feco) = PGD(defended_model(base, defense), verbose=0)._device_route(2)
    assert name == "pgd_run_defended_feco" and chain == [defense[0][1]] and feco is defense[1][1]
    avg = PGD(defended_model(base, defense, order='average'), verbose=0)
    assert _step_loop(avg)
    # and the other refusals at the same level
    assert PGD(defended_model(base, defense), verbose=0)._device_route(1) is None
    assert _step_loop(PGD(defended_model(_AnStepBase(), defense), verbose=0))
    assert _step_loop(PGD(defended_model(base, [(0, AS(3))] * 9 + [(1, FeCoDefense(0.5))]), verbose=0))  # past the cap
    # no chain: pgd_run_feco's model, never pgd_run_defended_feco's -- and this double has no pgd_run_feco
    assert _step_loop(PGD(defended_model(base, [(1, FeCoDefense(0.5))]), verbose=0))
    from speakerguard_amd.adaptive_attack.BPDA import BPDA
    assert _step_loop(PGD(defended_model(base, [(0, BPDA(AS(3))), (1, FeCoDefense(0.5))]), verbose=0))
    from speakerguard_amd.attack.CWinf import CWinf
    assert _step_loop(CWinf(defended_model(base, defense), verbose=0))  # CWinf's opt-out applies unchanged


# ---------------------------------------------------------------- header, library and ctypes mirror
def test_header_library_and_binding_agree_on_the_call():
    name = "sg_an_pgd_run_defended"
    assert name in set(re.findall(r"\b(sg_[a-z0-9_]+)\s*\(", _header())) and name in _native.EXPORTS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    fn = getattr(_native.load(), name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == declared_argtypes(name)
    # the x-vector call differs by the FeCo argument only, and the comparison sees that
    xv = declared_argtypes("sg_xv_pgd_run_defended")
    assert list(_native.load().sg_xv_pgd_run_defended.argtypes) == xv
    an = list(fn.argtypes)
    assert an[:10] == xv[:10] and an[10] is ctypes.POINTER(_native.FecoParams) and an[11:] == xv[10:]
