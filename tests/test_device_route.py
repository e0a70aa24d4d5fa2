"""``FGSM._device_route``: which defended models ``attack_batch`` hands to which device loop of the base model, and which keep
the step loop -- one table over everything the routing rules read, without a GPU.

A row is (base capability, defense list, order, attack class); its literal holds one letter per cell, the cells being the
fuse flags x the batch size in ``CELLS`` order.  The letters (``ROUTES``): ``.`` step loop, ``r`` pgd_run, ``f`` pgd_run_feco,
``c`` pgd_run_defended, ``b`` pgd_run_defended_feco.

The expected column was produced ONCE, on the commit before ``_device_route`` existed, by asking its four predicates in
``attack_batch``'s order (``_can_fuse``, ``_fused_feco``, ``_fused_input_chain``, ``_fused_chain_feco``) for every cell of this very
table; the same run checked that the chain / FeCo objects those predicates returned are the level-0 entries in list order and
the level-1 entry, which is what ``_expected_extras`` restates.  It is never produced from ``_device_route``.
"""
import itertools
import warnings

import pytest

from speakerguard_amd.adaptive_attack.BPDA import BPDA
from speakerguard_amd.attack.CWinf import CWinf
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.defense import AS, AT
from speakerguard_amd.defense.feature_level import FeCoDefense, WarpedFeCoDefense
from speakerguard_amd.model.defended_model import defended_model
from test_an_defended_loop_host import _AnBase, _AnChainBase
from test_defended_loop_host import _FusedBase, _StepBase

ROUTES = {".": None, "r": "pgd_run", "f": "pgd_run_feco", "c": "pgd_run_defended", "b": "pgd_run_defended_feco"}


def _offering(cls, *names):
    """the double `cls` with further loop methods: the route asks ``hasattr`` only"""
    return type(cls.__name__ + "".join("_" + n for n in names), (cls,), {n: (lambda self, *a, **kw: None) for n in names})


BASES = {
    "step-only": _StepBase,                                              # levels 0, 1, 2; no device loop at all
    "xv-like": _offering(_FusedBase, "pgd_run"),                        # levels 0, 1, 2; pgd_run, pgd_run_defended
    "an-like": _offering(_AnBase, "pgd_run", "pgd_run_feco"),           # levels 0, 1; all four
    "an-like-no-chain-feco": _offering(_AnChainBase, "pgd_run", "pgd_run_feco"),  # ... without pgd_run_defended_feco
}
NO_SUCH_LEVEL = 3  # an input level none of the doubles allows: defended_model warns and ignores the entry


def _chain(n):
    return [(0, AS(3)) for _ in range(n)]


DEFENSES = {
    "none": lambda: None,
    "empty": lambda: [],
    "chain-1": lambda: _chain(1),
    "chain-8": lambda: _chain(8),
    "chain-9": lambda: _chain(9),
    "chain-with-AT": lambda: [(0, AS(3)), (0, AT(25))],
    "bpda-stage": lambda: [(0, BPDA(AS(3)))],
    "feco": lambda: [(1, FeCoDefense(0.5))],
    "warped-feco": lambda: [(1, WarpedFeCoDefense(0.5))],
    "chain+feco": lambda: _chain(1) + [(1, FeCoDefense(0.5))],
    "chain-8+feco": lambda: _chain(8) + [(1, FeCoDefense(0.5))],
    "chain-9+feco": lambda: _chain(9) + [(1, FeCoDefense(0.5))],
    "chain+AT+feco": lambda: [(0, AS(3)), (0, AT(25)), (1, FeCoDefense(0.5))],
    "bpda-stage+feco": lambda: [(0, BPDA(AS(3))), (1, FeCoDefense(0.5))],
    "chain+warped-feco": lambda: _chain(1) + [(1, WarpedFeCoDefense(0.5))],
    "two-feco": lambda: [(1, FeCoDefense(0.5)), (1, FeCoDefense(0.5))],
    "chain+two-feco": lambda: _chain(1) + [(1, FeCoDefense(0.5)), (1, FeCoDefense(0.5))],
    "chain+ignored-level": lambda: _chain(1) + [(NO_SUCH_LEVEL, AS(3))],
    "feco+ignored-level": lambda: [(1, FeCoDefense(0.5)), (NO_SUCH_LEVEL, AS(3))],
    "chain+feco+ignored-level": lambda: _chain(1) + [(1, FeCoDefense(0.5)), (NO_SUCH_LEVEL, AS(3))],
}
ORDERS = ("sequential", "average")
ATTACKS = {"PGD": PGD, "CWinf": CWinf}
# a flag is SET on the attack object only where it leaves PGD's default (fuse_defended / fuse_input_defenses off,
# fuse_randomised_input_defenses on), so that CWinf's own class-level opt-out is what its default cells see
FLAGS = list(itertools.product((None, False), (None, False), (None, True)))
CELLS = [(flags, n) for flags in FLAGS for n in (1, 2)]  # 16 per row

# one line per (base, defense): sequential PGD, sequential CWinf, average PGD, average CWinf
EXPECTED = {
    ("step-only", "none"): ("................", "................", "................", "................"),
    ("step-only", "empty"): ("................", "................", "................", "................"),
    ("step-only", "chain-1"): ("................", "................", "................", "................"),
    ("step-only", "chain-8"): ("................", "................", "................", "................"),
    ("step-only", "chain-9"): ("................", "................", "................", "................"),
    ("step-only", "chain-with-AT"): ("................", "................", "................", "................"),
    ("step-only", "bpda-stage"): ("................", "................", "................", "................"),
    ("step-only", "feco"): ("................", "................", "................", "................"),
    ("step-only", "warped-feco"): ("................", "................", "................", "................"),
    ("step-only", "chain+feco"): ("................", "................", "................", "................"),
    ("step-only", "chain-8+feco"): ("................", "................", "................", "................"),
    ("step-only", "chain-9+feco"): ("................", "................", "................", "................"),
    ("step-only", "chain+AT+feco"): ("................", "................", "................", "................"),
    ("step-only", "bpda-stage+feco"): ("................", "................", "................", "................"),
    ("step-only", "chain+warped-feco"): ("................", "................", "................", "................"),
    ("step-only", "two-feco"): ("................", "................", "................", "................"),
    ("step-only", "chain+two-feco"): ("................", "................", "................", "................"),
    ("step-only", "chain+ignored-level"): ("................", "................", "................", "................"),
    ("step-only", "feco+ignored-level"): ("................", "................", "................", "................"),
    ("step-only", "chain+feco+ignored-level"): ("................", "................", "................", "................"),
    ("xv-like", "none"): ("rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr"),
    ("xv-like", "empty"): ("................", "................", "................", "................"),
    ("xv-like", "chain-1"): ("cccc....cccc....", "................", "................", "................"),
    ("xv-like", "chain-8"): ("cccc....cccc....", "................", "................", "................"),
    ("xv-like", "chain-9"): ("................", "................", "................", "................"),
    ("xv-like", "chain-with-AT"): ("..cc......cc....", "................", "................", "................"),
    ("xv-like", "bpda-stage"): ("................", "................", "................", "................"),
    ("xv-like", "feco"): ("................", "................", "................", "................"),
    ("xv-like", "warped-feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain+feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain-8+feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain-9+feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain+AT+feco"): ("................", "................", "................", "................"),
    ("xv-like", "bpda-stage+feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain+warped-feco"): ("................", "................", "................", "................"),
    ("xv-like", "two-feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain+two-feco"): ("................", "................", "................", "................"),
    ("xv-like", "chain+ignored-level"): ("................", "................", "................", "................"),
    ("xv-like", "feco+ignored-level"): ("................", "................", "................", "................"),
    ("xv-like", "chain+feco+ignored-level"): ("................", "................", "................", "................"),
    ("an-like", "none"): ("rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr"),
    ("an-like", "empty"): ("................", "................", "................", "................"),
    ("an-like", "chain-1"): ("cccc....cccc....", "................", "................", "................"),
    ("an-like", "chain-8"): ("cccc....cccc....", "................", "................", "................"),
    ("an-like", "chain-9"): ("................", "................", "................", "................"),
    ("an-like", "chain-with-AT"): ("..cc......cc....", "................", "................", "................"),
    ("an-like", "bpda-stage"): ("................", "................", "................", "................"),
    ("an-like", "feco"): (".f.f.f.f........", ".f.f.f.f........", "................", "................"),
    ("an-like", "warped-feco"): ("................", "................", "................", "................"),
    ("an-like", "chain+feco"): (".b.b............", "................", "................", "................"),
    ("an-like", "chain-8+feco"): (".b.b............", "................", "................", "................"),
    ("an-like", "chain-9+feco"): ("................", "................", "................", "................"),
    ("an-like", "chain+AT+feco"): ("................", "................", "................", "................"),
    ("an-like", "bpda-stage+feco"): ("................", "................", "................", "................"),
    ("an-like", "chain+warped-feco"): ("................", "................", "................", "................"),
    ("an-like", "two-feco"): ("................", "................", "................", "................"),
    ("an-like", "chain+two-feco"): ("................", "................", "................", "................"),
    ("an-like", "chain+ignored-level"): ("................", "................", "................", "................"),
    ("an-like", "feco+ignored-level"): ("................", "................", "................", "................"),
    ("an-like", "chain+feco+ignored-level"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "none"): ("rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr", "rrrrrrrrrrrrrrrr"),
    ("an-like-no-chain-feco", "empty"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-1"): ("cccc....cccc....", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-8"): ("cccc....cccc....", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-9"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-with-AT"): ("..cc......cc....", "................", "................", "................"),
    ("an-like-no-chain-feco", "bpda-stage"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "feco"): (".f.f.f.f........", ".f.f.f.f........", "................", "................"),
    ("an-like-no-chain-feco", "warped-feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-8+feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain-9+feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+AT+feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "bpda-stage+feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+warped-feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "two-feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+two-feco"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+ignored-level"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "feco+ignored-level"): ("................", "................", "................", "................"),
    ("an-like-no-chain-feco", "chain+feco+ignored-level"): ("................", "................", "................", "................"),
}


def make_attack(base, defense, order, attack):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # defended_model's 'Unsupported Input Level Flag' of the ignored-level rows
        model = defended_model(BASES[base](), DEFENSES[defense](), order=order)
    return ATTACKS[attack](model, verbose=0)


def set_flags(atk, flags):
    for name, v in zip(("fuse_defended", "fuse_input_defenses", "fuse_randomised_input_defenses"), flags):
        if v is not None:
            setattr(atk, name, v)
    return atk


def _expected_extras(name, defense):
    chain = [d for flag, d in defense or [] if flag == 0]
    feco = [d for flag, d in defense or [] if flag == 1]
    return {"pgd_run": [], "pgd_run_feco": feco, "pgd_run_defended": [chain], "pgd_run_defended_feco": [chain] + feco}[name]


ROWS = [(b, d, o, a) for b in BASES for d in DEFENSES for o in ORDERS for a in ATTACKS]


def test_the_table_has_every_row():
    assert len(ROWS) == len(BASES) * len(DEFENSES) * 4 == 320 and len(CELLS) == 16
    assert sorted(EXPECTED) == sorted((b, d) for b in BASES for d in DEFENSES)
    assert all(len(v) == 4 and all(len(s) == 16 and set(s) <= set(ROUTES) for s in v) for v in EXPECTED.values())
    # every route, and the step loop, occurs: the table is not a column of dots
    assert set("".join("".join(v) for v in EXPECTED.values())) == set(ROUTES)


@pytest.mark.parametrize("base,defense,order,attack", ROWS, ids=["/".join(r) for r in ROWS])
def test_device_route(base, defense, order, attack):
    expected = EXPECTED[(base, defense)][2 * ORDERS.index(order) + list(ATTACKS).index(attack)]
    got = ""
    for (flags, n), letter in zip(CELLS, expected):
        atk = set_flags(make_attack(base, defense, order, attack), flags)
        route = atk._device_route(n)
        if route is None:
            got += "."
            continue
        name, extra = route
        got += {v: k for k, v in ROUTES.items()}[name]
        if letter != "." and ROUTES[letter] == name:
            want = _expected_extras(name, atk.model.defense)
            assert isinstance(extra, tuple) and len(extra) == len(want), (flags, n, route)
            for e, w in zip(extra, want):  # the chain: the same objects in list order; the FeCo defense: the object itself
                assert (len(e) == len(w) and all(a is b for a, b in zip(e, w))) if isinstance(w, list) else e is w, (flags, n, route)
    assert got == expected, "cells (fuse_defended, fuse_input_defenses, fuse_randomised_input_defenses), n: %r" % (CELLS,)
