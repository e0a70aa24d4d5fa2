"""What ``xv_plda.pgd_run_feco`` hands to sg_xv_pgd_run_feco, without a GPU: the model is built with ``cls.__new__`` on the CPU
over the recording stand-in for the engine context of tests/test_loop_marshalling.py.

The expected record is written out from what that file already pins, not captured from the method: the parameter block and the
dither's key are those of ``xv.pgd_run`` there (same model state, same ``dither_seed``), FeCo's key is the one ``an.pgd_run_feco``
draws there for the same defense seed at the same point of the noise bookkeeping (``defense_seed`` does not know the model),
k = int(63 * 0.5) for the 63 frames of 10081 samples, ``index_base`` is the chunk's 40.  The argument positions are the
prototype's: x_adv, y, lower, upper, B, T, params, feco, level, then the six outputs and the stream."""
import pytest
import torch

from speakerguard_amd.attack.utils import resolve_loss
from speakerguard_amd.defense.feature_level import FeCoDefense
from speakerguard_amd.model.xv_plda import xv_plda
from test_loop_marshalling import B, EOT, EOT_BATCH, EXPECTED as PINNED, ITERS, S, STEP, T_FECO, _model

DITHER_KEY = PINNED[("xv.pgd_run", False)]["last_fused_seed"]
FECO_KEY = PINNED[("an.pgd_run_feco", False)]["last_fused_seed"]
PARAMS = PINNED[("xv.pgd_run", False)]["calls"][0][1][6]


def _run(level, trace, init="random", **kw):
    m = _model(xv_plda)
    feco = FeCoDefense(0.5, init=init, seed=7, max_iter=10)
    loss, grad_sign = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, y = torch.zeros(B, 1, T_FECO), torch.arange(B) % S
    if level is not None:
        kw["level"] = level
    out = m.pgd_run_feco(x, y, torch.full((B, 1, 1), -1.0), torch.full((B, 1, 1), 1.0), loss, STEP, ITERS, grad_sign, feco, EOT, EOT_BATCH,
                         trace=trace, **kw)
    return m, feco, x, out


@pytest.mark.parametrize("trace", [False, True], ids=["plain", "trace"])
@pytest.mark.parametrize("level", [None, 1, 2], ids=["default-level", "level-1", "level-2"])
@pytest.mark.parametrize("init", ["even", "random"])
def test_what_pgd_run_feco_hands_to_the_engine(level, trace, init):
    m, feco, x, out = _run(level, trace, init)
    assert out[0] is not x and out[0].data_ptr() != x.data_ptr() and torch.equal(out[0], x)  # the loop works on a copy
    rec = "ptr" if trace else "NULL"
    want = ("sg_xv_pgd_run_feco", [
        "ptr", "ptr", "ptr", "ptr", B, T_FECO,
        dict(PARAMS, dither=dict(PARAMS["dither"], seed=DITHER_KEY)),
        {"k": 31, "max_iter": 10, "random_init": int(init == "random"), "seed": FECO_KEY, "index_base": 40},
        1 if level is None else level,
        "ptr", "ptr", "ptr", "ptr", rec, rec, "stream",
    ])
    assert len(m.ctx.calls) == 1 and m.ctx.calls[0][0] == want[0]
    for i, (g, w) in enumerate(zip(m.ctx.calls[0][1], want[1])):
        assert g == w, "argument %d" % i
    assert m.ctx.calls[0] == want
    assert [None if o is None else (tuple(o.shape), str(o.dtype)) for o in out] == [
        ((B, 1, T_FECO), "torch.float32"), ((B,), "torch.uint8"), ((B,), "torch.int64"), ((B, S), "torch.float32"),
        ((B,), "torch.float32"), ((ITERS + 1, B), "torch.float32") if trace else None, ((ITERS + 1, B), "torch.int64") if trace else None]
    # keys are drawn in the documented order, dither first, then FeCo's: one draw of each counter, both base keys readable
    assert (m.last_fused_seed, m.last_fused_feco_seed) == (DITHER_KEY, FECO_KEY)
    assert (m._draw, m._def_draw, feco.calls) == (1, 1, 1)


def test_the_dither_key_is_drawn_before_fecos():
    m = _model(xv_plda)
    order = []
    dither, feco_params = m._pgd_dither, m._feco_params
    m._pgd_dither = lambda p: (order.append("dither"), dither(p))[1]
    m._feco_params = lambda f, t: (order.append("feco"), feco_params(f, t))[1]
    loss, grad_sign = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    m.pgd_run_feco(torch.zeros(B, 1, T_FECO), torch.arange(B) % S, torch.full((B, 1, 1), -1.0), torch.full((B, 1, 1), 1.0), loss, STEP,
                   ITERS, grad_sign, FeCoDefense(0.5), EOT, EOT_BATCH)
    assert order == ["dither", "feco"]


def test_a_level_the_loop_does_not_have_is_refused_before_any_draw_and_any_call():
    m = _model(xv_plda)
    feco = FeCoDefense(0.5, init="random")
    loss, grad_sign = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    for level in (0, 3):
        with pytest.raises(ValueError):
            m.pgd_run_feco(torch.zeros(B, 1, T_FECO), torch.arange(B) % S, torch.full((B, 1, 1), -1.0), torch.full((B, 1, 1), 1.0), loss,
                           STEP, ITERS, grad_sign, feco, EOT, EOT_BATCH, level=level)
    assert m.ctx.calls == [] and (m._draw, m._def_draw, feco.calls) == (0, 0, 0)
    assert not hasattr(m, "last_fused_seed") and not hasattr(m, "last_fused_feco_seed")


def test_the_model_says_what_the_route_reads():
    m = _model(xv_plda)
    assert m.feco_loop_levels == (1, 2) and m.feco_loop_rekeys is True and callable(m.pgd_run_feco)
