"""The defended iv_plda without a GPU: ``FeCoDefense.fwd`` routes by width (the old entries with their old argument lists up to
64 columns, sg_feco_kmeans_compress_wide from 65 to 128, the cosine distance never), an iv-like base keeps every attack on the
step loop, and ``defended_model``'s gradient routes walk the base model's own levels in ``process_sequential``'s order."""
import pytest
import torch

import speakerguard_amd.defense.feature_level as FL
from speakerguard_amd import _native as N
from speakerguard_amd.attack.CWinf import CWinf
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.attack.utils import SEC4SR_CrossEntropy
from speakerguard_amd.defense import AS
from speakerguard_amd.defense.feature_level import FeCoDefense, WarpedFeCoDefense
from speakerguard_amd.model import iv_plda as M
from speakerguard_amd.model._engine_ops import REP_KEY_STRIDE
from speakerguard_amd.model.defended_model import defended_model
from test_defended_loop_host import S, _StepBase
from test_feco_cos_host import FLAG_CELLS


# ---- FeCoDefense.fwd by width ----------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: ``fwd`` refuses host tensors before it routes"""
    is_cuda = property(lambda self: True)


class _Ctx:
    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name,) + tuple(getattr(a, "value", a) for a in args))  # (c_uint64 keys by value)


@pytest.fixture
def ctx(monkeypatch):
    c = _Ctx()
    monkeypatch.setattr(FL, "_context", lambda device: c)
    monkeypatch.setattr(N, "current_stream_ptr", lambda device: "stream")
    monkeypatch.setattr(N, "_ptr", lambda t: "ptr")
    return c


def _feat(B, F, D):
    return torch.zeros(B, F, D).as_subclass(_OnDevice)


def test_the_library_names_the_wide_entry():
    assert "sg_feco_kmeans_compress_wide" in N.EXPORTS and FL.WIDE_MIN_D == 65


@pytest.mark.parametrize("D", [24, 30, 64])
def test_narrow_widths_keep_their_entry_and_arguments(ctx, D):
    FeCoDefense(0.5).fwd(_feat(2, 40, D))
    assert ctx.calls == [("sg_feco_kmeans_compress", "ptr", 2, 40, D, 20, 10, 0, 0, 0, 1, "ptr", "ptr", "ptr", "stream")]
    ctx.calls.clear()
    FeCoDefense(0.5, other_param='cos').fwd(_feat(2, 40, D))
    assert ctx.calls == [("sg_feco_kmeans_compress_metric", "ptr", 2, 40, D, 20, 10, N.SG_FECO_COS, 0, 0, 0, 1, 0, "ptr", "ptr", "ptr",
                          "stream")]


@pytest.mark.parametrize("D", [65, 72, 128])
def test_wide_widths_take_the_wide_entry(ctx, D):
    FeCoDefense(0.5).fwd(_feat(2, 40, D))
    assert ctx.calls == [("sg_feco_kmeans_compress_wide", "ptr", 2, 40, D, 20, 10, 0, 0, 0, "ptr", "ptr", "ptr", "stream")]
    ctx.calls.clear()
    if D % 2 == 0:  # (:183: the cosine distance asserts an even width)
        FeCoDefense(0.5, other_param='cos').fwd(_feat(2, 40, D))
        assert [c[0] for c in ctx.calls] == ["sg_feco_kmeans_compress_metric"]  # ... which refuses D > 64 on the device


def test_keys_and_repeats_are_handled_alike(ctx):
    """the randomised defense inside a model call: (index_base, row_base, rep_rows) cuts the rows into one launch per EOT repeat,
    repeat r keyed seed + r * REP_KEY_STRIDE and the rows by their utterance -- the same cuts and keys at 64 and 72 columns"""
    seen = {}
    for D in (64, 72):
        ctx.calls.clear()
        d = FeCoDefense(0.5, init='random', seed=3)
        d.fwd(_feat(4, 40, D), seed=77, row_keys=(100, 2, 3))
        assert d.calls == 1
        seen[D] = [(c[0], c[2], c[7], c[8], c[9]) for c in ctx.calls]
    m64 = (1 << 64) - 1
    assert seen[64] == [("sg_feco_kmeans_compress", 1, 1, 77, 102), ("sg_feco_kmeans_compress", 3, 1, (77 + REP_KEY_STRIDE) & m64, 100)]
    assert seen[72] == [("sg_feco_kmeans_compress_wide", 1, 1, 77, 102), ("sg_feco_kmeans_compress_wide", 3, 1, (77 + REP_KEY_STRIDE) & m64, 100)]
    ctx.calls.clear()
    d = FeCoDefense(0.5, init='random', seed=3)
    d.fwd(_feat(2, 40, 72))
    d.fwd(_feat(2, 40, 72))
    assert [c[8] for c in ctx.calls] == [d.call_seed(0), d.call_seed(1)] and ctx.calls[0][9] == 0


# ---- an iv-like base keeps the step loop ------------------------------------------------------------------------------------------
class _IvLikeBase(_StepBase):
    """levels 0 .. 3; the loop methods exist only to refuse; ``device_loops = False`` (iv_plda)"""
    allowed_flags = [0, 1, 2, 3]
    device_loops = False
    dither = 0.0

    def pgd_run(self, *a, **kw):
        raise NotImplementedError(M._NO_GRAD % "pgd_run")

    pgd_run_defended = pgd_run_feco = pgd_run


IV_DEFENSES = {
    "feco-3": lambda: [(3, FeCoDefense(0.5))],
    "feco-2": lambda: [(2, FeCoDefense(0.5))],
    "feco-1": lambda: [(1, FeCoDefense(0.5))],
    "feco-1-random": lambda: [(1, FeCoDefense(0.5, init='random'))],
    "feco-1+3": lambda: [(1, FeCoDefense(0.5)), (3, FeCoDefense(0.5))],
    "chain": lambda: [(0, AS(3))],
    "chain+feco-3": lambda: [(0, AS(3)), (3, FeCoDefense(0.5))],
    "warped-1": lambda: [(1, WarpedFeCoDefense(0.5))],
    "none": lambda: None,
}


@pytest.mark.parametrize("name", sorted(IV_DEFENSES))
@pytest.mark.parametrize("attack", [PGD, CWinf])
def test_an_iv_like_base_never_takes_a_device_loop(name, attack):
    for flag, value in FLAG_CELLS:
        for n in (1, 2, 64):
            atk = attack(defended_model(_IvLikeBase(), IV_DEFENSES[name]()), verbose=0)
            if flag is not None:
                setattr(atk, flag, value)
            assert atk._device_route(n) is None, (flag, value, n)


def test_iv_plda_says_so():
    assert M.iv_plda.device_loops is False and M.iv_plda.allowed_flags == [0, 1, 2, 3]
    assert not hasattr(M.iv_plda, "feco_loop_levels")


# ---- defended_model on a recording double of iv_plda ------------------------------------------------------------------------------
class _RecIv:
    """iv_plda's stage methods as a recorder: level-1 features are 24 wide, levels 2 and 3 are 72 wide, any frame count"""
    allowed_flags = [0, 1, 2, 3]
    threshold = 0.0
    device = torch.device("cpu")
    WIDTH = {1: 24, 2: 72, 3: 72}

    def __init__(self, white_box=True):
        self.log, self.white_box, self._keys = [], white_box, 0

    def frontend_forward(self, x, dither_seed=None):
        self.log.append("front")
        return torch.zeros(x.shape[0], 10, 24), ("saved", x.shape)

    def frontend_backward(self, saved, g):
        assert saved[0] == "saved" and g.shape[2] == 24
        self.log.append("front_bwd")
        return torch.ones(saved[1])

    def comput_feat_from_feat(self, feats, ori_flag=1, des_flag=2):
        assert des_flag == ori_flag + 1 and feats.shape[2] == self.WIDTH[ori_flag]
        self.log.append("up%d%d" % (ori_flag, des_flag))
        return torch.zeros(feats.shape[0], feats.shape[1], self.WIDTH[des_flag])

    def feat_from_feat_backward(self, g, ori_flag, des_flag):
        assert des_flag == ori_flag + 1 and g.shape[2] == self.WIDTH[des_flag]
        self.log.append("down%d%d" % (des_flag, ori_flag))
        return torch.zeros(g.shape[0], g.shape[1], self.WIDTH[ori_flag])

    def compute_feat(self, x, flag=1):
        return torch.zeros(x.shape[0], 10, self.WIDTH[flag])

    def next_dither_seed(self):
        self._keys += 1
        return 1000 + self._keys

    def forward(self, x, flag=0, dither_seed=None, **kw):
        self.log.append("forward%d%s" % (flag, "" if dither_seed is None else "@%d" % dither_seed))
        return torch.zeros(x.shape[0], S)

    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, dither_seed=None, **kw):
        if want_grad and not self.white_box:
            raise NotImplementedError(M._NO_GRAD % "loss_grad(want_grad=True)")
        if flag:
            assert x.shape[2] == self.WIDTH[flag]
        self.log.append("loss_grad%d%s" % (flag, "" if dither_seed is None else "@%d" % dither_seed))
        n = x.shape[0]
        return torch.zeros(n, dtype=torch.int64), torch.zeros(n, S), torch.zeros(n), torch.ones_like(x)


class _RecDefense:
    """halves the frame count at a feature level, like FeCo; the waveform keeps its shape"""

    def __init__(self, name, log, level):
        self.name, self.log, self.level = name, log, level

    def fwd(self, x):
        self.log.append("fwd:" + self.name)
        return (x if self.level == 0 else x[:, :x.shape[1] // 2]), x.shape

    def bwd(self, saved, g):
        self.log.append("bwd:" + self.name)
        return torch.ones(saved)

    def __call__(self, x):
        return self.fwd(x)[0]


SEQUENTIAL = {
    (0,): ["fwd:d0", "loss_grad0", "bwd:d0"],
    (1,): ["front", "fwd:d1", "loss_grad1", "bwd:d1", "front_bwd"],
    (3,): ["front", "up12", "up23", "fwd:d3", "loss_grad3", "bwd:d3", "down32", "down21", "front_bwd"],
    (1, 3): ["front", "fwd:d1", "up12", "up23", "fwd:d3", "loss_grad3", "bwd:d3", "down32", "down21", "bwd:d1", "front_bwd"],
    (0, 2, 3): ["fwd:d0", "front", "up12", "fwd:d2", "up23", "fwd:d3", "loss_grad3", "bwd:d3", "down32", "bwd:d2", "down21", "front_bwd",
                "bwd:d0"],
}


@pytest.mark.parametrize("levels", sorted(SEQUENTIAL))
def test_sequential_order_walks_the_models_levels(levels):
    bm = _RecIv()
    dm = defended_model(bm, [(f, _RecDefense("d%d" % f, bm.log, f)) for f in levels])
    x = torch.zeros(2, 1, 64)
    dec, sc, loss, g = dm.loss_grad(x, torch.zeros(2, dtype=torch.int64), SEC4SR_CrossEntropy())
    assert bm.log == SEQUENTIAL[levels]
    assert g.shape == x.shape and sc.shape == (2, S)


def test_two_defenses_of_a_level_run_back_in_reverse():
    bm = _RecIv()
    dm = defended_model(bm, [(3, _RecDefense("a", bm.log, 3)), (3, _RecDefense("b", bm.log, 3))])
    dm.loss_grad(torch.zeros(2, 1, 64), torch.zeros(2, dtype=torch.int64), SEC4SR_CrossEntropy())
    assert bm.log == ["front", "up12", "up23", "fwd:a", "fwd:b", "loss_grad3", "bwd:b", "bwd:a", "down32", "down21", "front_bwd"]


def test_average_order_walks_the_models_levels(monkeypatch):
    import speakerguard_amd.attack.utils as U
    bm = _RecIv()
    monkeypatch.setattr(U, "loss_dscores", lambda model, mean, y, spec: (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.ones(2, S)))
    monkeypatch.setattr(U, "ScoreVJP", lambda coef: ("vjp", coef))
    dm = defended_model(bm, [(0, _RecDefense("d0", bm.log, 0)), (2, _RecDefense("d2", bm.log, 2))], order='average')
    x = torch.zeros(2, 1, 64)
    dec, mean, loss, g = dm.loss_grad(x, torch.zeros(2, dtype=torch.int64), SEC4SR_CrossEntropy())
    assert bm.log == ["front", "up12", "fwd:d0", "forward0@1001", "fwd:d2", "forward2", "loss_grad0@1001", "bwd:d0", "loss_grad2", "bwd:d2",
                      "down21", "front_bwd"]
    assert g.shape == x.shape


@pytest.mark.parametrize("levels", [(0,), (3,), (1, 3)])
def test_forward_only_model_raises_the_ivector_message(levels):
    bm = _RecIv(white_box=False)
    dm = defended_model(bm, [(f, _RecDefense("d%d" % f, bm.log, f)) for f in levels])
    with pytest.raises(NotImplementedError, match="the i-vector gradient is not built"):
        dm.loss_grad(torch.zeros(2, 1, 64), torch.zeros(2, dtype=torch.int64), SEC4SR_CrossEntropy())
    assert not [c for c in bm.log if c.startswith("bwd") or c.startswith("down") or c == "front_bwd"]


def test_the_real_forward_only_model_raises_it_too():
    m = object.__new__(M.iv_plda)
    m.threshold = 0.0
    dm = defended_model(m, [(0, _RecDefense("d0", [], 0))])
    with pytest.raises(NotImplementedError, match="the i-vector gradient is not built"):
        dm.loss_grad(torch.zeros(2, 1, 64), torch.zeros(2, dtype=torch.int64), SEC4SR_CrossEntropy())
    for call in (lambda: m.frontend_backward(None, None), lambda: m.feat_from_feat_backward(None, 2, 3)):
        with pytest.raises(NotImplementedError, match="the i-vector gradient is not built"):
            call()
    for name in ("frontend_forward", "frontend_backward", "feat_from_feat_backward"):
        assert callable(getattr(M.iv_plda, name))
    from speakerguard_amd.model.xv_plda import xv_plda
    assert callable(xv_plda.feat_from_feat_backward) and callable(xv_plda.cmvn_backward)
