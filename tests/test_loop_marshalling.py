"""What the six public device-loop methods (``xv_plda.pgd_run`` / ``pgd_run_defended``, ``audionet_csine.pgd_run`` / ``pgd_run_feco`` /
``pgd_run_defended`` / ``pgd_run_defended_feco``) hand to the C ABI, without a GPU: the models are built with ``cls.__new__`` on
the CPU and a recording stand-in for the engine context.

A record is the C entry's name and its arguments -- pointers reduced to NULL / not NULL, scalars verbatim, ``sg_pgd_params``,
``sg_feco_params`` and every ``sg_wav_stage`` expanded to their field values -- plus the shapes of what the method returns and
the noise bookkeeping after the call (``last_fused_seed``, ``last_fused_defense_seeds``, ``_draw``, ``_def_draw``, ``feco.calls``).
``EXPECTED`` holds the records captured ONCE on the commit before the marshalling moved into ``EngineOps`` (each model then
carried its own copy), by running ``record`` below against that commit.
"""
import ctypes

import pytest
import torch

from speakerguard_amd import _native as N
from speakerguard_amd.attack.utils import resolve_loss
from speakerguard_amd.defense import AS, AT, LPF
from speakerguard_amd.defense.feature_level import FeCoDefense
from speakerguard_amd.model.audionet_csine import audionet_csine
from speakerguard_amd.model.xv_plda import xv_plda

B, T, T_FECO, S = 3, 5043, 10081, 5
STEP, ITERS, EOT, EOT_BATCH = 0.0004, 5, 4, 2


class _Recorder:
    """stands in for ``N.Context``: appends (entry name, arguments) and returns"""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, [_plain(a) for a in args]))


def _struct(s):
    if isinstance(s, N.WavStage):
        return {"tag": s.tag, "u": _struct(s.u.filter if s.tag == N.SG_WAV_STAGE_FILTER else s.u.defense)}
    return {name: _plain(getattr(s, name)) for name, _ in s._fields_}


def _plain(a):
    if a is None:
        return "NULL"
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "NULL"
    if isinstance(a, ctypes.Structure):
        return _struct(a)
    if isinstance(a, ctypes.Array):
        return [_plain(v) for v in a]
    if isinstance(a, ctypes._Pointer):
        return "ptr" if a else "NULL"
    if hasattr(a, "_obj"):  # ctypes.byref(struct)
        return _plain(a._obj)
    assert isinstance(a, (int, float, str)), type(a)
    return a


def _model(cls):
    m = cls.__new__(cls)
    m.device, m.ctx, m.num_spks = torch.device("cpu"), _Recorder(), S
    m._stream = lambda: "stream"
    if cls is xv_plda:
        m.dither, m.dither_seed = 1.0, 9
    m.begin_attack()
    m.begin_batch(40, 1)
    return m


def _chain():
    return [AS(3), AT(25, seed=5), LPF(5000)]


def _chain_for_feco():
    return [AS(3), LPF(5000)]


def _feco():
    return FeCoDefense(0.5, init='random', seed=7)


CALLS = {
    # name: (model, method, what goes between grad_sign and eot_size, T)
    "xv.pgd_run": (xv_plda, "pgd_run", lambda: (), T),
    "xv.pgd_run_defended": (xv_plda, "pgd_run_defended", lambda: (_chain(),), T),
    "an.pgd_run": (audionet_csine, "pgd_run", lambda: (), T),
    "an.pgd_run_feco": (audionet_csine, "pgd_run_feco", lambda: (_feco(),), T_FECO),
    "an.pgd_run_defended": (audionet_csine, "pgd_run_defended", lambda: (_chain(),), T),
    "an.pgd_run_defended_feco": (audionet_csine, "pgd_run_defended_feco", lambda: (_chain_for_feco(), _feco()), T_FECO),
}


def record(name, trace):
    cls, method, extra, t = CALLS[name]
    m, extra = _model(cls), extra()
    loss, grad_sign = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, y = torch.zeros(B, 1, t), torch.arange(B) % S
    out = getattr(m, method)(x, y, torch.full((B, 1, 1), -1.0), torch.full((B, 1, 1), 1.0), loss, STEP, ITERS, grad_sign, *extra,
                             EOT, EOT_BATCH, trace=trace)
    assert out[0] is not x and out[0].data_ptr() != x.data_ptr() and torch.equal(out[0], x)  # the loop works on a copy
    feco = [e for e in extra if isinstance(e, FeCoDefense)]
    return {
        "calls": m.ctx.calls,
        "returns": [None if o is None else (tuple(o.shape), str(o.dtype)) for o in out],
        "last_fused_seed": getattr(m, "last_fused_seed", None),
        "last_fused_defense_seeds": getattr(m, "last_fused_defense_seeds", None),
        "_draw": m._draw, "_def_draw": m._def_draw,
        "feco.calls": feco[0].calls if feco else None,
    }


EXPECTED = {
    ('an.pgd_run', False): {
        "calls": [('sg_an_pgd_run', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': None,
        'last_fused_defense_seeds': None,
        '_draw': 0,
        '_def_draw': 0,
        'feco.calls': None,
    },
    ('an.pgd_run', True): {
        "calls": [('sg_an_pgd_run', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': None,
        'last_fused_defense_seeds': None,
        '_draw': 0,
        '_def_draw': 0,
        'feco.calls': None,
    },
    ('an.pgd_run_defended', False): {
        "calls": [('sg_an_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 0,
              'u': {'kind': 3, 'param': 25.0, 'seed': 13357288130501126842, 'index_base': 40, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            3, 'NULL', 'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': None,
        'last_fused_defense_seeds': [None, 13357288130501126842, None],
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': None,
    },
    ('an.pgd_run_defended', True): {
        "calls": [('sg_an_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 0,
              'u': {'kind': 3, 'param': 25.0, 'seed': 13357288130501126842, 'index_base': 40, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            3, 'NULL', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': None,
        'last_fused_defense_seeds': [None, 13357288130501126842, None],
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': None,
    },
    ('an.pgd_run_defended_feco', False): {
        "calls": [('sg_an_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 10081,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            2,
            {'k': 32, 'max_iter': 10, 'random_init': 1, 'seed': 6642029681321278496, 'index_base': 40},
            'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 10081), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': 6642029681321278496,
        'last_fused_defense_seeds': [None, None],
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': 1,
    },
    ('an.pgd_run_defended_feco', True): {
        "calls": [('sg_an_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 10081,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            2,
            {'k': 32, 'max_iter': 10, 'random_init': 1, 'seed': 6642029681321278496, 'index_base': 40},
            'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 10081), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': 6642029681321278496,
        'last_fused_defense_seeds': [None, None],
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': 1,
    },
    ('an.pgd_run_feco', False): {
        "calls": [('sg_an_pgd_run_feco', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 10081,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            {'k': 32, 'max_iter': 10, 'random_init': 1, 'seed': 6642029681321278496, 'index_base': 40},
            'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 10081), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': 6642029681321278496,
        'last_fused_defense_seeds': None,
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': 1,
    },
    ('an.pgd_run_feco', True): {
        "calls": [('sg_an_pgd_run_feco', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 10081,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 0.0, 'seed': 0, 'index_base': 0, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            {'k': 32, 'max_iter': 10, 'random_init': 1, 'seed': 6642029681321278496, 'index_base': 40},
            'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 10081), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': 6642029681321278496,
        'last_fused_defense_seeds': None,
        '_draw': 0,
        '_def_draw': 1,
        'feco.calls': 1,
    },
    ('xv.pgd_run', False): {
        "calls": [('sg_xv_pgd_run', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 1.0, 'seed': 16376009521482754076, 'index_base': 40, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': 16376009521482754076,
        'last_fused_defense_seeds': None,
        '_draw': 1,
        '_def_draw': 0,
        'feco.calls': None,
    },
    ('xv.pgd_run', True): {
        "calls": [('sg_xv_pgd_run', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 1.0, 'seed': 16376009521482754076, 'index_base': 40, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': 16376009521482754076,
        'last_fused_defense_seeds': None,
        '_draw': 1,
        '_def_draw': 0,
        'feco.calls': None,
    },
    ('xv.pgd_run_defended', False): {
        "calls": [('sg_xv_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 1.0, 'seed': 16376009521482754076, 'index_base': 40, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 0,
              'u': {'kind': 3, 'param': 25.0, 'seed': 13357288130501126842, 'index_base': 40, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            3, 'ptr', 'ptr', 'ptr', 'ptr', 'NULL', 'NULL', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), None, None],
        'last_fused_seed': 16376009521482754076,
        'last_fused_defense_seeds': [None, 13357288130501126842, None],
        '_draw': 1,
        '_def_draw': 1,
        'feco.calls': None,
    },
    ('xv.pgd_run_defended', True): {
        "calls": [('sg_xv_pgd_run_defended', [
            'ptr', 'ptr', 'ptr', 'ptr', 3, 5043,
            {'loss': {'loss': 0, 'task': 0, 'targeted': 0, 'clip_max': 0, 'confidence': 0.0, 'threshold': 0.0, 'coef_dev': 'NULL'},
             'step_size': 0.00039999998989515007,
             'max_iter': 5,
             'grad_sign': 1,
             'eot_size': 4,
             'eot_batch_size': 2,
             'dither': {'dither': 1.0, 'seed': 16376009521482754076, 'index_base': 40, 'noise_dev': 'NULL', 'row_base': 0, 'rep_rows': 0}},
            [{'tag': 0, 'u': {'kind': 1, 'param': 3.0, 'seed': 0, 'index_base': 0, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 0,
              'u': {'kind': 3, 'param': 25.0, 'seed': 13357288130501126842, 'index_base': 40, 'row_base': 0, 'rep_rows': 0, 'noise_dev': 'NULL'}},
             {'tag': 1, 'u': {'n_sections': 6, 'sos': 'ptr', 'clip_mode': 0, 'bits': 16, 'clip_lo': 0.0, 'clip_hi': 0.0}}],
            3, 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'stream',
        ])],
        'returns': [((3, 1, 5043), 'torch.float32'), ((3,), 'torch.uint8'), ((3,), 'torch.int64'), ((3, 5), 'torch.float32'),
                     ((3,), 'torch.float32'), ((6, 3), 'torch.float32'), ((6, 3), 'torch.int64')],
        'last_fused_seed': 16376009521482754076,
        'last_fused_defense_seeds': [None, 13357288130501126842, None],
        '_draw': 1,
        '_def_draw': 1,
        'feco.calls': None,
    },
}


def test_every_public_loop_method_is_pinned():
    assert sorted(EXPECTED) == sorted((name, trace) for name in CALLS for trace in (False, True))
    assert not hasattr(xv_plda, "pgd_run_feco") and not hasattr(xv_plda, "pgd_run_defended_feco")


@pytest.mark.parametrize("trace", [False, True], ids=["plain", "trace"])
@pytest.mark.parametrize("name", sorted(CALLS))
def test_what_the_loop_methods_hand_to_the_engine(name, trace):
    got = record(name, trace)
    want = EXPECTED[(name, trace)]
    assert len(got["calls"]) == 1 and got["calls"][0][0] == want["calls"][0][0]
    for i, (g, w) in enumerate(zip(got["calls"][0][1], want["calls"][0][1])):
        assert g == w, "argument %d of %s" % (i, want["calls"][0][0])
    assert got == want


@pytest.mark.parametrize("cls", [xv_plda, audionet_csine], ids=["xv", "an"])
@pytest.mark.parametrize("method,extra", [
    ("pgd_run_defended", lambda: ([],)),
    ("pgd_run_defended", lambda: ([AS(3)] * 9,)),
    ("pgd_run_defended_feco", lambda: ([], _feco())),
    ("pgd_run_defended_feco", lambda: ([AS(3)] * 9, _feco())),
    ("pgd_run_defended_feco", lambda: ([AS(3), AT(25)], _feco())),
], ids=["no-stage", "9-stages", "no-stage+feco", "9-stages+feco", "AT+feco"])
def test_host_refusals_come_before_any_draw_and_any_call(cls, method, extra):
    if not hasattr(cls, method):
        assert cls is xv_plda and method == "pgd_run_defended_feco"  # the x-vector model has no FeCo loop, and must not gain one
        return
    m, extra = _model(cls), extra()
    loss, grad_sign = resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, y = torch.zeros(B, 1, T_FECO), torch.arange(B) % S
    with pytest.raises(ValueError):
        getattr(m, method)(x, y, torch.full((B, 1, 1), -1.0), torch.full((B, 1, 1), 1.0), loss, STEP, ITERS, grad_sign, *extra,
                           EOT, EOT_BATCH)
    assert m.ctx.calls == [] and (m._draw, m._def_draw) == (0, 0)
    assert not hasattr(m, "last_fused_seed") and not hasattr(m, "last_fused_defense_seeds")
    assert all(e.calls == 0 for e in extra if isinstance(e, FeCoDefense))
