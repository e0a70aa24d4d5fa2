"""Host logic of batches of unequal lengths (``lengths=``), without a GPU: ``audio_io.pad_batch``, how FGSM / PGD / CWinf cut,
mask and hand on the lengths, what the x-vector model hands to the C ABI with and without them, every refusal, and
``ShardedAttack`` at gloo world 2.

The engine is the CPU double of tests/engine_doubles.py around the toy model, made length-aware the way the engine is: row b
is scored as utterance b alone (its own samples, whatever the padding holds), and its gradient is 0 behind them.  The marshalling
records are those of tests/test_loop_marshalling.py: a call without lengths must leave exactly the literal lists pinned there.
"""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from engine_doubles import AutogradEngine
from speakerguard_amd.attack.CWinf import CWinf
from speakerguard_amd.attack.FGSM import FGSM
from speakerguard_amd.attack.PGD import PGD
from speakerguard_amd.audio_io import pad_batch
from speakerguard_amd.shard import ShardedAttack
from toy_model import ToyModel, toy_inputs

LENGTHS = (800, 600, 720, 440, 655)
T_TOY = 800


class RaggedToyEngine(AutogradEngine):
    """the toy model behind the engine protocol with ``lengths=``; records (entry, rows, width, lengths) of every call"""
    takes_lengths = True
    allowed_flags = [0]

    def __init__(self):
        toy = ToyModel().eval()
        for p in toy.parameters():
            p.requires_grad_(False)
        super().__init__(toy, per_row=True)
        self.calls, self.updates = [], []

    @staticmethod
    def _keep(x, lengths):
        return (torch.arange(x.shape[2]).unsqueeze(0) < lengths.to(torch.int64).unsqueeze(1)).unsqueeze(1)

    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True, lengths=None):
        self.calls.append(("loss_grad", x.shape[0], x.shape[2], None if lengths is None else lengths.tolist()))
        if lengths is None:
            return super().loss_grad(x, y, loss_spec, flag, want_grad)
        assert lengths.dtype == torch.int32 and int(lengths.max()) == x.shape[2], "the longest utterance fills the row"
        keep = self._keep(x, lengths)
        full = torch.nn.functional.pad(torch.where(keep, x, torch.zeros(())), (0, T_TOY - x.shape[2]))
        dec, sc, loss, grad = super().loss_grad(full, y, loss_spec, flag, want_grad)
        if grad is not None:
            grad = torch.where(keep, grad[:, :, :x.shape[2]], torch.zeros(()))
        return dec, sc, loss, grad

    def pgd_update(self, x, grad, lower, upper, step_size, grad_sign):
        self.updates.append((x.clone(), lower.clone(), upper.clone()))
        return super().pgd_update(x, grad, lower, upper, step_size, grad_sign)


def _data(fill=0.0):
    full = toy_inputs(B=len(LENGTHS), T=T_TOY, seed=5)
    x, lens = pad_batch([full[b, :, :t] for b, t in enumerate(LENGTHS)])
    for b, t in enumerate(LENGTHS):
        x[b, 0, t:] = fill
    with torch.no_grad():
        y = ToyModel().eval().make_decision(pad_batch([full[b, :, :t] for b, t in enumerate(LENGTHS)])[0])[0]
    return x, lens, y


def _attack(cls=PGD, **kw):
    args = dict(epsilon=0.01, step_size=0.002, max_iter=4, batch_size=2, verbose=0)
    if cls is FGSM:
        args = dict(epsilon=0.01, batch_size=2, verbose=0)
    args.update(kw)
    return cls(RaggedToyEngine(), **args)


# ------------------------------------------------------------------------------ pad_batch
def test_pad_batch():
    a, b, c = torch.arange(1.0, 6.0), torch.arange(1.0, 4.0).view(1, 3), torch.ones(7, dtype=torch.float64)
    x, lens = pad_batch([a, b, c])
    assert x.shape == (3, 1, 7) and x.dtype == torch.float32 and lens.dtype == torch.int32 and lens.tolist() == [5, 3, 7]
    assert x[0, 0].tolist() == [1, 2, 3, 4, 5, 0, 0] and x[1, 0].tolist() == [1, 2, 3, 0, 0, 0, 0] and x[2, 0].tolist() == [1] * 7
    assert not lens.is_cuda and pad_batch([b])[0].shape == (1, 1, 3)
    for bad in ([], [torch.zeros(2, 5)], [torch.zeros(1, 1, 5)], [torch.zeros(0)], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            pad_batch(bad)


# ------------------------------------------------------------------------------ chunks, bounds, masks
@pytest.mark.parametrize("cls", [FGSM, PGD, CWinf])
def test_chunks_are_cut_to_their_longest_utterance_and_rows_equal_the_solo_attacks(cls):
    x, lens, y = _data(fill=0.7)
    atk = _attack(cls)
    adv, succ = atk.attack(x, y, lengths=lens)
    eng = atk.model
    assert adv.shape == x.shape and len(succ) == len(LENGTHS)
    # chunks of 2, 2, 1 utterances: every call as wide as ITS longest utterance, with its slice of the lengths
    want = [(2, 800, [800, 600]), (2, 720, [720, 440]), (1, 655, [655])]
    seen = [c[1:] for c in eng.calls]
    per_chunk = len(seen) // 3
    assert seen == [w for w in want for _ in range(per_chunk)] and per_chunk == atk.max_iter + 1
    eps = atk.epsilon
    for b, t in enumerate(LENGTHS):
        assert not adv[b, :, t:].any(), "the padding of the result is 0 whatever the caller put there"
        assert 0 < (adv[b, :, :t] - x[b, :, :t]).abs().max() <= eps + 1e-7
        solo = _attack(cls, batch_size=1)
        a1, s1 = solo.attack(x[b:b + 1, :, :t].contiguous(), y[b:b + 1], lengths=lens[b:b + 1])
        assert torch.equal(a1[0], adv[b, :, :t]) and s1[0] == succ[b], b
    # the bounds are 0 in the padding, the start point too
    for xs, lo, hi in eng.updates:
        n, width = xs.shape[0], xs.shape[2]
        chunk = next(w[2] for w in want if w[0] == n and w[1] == width)
        for r, t in enumerate(chunk):
            assert not lo[r, :, t:].any() and not hi[r, :, t:].any() and not xs[r, :, t:].any()
            assert (hi[r, :, :t] - lo[r, :, :t]).min() > 0
    # padding content does not matter
    adv0, succ0 = _attack(cls).attack(_data(fill=0.0)[0], y, lengths=lens)
    assert torch.equal(adv0, adv) and succ0 == succ


def test_random_restarts_draw_no_noise_into_the_padding():
    x, lens, y = _data(fill=0.7)
    np.random.seed(3)
    atk = _attack(PGD, num_random_init=2, batch_size=5)
    adv, _ = atk.attack(x, y, lengths=lens)
    starts = [u[0] for u in atk.model.updates[::atk.max_iter]]  # the iterate before the first step of each restart
    assert len(starts) == 2 and not torch.equal(starts[0], starts[1])
    for s in starts:
        for b, t in enumerate(LENGTHS):
            assert not s[b, :, t:].any() and (s[b, :, :t] - x[b, :, :t]).abs().max() > 0
    for b, t in enumerate(LENGTHS):
        assert not adv[b, :, t:].any()


def test_without_lengths_the_engine_is_called_as_before():
    """an engine double whose methods know no ``lengths`` keyword (tests/engine_doubles.py as it stands) still works"""
    toy = ToyModel().eval()
    for p in toy.parameters():
        p.requires_grad_(False)
    x = toy_inputs(B=3, T=T_TOY, seed=5)
    y = toy.make_decision(x)[0]
    adv, succ = PGD(AutogradEngine(toy), epsilon=0.01, step_size=0.002, max_iter=2, batch_size=2, verbose=0).attack(x, y)
    assert adv.shape == x.shape and len(succ) == 3


# ------------------------------------------------------------------------------ what the model hands to the C ABI
def test_marshalling_without_lengths_is_the_pinned_one_and_with_lengths_inserts_the_two_copies():
    import test_loop_marshalling as M
    from speakerguard_amd.model.xv_plda import xv_plda
    for trace in (False, True):
        assert M.record("xv.pgd_run", trace) == M.EXPECTED["xv.pgd_run", trace]  # (the literal lists of that file)
        m = M._model(xv_plda)
        loss, grad_sign = M.resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
        x, y = torch.zeros(M.B, 1, M.T), torch.arange(M.B) % M.S
        lens = torch.tensor([M.T, M.T - 1, 5040], dtype=torch.int32)
        out = m.pgd_run(x, y, torch.full((M.B, 1, 1), -1.0), torch.full((M.B, 1, 1), 1.0), loss, M.STEP, M.ITERS, grad_sign, M.EOT,
                        M.EOT_BATCH, trace=trace, lengths=lens)
        want = copy.deepcopy(M.EXPECTED["xv.pgd_run", trace]["calls"])
        name, args = want[0]
        assert name == "sg_xv_pgd_run"
        assert m.ctx.calls == [("sg_xv_pgd_run_ragged", args[:4] + ["ptr", "ptr"] + args[4:])]
        assert [None if o is None else tuple(o.shape) for o in out] == [None if r is None else r[0] for r in M.EXPECTED["xv.pgd_run", trace]["returns"]]
        assert (m._draw, m.last_fused_seed) == (1, M.EXPECTED["xv.pgd_run", trace]["last_fused_seed"])


def test_loss_grad_and_make_decision_entries_with_and_without_lengths():
    import test_loop_marshalling as M
    from speakerguard_amd.model.xv_plda import xv_plda
    loss, _ = M.resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, y = torch.zeros(M.B, 1, M.T), torch.arange(M.B) % M.S
    lens = torch.tensor([M.T, M.T - 1, 5040], dtype=torch.int32)
    m = M._model(xv_plda)
    m.dim, m._has_enroll = 7, True
    m.loss_grad(x, y, loss)
    m.make_decision(x)
    plain = m.ctx.calls
    assert [c[0] for c in plain] == ["sg_xv_loss_grad", "sg_xv_forward"]
    m2 = M._model(xv_plda)
    m2.dim, m2._has_enroll = 7, True
    m2.loss_grad(x, y, loss, lengths=lens)
    m2.make_decision(x, lengths=lens)
    m2.loss_grad(x, y, loss, lengths=lens)  # (the same tensor again: no new check, same call)
    (n1, a1), (n2, a2), (n3, a3) = m2.ctx.calls
    assert (n1, n2, n3) == ("sg_xv_loss_grad_ragged", "sg_xv_forward_ragged", "sg_xv_loss_grad_ragged")
    # x, [lengths_dev, lengths_host,] y, B, T, [flag,] loss, dither, outputs..., stream
    assert a1[:1] + a1[3:6] + a1[6:] == plain[0][1][:4] + plain[0][1][5:6] + [dict(plain[0][1][6], seed=a1[7]["seed"])] + plain[0][1][7:]
    assert a1[1:3] == ["ptr", "ptr"] and a2[1:3] == ["ptr", "ptr"]
    assert a2[:1] + a2[3:5] + a2[6:] == plain[1][1][:3] + plain[1][1][5:]
    assert a3[:7] == a1[:7] and m2._draw == 3


# ------------------------------------------------------------------------------ refusals
def test_bad_lengths_are_refused_before_anything_is_drawn_or_called():
    import test_loop_marshalling as M
    from speakerguard_amd.model.xv_plda import xv_plda
    loss, grad_sign = M.resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, y = torch.zeros(M.B, 1, 16000), torch.arange(M.B) % M.S
    lo, hi = torch.full((M.B, 1, 1), -1.0), torch.full((M.B, 1, 1), 1.0)

    def i32(*v):
        return torch.tensor(v, dtype=torch.int32)
    cases = ((i32(16001, 9999, 8000), "lengths[0] = 16001 exceeds"), (i32(16000, 399, 8000), "lengths[1] = 399 is shorter than one 25 ms window"),
             (i32(16000, 9999, 5039), "lengths[2] = 5039 gives 31 frames, too few for the TDNN context"),
             (i32(15999, 9999, 8000), "no utterance has the padded length 16000"), (i32(16000, 9999), "int32 tensor of shape (3,)"),
             (torch.tensor([16000, 9999, 8000]), "int32 tensor of shape (3,)"), ([16000, 9999, 8000], "int32 tensor of shape (3,)"))
    for lens, text in cases:
        m = M._model(xv_plda)
        m.dim, m._has_enroll = 7, True
        for call in (lambda: m.loss_grad(x, y, loss, lengths=lens), lambda: m.make_decision(x, lengths=lens),
                     lambda: m.score(x, lengths=lens), lambda: m.pgd_run(x, y, lo, hi, loss, M.STEP, M.ITERS, grad_sign, lengths=lens)):
            with pytest.raises(ValueError) as e:
                call()
            assert text in str(e.value)
        assert m.ctx.calls == [] and m._draw == 0
    m = M._model(xv_plda)
    with pytest.raises(ValueError, match="flag 0"):
        m.loss_grad(torch.zeros(M.B, 100, 30), y, loss, flag=1, lengths=i32(100, 100, 100))
    with pytest.raises(ValueError, match="explicit dither tensor"):
        m.loss_grad(x, y, loss, lengths=i32(16000, 9999, 8000), dither_noise=torch.zeros(3, 100, 400))
    assert m.ctx.calls == []


def test_models_and_attacks_that_cannot_take_lengths_say_so_by_name():
    import test_loop_marshalling as M
    from speakerguard_amd.attack.CW2 import CW2
    from speakerguard_amd.attack.FAKEBOB import FAKEBOB
    from speakerguard_amd.attack.Kenan import Kenan
    from speakerguard_amd.attack.KenanSSA import KenanSSA
    from speakerguard_amd.attack.SirenAttack import SirenAttack
    from speakerguard_amd.defense import AS
    from speakerguard_amd.model.audionet_csine import audionet_csine
    from speakerguard_amd.model.defended_model import defended_model
    from speakerguard_amd.model.iv_plda import iv_plda
    from speakerguard_amd.model.xv_plda import xv_plda
    loss, _ = M.resolve_loss('Entropy', targeted=False, task='CSI', threshold=None, clip_max=False)
    x, lens, y = _data()
    for cls in (audionet_csine, iv_plda):
        m = M._model(cls)
        m.dim, m._has_enroll, m._white_box, m.allowed_flags = 7, True, True, [0]
        for call in (lambda: m.make_decision(x, lengths=lens), lambda: m.score(x, lengths=lens), lambda: m(x, lengths=lens),
                     lambda: m.loss_grad(x, y, loss, lengths=lens), lambda: PGD(m, verbose=0).attack(x, y, lengths=lens)):
            with pytest.raises(ValueError, match=cls.__name__):
                call()
        assert m.ctx.calls == [] and m._draw == 0
    eng = RaggedToyEngine()
    defended = defended_model(eng, defense=[(0, AS(3))])
    for call in (lambda: defended.make_decision(x, lengths=lens), lambda: defended.score(x, lengths=lens), lambda: defended(x, lengths=lens),
                 lambda: defended.loss_grad(x, y, loss, lengths=lens), lambda: PGD(defended, verbose=0).attack(x, y, lengths=lens),
                 lambda: CWinf(defended, verbose=0).attack(x, y, lengths=lens), lambda: FGSM(defended, verbose=0).attack(x, y, lengths=lens)):
        with pytest.raises(ValueError, match="defended_model"):
            call()
    assert eng.calls == []
    # a wrapper without defenses hands the lengths on
    bare = defended_model(eng)
    bare.loss_grad(x, y, loss, lengths=lens)
    assert eng.calls == [("loss_grad", 5, 800, list(LENGTHS))]
    # an engine double that knows no lengths (no ``takes_lengths``) is refused by its class name
    with pytest.raises(ValueError, match="AutogradEngine"):
        PGD(AutogradEngine(ToyModel().eval()), verbose=0).attack(x, y, lengths=lens)
    for cls in (CW2, FAKEBOB, SirenAttack, Kenan, KenanSSA):
        with pytest.raises(ValueError, match=cls.__name__):
            cls.__new__(cls).attack(x, y, lengths=lens)
    for bad, text in ((lens[:3], "shape (5,)"), (lens.to(torch.int64), "int32"), (torch.tensor([801, 600, 720, 440, 655], dtype=torch.int32), "1 .. 800"),
                      (torch.tensor([800, 0, 720, 440, 655], dtype=torch.int32), "1 .. 800")):
        with pytest.raises(ValueError) as e:
            _attack(PGD).attack(x, y, lengths=bad)
        assert text in str(e.value)


# ------------------------------------------------------------------------------ ShardedAttack, gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    x, lens, y = _data(fill=0.7)
    atk = _attack(PGD)
    adv, succ = ShardedAttack(atk).attack(x, y, lengths=lens)
    seen = [None] * world
    dist.all_gather_object(seen, sorted(set((c[1], tuple(c[3])) for c in atk.model.calls)))
    if rank == 0:
        torch.save({"adv": adv, "succ": succ, "seen": seen}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_attack_slices_the_lengths_with_the_batch(tmp_path):
    x, lens, y = _data(fill=0.7)
    ref_adv, ref_succ = _attack(PGD).attack(x, y, lengths=lens)
    out = str(tmp_path / "ragged.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    assert got["succ"] == list(ref_succ) and torch.equal(got["adv"], ref_adv)
    # rank 0: utterances 0 .. 2 in chunks of 2 and 1; rank 1: utterances 3, 4 -- each with its own lengths
    assert got["seen"] == [[(1, (720,)), (2, (800, 600))], [(2, (440, 655))]]
    with pytest.raises(ValueError, match="random restarts"):
        ShardedAttack(_attack(PGD, num_random_init=2)).attack(x, y, lengths=lens)
