"""The entry points for batches of unequal lengths (sg_xv_forward_ragged, sg_xv_loss_grad_ragged, sg_xv_pgd_run_ragged) in the
sweep of tests/test_gpu_caller_buffers.py: every device buffer a caller hands them -- waveform, bounds, labels, the device
copy of the lengths, every output -- k elements off a 16-byte boundary between poisoned guards, bit-equal to the plain call
and the guards intact.  The guards matter doubly here: a row's own samples end mid-row, and nothing may be read or written
behind the row whatever the lengths say.

The cases register themselves with that file's ``sweeps`` decorator, which is what places the three entries for
tests/test_caller_buffers_host.py (every export with a caller's buffer is swept or excused): the registration happens when this
module is imported, i.e. whenever the suite is collected.  The sweep's own test was parametrised before that, so the moved-buffer
test of these three entries is the one below, the same judge on the same machinery.
"""
import pytest
import torch

import test_gpu_caller_buffers as sweep

pytestmark = pytest.mark.gpu

LENGTHS = (6403, 5043, 5999)  # T_max odd (a row starts 12 bytes off a boundary), the shortest utterance the engine takes, one between


def batch(e):
    x = e.wave(len(LENGTHS), max(LENGTHS), seed=5)
    for b, t in enumerate(LENGTHS):
        x[b, 0, t:] = 0.9  # padding content must not matter on moved buffers either
    return x, torch.tensor(LENGTHS, dtype=torch.int32), torch.tensor([1, 7, 4], device=e.dev)


@sweep.sweeps("sg_xv_forward_ragged")
def case_xv_forward_ragged(e):
    x, lens, _ = batch(e)
    out = sweep.named("wav", e.xv._forward(x, 0, want_emb=True, want_tdnn=True, lengths=lens), ("dec", "scores", "emb", "tdnn"))
    own = (LENGTHS[1] + 80) // 160 - 12
    out["act2"] = e.xv.read_activation(2, len(LENGTHS))[1, :own].contiguous()  # (an utterance's own rows: the rest is unspecified)
    return out


@sweep.sweeps("sg_xv_loss_grad_ragged")
def case_xv_loss_grad_ragged(e):
    x, lens, y = batch(e)
    out = sweep.named("ce", e.xv.loss_grad(x, y, sweep.ce(), lengths=lens), ("dec", "scores", "loss", "grad"))
    out.update(dact5=e.xv.read_gradient("dact5"), dfeats_raw=e.xv.read_gradient("dfeats_raw"))  # zeros behind the utterances included
    out.update(sweep.named("margin", e.xv.loss_grad(x, y, sweep.margin(), lengths=lens), ("dec", "scores", "loss", "grad")))
    return out


@sweep.sweeps("sg_xv_pgd_run_ragged")
def case_xv_pgd_run_ragged(e):
    x, lens, y = batch(e)
    keep = (torch.arange(x.shape[2]).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1).to(e.dev)
    x = torch.where(keep, x, torch.zeros((), device=e.dev))
    lo, hi = sweep.box(x)
    lo, hi = torch.where(keep, lo, torch.zeros((), device=e.dev)), torch.where(keep, hi, torch.zeros((), device=e.dev))
    return dict(zip(sweep.LOOP_OUT, e.xv.pgd_run(x, y, lo, hi, sweep.ce(), 0.0004, 2, 1, trace=True, lengths=lens)))


@pytest.mark.parametrize("k", sweep.KS, ids=lambda k: "k%s" % k)
@pytest.mark.parametrize("entry", ["sg_xv_forward_ragged", "sg_xv_loss_grad_ragged", "sg_xv_pgd_run_ragged"])
def test_ragged_entry_on_moved_buffers(entry, k):
    fn = sweep.CASES[entry]
    ok, why, entries = sweep.verdict_of(fn, k)
    sweep.log("caller_buffers %-34s k %-5s stream default  %s" % (entry, k, why))
    assert ok, (entry, k, why)
    assert entries.get(entry, 0) > 0, "%s: the case never handed it a moved buffer (%s)" % (entry, sorted(entries))
