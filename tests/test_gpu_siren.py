"""SirenAttack's swarm on the device (csrc/k_pso.hip) and the attack on it (speakerguard_amd/attack/SirenAttack.py).

The three entries are judged against tests/pso_restate.py BIT FOR BIT -- every output, the queries included, with given draws
and with the library's own generator (which pins the Philox keying) -- over shapes on both sides of every path: one element,
T below a vector, T a multiple of 4 (both kernel widths) and not (scalar kernels only: 1023, 1025), more than one block per row,
and the workload's (2, 25, 48000).  Row lists: all slots, and a strict subset in non-trivial order; the slots outside the list hold
a sentinel and must keep it.

The whole attack runs on the synthetic xv_plda and once on audionet_csine, with the invariants the host logic promises, and is
REPLAYED on the CPU: the host class on the restated swarm, the same seed, and a model double that hands back the recorded loss
matrices must give the device run's adversarial audio and flags bit for bit -- the device swarm judged over a real trajectory
without asking two models to agree in the last bit of a comparison."""
import numpy as np
import pytest
import torch

from pso_restate import RestatedSwarm
from speakerguard_amd.attack.SirenAttack import SirenAttack, SwarmState
from speakerguard_amd.model._engine_ops import mix64
from test_gpu_time_domain import AN_T, XV_T, _models

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = ((1, 1, 1), (1, 2, 3), (2, 5, 800), (3, 4, 1023), (2, 3, 1025), (2, 25, 48000))
SENTINEL = 777.0
STATE = ("loc", "vel", "pbest_loc", "gbest_loc", "pbest", "gbest")
KEY = 0x0123456789ABCDEF
INDEX_BASE = (1 << 32) + 5  # past 32 bits: both counter words of the utterance index count


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32 if t.dtype == torch.float32 else np.uint8)


def row_lists(n):
    """all slots, and a strict subset in non-trivial order ([2, 0] of 3)"""
    return [list(range(n))] + ([[2, 0]] if n == 3 else [[1]] if n == 2 else [])


CASES = [(s, rows) for s in SHAPES for rows in row_lists(s[0])]
IDS = ["%dx%dx%d-rows%s" % (s + ("".join(map(str, r)),)) for s, r in CASES]
# the streaming kernels exist at two widths; the library's rule takes 16 bytes per lane only from two waves per SIMD of the chip
# on, which none of these shapes reaches: where T allows them, SG_PSO_VEC=4 (behind SG_TUNE=1, tests/conftest.py) runs them too
WIDE = [(s, rows, w) for s, rows in CASES for w in (["rule", "4"] if s[2] % 4 == 0 else ["rule"])]
WIDE_IDS = ["%dx%dx%d-rows%s-%s" % (s + ("".join(map(str, r)), w)) for s, r, w in WIDE]


def set_width(monkeypatch, width):
    if width == "rule":
        monkeypatch.delenv("SG_PSO_VEC", raising=False)
    else:
        monkeypatch.setenv("SG_PSO_VEC", width)

_MODEL = []


def engine():
    if not _MODEL:
        _MODEL.append(_models()[0][1]())
    return _MODEL[0]


def problem(n, P, T, rows, seed=0):
    """a chunk's inputs and a random swarm state, the slots outside `rows` at the sentinel -> (x, lower, upper, state), on the CPU"""
    rs = np.random.RandomState(seed + 7 * n + 13 * P + T)
    x = torch.from_numpy(np.clip(0.4 * rs.randn(n, 1, T), -0.999, 0.999).astype(np.float32))
    eps = 0.01
    lower, upper = torch.clamp(-1 - x, min=-eps), torch.clamp(1 - x, max=eps)  # attack/SirenAttack.py:251-252
    st = SwarmState(n, P, T, "cpu")
    for name in STATE:
        t = getattr(st, name)
        t.copy_(torch.from_numpy(rs.uniform(-eps, eps, tuple(t.shape)).astype(np.float32)))
        for slot in range(n):
            if slot not in rows:
                t[slot] = SENTINEL
    return x, lower, upper, st


def to_device(st):
    out = SwarmState(*st.loc.shape, DEV)
    for name in STATE:
        getattr(out, name).copy_(getattr(st, name))
    if st.improved is not None:
        out.improved = st.improved.to(DEV)
    return out


def same_state(dev, cpu, rows, what):
    n = cpu.loc.shape[0]
    for name in STATE:
        d, c = getattr(dev, name), getattr(cpu, name)
        assert np.array_equal(bits(d), bits(c)), (what, name, float((d.cpu() - c).abs().max()))
        for slot in range(n):
            if slot not in rows:
                assert bool((d[slot] == SENTINEL).all()), (what, name, slot)


def same_queries(dev, cpu, what):
    assert (dev is None) == (cpu is None), what
    if cpu is not None:
        assert dev.shape == cpu.shape and np.array_equal(bits(dev), bits(cpu)), (what, float((dev.cpu() - cpu).abs().max()))


def given(rs, shape, lo, hi):
    return torch.from_numpy(rs.uniform(lo, hi, shape).astype(np.float32))


@pytest.mark.parametrize("own", [False, True], ids=["given-draws", "own-generator"])
@pytest.mark.parametrize("shape,rows,width", WIDE, ids=WIDE_IDS)
def test_init_equals_its_restatement(shape, rows, width, own, monkeypatch):
    """epoch 0, then two epochs > 0 on the state the first left: best_index = P - 1 and a non-zero index in between"""
    set_width(monkeypatch, width)
    n, P, T = shape
    x, lower, upper, cpu = problem(n, P, T, rows)
    dev = to_device(cpu)
    xd, ld, ud = x.to(DEV), lower.to(DEV), upper.to(DEV)
    rs = np.random.RandomState(1)
    for epoch, best in ((0, None), (1, [P - 1] * len(rows)), (2, [(P - 1) // 2 + (k % 2) * (P > 2) for k in range(len(rows))])):
        pos = vel = None
        if not own:
            pos = given(rs, (len(rows), P - (epoch > 0), 1, T), -0.01, 0.01)
            vel = given(rs, (len(rows), P, 1, T), -0.02, 0.02)
        if epoch:  # personal best values worth carrying
            cpu.pbest[rows] = torch.from_numpy(rs.uniform(-1, 1, (len(rows), P)).astype(np.float32))
            dev.pbest.copy_(cpu.pbest)
        want = RestatedSwarm().pso_init(cpu, x, lower, upper, rows, epoch, best, KEY + epoch, INDEX_BASE, pos, vel)
        got = engine().pso_init(dev, xd, ld, ud, rows, epoch, best, KEY + epoch, INDEX_BASE,
                                None if pos is None or pos.numel() == 0 else pos.to(DEV), None if vel is None else vel.to(DEV))
        torch.cuda.synchronize()
        same_queries(got, want, ("init", epoch))
        same_state(dev, cpu, rows, ("init", epoch))
        if own:  # the draws are inside their boxes, and not degenerate
            loc = cpu.loc[rows]
            assert bool((loc >= lower[rows]).all()) and bool((loc <= upper[rows]).all())
            assert bool((cpu.vel[rows].abs() <= (lower[rows] - upper[rows]).abs()).all())
            if T * P >= 800:
                assert float(cpu.vel[rows].std()) > 0.004 and float(cpu.loc[rows].std()) > 0.002


@pytest.mark.parametrize("shape,rows", CASES, ids=IDS)
def test_select_equals_its_restatement(shape, rows):
    """ties across particles, loss == pbest (no update), +inf and the largest finite values; three calls in a row"""
    n, P, T = shape
    _, _, _, cpu = problem(n, P, 1, rows)
    rs = np.random.RandomState(2)
    cpu.pbest[rows] = float("inf")
    cpu.gbest[rows] = float("inf")
    dev = to_device(cpu)
    big = np.float32(3.4028235e38)
    for call in range(3):
        loss = rs.randint(-3, 4, (len(rows), P)).astype(np.float32) / np.float32(4)  # a few values: ties everywhere
        if call == 0:
            loss[0, 0] = np.inf
            loss[-1, -1] = big
        if call == 1:
            loss[0] = cpu.pbest[rows[0]].numpy()  # equal to pbest: nothing improves in this row
        if call == 2:
            loss[-1, 0] = -big
        loss = torch.from_numpy(loss)
        want = RestatedSwarm().pso_select(cpu, loss, rows)
        got = engine().pso_select(dev, loss.to(DEV), rows)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (call, got, want)
        assert np.array_equal(bits(dev.improved), bits(cpu.improved)), call
        same_state(dev, cpu, rows, ("select", call))
        if call == 1:
            assert not bool(cpu.improved.reshape(len(rows), P)[0].any()) and want[2][0] == -1
    assert np.isfinite(want[0]).all()


@pytest.mark.parametrize("own", [False, True], ids=["given-draws", "own-generator"])
@pytest.mark.parametrize("shape,rows,width", WIDE, ids=WIDE_IDS)
def test_move_equals_its_restatement(shape, rows, width, own, monkeypatch):
    """a mix of continuing and found rows, every gbest_from (none, first, last), then the last iteration (nothing moves) and a
    call in which every row was found"""
    set_width(monkeypatch, width)
    n, P, T = shape
    x, lower, upper, cpu = problem(n, P, T, rows)
    rs = np.random.RandomState(3)
    xd, ld, ud = x.to(DEV), lower.to(DEV), upper.to(DEV)
    dev = to_device(cpu)
    na = len(rows)
    plans = [([1] * na, 1), ([k % 2 for k in range(na)], 1), ([1] * na, 0), ([0] * na, 1)]  # (continue flags, do_move)
    for step, (cont, do_move) in enumerate(plans):
        improved = torch.from_numpy((rs.rand(na * P) < 0.5).astype(np.uint8))
        cpu.improved, dev.improved = improved, improved.to(DEV)
        gbest_from = [(-1, 0, P - 1)[(k + step) % 3] for k in range(na)]
        n_cont = sum(cont) if do_move else 0
        r1 = r2 = None
        if not own and n_cont:
            r1, r2 = given(rs, (n_cont, P, 1, T), 1e-5, 1.0), given(rs, (n_cont, P, 1, T), 1e-5, 1.0)
        w = (0.9 - 0.1) * (5 - step - 1) / 5 + 0.1  # :164
        args = (rows, gbest_from, cont, do_move, w, 1.4961, 1.4961, KEY + step, INDEX_BASE)
        want = RestatedSwarm().pso_move(cpu, x, lower, upper, *args, r1, r2)
        got = engine().pso_move(dev, xd, ld, ud, *args, None if r1 is None else r1.to(DEV), None if r2 is None else r2.to(DEV))
        torch.cuda.synchronize()
        same_queries(got, want, ("move", step))
        same_state(dev, cpu, rows, ("move", step))
        assert (want is None) == (n_cont == 0)
        moved = [r for r, c in zip(rows, cont) if c and do_move]
        assert bool((cpu.loc[moved] >= lower[moved]).all()) and bool((cpu.loc[moved] <= upper[moved]).all())


def test_refusals_launch_nothing():
    from speakerguard_amd import _native as N
    m = engine()
    x, lower, upper, cpu = problem(3, 4, 8, [0, 1, 2])
    dev = to_device(cpu)
    dev.improved = torch.zeros(12, dtype=torch.uint8, device=DEV)
    xd, ld, ud = x.to(DEV), lower.to(DEV), upper.to(DEV)
    loss = torch.zeros(3, 4, device=DEV)
    for bad in ([0, 0, 1], [0, 3], [-1], [0, 1, 2, 0], []):
        with pytest.raises(N.NativeError):
            m.pso_init(dev, xd, ld, ud, bad, 0, None, KEY)
        with pytest.raises(N.NativeError):
            m.pso_select(dev, loss, bad)
        with pytest.raises(N.NativeError):
            m.pso_move(dev, xd, ld, ud, bad, [0] * len(bad), [1] * len(bad), 1, 0.5, 1.0, 1.0, KEY)
    with pytest.raises(N.NativeError):
        m.pso_init(dev, xd, ld, ud, [0, 1, 2], 1, [0, 4, 0], KEY)
    with pytest.raises(N.NativeError):
        m.pso_init(dev, xd, ld, ud, [0, 1, 2], 1, None, KEY)
    with pytest.raises(N.NativeError):
        m.pso_move(dev, xd, ld, ud, [0, 1, 2], [0, 4, -1], [1, 1, 1], 1, 0.5, 1.0, 1.0, KEY)
    with pytest.raises(N.NativeError):
        m.pso_move(dev, xd, ld, ud, [0, 1, 2], [0, -2, -1], [1, 1, 1], 1, 0.5, 1.0, 1.0, KEY)
    torch.cuda.synchronize()
    same_state(dev, cpu, [0, 1, 2], "refusals")


# ---------------------------------------------------------------- the attack, end to end
# (model, its index in _models(), the shortest utterance its own tests use, epsilon).  The epsilons come from the synthetic
# weights, probed on the CPU oracles with the restated swarm.  xv_plda: the four utterances' CSI margins are 4.4, 3.0, 3.6 and
# 14.4; at 0.002 a swarm of 8 over 2 x 6 evaluations ends at -0.2, -0.3, -1.3 and +5.4 (at 0.001 one success, at 0.004 four).
# audionet: margins 0.41, 0.43, 0.62, 0.12; at 0.03 it ends at +0.05, -0.03, +0.25, -0.09 (at 0.008 no success).  The test
# asserts that both outcomes occur.
E2E = (("xv_plda", 0, XV_T, 0.002), ("audionet", 1, AN_T, 0.03))
KW = dict(task="CSI", n_particles=8, max_epoch=2, max_iter=5, batch_size=4, verbose=0, seed=1)


class ReplayModel:
    """hands back the recorded loss matrices in order; keys its draws like the engine (EngineOps.noise_seed)"""

    def __init__(self, losses, noise_epoch, n_spk):
        self.losses, self._noise_epoch, self.n_spk, self._batch_salt, self.calls = list(losses), noise_epoch, n_spk, 0, 0

    def begin_attack(self):
        self._noise_epoch += 1

    def begin_batch(self, index_base=0, salt=0):
        self._batch_salt = int(salt)

    def noise_seed(self, user_seed, draw):
        return mix64(user_seed, self._noise_epoch, self._batch_salt, draw)

    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True):
        rows, loss = self.losses[self.calls]
        self.calls += 1
        assert x.shape[0] == loss.size and not want_grad
        return (torch.zeros(x.shape[0], dtype=torch.int64), torch.zeros(x.shape[0], self.n_spk),
                torch.from_numpy(loss.reshape(-1).copy()), None)


_RUNS = {}


def _run(which):
    if which not in _RUNS:
        from speakerguard_amd import synth
        name, idx, T, eps = E2E[which]
        model = engine() if idx == 0 else _models()[idx][1]()
        x = torch.from_numpy(synth.make_waveforms(4, T, seed=3)).to(DEV)
        dec, scores = model.make_decision(x)
        y = dec.clone()
        atk = SirenAttack(model, epsilon=eps, record=True, **KW)
        adv, succ = atk.attack(x, y)
        torch.cuda.synchronize()
        _RUNS[which] = dict(model=model, x=x, y=y, atk=atk, adv=adv, succ=list(succ), noise_epoch=model._noise_epoch,
                            n_spk=scores.shape[1], eps=eps)
    return _RUNS[which]


@pytest.mark.parametrize("which", [0, 1], ids=[e[0] for e in E2E])
def test_attack_invariants(which):
    r = _run(which)
    model, x, y, atk, adv, succ, eps = r["model"], r["x"], r["y"], r["atk"], r["adv"], r["succ"], r["eps"]
    gbest = np.array(atk.final_gbest, np.float32)
    print("siren %s eps %g: success %s gbest %s epochs %s evaluations %s" % (E2E[which][0], eps, succ, gbest.tolist(), atk.epochs_run,
                                                                          atk.iters_run))
    assert set(succ) == {True, False}, "both outcomes must occur"
    assert succ == [bool(g < 0) for g in gbest]
    # |adv - x| <= eps up to one float32 rounding of gbest_location + x (half an ulp below 1: 2^-25) and epsilon's own (2^-30)
    a64, x64 = adv.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64)
    assert np.abs(a64 - x64).max() <= eps + 2.0 ** -24 and np.abs(a64).max() <= 1.0
    # the loss of the returned audio IS the recorded global best, and the best of everything the utterance was evaluated at
    loss = model.loss_grad(adv, y, atk.loss, want_grad=False)[2]
    assert np.array_equal(bits(loss), gbest.view(np.uint32))
    best_seen = np.full(4, np.inf, np.float32)
    for rows, l in atk.loss_record[0]:
        best_seen[rows] = np.minimum(best_seen[rows], l.min(1))
    assert np.array_equal(best_seen.view(np.uint32), gbest.view(np.uint32))
    dec = model.make_decision(adv)[0].cpu().tolist()
    for i, s in enumerate(succ):
        assert not torch.equal(adv[i], x[i])  # a failed utterance returns its best location too
        if s:
            assert dec[i] != int(y[i])
    assert all(1 <= e <= 2 for e in atk.epochs_run) and all(1 <= i <= 12 for i in atk.iters_run)
    assert any(i < 12 for i in atk.iters_run), "a found utterance leaves the active set"


@pytest.mark.parametrize("which", [0, 1], ids=[e[0] for e in E2E])
def test_attack_replays_on_the_restated_swarm(which):
    r = _run(which)
    atk = r["atk"]
    double = ReplayModel(atk.loss_record[0], r["noise_epoch"] - 1, r["n_spk"])
    replay = SirenAttack(double, epsilon=r["eps"], swarm=RestatedSwarm(), record=True, **KW)
    adv, succ = replay.attack(r["x"].cpu(), r["y"].cpu())
    assert double.calls == len(atk.loss_record[0])
    assert list(succ) == r["succ"]
    assert np.array_equal(bits(adv), bits(r["adv"]))
    assert replay.final_gbest == atk.final_gbest and replay.iters_run == atk.iters_run


def test_dither_is_keyed_by_slot_after_a_deletion():
    """xv_plda with its default dither: the model call's noise is keyed by the utterance's global index also after delete_found
    has shortened the list of slots (SirenAttack._evaluate), so batch_size 4 and 1 give the same bits (abort tests off: they
    couple a chunk through a mean).  The noise keys hold the attack call's number: both runs are the model's first attack."""
    from speakerguard_amd import synth
    from speakerguard_amd.model.xv_plda import xv_plda
    model = xv_plda.from_weights(synth.make_xv_weights(), device=DEV, dither=1.0)
    x = torch.from_numpy(synth.make_waveforms(4, XV_T, seed=3)).to(DEV)
    y = engine().make_decision(x)[0]
    out = []
    for bs, call in ((4, 0), (1, 0), (4, 1)):
        model._noise_epoch = call
        atk = SirenAttack(model, epsilon=0.002, abort_early=False, **dict(KW, batch_size=bs))
        adv, succ = atk.attack(x, y)
        out.append((bits(adv), list(succ), list(atk.final_gbest), list(atk.iters_run)))
    print("siren dither: success %s gbest %s evaluations %s" % out[0][1:])
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]
    iters = out[0][3]
    assert any(iters[i] < iters[j] for i in range(4) for j in range(i + 1, 4)), "no utterance left the chunk before a later one"
    assert out[2][2] != out[0][2], "another attack call draws other noise: the dither is in the loss"
