"""The HOST logic of speakerguard_amd.attack.SirenAttack against the reference's own runs (tests/golden/siren_ref.npz, written
by tests/golden/make_golden_siren.py): the class drives the CPU restatement of the swarm (tests/pso_restate.py) on a CPU
engine double, is fed the draws the reference made, and must give the reference's adversarial audio, success flags and final
global bests BIT FOR BIT -- every operation is the reference's float32 operation on the same operands.  No GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from engine_doubles import AutogradEngine
from pso_restate import RestatedSwarm
from speakerguard_amd.attack.SirenAttack import SirenAttack
from toy_model import ToyModel, toy_inputs


@pytest.fixture(scope="module")
def golden():
    return load_golden("siren_ref.npz")


CASES = ["csi_u_b4", "csi_u_b1", "csi_t_b4", "csi_t_b1", "osi_u_b4", "osi_u_b1", "osi_t_b4", "osi_t_b1", "csi_u_b4_p1"]


def recorded_draws(g, name):
    """draw_fn that hands out the reference's draws in call order, checking every shape it is asked for"""
    flat, shapes, at = g[name + "_draws"], g[name + "_draw_shapes"], [0, 0]

    def draw_fn(kind, shape, low, high):
        want = tuple(int(v) for v in shapes[at[0]])
        assert tuple(shape) == want, (name, at[0], kind, shape, want)
        n = int(np.prod(want))
        d = flat[at[1]:at[1] + n].reshape(want)
        assert np.all(d >= low) and np.all(d < high) if n else True
        at[0] += 1
        at[1] += n
        return d
    draw_fn.left = lambda: len(shapes) - at[0]
    return draw_fn


def make_attack(g, name, **over):
    task, targeted, bs, P, eps, max_iter = g["meta"]["cases"][name][:6]
    kw = dict(g["meta"]["common"])
    if len(g["meta"]["cases"][name]) > 7:
        kw["abort_early_epoch"] = g["meta"]["cases"][name][7]
    thr = g["meta"]["threshold"] if task == "OSI" else None
    model = AutogradEngine(ToyModel(T=40, n_spk=4, threshold=thr).eval())
    kw.update(threshold=thr, task=task, targeted=bool(targeted), epsilon=eps, max_iter=max_iter, n_particles=P, batch_size=bs,
              swarm=RestatedSwarm())
    kw.update(over)
    return SirenAttack(model, **kw)


def test_fixture_is_the_toy_model_and_covers_every_path(golden):
    assert np.array_equal(golden["x"], toy_inputs(B=4, T=40).numpy())
    stats = golden["meta"]["stats"]
    assert sorted(stats) == sorted(CASES) and golden["meta"]["accommodations"] == ["numpy.infty alias"]
    flags = [s for name in CASES for s in golden[name + "_succ"].tolist()]
    assert True in flags and False in flags
    for task in ("csi", "osi"):
        for kind in ("_u_", "_t_"):  # mixed flags per task, and targeted runs that succeed
            got = [s for name in CASES if name.startswith(task) and kind in name for s in golden[name + "_succ"].tolist()]
            assert True in got and False in got, (task, kind)
    assert any(st["abort_inner"] for st in stats.values()) and any(st["abort_outer"] for st in stats.values())
    assert any(st["partial_delete"] for st in stats.values())
    assert {golden["meta"]["cases"][n][2] for n in CASES} == {1, 4} and {golden["meta"]["cases"][n][3] for n in CASES} == {1, 5}


@pytest.mark.parametrize("name", CASES)
def test_reproduces_the_reference_bit_for_bit(golden, name):
    draw_fn = recorded_draws(golden, name)
    atk = make_attack(golden, name, draw_fn=draw_fn)
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden[name + "_y"])
    adv, success = atk.attack(x.clone(), y)
    assert draw_fn.left() == 0, "the reference made %d more draws" % draw_fn.left()
    assert success == golden[name + "_succ"].tolist()
    assert np.array_equal(np.array(atk.final_gbest, np.float32).view(np.uint32), golden[name + "_gbest"].view(np.uint32))
    assert np.array_equal(adv.numpy().view(np.uint32), golden[name + "_adv"].view(np.uint32))
    assert len(atk.epochs_run) == len(atk.iters_run) == 4 and min(atk.epochs_run) >= 1


def test_own_draws_do_not_depend_on_the_chunking(golden):
    """the generator's draws are keyed by the utterance's global index: without the abort tests (which couple a chunk through a
    mean) batch_size 4 and batch_size 1 give the same bits.  The model double takes its rows one by one, like the engine."""
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden["csi_u_b4_y"])
    out = []
    for bs in (4, 1):
        atk = make_attack(golden, "csi_u_b4", batch_size=bs, abort_early=False, seed=3)
        atk.model = AutogradEngine(ToyModel(T=40, n_spk=4).eval(), per_row=True)
        adv, success = atk.attack(x.clone(), y)
        out.append((adv.numpy().view(np.uint32), success, np.array(atk.final_gbest, np.float32).view(np.uint32)))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    assert not np.array_equal(out[0][0], x.numpy().view(np.uint32))
    # :251-252: the distortion stays inside the box, up to one float32 rounding of gbest_location + x (half an ulp below 1,
    # 2^-25) and the rounding of epsilon itself (2^-30)
    adv = out[0][0].view(np.float32).astype(np.float64)
    assert np.all(np.abs(adv - x.numpy().astype(np.float64)) <= 0.02 + 2.0 ** -24) and np.all(np.abs(adv) <= 1)
    other = make_attack(golden, "csi_u_b4", abort_early=False, seed=4).attack(x.clone(), y)[0]
    assert not np.array_equal(other.numpy().view(np.uint32), out[0][0])  # another seed, another swarm


def test_records(golden):
    atk = make_attack(golden, "csi_u_b4", draw_fn=recorded_draws(golden, "csi_u_b4"), record=True)
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden["csi_u_b4_y"])
    atk.attack(x.clone(), y)
    assert len(atk.loss_record) == 1
    rows0, loss0 = atk.loss_record[0][0]
    assert rows0 == [0, 1, 2, 3] and loss0.shape == (4, 5) and loss0.dtype == np.float32
    assert sum(len(rows) for rows, _ in atk.loss_record[0]) == sum(atk.iters_run)
    assert all(l.shape == (len(rows), 5) for rows, l in atk.loss_record[0])


def test_asserts_and_raises_of_the_reference(golden):
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden["csi_u_b4_y"])
    for task in ("SV", "OSI"):  # :237-239
        atk = make_attack(golden, "csi_u_b4", task=task, threshold=None)
        with pytest.raises(NotImplementedError):
            atk.attack(x.clone(), y)
    atk = make_attack(golden, "csi_u_b4")
    with pytest.raises(AssertionError, match="float domain"):   # :245
        atk.attack(x.clone() + 1.0, y)
    with pytest.raises(AssertionError, match="Mono"):           # :247
        atk.attack(x.repeat(1, 2, 1), y)
    with pytest.raises(AssertionError, match="should be equal"):  # :248
        atk.attack(x.clone(), y[:3])


def test_constructor_is_the_reference_s(golden):
    import inspect
    params = inspect.signature(SirenAttack.__init__).parameters
    names = list(params)[1:]
    assert names[:22] == ["model", "threshold", "task", "targeted", "confidence", "epsilon", "max_epoch", "max_iter", "c1", "c2",
                          "n_particles", "w_init", "w_end", "batch_size", "EOT_size", "EOT_batch_size", "verbose", "abort_early",
                          "abort_early_iter", "abort_early_epoch", "seed", "draw_fn"]
    want = dict(threshold=None, task='CSI', targeted=False, confidence=0., epsilon=0.002, max_epoch=300, max_iter=30, c1=1.4961,
                c2=1.4961, n_particles=25, w_init=0.9, w_end=0.1, batch_size=1, EOT_size=1, EOT_batch_size=1, verbose=1,
                abort_early=True, abort_early_iter=10, abort_early_epoch=10, seed=0, draw_fn=None, swarm=None)
    assert {k: params[k].default for k in want} == want


def test_chunk_coupling_follows_abort_early(golden):
    assert make_attack(golden, "csi_u_b4").chunk_coupling == 'chunk'
    assert make_attack(golden, "csi_u_b4", abort_early=False).chunk_coupling is None
    from speakerguard_amd import attack
    assert attack.SirenAttack is SirenAttack


class KeyedEngine(AutogradEngine):
    """the toy model behind the engine's noise bookkeeping (EngineOps: ``row_keys``, pass counter, chunk base): every row's loss
    gets noise keyed by (the utterance index the engine would derive for that row, the pass number), like dither is"""
    dither = 1.0
    _index_base, _row_scale, _row_base, _rep_rows, _draw, _def_draw = 0, 1, 0, 0, 0, 0

    def begin_batch(self, index_base=0, salt=0):
        self._index_base, self._draw, self._def_draw = int(index_base), 0, 0

    def row_keys(self):
        return self._index_base * self._row_scale, self._row_base, self._rep_rows

    def loss_grad(self, x, y, loss_spec, flag=0, want_grad=True):
        from speakerguard_amd.model._engine_ops import mix64
        dec, sc, loss, g = super().loss_grad(x, y, loss_spec, flag, want_grad)
        base, row_base, _ = self.row_keys()
        noise = [(mix64(base + row_base + r, self._draw) % 2001 - 1000) * 1e-4 for r in range(x.shape[0])]
        self._draw += 1
        self.seen.append((base, x.shape[0]))
        return dec, sc, loss + torch.tensor(noise, dtype=torch.float32), g


def test_model_noise_is_keyed_by_slot_after_a_deletion(golden):
    """the queries are dense in active order; once delete_found has shortened the list, the model call must still key every
    row by its utterance's slot.  With noise in the model, batch_size 4 and 1 give the same bits (abort tests off)."""
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden["csi_u_b4_y"])
    out = []
    for bs in (4, 1):
        atk = make_attack(golden, "csi_u_b4", batch_size=bs, abort_early=False, seed=3)
        atk.model = KeyedEngine(ToyModel(T=40, n_spk=4).eval(), per_row=True)
        atk.model.seen = []
        adv, success = atk.attack(x.clone(), y)
        out.append((adv.numpy().view(np.uint32), success, list(atk.final_gbest), list(atk.iters_run), atk.model.seen))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:4] == out[1][1:4]
    iters = out[0][3]
    assert any(iters[i] < iters[j] for i in range(4) for j in range(i + 1, 4)), "no utterance left the chunk before a later one"
    P = 5
    assert (0, 4 * P) in out[0][4] and any(b > 0 for b, _ in out[0][4]), "a shortened list is keyed from its first slot"
    assert {b for b, _ in out[1][4]} == {0, P, 2 * P, 3 * P}


def test_chunk_and_particle_caps_are_refused_before_anything_runs(golden):
    x, y = torch.from_numpy(golden["x"]), torch.from_numpy(golden["csi_u_b4_y"])
    with pytest.raises(ValueError, match="at most 256"):
        make_attack(golden, "csi_u_b4", batch_size=300).attack(x.repeat(75, 1, 1)[:257], y.repeat(75)[:257])
    with pytest.raises(ValueError, match="particles"):
        make_attack(golden, "csi_u_b4", n_particles=1025).attack(x.clone(), y)
