"""SirenAttack: the particle-swarm black-box attack; mirrors reference attack/SirenAttack.py (``attack`` :235-269,
``attack_batch`` :40-188, ``delete_found`` :191-232).  Queries are forward-only passes of the native engine; the swarm
lives on the device (csrc/k_pso.hip: ``pso_init`` / ``pso_select`` / ``pso_move`` of the model), every utterance in its
own slot for the whole chunk, so that ``delete_found`` shortens a list of slots and copies nothing.

What differs from the reference, on purpose:
  * The reference draws the swarm with numpy on the host (``np.random.uniform`` :67, :74, :84, ``np.random.rand``
    :167-168: two (n, P, 1, T) float64 arrays per iteration, cast and copied to the device).  Here the draws come from
    the library's counter-based generator inside the kernels, keyed by (seed, attack call, draw number) and the utterance's
    GLOBAL index -- a stream of its own, independent of chunking and sharding.  ``draw_fn(kind, shape, low, high)``
    (kind 'uniform' or 'rand') supplies explicit draws instead (tests: the reference's recorded ones give its bits).
  * After the inner abort test fires (:138-144) the reference still computes one more update (:163-174) whose result the
    next epoch overwrites (:81-86); here that update is not computed (its draws are still taken from ``draw_fn``).
  * ``gbest_predict`` (:56, :132) only feeds the progress line; it is kept when ``verbose`` is set.

A chunk holds at most ``MAX_CHUNK`` = 256 utterances (the swarm's row list travels as launch arguments, csrc/k_pso.hip) and
1024 particles: ``attack`` refuses a larger ``batch_size`` or ``n_particles`` before anything runs.

Per-utterance records of the last ``attack`` call: ``final_gbest``, ``epochs_run``, ``iters_run`` (evaluations the
utterance took part in) and, with ``record=True``, ``loss_record``: per chunk the list of (slots, loss matrix) of every
evaluation.
"""
import numpy as np
import torch

from ..adaptive_attack.EOT import EOT
from ..model._engine_ops import mix64
from .Attack import Attack
from .utils import resolve_loss, resolve_prediction, refuse_lengths

MAX_CHUNK, MAX_PARTICLES = 256, 1024  # kPsoMaxRows / kPsoMaxParticles of csrc/k_pso.hip
SEED_TAG = 0x5349524E  # 'SIRN': the key domain of the swarm's draws (EngineOps.noise_seed)


class SwarmState:
    """The state of one chunk (n utterances, P particles, T samples), float32, every utterance in its slot."""

    def __init__(self, n, P, T, device):
        f = dict(device=device, dtype=torch.float32)
        self.loc = torch.empty(n, P, T, **f)
        self.vel = torch.empty(n, P, T, **f)
        self.pbest_loc = torch.empty(n, P, T, **f)
        self.gbest_loc = torch.zeros(n, T, **f)          # :54
        self.pbest = torch.full((n, P), np.inf, **f)     # :70
        self.gbest = torch.full((n,), np.inf, **f)       # :55
        self.improved = None                             # who improved at the last select (len(rows) * P bytes)


class SirenAttack(Attack):

    def __init__(self, model, threshold=None,
                 task='CSI', targeted=False, confidence=0.,
                 epsilon=0.002, max_epoch=300, max_iter=30,
                 c1=1.4961, c2=1.4961, n_particles=25, w_init=0.9, w_end=0.1,
                 batch_size=1, EOT_size=1, EOT_batch_size=1, verbose=1, abort_early=True, abort_early_iter=10,
                 abort_early_epoch=10, seed=0, draw_fn=None, swarm=None, record=False):
        self.model = model
        self.threshold = threshold
        self.task = task
        self.targeted = targeted
        self.confidence = confidence
        self.epsilon = epsilon
        self.max_epoch = max_epoch
        self.max_iter = max_iter
        self.c1 = c1
        self.c2 = c2
        self.n_particles = n_particles
        self.w_init = w_init
        self.w_end = w_end
        self.batch_size = batch_size
        self.EOT_size = EOT_size
        self.EOT_batch_size = EOT_batch_size
        self.verbose = verbose
        self.abort_early = abort_early
        self.abort_early_iter = abort_early_iter
        self.abort_early_epoch = abort_early_epoch
        self.seed = seed
        self.draw_fn = draw_fn  # optional explicit draws (tests); default: the engine's generator
        self.swarm = swarm      # the object with pso_init / pso_select / pso_move; default: the (base) model
        self.record = record
        self.final_gbest = self.epochs_run = self.iters_run = self.loss_record = None

    index_offset = 0  # global index of x[0] when this object attacks one shard of a larger batch (shard.py)

    @property
    def chunk_coupling(self):
        """Both abort tests compare means over the chunk's global bests (:139, :177)."""
        return 'chunk' if self.abort_early else None

    def _key(self, base, draw):
        if hasattr(base, 'noise_seed'):
            return base.noise_seed(self.seed ^ SEED_TAG, draw)
        return mix64(self.seed ^ SEED_TAG, draw)

    def _draw(self, kind, shape, low, high, offset=0.0):
        """An explicit draw as the reference makes it: float64 on the host (+ `offset`), then one rounding to float32."""
        d = np.asarray(self.draw_fn(kind, tuple(shape), low, high), dtype=np.float64)
        assert d.shape == tuple(shape), (d.shape, shape)
        return torch.from_numpy((d + offset).astype(np.float32))

    def _evaluate(self, base, eval_x, eval_y, consider_index, index_base):
        """The model call on the queries of the active slots (:109) -> (summed loss, decisions).  The engine keys its noise
        (dither, randomised defenses) by the row of the call: with ``_row_scale = P`` row r belongs to utterance
        ``_index_base + r // P``.  The queries are dense in ACTIVE order, so once ``delete_found`` has left a gap that would key
        slot s as the utterance at its position in the list.  Where noise is drawn, every run of consecutive slots therefore
        goes through the model as a call of its own, keyed from its first slot, and all runs of an evaluation share the pass
        numbers one call would have used: an utterance's noise does not depend on what else is, or still is, in the chunk."""
        P = self.n_particles
        if not hasattr(base, 'row_keys'):
            _, loss, _, decisions = self.EOT_wrapper(eval_x, eval_y)
            return loss, decisions
        runs = [(0, len(consider_index))]
        noisy = getattr(base, 'dither', 0.0) != 0 or self.model is not base  # (a defended model may hold a randomised defense)
        if noisy:
            cuts = [0] + [k for k in range(1, len(consider_index)) if consider_index[k] != consider_index[k - 1] + 1]
            runs = list(zip(cuts, cuts[1:] + [len(consider_index)]))
        saved = base._index_base, base._draw, base._def_draw
        losses, decisions = [], []
        try:
            base._row_scale = P  # slot e of the chunk owns rows [e * P, (e + 1) * P) of the full call
            for k0, k1 in runs:
                base._index_base = index_base + (consider_index[k0] if noisy else 0)
                base._draw, base._def_draw = saved[1], saved[2]
                _, loss, _, dec = self.EOT_wrapper(eval_x[k0 * P:k1 * P], eval_y[k0 * P:k1 * P])
                losses.append(loss)
                decisions += dec
        finally:
            base._row_scale, base._index_base = 1, saved[0]
        return (losses[0] if len(losses) == 1 else torch.cat(losses)), decisions

    def attack_batch(self, x_batch, y_batch, lower, upper, batch_id):
        n_audios, n_channels, N = x_batch.shape
        P = self.n_particles
        device = x_batch.device
        base = getattr(self.model, 'base_model', self.model)
        swarm = self.swarm if self.swarm is not None else base
        x_batch, lower, upper = x_batch.contiguous(), lower.contiguous(), upper.contiguous()
        st = SwarmState(n_audios, P, N, device)
        index_base = self.index_offset + self._chunk_start
        consider_index = list(range(n_audios))
        # the values the host decides on, on the host (the swarm keeps its own): :55-58
        gbests = torch.full((n_audios,), np.inf, dtype=torch.float32)
        gbest_predict = np.array([None] * n_audios)
        prev_gbest = gbests.clone()
        prev_gbest_epoch = gbests.clone()
        EOT_num_batches = int(self.EOT_wrapper.EOT_size // self.EOT_wrapper.EOT_batch_size)
        epochs_run, iters_run, losses = [0] * n_audios, [0] * n_audios, []
        best_index = None

        continue_flag = True
        for epoch in range(self.max_epoch):
            if not continue_flag:
                break
            rows = torch.tensor(consider_index, dtype=torch.long, device=device)
            pos_in = vel_in = None
            if self.draw_fn is not None:  # :67 / :74, :84 with the reference's bounds
                lo, hi = lower[rows].unsqueeze(1).cpu().numpy(), upper[rows].unsqueeze(1).cpu().numpy()
                v_hi = torch.abs(lower[rows] - upper[rows]).unsqueeze(1).cpu().numpy()
                fresh = P if epoch == 0 else P - 1
                pos_in = self._draw('uniform', (len(consider_index), fresh, n_channels, N), lo, hi).to(device)
                vel_in = self._draw('uniform', (len(consider_index), P, n_channels, N), -v_hi, v_hi).to(device)
            eval_x = swarm.pso_init(st, x_batch, lower, upper, consider_index, epoch, best_index,
                                    self._key(base, epoch * (self.max_iter + 2)), index_base, pos_in, vel_in)
            for ii in consider_index:
                epochs_run[ii] += 1

            continue_flag_inner = True
            for iter in range(self.max_iter + 1):
                if not continue_flag_inner:
                    break
                loss, decisions = self._evaluate(base, eval_x, y_batch[rows].repeat_interleave(P), consider_index, index_base)
                loss = (loss / EOT_num_batches).view(len(consider_index), -1).contiguous()  # :111-112
                if self.record:
                    losses.append((list(consider_index), loss.cpu().numpy().copy()))
                for ii in consider_index:
                    iters_run[ii] += 1

                # :115-132: values on the device, one read
                g_rows, argmin, gbest_from = swarm.pso_select(st, loss, consider_index)
                gbests[consider_index] = torch.from_numpy(np.asarray(g_rows, dtype=np.float32))
                if self.verbose:
                    predict = resolve_prediction(decisions).reshape(len(consider_index), -1)
                    for kk, index in enumerate(consider_index):
                        if gbest_from[kk] >= 0:
                            gbest_predict[index] = predict[kk, gbest_from[kk]]
                    print('batch: {}, epoch: {}, iter: {}, y: {}, y_pred: {}, gbest: {}'.format(
                        batch_id, epoch, iter, y_batch[rows].cpu().numpy().tolist(), gbest_predict[consider_index],
                        gbests[consider_index].numpy().tolist()))

                if self.abort_early and (iter + 1) % self.abort_early_iter == 0:
                    if torch.mean(gbests) > 0.9999 * torch.mean(prev_gbest):
                        if self.verbose:
                            print('Converge, Break Inner Loop')
                        continue_flag_inner = False
                    prev_gbest = gbests.clone()

                # delete_found (:191-232): the rows whose global best is negative leave the list, their state stays
                cont = [0 if g < 0 else 1 for g in g_rows]
                consider_index_u = [index for index, c in zip(consider_index, cont) if c]
                moves = iter < self.max_iter and len(consider_index_u) > 0
                r1 = r2 = None
                if moves and self.draw_fn is not None:  # :167-168
                    shape = (len(consider_index_u), P, n_channels, N)
                    r1 = self._draw('rand', shape, 0.0, 1.0, 0.00001)
                    r2 = self._draw('rand', shape, 0.0, 1.0, 0.00001)
                    # (taken in the reference's order even when the update they feed is not computed, see above)
                    r1, r2 = (r1.to(device), r2.to(device)) if continue_flag_inner else (None, None)
                w = (self.w_init - self.w_end) * (self.max_iter - iter - 1) / self.max_iter + self.w_end  # :164
                # :121, :131 for every row, :171-174 and the next queries for the rows that go on
                eval_x = swarm.pso_move(st, x_batch, lower, upper, consider_index, gbest_from, cont,
                                        moves and continue_flag_inner, w, self.c1, self.c2,
                                        self._key(base, epoch * (self.max_iter + 2) + 1 + iter), index_base, r1, r2)
                best_index = [int(a) for a, c in zip(argmin, cont) if c]  # :72 of the next epoch
                consider_index = consider_index_u
                if len(consider_index) == 0:
                    continue_flag = False  # used to break the outer loop
                    break
                rows = torch.tensor(consider_index, dtype=torch.long, device=device)

            if self.abort_early and (epoch + 1) % self.abort_early_epoch == 0:
                if torch.mean(gbests) > 0.9999 * torch.mean(prev_gbest_epoch):
                    if self.verbose:
                        print('Converge, Break Outer Loop')
                    continue_flag = False
                prev_gbest_epoch = gbests.clone()

        success = [bool(best_l < 0) for best_l in gbests]
        self.final_gbest += gbests.tolist()
        self.epochs_run += epochs_run
        self.iters_run += iters_run
        if self.record:
            self.loss_record.append(losses)
        return st.gbest_loc.view(n_audios, n_channels, N) + x_batch, success

    def attack(self, x, y, lengths=None):
        refuse_lengths(self, lengths)
        if self.task in ['SV', 'OSI'] and self.threshold is None:
            raise NotImplementedError('You are running black box attack for {} task, '
                                      'but the threshold not specified. Consider Estimating the threshold by FAKEBOB!'.format(self.task))
        self.loss, self.grad_sign = resolve_loss('Margin', self.targeted, self.confidence, self.task, self.threshold, False)
        self.EOT_wrapper = EOT(self.model, self.loss, self.EOT_size, self.EOT_batch_size, False)

        lower, upper = -1, 1
        assert lower <= x.max() < upper, 'generating adversarial examples should be done in [-1, 1) float domain'
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        lower = torch.clamp(-1 - x, min=-self.epsilon)  # for distortion, not adver audio
        upper = torch.clamp(1 - x, max=self.epsilon)    # for distortion, not adver audio

        batch_size = min(self.batch_size, n_audios)
        if batch_size > MAX_CHUNK or not 1 <= self.n_particles <= MAX_PARTICLES:
            raise ValueError('SirenAttack takes chunks of at most %d utterances (batch_size) and 1 .. %d particles, got %d and %d'
                             % (MAX_CHUNK, MAX_PARTICLES, batch_size, self.n_particles))
        n_batches = int(np.ceil(n_audios / float(batch_size)))
        self.final_gbest, self.epochs_run, self.iters_run = [], [], []
        self.loss_record = [] if self.record else None
        base = getattr(self.model, 'base_model', self.model)
        if hasattr(base, 'begin_attack'):
            base.begin_attack()
        adver, success = [], []
        for batch_id in range(n_batches):
            sl = slice(batch_id * batch_size, (batch_id + 1) * batch_size)
            self._chunk_start = sl.start
            if hasattr(base, 'begin_batch'):  # swarm draws and the model's noise are keyed by global utterance index (_evaluate)
                base.begin_batch(self.index_offset + sl.start, 0)
            a, s = self.attack_batch(x[sl], y[sl], lower[sl], upper[sl], batch_id)
            adver.append(a)
            success += s
        if hasattr(base, 'check_health'):  # see FGSM._run_batches
            base.check_health()
        return torch.cat(adver, 0), success
