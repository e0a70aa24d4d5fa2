"""FGSM and the shared PGD inner loop; mirrors reference attack/FGSM.py.

``attack_batch`` is the hot loop (FGSM.py:38-70).  When the model is the native x-vector engine
and nothing between attack and model needs Python (no defense wrapper), the whole loop, EOT repeats
over the front-end's random dither included -- max_iter x (forward, hand-coded backward, sign step,
projection) + the final forward-only pass -- is ONE C-ABI call (``model.pgd_run``).  A wrapper that
carries only native waveform-level defenses in sequential order runs the same way, the chain inside
the loop (``model.pgd_run_defended``), and so do one FeCoDefense on AudioNet or on the x-vector model
(``model.pgd_run_feco``) and, on AudioNet, such a chain in front of it (``model.pgd_run_defended_feco``).  ``_device_route`` is the one place that
decides this, once per batch, from one reading of the model; ``attack_batch`` makes the one call it
names.  Otherwise the same loop runs step by step over ``model.loss_grad`` / ``model.pgd_update``.
"""
import types

import numpy as np
import torch

from ..adaptive_attack.EOT import EOT
from .Attack import Attack
from .utils import resolve_loss, resolve_prediction


class _Route(tuple):
    """``(method name, extra positional arguments)`` of a device loop, with the keyword arguments the call takes besides.
    A tuple subclass and not a 3-tuple because tests/test_device_route.py and the GPU tests pin the routes as 2-tuples
    (``name, extra = route``, ``route == ('pgd_run', ())``); the one keyword so far is FeCo's ``level``."""
    kwargs = types.MappingProxyType({})  # (read-only default; every instance gets its own dict)

    def __new__(cls, name, extra, **kwargs):
        self = super().__new__(cls, (name, extra))
        self.kwargs = kwargs
        return self


class FGSM(Attack):

    def __init__(self, model, task='CSI', epsilon=0.002, loss='Entropy', targeted=False,
                 batch_size=1, EOT_size=1, EOT_batch_size=1,
                 verbose=1):
        self.model = model  # the engine has no train mode
        self.task = task
        self.epsilon = epsilon
        self.loss_name = loss
        self.targeted = targeted
        self.batch_size = batch_size
        self._init_common(EOT_size, EOT_batch_size, verbose)
        self.max_iter = 1  # FGSM is the single-step case of PGD (FGSM.py:35-36)
        self.step_size = epsilon

    def _init_common(self, EOT_size, EOT_batch_size, verbose):
        EOT_size = max(1, EOT_size)
        EOT_batch_size = max(1, EOT_batch_size)
        assert EOT_size % EOT_batch_size == 0, 'EOT size should be divisible by EOT batch size'
        self.EOT_size = EOT_size
        self.EOT_batch_size = EOT_batch_size
        self.verbose = verbose
        self.threshold = None
        if self.task in ['SV', 'OSI']:
            self.threshold = self.model.threshold
            print('Running white box attack for {} task, directly using the true threshold {}'.format(self.task, self.threshold))
        self.loss, self.grad_sign = resolve_loss(loss_name=self.loss_name, targeted=self.targeted,
                                                 task=self.task, threshold=self.threshold, clip_max=False)
        self.EOT_wrapper = EOT(self.model, self.loss, self.EOT_size, self.EOT_batch_size, True)

    # ---- device-resident loop ---------------------------------------------------------------
    fuse_defended = True  # False: PGD against a FeCo-defended model runs the host-chained loop (tests compare the two)
    fuse_input_defenses = True  # False: ... against native input-level defenses likewise (tests, tools/defended_loop_time.py)
    fuse_randomised_input_defenses = False  # True: chains holding AT run on the device too, with the device loop's noise keys
    fuse_randomised_feco = False  # True: FeCo on a base that re-keys (xv_plda) takes its loop with dither / random init too

    def _device_route(self, n_audios):
        """Which device-resident loop of the base model runs ``attack_batch`` for a batch of `n_audios`: None for the step loop
        below, else ``(method name, extra arguments)`` -- ``('pgd_run', ())`` for a model without defenses, ``('pgd_run_feco',
        (feco,))``, ``('pgd_run_defended', (chain,))`` or ``('pgd_run_defended_feco', (chain, feco))`` for a ``defended_model`` in
        sequential order whose defenses are

          * chain: 1 .. 8 native waveform defense objects (defense.time_domain / defense.frequency_domain) as they stand -- no
            BPDA wrapper, no Python callable -- and exactly what the model applies at level 0 (``flag2defense[0]``); a defense
            that is no stage of the loops yet (``device_loop`` False: ``DS``) keeps the whole chain on the step loop;
          * feco: the one entry that is not at level 0, a FeCoDefense at level 1 -- or at another level the base model lists in
            ``feco_loop_levels`` (xv_plda: 2; the route then carries ``level=``), without a chain; needs ``fuse_defended`` and two
            utterances (one: the reference drops empty clusters, the frame count varies -> host path).  Only the L2 distance:
            the loops cluster with L2, a cosine FeCo (``other_param='cos'``) inside one would silently be another defense.

        A randomised stage (AT) draws DIFFERENT noise on the two routes for the same seed: the device loop keys a pass by
        (step, repeat), the step loop by the defense's call number.  An attack's result must not change under its user, so such
        a chain keeps the step loop unless ``fuse_randomised_input_defenses`` asks for the device loop's schedule, and always
        in front of FeCo (the clusterings' gradients are summed behind ONE chain pass).  The same holds for FeCo on a base whose
        loop re-keys the noise (``feco_loop_rekeys``: xv_plda, whose loop keys dither and random init by (step, repeat)): with a
        dithered front-end or ``init='random'`` it keeps the step loop unless ``fuse_randomised_feco`` is set; the deterministic
        configuration is bit-equal on both routes and takes the loop by default.  AudioNet's loop does not re-key.  The base
        model says what it offers by having the method; one that has the methods only to refuse them (iv_plda) says
        ``device_loops = False`` and keeps the step loop."""
        m = self.model
        defense = getattr(m, 'defense', None)
        base = getattr(m, 'base_model', m if defense is None else None)
        route = None
        if defense is None:
            # EOT repeats of a deterministic model are identical (one pass stands for all of them); with random dither
            # the engine runs the repeats itself and sums their gradients on the device
            route = 'pgd_run', ()
        elif getattr(m, 'order', None) == 'sequential':
            from ..defense.feature_level import FeCoDefense
            from ..defense.time_domain import _WavDefense
            chain = [d for flag, d in defense if flag == 0]
            rest = [(flag, d) for flag, d in defense if flag != 0]
            chain_ok = (self.fuse_input_defenses and 1 <= len(chain) <= 8 and all(isinstance(d, _WavDefense) for d in chain)
                        and all(getattr(d, 'device_loop', True) for d in chain)
                        and chain == m.flag2defense.get(0, []))  # (what process_sequential applies, in its order)
            randomised = any(getattr(d, 'randomised', False) for d in chain)
            if not rest:
                if chain_ok and (self.fuse_randomised_input_defenses or not randomised):
                    route = 'pgd_run_defended', (chain,)
            elif (len(rest) == 1 and isinstance(rest[0][1], FeCoDefense) and getattr(rest[0][1], 'other_param', 'L2') == 'L2'
                  and self.fuse_defended and n_audios >= 2):
                level, feco = rest[0]
                noisy = feco.init == 'random' or float(getattr(base, 'dither', 0.0)) != 0.0
                if getattr(base, 'feco_loop_rekeys', False) and noisy and not self.fuse_randomised_feco:
                    pass  # the loop would draw other noise than the step loop does for this seed
                elif level == 1:
                    if not chain:
                        route = 'pgd_run_feco', (feco,)
                    elif chain_ok and not randomised and m.flag2defense.get(1, []) == [feco]:
                        route = 'pgd_run_defended_feco', (chain, feco)
                elif not chain and level in getattr(base, 'feco_loop_levels', (1,)):
                    route = _Route('pgd_run_feco', (feco,), level=level)
        if route is None or not hasattr(base, route[0]) or not getattr(base, 'device_loops', True):
            return None
        return route if isinstance(route, _Route) else _Route(*route)

    def _attack_batch_fused(self, x_batch, y_batch, lower, upper, batch_id, name, extra, **kwargs):
        # (kwargs: the route's own keywords and, for a padded batch of unequal lengths, ``lengths`` -- never passed when None)
        base = getattr(self.model, 'base_model', self.model)
        x_adv, success, dec, scores, loss, ltr, dtr = getattr(base, name)(
            x_batch, y_batch, lower, upper, self.loss, self.step_size, self.max_iter, self.grad_sign, *extra,
            self.EOT_size, self.EOT_batch_size, trace=bool(self.verbose), **kwargs)
        if self.verbose:
            ltr, dtr = ltr.cpu().numpy(), dtr.cpu().numpy()
            target = y_batch.detach().cpu().numpy()
            for it in range(self.max_iter + 1):
                print("batch:{} iter:{} loss: {} predict: {}, target: {}".format(batch_id, it, ltr[it].tolist(), dtr[it], target))
        return x_adv, [bool(v) for v in success.tolist()]  # (one device round trip, no conversion launch)

    # ---- step-by-step loop (FGSM.py:38-70) ---------------------------------------------------
    def attack_batch(self, x_batch, y_batch, lower, upper, batch_id, lengths=None):
        """`lengths` (n,) int32: the chunk is a padded batch of unequal lengths, its longest utterance filling the row; bounds
        and start point are already 0 in the padding (``_mask_padding``).  It goes to ``pgd_run`` / ``loss_grad`` as the
        keyword ``lengths`` -- a call without lengths is made exactly as before."""
        ragged = {} if lengths is None else {'lengths': lengths}
        route = self._device_route(x_batch.shape[0])
        if route is not None:
            return self._attack_batch_fused(x_batch, y_batch, lower, upper, batch_id, *route, **getattr(route, 'kwargs', {}), **ragged)
        x_batch = x_batch.clone()
        lower = lower.expand_as(x_batch).contiguous()
        upper = upper.expand_as(x_batch).contiguous()
        base = getattr(self.model, 'base_model', self.model)
        success = None
        for it in range(self.max_iter + 1):
            EOT_num_batches = int(self.EOT_size // self.EOT_batch_size) if it < self.max_iter else 1
            real_EOT_batch_size = self.EOT_batch_size if it < self.max_iter else 1
            use_grad = it < self.max_iter
            scores, loss, grad, decisions = self.EOT_wrapper(x_batch, y_batch, EOT_num_batches, real_EOT_batch_size, use_grad, **ragged)
            loss = loss / EOT_num_batches
            predict = resolve_prediction(decisions)
            target = y_batch.detach().cpu().numpy()
            success = self.compare(target, predict, self.targeted)
            if self.verbose:
                print("batch:{} iter:{} loss: {} predict: {}, target: {}".format(batch_id, it, loss.cpu().numpy().tolist(), predict, target))
            if it < self.max_iter:
                grad = (grad / EOT_num_batches).contiguous()
                base.pgd_update(x_batch, grad, lower, upper, self.step_size, self.grad_sign)
        return x_batch, success

    index_offset = 0  # global index of x[0] when this object attacks one shard of a larger batch (shard.py)
    chunk_coupling = None  # nothing ties the examples of a chunk together (EOT.py:33-35: per-example loss vector)

    def _begin_attack(self):
        base = getattr(self.model, 'base_model', self.model)
        if hasattr(base, 'begin_attack'):
            base.begin_attack()

    def _begin_batch(self, start, tag=None):
        # noise streams (dither, NES) are keyed by the chunk's GLOBAL position, not by what ran before it
        base = getattr(self.model, 'base_model', self.model)
        if hasattr(base, 'begin_batch'):
            base.begin_batch(self.index_offset + start, 0 if tag is None else int(tag) + 1)

    def _run_batches(self, x, y, lower, upper, tag=None, lengths=None):
        base = getattr(self.model, 'base_model', self.model)
        if lengths is not None:  # (no stream-K retry around a padded batch: kept to the one path the tests pin)
            return self._run_batches_once(x, y, lower, upper, tag, lengths)
        try:
            return self._run_batches_once(x, y, lower, upper, tag)
        except Exception as e:  # the engine's NativeError (kept generic: the CPU test double has no such class)
            # A stream-K hand-off that timed out (the GPU was shared: include/speakerguard_hip.h, sg_set_streamk): the
            # inputs are untouched (attack_batch works on copies) and the noise keys depend on positions only, so the
            # batches are run again, once, as one block per tile -- the same bits, no residency requirement.
            if 'hand-off' not in str(e) or not hasattr(base, 'set_streamk') or getattr(base, 'streamk', True) is False:
                raise
            import warnings
            warnings.warn('a stream-K hand-off timed out (is another process using this GPU?): this model now runs its contractions '
                          'as one block per tile (same results, a few percent slower); model.set_streamk(True) switches back')
            base.set_streamk(False)
            return self._run_batches_once(x, y, lower, upper, tag)

    def _run_batches_once(self, x, y, lower, upper, tag=None, lengths=None):
        """`lengths`: sliced with the batch.  A chunk is cut to ITS longest utterance (the engine wants the longest to fill the
        row, and shorter rows cost less) and its result is zero-padded back to the width of x."""
        n_audios = x.shape[0]
        batch_size = min(self.batch_size, n_audios)
        n_batches = int(np.ceil(n_audios / float(batch_size)))
        adver, success = [], []
        for batch_id in range(n_batches):
            sl = slice(batch_id * batch_size, (batch_id + 1) * batch_size)
            bid = batch_id if tag is None else '{}-{}'.format(tag, batch_id)
            self._begin_batch(sl.start, tag)
            if lengths is not None:
                T = int(lengths[sl].max())
                a, s = self.attack_batch(x[sl, :, :T], y[sl], lower[sl, :, :T], upper[sl, :, :T], bid, lengths=lengths[sl])
                a = torch.nn.functional.pad(a, (0, x.shape[2] - T))
            else:
                a, s = self.attack_batch(x[sl], y[sl], lower[sl], upper[sl], bid)
            adver.append(a)
            success += s
        # the success flags are on the host, so every launch of these batches has finished: a kernel that flagged
        # its own output as invalid (engine health word) must not go unnoticed
        base = getattr(self.model, 'base_model', self.model)
        if hasattr(base, 'check_health'):
            base.check_health()
        return (adver[0] if len(adver) == 1 else torch.cat(adver, 0)), success  # (one batch: attack_batch's own output tensor)

    def _check_inputs(self, x, y):
        lower, upper = -1, 1
        peak = float(x.max())  # one device round trip (the reference's chained comparison on the tensor makes two)
        assert lower <= peak < upper, 'generating adversarial examples should be done in [-1, 1) float domain'
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'

    # ---- padded batches of unequal lengths ---------------------------------------------------
    def _check_lengths(self, x, lengths):
        """What ``attack(x, y, lengths=)`` refuses before anything runs: a model that cannot take lengths -- by name, so that
        nobody attacks padding unawares -- and lengths that do not describe x.  -> lengths as a host int32 tensor."""
        m = self.model
        if getattr(m, 'defense', None) is not None:
            raise ValueError("%s with a defense in place does not take lengths=: the defenses handle batches of one length only"
                             % type(m).__name__)
        base = getattr(m, 'base_model', m)
        if not getattr(base, 'takes_lengths', False):
            raise ValueError("%s does not take lengths=: it handles batches of one length only" % type(base).__name__)
        if not torch.is_tensor(lengths) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (x.shape[0],):
            raise ValueError("lengths must be an int32 tensor of shape (%d,), one sample count per row of x" % x.shape[0])
        lengths = lengths.detach().cpu()
        if int(lengths.min()) < 1 or int(lengths.max()) > x.shape[2]:
            raise ValueError("lengths must lie in 1 .. %d, the width of x" % x.shape[2])
        return lengths

    @staticmethod
    def _mask_padding(lengths, *tensors):
        """every (B, 1, T) tensor with zeros behind its rows' own samples: start point, bounds, random-init noise"""
        T = tensors[0].shape[2]
        keep = (torch.arange(T).unsqueeze(0) < lengths.to(torch.int64).unsqueeze(1)).unsqueeze(1).to(tensors[0].device)
        out = tuple(torch.where(keep, t, torch.zeros((), dtype=t.dtype, device=t.device)) for t in tensors)
        return out if len(out) > 1 else out[0]

    def attack(self, x, y, lengths=None):
        """`lengths` (B,) int32: x is a padded batch of utterances of unequal lengths (``audio_io.pad_batch``).  Every utterance
        is attacked as it would be alone at its own length; the returned audio is 0 in the padding whatever x held there."""
        if lengths is not None:
            lengths = self._check_lengths(x, lengths)
            x = self._mask_padding(lengths, x)
        self._check_inputs(x, y)
        self._begin_attack()
        lower = torch.tensor(-1, device=x.device, dtype=x.dtype).expand_as(x)
        upper = torch.tensor(1, device=x.device, dtype=x.dtype).expand_as(x)
        if lengths is not None:
            lower, upper = self._mask_padding(lengths, lower, upper)
            return self._run_batches(x, y, lower, upper, lengths=lengths)
        return self._run_batches(x, y, lower, upper)
