"""Kenan's signal-processing black-box attack, the batched ``fft`` variant (reference attack/Kenan.py and
attack/_kenan_fft.py:57-82, :180-245): zero every frequency bin below a per-utterance magnitude and bisect that magnitude on the
model's decision.  The gate -- whole-utterance rfft, magnitude gate, irfft -- is one native launch (csrc/k_spectrum.hip); the
model is queried through ``make_decision`` only.

Faithfulness notes:
  * the factor bisection runs per utterance in float32, ``|(min + max) / 2|``, from ``peak / 2`` (:196-200, :236-241); here
    the three float32 vectors live on the host (the same IEEE operations), and the peak is the native ``max_k |rfft(x)|``
    (the reference takes it over the full complex FFT: the same set of magnitudes);
  * ``succ`` is sticky and ``mistranscribed_audio`` changes only on a success (:232-238): a failed utterance comes back
    equal to its input;
  * ``early_stop`` is accepted and unused (:180), ``raster_width`` is not read by the ``fft`` variant (:196-198);
  * the whole chunk is queried at every iteration, succeeded utterances included (:226);
  * ``atk_name='ssa'`` is a class of its own, ``speakerguard_amd.attack.KenanSSA.KenanSSA`` (int16 audio, a native
    decomposition per utterance, a native reconstruction per query); asked for here it is a NotImplementedError that says so.
"""
from .utils import refuse_lengths
import numpy as np
import torch

from .. import _native as N


def _rows(audio):
    if not isinstance(audio, torch.Tensor) or audio.dim() != 3 or audio.shape[1] != 1:
        raise ValueError("the spectrum gate takes a (N, 1, T) tensor")
    from ..metric.metric import _context
    ctx = _context(audio.device)  # (a CPU tensor: NativeError)
    x = audio.detach().to(torch.float32).contiguous()
    return ctx, x, x.shape[0], x.shape[2]


def wav_spectrum(audio, want_spec=True):
    """(rfft of every utterance as a complex64 (N, 1, T/2+1) tensor or None, peak (N,) = the largest magnitude)"""
    ctx, x, n, T = _rows(audio)
    spec = torch.empty((n, 1, T // 2 + 1, 2), dtype=torch.float32, device=x.device) if want_spec else None
    peak = torch.empty((n,), dtype=torch.float32, device=x.device)
    ctx.call("sg_wav_spectrum", N._ptr(x), n, T, N._ptr(spec), N._ptr(peak), N.current_stream_ptr(x.device))
    return (torch.view_as_complex(spec) if want_spec else None), peak


def wav_spectrum_gate(audio, factor, want_keep=False):
    """irfft of the spectrum with every bin below factor[n] zeroed: (N, 1, T); with ``want_keep`` also the mask of the bins
    that stayed (N, T/2+1) uint8 and their count (N,) int32"""
    ctx, x, n, T = _rows(audio)
    f = torch.as_tensor(factor, dtype=torch.float32).to(x.device).reshape(-1).contiguous()
    if f.shape[0] != n:
        raise ValueError("one factor per utterance: %d for %d" % (f.shape[0], n))
    out = torch.empty_like(x)
    keep = torch.empty((n, T // 2 + 1), dtype=torch.uint8, device=x.device) if want_keep else None
    kept = torch.empty((n,), dtype=torch.int32, device=x.device) if want_keep else None
    ctx.call("sg_wav_spectrum_gate", N._ptr(x), n, T, N._ptr(f), N._ptr(out), N._ptr(keep), N._ptr(kept),
             N.current_stream_ptr(x.device))
    return (out, keep, kept) if want_keep else out


def fft_compression(audio, factor):
    """the reference's ``fft_compression(audio_image, factor, fs)`` (_kenan_fft.py:57-82) on (N, 1, T), natively"""
    return wav_spectrum_gate(audio, factor)


def spectrum_peak(audio):
    """max_k |fft(x)[k]| per utterance (_kenan_fft.py:198), natively"""
    return wav_spectrum(audio, want_spec=False)[1]


class Kenan(object):

    chunk_coupling = None  # utterances are independent: shard.ShardedAttack may cut anywhere

    def __init__(self, model, atk_name='fft', max_iter=15, raster_width=100, early_stop=False, targeted=False, verbose=1,
                 BITS=16, batch_size=1, gate=None, peak=None):
        if atk_name == 'ssa':
            raise NotImplementedError("Kenan's ssa variant is speakerguard_amd.attack.KenanSSA.KenanSSA(model, ...); this class runs atk_name='fft'")
        if atk_name != 'fft':
            raise NotImplementedError("unknown Kenan variant %r (built: 'fft')" % (atk_name,))
        self.model = model  # remember to call model.eval()
        self.atk_name = atk_name
        self.max_iter = max_iter
        self.raster_width = raster_width  # for ssa
        self.targeted = targeted
        self.verbose = verbose
        self.BITS = BITS
        self.early_stop = early_stop
        self.batch_size = batch_size
        # the gate (audio (N,1,T), factor (N,)) -> (N,1,T) and the peak audio -> (N,): the native ones unless given
        self.gate = fft_compression if gate is None else gate
        self.peak = spectrum_peak if peak is None else peak
        self.last_factors = None
        self.factor_history = None
        self.decision_history = None

    def atk_bst_fft(self, data, og_label):
        """_kenan_fft.py:180-245 -> (mistranscribed audio, succ list, last successful factor (n,), factors (iters, n),
        decisions (iters, n))"""
        n_audios = data.shape[0]
        device = data.device
        labels = [int(v) for v in torch.as_tensor(og_label).reshape(-1).tolist()]
        mistranscribed_audio = data.clone()
        min_attack_factor = torch.zeros(n_audios, dtype=torch.float32)
        max_attack_factor = self.peak(data).detach().to(torch.float32).cpu().reshape(-1).clone()
        attack_factor = max_attack_factor / 2
        last = torch.full((n_audios,), float('nan'), dtype=torch.float32)
        succ = [False] * n_audios
        factors, decisions = [], []
        itr = 0
        while itr < self.max_iter:
            perturbed_audio = self.gate(data.clone(), attack_factor.to(device))
            transcribed, _ = self.model.make_decision(perturbed_audio)
            transcribed = [int(v) for v in torch.as_tensor(transcribed).reshape(-1).tolist()]
            if self.verbose:
                print('Iter: {} ori: {} atk: {} f: {}'.format(itr + 1, labels, transcribed, attack_factor))
            factors.append(attack_factor.clone())
            decisions.append(torch.tensor(transcribed, dtype=torch.int64))
            hit = torch.tensor([(labels[p] != transcribed[p] and not self.targeted) or
                                (labels[p] == transcribed[p] and self.targeted) for p in range(n_audios)], dtype=torch.bool)
            mistranscribed_audio = torch.where(hit.to(device).view(-1, 1, 1), perturbed_audio, mistranscribed_audio)
            last = torch.where(hit, attack_factor, last)
            max_attack_factor = torch.where(hit, attack_factor, max_attack_factor)
            min_attack_factor = torch.where(hit, min_attack_factor, attack_factor)
            attack_factor = ((min_attack_factor + max_attack_factor) / 2).abs()
            succ = [s or bool(h) for s, h in zip(succ, hit.tolist())]
            itr = itr + 1
        empty_f, empty_d = torch.zeros((0, n_audios), dtype=torch.float32), torch.zeros((0, n_audios), dtype=torch.int64)
        return (mistranscribed_audio, succ, last, torch.stack(factors) if factors else empty_f,
                torch.stack(decisions) if decisions else empty_d)

    def attack_batch(self, x_batch, y_batch, batch_id, fs=16_000):
        adv, success, last, factors, decisions = self.atk_bst_fft(x_batch, y_batch)
        self._records.append((last, factors, decisions))
        return adv, success

    def attack(self, x, y, fs=16_000, lengths=None):
        refuse_lengths(self, lengths)
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        self._records = []
        batch_size = min(self.batch_size, n_audios)
        n_batches = int(np.ceil(n_audios / float(batch_size)))
        for batch_id in range(n_batches):
            x_batch = x[batch_id * batch_size:(batch_id + 1) * batch_size]  # (batch_size, 1, max_len)
            y_batch = y[batch_id * batch_size:(batch_id + 1) * batch_size]
            adver_x_batch, success_batch = self.attack_batch(x_batch, y_batch, batch_id, fs=fs)
            if batch_id == 0:
                adver_x = adver_x_batch
                success = success_batch
            else:
                adver_x = torch.cat((adver_x, adver_x_batch), 0)
                success += success_batch
        # per utterance: the factor of its last success (NaN: none), and every iteration's factor and decision
        self.last_factors = torch.cat([r[0] for r in self._records])
        self.factor_history = torch.cat([r[1] for r in self._records], 1)
        self.decision_history = torch.cat([r[2] for r in self._records], 1)
        return adver_x, success
