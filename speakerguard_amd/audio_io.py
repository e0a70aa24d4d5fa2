"""On-disk format of the adversarial audio; mirrors reference attackMain.py:154-166 save_audio.

The int16 quantisation (x * 2^15 when the utterance is in the float domain, then numpy's truncating, wrapping
astype(int16)) runs on the device in the same pass as the perturbation metrics (C-ABI ``sg_wav_finalize``);
only the resulting PCM crosses PCIe (96 KB per 3-s utterance instead of 192 KB).
"""
import os

import torch
from scipy.io.wavfile import write

from . import _native as N
from .metric.metric import _context


def pad_batch(waves):
    """Utterances of unequal lengths as one batch: a list of (1, T_b) or (T_b,) tensors -> (x, lengths), x (B, 1, T_max)
    zero-padded on the right (dtype and device of the first utterance) and lengths (B,) int32 sample counts on the host.
    The pair is what ``xv_plda.make_decision / score / forward / loss_grad / pgd_run`` and ``FGSM / PGD / CWinf.attack`` take
    as ``(x, lengths=lengths)``: row b is then treated as utterance b alone at its own length."""
    waves = list(waves)
    if not waves:
        raise ValueError("pad_batch needs at least one utterance")
    flat = []
    for i, w in enumerate(waves):
        if not torch.is_tensor(w) or w.dim() not in (1, 2) or (w.dim() == 2 and w.shape[0] != 1) or w.shape[-1] < 1:
            raise ValueError("utterance %d: expected a (1, T) or (T,) tensor, got %s" % (
                i, tuple(w.shape) if torch.is_tensor(w) else type(w).__name__))
        flat.append(w.reshape(-1))
    lengths = torch.tensor([w.shape[0] for w in flat], dtype=torch.int32)
    x = torch.zeros(len(flat), 1, int(lengths.max()), dtype=flat[0].dtype, device=flat[0].device)
    for b, w in enumerate(flat):
        x[b, 0, :w.shape[0]] = w.to(x.device, x.dtype)
    return x, lengths


def quantize_pcm(advers):
    """(N,1,T) or (N,T) float tensor -> (N,T) int16 CPU numpy array, reference save_audio rounding."""
    a = advers.detach().to(torch.float32)
    a = a.reshape(a.shape[0], -1)
    if not a.is_cuda:
        a = a.to("cuda:0")
    a = a.contiguous()
    pcm = torch.empty(a.shape, device=a.device, dtype=torch.int16)
    _context(a.device).call("sg_wav_finalize", None, N._ptr(a), a.shape[0], a.shape[1], N._ptr(pcm), None,
                            N.current_stream_ptr(a.device))
    return pcm.cpu().numpy()


def save_audio(advers, names, root, fs=16000):
    """Writes root/<spk_id>/<name>.wav for every utterance (spk_id = name.split('-')[0], :161-166)."""
    pcm = quantize_pcm(advers)
    for adver, name in zip(pcm, names):
        spk_dir = os.path.join(root, name.split("-")[0])
        os.makedirs(spk_dir, exist_ok=True)
        write(os.path.join(spk_dir, name + ".wav"), fs, adver)
