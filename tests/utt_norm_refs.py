"""Plain references of the utterance normalisation (processor.compute_w2vbert_fbank,
processor.py:269-270): the reference's two torch calls on ONE utterance, in fp64 or fp32."""
import torch

import kernel_refs as KR

SLAB = 128                     # csrc/kernels.h UTT_SLAB
# 0 and 1 (no statistics, no row) between live utterances; both sides of one slab, of a wave's 32
# frames inside the third slab (2 slab + 1), and 1000 frames = 8 slabs, the last one partial
LENS = [3, 0, SLAB - 1, 1, SLAB, 2, SLAB + 1, 2 * SLAB + 1, 1000]
T_PAD = 1001
REGIMES = ['unit', 'fbank', 'offset', 'scaled']


def normalize(x, fp32=False):
    """(n, F), n >= 2 -> (mean, std, normalised) in fp64 or fp32."""
    x = x.float() if fp32 else x.double()
    std, mean = torch.std_mean(x, dim=0)
    return mean, std, x.subtract(mean).divide(std)


def stack_ln(y, w, b, eps=1e-5):
    """Normalised frames (n, F) -> LayerNorm over frames 2t | 2t + 1, (n // 2, 2 F)."""
    n = y.shape[0] // 2
    y = y[:2 * n].reshape(n, -1)
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    return (y - mu) / torch.sqrt(var + eps) * w.to(y.dtype) + b.to(y.dtype)


def utterance(regime, F, i, n):
    """Utterance i of a regime: the same values wherever it stands in the batch."""
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + i)
    x = torch.randn(n, F, generator=g)
    if regime == 'fbank':          # log-mel energies: mean 8, std 2, both varying with the bin
        x = x * (2.0 + 0.5 * torch.sin(torch.arange(F) * 0.3)) + 8.0 + torch.cos(
            torch.arange(F) * 0.2)
    elif regime == 'offset':
        # mean 1e3, std 1: a raw one-pass variance loses every digit here.  On a grid of 2^-10, so
        # that the mean of a 2-frame utterance is a fp32 number: off the grid the plain fp32
        # formula itself breaks the cap there (a bin whose two frames differ by 0.02 turns the
        # half ulp of its mean, 3e-5, into 1.5e-3 of an output of size 0.7)
        x = torch.round((x + 1e3) * 1024) / 1024
    elif regime == 'scaled':
        x[:, F // 3] *= 1e-3
    return x


def make_batch(regime, F, order=None):
    """-> (feats (B, T_PAD, F) with +-1e18 behind every utterance's end, lens), in `order`."""
    order = list(range(len(LENS))) if order is None else order
    feats = torch.empty(len(order), T_PAD, F)
    for b, i in enumerate(order):
        feats[b] = KR.POISON if b % 2 else -KR.POISON
        feats[b, :LENS[i]] = utterance(regime, F, i, LENS[i])
    return feats, [LENS[i] for i in order]
