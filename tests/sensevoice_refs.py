"""Plain restatements of what SenseVoice Small (wenet/models/sensevoice/) computes on ONE
utterance, in fp64 (`fp32=True`: the SAME plain formula in fp32, the yardstick e_plain of the GPU
tolerances), the packed cases of the front-end operator test and the fixture loaders.  Written
from the reference's module text, cited file:line; nothing of the reference is imported.  The
SANM layer pieces are those of tests/paraformer_refs.py.  No GPU in here.

  * the query rows and their place              sensevoice_small_model.py:267-285
  * LFR, one utterance alone                    paraformer/layers.py:24-92
  * the position term over the whole sequence   paraformer/embedding.py, transformer/embedding.py:150-164
  * both layer stacks                           sensevoice_small_model.py:74-140, paraformer/layers.py:144-180
"""
import math
import os

import numpy as np
import torch

import paraformer_refs as PR

N_QUERY, N_EMBED, D0 = 4, 16, 560
LID = {'auto': 0, 'zh': 3, 'en': 4, 'yue': 7, 'ja': 11, 'ko': 12, 'nospeech': 13}
ITN = {'withitn': 14, 'woitn': 15}


def query_rows(lid='auto', itn='woitn'):
    """sensevoice_small_model.py:270-284: language | event (1) | emotion (2) | text norm; an
    unknown language is row 0, an unknown text norm row 15."""
    return [LID.get(lid, 0), 1, 2, ITN.get(itn, 15)]


def enc_rows(n):
    return PR.lfr_rows(n) + N_QUERY if n > 0 else 0


def ref_sv_front(feats, qid, embed, mean, istd, pe, ln_w, ln_b, xscale, eps, m=7, n_step=6,
                 fp32=False):
    """feats (n, F) of ONE utterance, qid its 4 table rows -> (4 + T', m F): the query rows as the
    table holds them (no CMVN) in front of the LFR rows with GlobalCMVN (x - mean) * istd; every
    row then x * xscale + pe[t + 1] -- positions run over the concatenated sequence and start at
    1 -- and the LayerNorm of layer 0."""
    dt = torch.float32 if fp32 else torch.float64
    idx = torch.from_numpy(PR.lfr_indices(feats.shape[0], m, n_step))
    x = feats.to(dt)[idx].reshape(idx.shape[0], -1)
    if mean is not None:
        x = (x - mean.to(dt)) * istd.to(dt)
    x = torch.cat([embed.to(dt)[torch.as_tensor(list(qid), dtype=torch.long)], x], dim=0)
    x = x * torch.tensor(xscale, dtype=dt) + pe.to(dt)[1:x.shape[0] + 1]
    return PR.ref_layernorm(x, ln_w, ln_b, eps, fp32)


def _layer(x, sd, p, H, dt, residual, softmax32):
    """AliParaformerEncoderLayer.forward (layers.py:144-180)."""
    att = PR.ref_sanm_attention(PR._norm(x, sd, p + '.norm1', 1e-5, dt), sd, p + '.self_attn', H,
                                dt, softmax32)
    x = x + att if residual else att
    h = torch.relu(PR._lin(PR._norm(x, sd, p + '.norm2', 1e-5, dt), sd, p + '.feed_forward.w_1',
                           dt))
    return x + PR._lin(h, sd, p + '.feed_forward.w_2', dt)


def ref_sensevoice(sd, configs, feats, qid=(0, 1, 2, 15), fp32=False, softmax32=False,
                   pe=None):
    """SenseVoiceSmall.decode up to the CTC head (sensevoice_small_model.py:249-290, 74-118) on
    ONE utterance of fbank frames (n, 80), written out.  Returns dict(enc (4 + T', d), logp
    (4 + T', V)), fp64 tensors.  softmax32: the attention softmax alone in fp32, as the
    reference's .double() module runs it (paraformer_refs._mha).  pe: the position table to read
    (rows = positions) in place of the fp64 sinusoids -- the reference's is an fp32 buffer."""
    dt = torch.float32 if fp32 else torch.float64
    ec = configs['encoder_conf']
    d, H = ec['output_size'], ec['attention_heads']
    idx = torch.from_numpy(PR.lfr_indices(feats.shape[0]))
    x = feats.to(dt)[idx].reshape(idx.shape[0], -1)
    x = (x - sd['global_cmvn.mean'].to(dt)) * sd['global_cmvn.istd'].to(dt)
    x = torch.cat([sd['embed.weight'].to(dt)[torch.as_tensor(list(qid), dtype=torch.long)], x],
                  dim=0)
    T = x.shape[0]
    pe = PR.whisper_sinusoids(T + 1, D0) if pe is None else pe.reshape(-1, D0)
    x = x * torch.tensor(math.sqrt(d), dtype=dt) + pe[1:T + 1].to(dt)
    for i in range(ec['num_blocks']):
        p = 'encoder.encoders0.0' if i == 0 else f'encoder.encoders.{i - 1}'
        x = _layer(x, sd, p, H, dt, i > 0, softmax32)
    x = PR._norm(x, sd, 'encoder.after_norm', 1e-5, dt)
    for i in range(ec['tp_blocks']):
        x = _layer(x, sd, f'encoder.tp_encoders.{i}', H, dt, True, softmax32)
    enc = PR._norm(x, sd, 'encoder.tp_norm', 1e-5, dt)
    logp = torch.log_softmax(PR._lin(enc, sd, 'ctc.ctc_lo', dt), dim=-1)
    return dict(enc=enc.double(), logp=logp.double())


# ---------------------------------------------------------------------------------------------
# the fixtures of tools/gen_golden_sensevoice.py (tests/golden/sensevoice/)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sensevoice')
TINY_CONFIGS = ('tiny_sensevoice', 'tiny_sensevoice_h64')
# 5, 5, 6, 32, 33, 64 and 76 encoder rows: either side of the 32-row query tiles
TINY_LENS = [1, 6, 7, 167, 169, 360, 431]
TINY_ENC_SAVED = [7, 169]        # utterances whose fp64 encoder output is recorded
TINY_FSEED = 2025
CTC_BEAM = 5
# name -> infos of SenseVoiceSmall.decode; the third must equal the first inside the reference
SETTINGS = {'default': {}, 'en_withitn': {'lid': 'en', 'itn': 'withitn'},
            'unknown': {'lid': 'tlh', 'itn': 'maybe'}}
METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search')


def tiny_features():
    return [PR.features(n, TINY_FSEED) for n in TINY_LENS]


def load_tiny(config):
    """(meta, arrays) of one tiny configuration's recordings."""
    return PR.load_golden(GOLDEN_DIR, config)


def setting_qid(name):
    return query_rows(SETTINGS[name].get('lid', 'auto'), SETTINGS[name].get('itn', 'woitn'))


# ---------------------------------------------------------------------------------------------
# the operator case: B = 3, lengths 1 / 7 / 40


def make_front_case(lens=(1, 7, 40), seed=5, cmvn=True, order=None, gap=2, lead=1, ldo=576):
    """Seeded inputs of wn_op_sv_front and the packing of its output rows (`order`: packing
    order of the utterances; offsets are by utterance index).  The output buffer is POISON
    wherever no utterance owns."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(max(lens), 1)
    feats = torch.zeros(B, T, 80)
    for b, n in enumerate(lens):
        if n > 0:
            feats[b, :n] = PR.features(n, seed + 17 * b)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(feats=feats, lens=list(lens), T=T,
             mean=(11.0 + 1.5 * r(D0)) if cmvn else None,
             istd=(1.0 / (2.5 + 0.5 * r(D0).abs())) if cmvn else None,
             embed=r(N_EMBED, D0), ln_w=1.0 + 0.1 * r(D0), ln_b=0.1 * r(D0),
             qid=[[int(v) for v in torch.randint(0, N_EMBED, (N_QUERY, ), generator=g)]
                  for _ in lens],
             xscale=math.sqrt(512.0), eps=1e-5, ldo=ldo)
    rows = [enc_rows(n) for n in lens]
    c['pe'] = PR.whisper_sinusoids(max(rows) + 1, D0).float()
    order = list(range(B)) if order is None else list(order)
    offs, at = [0] * B, lead
    for u in order:
        offs[u] = at
        at += rows[u] + gap
    c.update(rows=rows, offs=offs, total=at, order=order)
    return c


def front_refs(c):
    """Per utterance (fp64 reference rows, the same formula in fp32)."""
    out = []
    for b, n in enumerate(c['lens']):
        if n == 0:
            out.append((torch.zeros(0, D0, dtype=torch.float64), ) * 2)
            continue
        args = (c['feats'][b, :n], c['qid'][b], c['embed'], c['mean'], c['istd'], c['pe'],
                c['ln_w'], c['ln_b'], c['xscale'], c['eps'])
        out.append((ref_sv_front(*args), ref_sv_front(*args, fp32=True)))
    return out
