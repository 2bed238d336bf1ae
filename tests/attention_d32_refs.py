"""References, cases and fixtures of the decoders with heads of 32 (csrc/attention_d32.hip, the
d_k = 32 form of the step kernel in csrc/attn_search.hip): tests/test_attention_d32_host.py on the
CPU, tests/test_gpu_attention_d32.py and tests/test_gpu_dec32.py on the GPU.

`kernel_refs.ref_attention` is fixed at heads of 64; `ref_attention_w` restates it for a head
width parameter -- the same loops and matmuls, in fp64, and with fp32=True as the same plain
formula in fp32 (the yardstick e_plain of the tolerances).  The packed cases hold +-1e18 wherever
no sequence owns (paraformer_refs.pack_rows), the step cases are kernel_refs.make_self_step_case at
32.  The data regimes are those of kernel_refs.make_attention_case, written for a width: coordinate
0 of every head steers the scores by the key's POSITION.

ATTENTION_CASES / STEP_CASES name every case the GPU file runs; the host test evaluates the cap
(kernel_refs.cap_ok) on each of them.

No GPU in here.
"""
import json
import math
import os

import numpy as np
import torch

import kernel_refs as KR
import paraformer_refs as PR

DK = 32
SCALE = 1.0 / math.sqrt(DK)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dec32')


def ref_attention_w(q, k, v, seqs, H, dk, scale, mask_mode=0, fp32=False, want_weights=False):
    """q (q_rows, >= H dk), k / v (kv_rows, >= H dk); seqs = [(q_off, q_len, kv_off, kv_len)].
    Per (sequence, head): softmax(mask((q k^T) * scale)) v, mask_mode 0 every key < kv_len, 1 key
    j <= query i as well (kernel_refs.chunk_window).  (q_rows, H dk) fp64, zero in rows no sequence
    owns; with want_weights also the largest weight of every owned (row, head)."""
    dt = torch.float32 if fp32 else torch.float64
    d = H * dk
    out = torch.zeros(q.shape[0], d, dtype=torch.float64)
    wmax = []
    for (qo, ql, ko, kl) in seqs:
        if ql == 0:
            continue
        qs = q[qo:qo + ql, :d].to(dt).reshape(ql, H, dk).transpose(0, 1)      # (H, ql, dk)
        ks = k[ko:ko + kl, :d].to(dt).reshape(kl, H, dk).transpose(0, 1)
        vs = v[ko:ko + kl, :d].to(dt).reshape(kl, H, dk).transpose(0, 1)
        scores = torch.matmul(qs, ks.transpose(1, 2)) * scale
        hidden = ~KR.chunk_window(ql, kl, mask_mode, 0, -1)
        scores = scores.masked_fill(hidden, -float('inf'))
        attn = torch.softmax(scores, dim=-1).masked_fill(hidden, 0.0)
        if want_weights:
            wmax.append(attn.max(dim=-1).values.reshape(-1).double())
        o = torch.matmul(attn, vs)
        out[qo:qo + ql] = o.transpose(0, 1).reshape(ql, d).double()
    if want_weights:
        return out, torch.cat(wmax)
    return out


# ---------------------------------------------------------------------------------------------
# the data of a case, utterance by utterance (so that a packing order does not change it)

# needle positions: a key index, or the last key the sequence shows to anybody
NEEDLES = {'0': 0, '31': 31, '32': 32, '63': 63, '64': 64}


def raw_rows(regime, param, H, q_lens, kv_lens, n_key_rows, seed, dk=DK):
    """Per utterance u: q (q_lens[u], H dk), k and v (n_key_rows[u], H dk) of which the first
    kv_lens[u] are visible.  Regimes as kernel_refs.make_attention_case: `unit`; `peaked` p (the
    scores scaled to a standard deviation of p); `ascending` / `descending` s (s per key);
    `needle` at '0' / '31' / '32' / '63' / '64' / 'last' (60 on one key, clamped to the last
    visible one) or 'last_visible' (40 more per key); `shifted` s (every score + s, v + 100);
    `tied` (q = 0)."""
    d = H * dk
    scale = 1.0 / math.sqrt(dk)
    qs, ks, vs = [], [], []
    for u, (ql, kr) in enumerate(zip(q_lens, n_key_rows)):
        g = torch.Generator().manual_seed(seed * 1000 + u)
        qs.append(torch.randn(ql, d, generator=g))
        ks.append(torch.randn(kr, d, generator=g))
        vs.append(torch.randn(kr, d, generator=g))
    steer = regime in ('ascending', 'descending', 'shifted', 'needle')
    for u in range(len(q_lens)):
        q3, k3 = qs[u].view(-1, H, dk), ks[u].view(-1, H, dk)
        kl, kr = kv_lens[u], n_key_rows[u]
        if steer:
            q3[:, :, 0] = 0
            k3[:, :, 0] = 0
        if regime in ('ascending', 'descending'):
            step = float(param) * (1.0 if regime == 'ascending' else -1.0)
            q3[:, :, 0] = 1.0 / scale
            k3[:, :, 0] = (torch.arange(kr, dtype=torch.float32) * step).unsqueeze(1)
        elif regime == 'needle':
            q3[:, :, 0] = 1.0 / scale
            if param == 'last_visible':
                k3[:, :, 0] = (torch.arange(kr, dtype=torch.float32) * 40.0).unsqueeze(1)
            elif kl > 0:
                j = kl - 1 if param == 'last' else min(NEEDLES[param], kl - 1)
                k3[j, :, 0] = 60.0
        elif regime == 'shifted':
            q3[:, :, 0] = float(param) / scale
            k3[:, :, 0] = 1.0
            vs[u] += 100.0
        elif regime == 'tied':
            qs[u].zero_()
        elif regime not in ('unit', 'peaked'):
            raise ValueError(regime)
    if regime == 'peaked':
        vals = []
        for u in range(len(q_lens)):
            if q_lens[u] and kv_lens[u]:
                s = torch.matmul(qs[u].double().view(-1, H, dk).transpose(0, 1),
                                 ks[u][:kv_lens[u]].double().view(-1, H, dk).permute(1, 2, 0))
                vals.append((s * scale).reshape(-1))
        sd0 = torch.cat(vals).std().item() if sum(v.numel() for v in vals) > 1 else 1.0
        c = float(param) / (sd0 if sd0 > 0 else 1.0)
        for u in range(len(q_lens)):
            qs[u] *= c
    return qs, ks, vs


def make_case(regime, param, H, q_lens, kv_lens=None, self_kv=None, mask_mode=0, seed=0,
              order=None, dk=DK):
    """kv_lens None: self attention, Q | K | V are the three column blocks of ONE buffer of 3 H dk
    columns as the decoder's QKV projection leaves them; self_kv (or None) = keys visible per
    sequence, <= its rows (the padded batches of wn_decoder_forward).  Else cross attention: Q in
    a buffer of H dk + 4 columns, K | V in one of 2 H dk: ldq != ldk.  `order` = packing order."""
    d = H * dk
    n = len(q_lens)
    self_attn = kv_lens is None
    if self_attn:
        vis = list(q_lens) if self_kv is None else list(self_kv)
        assert all(a <= b for a, b in zip(vis, q_lens))
        qs, ks, vs = raw_rows(regime, param, H, q_lens, vis, q_lens, seed, dk)
        rows = [torch.cat([qs[u], ks[u], vs[u]], 1) for u in range(n)]
        buf, offs, total = PR.pack_rows(rows, order, gap=3, lead=2)
        c = dict(q=buf[:, :d], k=buf[:, d:2 * d], v=buf[:, 2 * d:], buf_q=buf, buf_kv=buf,
                 ldq=3 * d, ldk=3 * d, q_cols=(0, d, 2 * d), q_rows=total, kv_rows=total,
                 q_offs=offs, kv_offs=offs, kv_lens=vis)
    else:
        qs, ks, vs = raw_rows(regime, param, H, q_lens, kv_lens, kv_lens, seed, dk)
        kr = [torch.cat([ks[u], vs[u]], 1) for u in range(n)]
        bq, qo, qt = PR.pack_rows(qs, order, gap=2, lead=1, ld=d + 4)
        bk, ko, kt = PR.pack_rows(kr, order, gap=3, lead=3)
        c = dict(q=bq[:, :d], k=bk[:, :d], v=bk[:, d:], buf_q=bq, buf_kv=bk, ldq=d + 4,
                 ldk=2 * d, q_cols=(0, 0, d), q_rows=qt, kv_rows=kt, q_offs=qo, kv_offs=ko,
                 kv_lens=list(kv_lens))
    c.update(H=H, d=d, dk=dk, q_lens=list(q_lens), self_attn=self_attn, scale=1.0 / math.sqrt(dk),
             mask_mode=mask_mode,
             seqs=[(c['q_offs'][u], q_lens[u], c['kv_offs'][u], c['kv_lens'][u])
                   for u in range(n)])
    return c


def case_refs(c):
    """(fp64 reference, e_plain, scale = the largest |v| a sequence sees, largest weights)."""
    a = (c['q'], c['k'], c['v'], c['seqs'], c['H'], c['dk'], c['scale'], c['mask_mode'])
    ref, w = ref_attention_w(*a, want_weights=True)
    plain = ref_attention_w(*a, fp32=True)
    vmax = max(c['v'][ko:ko + kl].abs().max().item() for (_, ql, ko, kl) in c['seqs'] if ql > 0)
    return ref, (plain - ref).abs().max().item(), vmax, w


# the regimes of the issue; needle at keys 0, 31, 32 and the last visible
REGIMES = [('unit', None), ('peaked', 10.0), ('peaked', 30.0), ('ascending', 1.0),
           ('descending', 1.0), ('shifted', 80.0), ('shifted', -80.0), ('tied', None),
           ('needle', '0'), ('needle', '31'), ('needle', '32'), ('needle', 'last_visible')]

CAUSAL_LENS = [1, 31, 32, 33, 64, 65]
PADDED = ([9, 9, 33], [4, 1, 31])                      # rows, visible keys
CROSS = ([1, 5, 33, 2, 40], [3, 32, 70, 1, 125])

# name -> keyword arguments of make_case (without `order`): every packed case of the GPU file
ATTENTION_CASES = {
    'causal': dict(regime='unit', param=None, H=4, q_lens=CAUSAL_LENS, mask_mode=1, seed=11),
    'padded': dict(regime='unit', param=None, H=4, q_lens=PADDED[0], self_kv=PADDED[1],
                   mask_mode=1, seed=12),
}
for _H in (1, 4, 8):
    ATTENTION_CASES[f'cross_h{_H}'] = dict(regime='unit', param=None, H=_H, q_lens=CROSS[0],
                                           kv_lens=CROSS[1], mask_mode=0, seed=13 + _H)
for _r, _p in REGIMES:
    ATTENTION_CASES[f'cross_{_r}_{_p}'] = dict(regime=_r, param=_p, H=4, q_lens=[33],
                                               kv_lens=[70], mask_mode=0, seed=31)
    ATTENTION_CASES[f'causal_{_r}_{_p}'] = dict(regime=_r, param=_p, H=4, q_lens=[65],
                                                mask_mode=1, seed=32)


# ---------------------------------------------------------------------------------------------
# the step kernel: kernel_refs.make_self_step_case at a head width


def make_step_case(regime, param, H, n, length, seed=0, beam=0, prompt=0, dk=DK):
    """One decoder step of n hypothesis rows over `length` positions (the newest included), as
    kernel_refs.make_self_step_case lays it out: qkv (n, 3d), cache (max_len, n, 2d) with +-POISON
    in the rows no path names and in every step >= length - 1, path (n, max_len).  beam = N > 0
    with prompt = P: B x N hypotheses whose first P positions live in their utterance's first
    slot, the later ones in slots of the utterance."""
    qs, ks_, vs_ = raw_rows(regime, param, H, [1] * n, [length] * n, [length] * n, seed, dk)
    d, step, max_len = H * dk, length - 1, length + 2
    g = torch.Generator().manual_seed(seed + 1000)
    if beam:
        assert n % beam == 0 and prompt < length
        first = (torch.arange(n) // beam * beam).unsqueeze(1)
        path = first + torch.randint(0, beam, (n, max_len), generator=g)
        path[:, :prompt] = first
    else:
        path = torch.randint(0, n, (n, max_len), generator=g)
    path[:, step] = torch.arange(n)
    q = torch.cat(qs)                                  # (n, d)
    ks, vs = torch.stack(ks_), torch.stack(vs_)        # (slot, pos, d)
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0) * KR.POISON
    cache = torch.cat([-sign, sign]).repeat(max_len, n, 1)
    named = torch.zeros(max_len, n, dtype=torch.bool)
    pos = torch.arange(step)
    for r in range(n):
        named[pos, path[r, :step]] = True
    cache[:step][named[:step]] = torch.cat([ks, vs], 2).transpose(0, 1)[:step][named[:step]]
    qkv = torch.cat([q, ks[:, step], vs[:, step]], 1)
    idx = path[:, :length].long()
    kg = ks[idx, torch.arange(length).unsqueeze(0)].reshape(n * length, d)
    vg = vs[idx, torch.arange(length).unsqueeze(0)].reshape(n * length, d)
    seqs = [(r, 1, r * length, length) for r in range(n)]
    return dict(qkv=qkv.contiguous(), cache=cache.contiguous(), path=path.to(torch.int32),
                named=named, n=n, H=H, d=d, dk=dk, step=step, length=length, max_len=max_len, q=q,
                kg=kg, vg=vg, seqs=seqs, scale=1.0 / math.sqrt(dk))


def step_refs(case):
    a = (case['q'], case['kg'], case['vg'], case['seqs'], case['H'], case['dk'], case['scale'], 0)
    ref, w = ref_attention_w(*a, want_weights=True)
    plain = ref_attention_w(*a, fp32=True)
    vmax = case['vg'].abs().max().item()
    return ref, (plain - ref).abs().max().item(), vmax, w


STEP_SHAPES = [(1, 1, 1), (4, 5, 2), (8, 30, 63), (1, 5, 64), (4, 30, 65), (8, 5, 129)]
STEP_CASES = {}
for (_H, _n, _len) in STEP_SHAPES:
    for _r, _p in ([('unit', None)] if _len == 1 else [('unit', None), ('peaked', 10.0)]):
        STEP_CASES[f'shape_h{_H}_n{_n}_len{_len}_{_r}'] = dict(
            regime=_r, param=_p, H=_H, n=_n, length=_len, seed=_H + _n + _len)
for _p in ('0', '63', '64', 'last'):
    STEP_CASES[f'needle_{_p}'] = dict(regime='needle', param=_p, H=4, n=5, length=129, seed=51)
# 6 utterances x 5 hypotheses behind a prompt of 3
STEP_CASES['prompt_paths'] = dict(regime='peaked', param=10.0, H=4, n=30, length=65, seed=61,
                                  beam=5, prompt=3)


# ---------------------------------------------------------------------------------------------
# the recorded models (tools/gen_golden_dec32.py -> tests/golden/dec32/)

# rate 4: T' = 72, 33, 32, 31, 16, 8, 5; rate 8 behind the stride layer: 36, 16, 16, 15, 8, 4, 2
MODELS = {
    'tiny_dec32': dict(frames=[291, 135, 131, 127, 67, 35, 23], fseed=700, reverse_weight=0.3,
                       long_attention=True),
    'tiny_efficonformer_v1_dec32': dict(frames=[291, 135, 131, 127, 67, 35, 23], fseed=700,
                                        reverse_weight=0.3, long_attention=False),
}
WIDTH_MODEL = 'aishell_efficonformer_v1_dec8_1blk'
WIDTH_WSEED = 2
CTC_BEAM = 5
RESCORE_CTC_WEIGHT = 0.5
ATTENTION_BEAMS = (1, 5)
BEAM_METHODS = ('ctc_prefix_beam_search', 'attention_rescoring')
RECIPES = ('aishell_v1', 'aishell_v1_stream', 'aishell_v2', 'librispeech_v1', 'librispeech_v2')


def model_features(name):
    """The utterances of a model fixture, one (n, 80) fp32 matrix each."""
    from wenet_amd import synthetic as S
    t = MODELS[name]
    return [S.make_features(1, n, seed=t['fseed'] + i)[0][0] for i, n in enumerate(t['frames'])]


def width_inputs(configs):
    """The five padded hypotheses of tests/test_gpu_parity.py (lens 9, 4, 1, 6, 9) over 31 random
    encoder frames: (hyps (5, 9) int64, lens, enc (1, 31, d) fp32)."""
    st = configs['tokenizer_conf']['special_tokens']
    sos, eos = st['<sos>'], st['<eos>']
    g = torch.Generator().manual_seed(21)
    V = configs['output_dim']
    lens = torch.tensor([9, 4, 1, 6, 9])
    hyps = torch.full((5, 9), eos, dtype=torch.long)
    for i, n in enumerate(lens.tolist()):
        hyps[i, 0] = sos
        hyps[i, 1:n] = torch.randint(1, V - 1, (n - 1, ), generator=g)
    enc = torch.randn(1, 31, configs['encoder_conf']['output_size'], generator=g)
    return hyps, lens, enc


def load_fixture(stem):
    """(meta, arrays) of tests/golden/dec32/<stem>.npz and its continuation files <stem>_<i>.npz;
    arrays cut into row blocks (`<name>__part<i>`) are put together again."""
    raw, meta, i = {}, None, 0
    while True:
        path = os.path.join(GOLDEN_DIR, f'{stem}.npz' if i == 0 else f'{stem}_{i}.npz')
        if not os.path.exists(path):
            break
        with np.load(path) as z:
            for k in z.files:
                if k == 'meta':
                    meta = json.loads(bytes(z[k]).decode())
                else:
                    raw[k] = z[k]
        i += 1
    assert meta is not None, f'{stem}.npz is missing (tools/gen_golden_dec32.py)'
    arrays = {}
    for k in sorted(raw, key=lambda s: (s.split('__part')[0], int(s.split('__part')[1])
                                        if '__part' in s else 0)):
        base = k.split('__part')[0]
        arrays[base] = raw[k] if base not in arrays else np.concatenate([arrays[base], raw[k]])
    return meta, arrays
