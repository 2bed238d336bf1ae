"""Plain formulas of the W2v-BERT 2.0 / conformer_shaw kernels (csrc/attention_shaw.hip): the Shaw
attention (wenet/models/transformer/attention.py:546-578) and the stacked-frame front end
(subsampling.py:376-388), in fp64 and -- the yardstick e_plain of the tolerances -- in fp32.

No GPU in here.
"""
import math

import torch

import attention_d32_refs as D
import paraformer_refs as PR

LEFT, RIGHT, ROWS, DK = 64, 8, 73, 64
SCALE = 1.0 / math.sqrt(DK)
# one packed batch of the smallest lengths that reach each branch of attention_shaw_kernel
LENS = [1, 8, 9, 10, 32, 0, 33, 64, 65, 66, 97, 129, 200]


def shaw_index(n, h):
    """(n, n): row of the table for query i, key j -- clamp(j - i, -64, 8) + 64, whatever the head."""
    i = torch.arange(n)
    return torch.clamp(i.unsqueeze(0) - i.unsqueeze(1), -LEFT, RIGHT) + LEFT


# the four wrong readings of the table the coded regime must expose; each maps (n, h) to rows of
# `table_ext` = the table followed by its rows in reverse (what a read past row 72 would hit)
def _off_by_one(n, h):
    return torch.clamp(shaw_index(n, h) + 1, max=ROWS - 1)


def _wrap(n, h):
    i = torch.arange(n)
    return (i.unsqueeze(0) - i.unsqueeze(1) + LEFT) % ROWS


def _zero_row(n, h):          # 2 * ROWS: a row of zeros behind table_ext
    i = torch.arange(n)
    dlt = i.unsqueeze(0) - i.unsqueeze(1)
    return torch.where((dlt < -LEFT) | (dlt > RIGHT), 2 * ROWS, dlt + LEFT)


def _per_head(n, h):
    return shaw_index(n, h) + h * ROWS


WRONG_INDEX = {'off_by_one': _off_by_one, 'wrap': _wrap, 'zero_row': _zero_row,
               'per_head': _per_head}


def ref_attention_shaw(buf, table, offs, lens, H, scale=SCALE, fp32=False, index=shaw_index):
    """buf (rows, 3 H 64) = Q | K | V; table (73, 64).  Per (sequence, head):
    softmax((q k^T + einsum(q, table[index])) * scale) v.  (rows, H 64) fp64, zero in rows no
    sequence owns."""
    dt = torch.float32 if fp32 else torch.float64
    d = H * DK
    ext = torch.cat([table, table.flip(0), torch.zeros(1, DK)]).to(dt)
    out = torch.zeros(buf.shape[0], d, dtype=torch.float64)
    for o, n in zip(offs, lens):
        if n == 0:
            continue
        q, k, v = (buf[o:o + n, i * d:(i + 1) * d].to(dt).view(n, H, DK).transpose(0, 1)
                   for i in range(3))
        for h in range(H):
            rel = ext[index(n, h)]                                   # (n, n, 64)
            s = (q[h] @ k[h].T + torch.einsum('ld,lrd->lr', q[h], rel)) * scale
            out[o:o + n, h * DK:(h + 1) * DK] = (torch.softmax(s, dim=-1) @ v[h]).double()
    return out


def coded_table(seed=0):
    """A table that codes its row index: row c = a_c * e for one unit row e, every a_c different,
    |a_0| and |a_72| the largest -- a wrong row moves the score by (a_c' - a_c) (q . e)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(DK, generator=g)
    e = e / e.norm()
    a = torch.tensor([((c * 37) % ROWS) / ROWS * 8.0 - 4.0 for c in range(ROWS)])
    a[0], a[ROWS - 1] = 12.0, -12.0
    return (a.unsqueeze(1) * e.unsqueeze(0)).float().contiguous() * 4.0


def make_case(H, regime, param, order=None, lens=LENS, seed=5):
    """Q | K | V of every sequence as the three column blocks of one packed buffer (ld = 3 d) in a
    regime of attention_d32_refs.raw_rows, or `coded`: unit data under coded_table."""
    coded = regime == 'coded'
    qs, ks, vs = D.raw_rows('unit' if coded else regime, param, H, lens, lens, lens, seed, dk=DK)
    buf, offs, total = PR.pack_rows([torch.cat(r, 1) for r in zip(qs, ks, vs)], order, gap=3,
                                    lead=2)
    table = coded_table(seed) if coded else \
        torch.randn(ROWS, DK, generator=torch.Generator().manual_seed(seed + 900))
    return dict(H=H, d=H * DK, lens=list(lens), buf=buf, offs=offs, rows=total, table=table)


def case_refs(c, **kw):
    """(fp64 reference, e_plain, scale = the largest |v| a sequence sees)."""
    ref = ref_attention_shaw(c['buf'], c['table'], c['offs'], c['lens'], c['H'], **kw)
    plain = ref_attention_shaw(c['buf'], c['table'], c['offs'], c['lens'], c['H'], fp32=True)
    vmax = max(c['buf'][o:o + n, 2 * c['d']:].abs().max().item()
               for o, n in zip(c['offs'], c['lens']) if n > 0)
    return ref, (plain - ref).abs().max().item(), vmax


def ref_stack_frames_ln(feats, lens, mean, istd, w, b, fp32=False, eps=1e-5):
    """feats (B, T, F) -> list of (lens[b] // 2, 2 F) fp64: LayerNorm over frames 2t | 2t + 1."""
    dt = torch.float32 if fp32 else torch.float64
    out = []
    for x, n in zip(feats, lens):
        x = x[:n - n % 2].to(dt)
        if mean is not None:
            x = (x - mean.to(dt)) * istd.to(dt)
        x = x.reshape(n // 2, 2 * feats.shape[-1])
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        out.append(((x - mu) / torch.sqrt(var + eps) * w.to(dt) + b.to(dt)).double())
    return out


# the recorded model (tools/gen_golden_shaw.py -> tests/golden/shaw/tiny_shaw.npz): T' = 72 .. 0
TINY = dict(config='tiny_shaw', frames=[145, 131, 64, 19, 3, 1], fseed=900, beam=5,
            ctc_weight=0.5)


def tiny_features():
    """The utterances of the model fixture, one (n, 80) fp32 matrix each."""
    from wenet_amd import synthetic as S
    return [S.make_features(1, n, seed=TINY['fseed'] + i)[0][0]
            for i, n in enumerate(TINY['frames'])]


def ref_encoder(feats, sd, configs, fp32=False, softmax_fp32=False):
    """The encoder of a shaw recipe on ONE utterance (n, F), from the state dict: front end, the
    Conformer layers (encoder_layer.py, convolution.py with causal left padding and no biases),
    after_norm.  (n // 2, d) fp64.  softmax_fp32: the softmax alone in fp32, as the reference's
    forward_attention runs it whatever the model's dtype (attention.py:163-171)."""
    import torch.nn.functional as Fn
    dt = torch.float32 if fp32 else torch.float64
    ec = configs['encoder_conf']
    d, H, K = ec['output_size'], ec['attention_heads'], ec['cnn_module_kernel']
    W = {k: v.to(dt) for k, v in sd.items() if k.startswith('encoder.')}

    def ln(x, p):
        return Fn.layer_norm(x, (x.shape[-1], ), W[p + '.weight'], W[p + '.bias'], 1e-5)

    def lin(x, p):
        return Fn.linear(x, W[p + '.weight'], W.get(p + '.bias'))

    mean, istd = sd.get('encoder.global_cmvn.mean'), sd.get('encoder.global_cmvn.istd')
    n = feats.shape[0] // 2
    x = feats[:2 * n].to(dt)
    if mean is not None:
        x = (x - mean.to(dt)) * istd.to(dt)
    x = lin(ln(x.reshape(n, -1), 'encoder.embed.norm'), 'encoder.embed.out')
    idx = shaw_index(n, 0)
    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        ff = p + '.feed_forward_macaron'
        x = x + 0.5 * lin(Fn.silu(lin(ln(x, p + '.norm_ff_macaron'), ff + '.w_1')), ff + '.w_2')
        y = ln(x, p + '.norm_mha')
        q, k, v = (lin(y, f'{p}.self_attn.linear_{c}').view(n, H, DK).transpose(0, 1)
                   for c in 'qkv')
        rel = W[p + '.self_attn.rel_k_embed.weight'][idx]
        s = (q @ k.transpose(1, 2) + torch.einsum('hld,lrd->hlr', q, rel)) / math.sqrt(DK)
        w = torch.softmax(s.float(), -1).to(dt) if softmax_fp32 else torch.softmax(s, -1)
        a = (w @ v).transpose(0, 1).reshape(n, d)
        x = x + lin(a, p + '.self_attn.linear_out')
        c = p + '.conv_module'
        y = ln(x, p + '.norm_conv').T.unsqueeze(0)                       # (1, d, n)
        lpad = K - 1 if ec['causal'] else (K - 1) // 2
        y = Fn.pad(y, (lpad, K - 1 - lpad))                              # pads BEFORE pointwise1
        y = Fn.glu(Fn.conv1d(y, W[c + '.pointwise_conv1.weight']), dim=1)
        y = Fn.conv1d(y, W[c + '.depthwise_conv.weight'], groups=d)
        y = Fn.silu(ln(y[0].T, c + '.norm'))
        x = x + Fn.conv1d(y.T.unsqueeze(0), W[c + '.pointwise_conv2.weight'])[0].T
        ff = p + '.feed_forward'
        x = x + 0.5 * lin(Fn.silu(lin(ln(x, p + '.norm_ff'), ff + '.w_1')), ff + '.w_2')
        x = ln(x, p + '.norm_final')
    return ln(x, 'encoder.after_norm').double()
