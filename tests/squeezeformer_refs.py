"""Plain references of the Squeezeformer kernels (csrc/squeezeformer.hip: the attention with the
WRAPPED shift, the time reduction's depthwise conv, the time recovery), of the modules and of one
encoder block, and the cases the tests run them on (tests/test_squeezeformer_host.py on the CPU,
tests/test_gpu_squeezeformer_ops.py and tests/test_gpu_squeezeformer.py on the GPU).

The shift is written from its CLOSED FORM, not from the reference's pad-and-view trick
(squeezeformer/attention.py:75-99).  With bd[i][c] = (q_i + v) . p_c over a T-row table:
    j <= i     : shifted[i][j] = bd[i][T - 1 - (i - j)]
    j == i + 1 : shifted[i][j] = 0
    j >= i + 2 : shifted[i][j] = bd[i + 1][j - i - 2]          (the NEXT query row)
Every formulation is fp64 torch and evaluates ONE utterance alone;
dtype / fp32 evaluates the SAME formula in fp32, the yardstick `e_plain` of the GPU tolerances
(tests/kernel_refs.py bound / cap_ok).  The fixtures of tests/golden/squeezeformer/
(tools/gen_golden_squeezeformer.py) pin the formulations to the reference's own modules.

No GPU in here.
"""
import math

import torch
import torch.nn.functional as F

import kernel_refs as KR

# ---------------------------------------------------------------------------------------------
# the wrapped shift

MUTANTS = ('txl', 'lower_row_plus', 'lower_row_minus', 'upper_row_plus', 'upper_row_minus',
           'diag1_nonzero', 'upper_same_query', 'max_len_centre')


def wrapped_shift(bd, T, mutate=None, centre=None):
    """bd (H, T, Tt), Tt >= T columns of position rows -> the shifted (H, T, T) term.
    mutate: the mistakes tests/test_squeezeformer_host.py shows the cases would catch --
      'txl'               the Transformer-XL shift: the row of distance |i - j| with q_i on both
                          sides of the diagonal
      'lower_row_plus' / 'lower_row_minus' / 'upper_row_plus' / 'upper_row_minus'
                          a band row off by one in one branch
      'diag1_nonzero'     bd[i + 1][0] instead of 0 at j == i + 1
      'upper_same_query'  the upper branch with q_i instead of q_{i+1}
      'max_len_centre'    `centre` (the batch's max_len - 1) instead of T - 1"""
    H, _, Tt = bd.shape
    c0 = T - 1 if (mutate != 'max_len_centre' or centre is None) else centre
    out = torch.zeros(H, T, T, dtype=bd.dtype)
    for i in range(T):
        for j in range(T):
            if j <= i:
                col = c0 - (i - j) + {'lower_row_plus': 1, 'lower_row_minus': -1}.get(mutate, 0)
                row = i
            elif j == i + 1:
                if mutate == 'diag1_nonzero' and i + 1 < T:
                    out[:, i, j] = bd[:, i + 1, 0]
                if mutate == 'txl':
                    out[:, i, j] = bd[:, i, c0 - 1]
                continue
            else:
                col = j - i - 2 + {'upper_row_plus': 1, 'upper_row_minus': -1}.get(mutate, 0)
                row = i if mutate == 'upper_same_query' else i + 1
                if mutate == 'txl':
                    row, col = i, c0 - (j - i)
            if 0 <= col < Tt:
                out[:, i, j] = bd[:, row, col]
    return out


def ref_attention_sqshift(q, k, v, P, bias_u, bias_v, seqs, scale=0.125, fp32=False, mutate=None,
                          want_scores=False):
    """q / k / v (rows, H * 64); P (p_rows, H * 64) = linear_pos of the first p_rows position
    rows; bias_u / bias_v (H, 64); seqs = [(off, len)].  Per (sequence, head), with T = len:
        softmax(((q + u) k^T + wrapped_shift((q + v) P[:T]^T)) * scale) v
    Returns (rows, H * 64) fp64, zero in rows no sequence owns."""
    dt = torch.float32 if fp32 else torch.float64
    H = q.shape[1] // 64
    out = torch.zeros(q.shape[0], H * 64, dtype=torch.float64)
    max_len = max(T for _, T in seqs)
    scores = []
    for (off, T) in seqs:
        if T == 0:
            continue
        qs = q[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)        # (H, T, 64)
        ks = k[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)
        vs = v[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)
        Tt = P.shape[0] if mutate == 'max_len_centre' else T
        ps = P[:Tt].to(dt).view(Tt, H, 64).transpose(0, 1)
        ac = torch.matmul(qs + bias_u.to(dt).unsqueeze(1), ks.transpose(1, 2))
        bd = torch.matmul(qs + bias_v.to(dt).unsqueeze(1), ps.transpose(1, 2))
        sc = (ac + wrapped_shift(bd, T, mutate, max_len - 1)) * scale
        scores.append(sc.reshape(-1).double())
        o = torch.matmul(torch.softmax(sc, dim=-1), vs)
        out[off:off + T] = o.transpose(0, 1).reshape(T, H * 64).double()
    if want_scores:
        return out, torch.cat(scores)
    return out


def make_sqshift_case(H, lens, seed=0, gap=3, lead=5, t_table=None, regime='unit', param=None,
                      sign=False):
    """One packed self-attention batch.  P is a table of t_table >= max(lens) rows.  Rows of
    Q / K / V no sequence owns hold +-POISON.  regime 'peaked': (q, u, v) scaled so that the
    scores have the standard deviation `param`.  sign: the position rows alternate between 0.05
    and 2 times a unit row, so a band row off by one, the other branch or another query row moves
    the scores by many standard deviations."""
    g = torch.Generator().manual_seed(seed)
    offs, rows = KR.pack_layout(lens, gap, lead)
    d = H * 64
    t_table = t_table or max(lens)
    q = torch.randn(rows, d, generator=g)
    k = torch.randn(rows, d, generator=g)
    v = torch.randn(rows, d, generator=g)
    P = torch.randn(t_table, d, generator=g)
    bu = torch.randn(H, 64, generator=g) * 0.5
    bv = torch.randn(H, 64, generator=g) * 0.5
    if sign:
        P[0::2] *= 0.05
        P[1::2] *= 2.0
    seqs = [(offs[s], lens[s]) for s in range(len(lens))]
    if regime == 'peaked':
        _, sc = ref_attention_sqshift(q, k, v, P, bu, bv, seqs, want_scores=True)
        c = float(param) / sc.std().item()
        q *= c
        bu *= c
        bv *= c
    own = torch.zeros(rows, dtype=torch.bool)
    for (o, T) in seqs:
        own[o:o + T] = True
    sgn = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0) * KR.POISON
    q[~own] = sgn
    k[~own] = -sgn
    v[~own] = sgn
    return dict(q=q, k=k, v=v, P=P, bias_u=bu, bias_v=bv, seqs=seqs, H=H, scale=0.125, rows=rows,
                own=own)


def sqshift_refs(c, mutate=None):
    """(fp64 reference, e_plain, scale)."""
    a = (c['q'], c['k'], c['v'], c['P'], c['bias_u'], c['bias_v'], c['seqs'], c['scale'])
    ref = ref_attention_sqshift(*a, mutate=mutate)
    plain = ref_attention_sqshift(*a, fp32=True, mutate=mutate)
    scale = max(c['v'][o:o + T].abs().max().item() for o, T in c['seqs'] if T > 0)
    return ref, (plain - ref).abs().max().item(), scale


RAGGED = [1, 2, 31, 32, 33, 65, 100]
SIGN_LENS = [33, 97, 64]
# name -> make_sqshift_case arguments: the operator cases of the GPU test
SQSHIFT_CASES = {
    'ragged_h2': dict(H=2, lens=RAGGED, seed=1),
    'ragged_h8': dict(H=8, lens=RAGGED, seed=2),
    'peaked': dict(H=2, lens=[33, 65, 100], seed=3, regime='peaked', param=10.0),
    'sign': dict(H=2, lens=SIGN_LENS, seed=4, sign=True),
    'sign_h8': dict(H=8, lens=SIGN_LENS, seed=5, sign=True),
    'long_table': dict(H=2, lens=[70, 5], seed=6, t_table=300, sign=True),
}
SIGN_CASES = ('sign', 'sign_h8', 'long_table')

# ---------------------------------------------------------------------------------------------
# time reduction / recovery


def ref_time_reduce(x, wt, bias, K, pad, seqs, out_offs, out_rows, dtype=torch.float64):
    """x (rows, C) packed full-rate rows, wt (C, 1, K) / bias (C) as Conv1d(groups=C) holds them:
    y[t] = bias + sum_k wt[:, 0, k] * x[2 t - pad + k] for t < ceil(len / 2), frames outside the
    utterance's own [0, len) being zeros.  Returns (out_rows, C) fp64, zero in unowned rows."""
    C = x.shape[1]
    out = torch.zeros(out_rows, C, dtype=torch.float64)
    w = wt.to(dtype)[:, 0, :]
    for (off, T), o2 in zip(seqs, out_offs):
        xs = x[off:off + T].to(dtype)
        for t in range((T + 1) // 2):
            acc = bias.to(dtype).clone()
            for kk in range(K):
                s = 2 * t - pad + kk
                if 0 <= s < T:
                    acc = acc + w[:, kk] * xs[s]
            out[o2 + t] = acc.double()
    return out


def ref_time_recover(skip, z, seqs, z_offs, dtype=torch.float64):
    """y[off + t] = skip[off + t] + z[z_off + t // 2]; zero in unowned rows."""
    out = torch.zeros(skip.shape, dtype=torch.float64)
    for (off, T), zo in zip(seqs, z_offs):
        for t in range(T):
            out[off + t] = (skip[off + t].to(dtype) + z[zo + t // 2].to(dtype)).double()
    return out


TIME_LENS = [1, 2, 5, 31, 32, 33, 64, 65]


def make_time_case(C, K, lens=TIME_LENS, seed=0, gap=2, lead=3):
    """Packed full-rate rows x / skip (POISON in unowned rows), the half-rate layout (its own
    gaps) with z, taps of order 1 / sqrt(K)."""
    g = torch.Generator().manual_seed(seed)
    offs, rows = KR.pack_layout(lens, gap, lead)
    lens2 = [(n + 1) // 2 for n in lens]
    offs2, rows2 = KR.pack_layout(lens2, gap + 1, lead - 1)
    x = torch.full((rows, C), KR.POISON)
    z = torch.full((rows2, C), -KR.POISON)
    for o, n in zip(offs, lens):
        x[o:o + n] = torch.randn(n, C, generator=g) * 1.5 + 0.2
    for o, n in zip(offs2, lens2):
        z[o:o + n] = torch.randn(n, C, generator=g)
    wt = (torch.rand(C, 1, K, generator=g) * 2 - 1) / math.sqrt(K)
    bias = (torch.rand(C, generator=g) * 2 - 1) * 0.5
    return dict(x=x, z=z, wt=wt, bias=bias, K=K, pad=3 if K == 5 else 0, C=C,
                seqs=list(zip(offs, lens)), offs2=offs2, lens2=lens2, rows=rows, rows2=rows2)


def time_reduce_refs(c):
    a = (c['x'], c['wt'], c['bias'], c['K'], c['pad'], c['seqs'], c['offs2'], c['rows2'])
    ref = ref_time_reduce(*a)
    plain = ref_time_reduce(*a, dtype=torch.float32)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# modules, written from the module text


def _ada(x, w, p):
    return w[p + '.ada_scale'].reshape(-1) * x + w[p + '.ada_bias'].reshape(-1)


def attention_module(x, w, p, H, pos, shift, visible=None):
    """squeezeformer RelPositionMultiHeadedAttention.forward (adaptive scale on) on one utterance
    x (T, d); pos (>= T, d) position rows; visible (T, T) bool or None."""
    T, d = x.shape
    dk = d // H
    xa = _ada(x, w, p)
    heads = lambda t: t.view(-1, H, dk).transpose(0, 1)
    q = heads(xa @ w[p + '.linear_q.weight'].t() + w[p + '.linear_q.bias'])
    k = heads(xa @ w[p + '.linear_k.weight'].t() + w[p + '.linear_k.bias'])
    v = heads(xa @ w[p + '.linear_v.weight'].t() + w[p + '.linear_v.bias'])
    pp = heads(pos[:T].to(x.dtype) @ w[p + '.linear_pos.weight'].t())
    ac = (q + w[p + '.pos_bias_u'].unsqueeze(1)) @ k.transpose(1, 2)
    bd = (q + w[p + '.pos_bias_v'].unsqueeze(1)) @ pp.transpose(1, 2)
    if shift:
        bd = wrapped_shift(bd, T)
    scores = (ac + bd) / math.sqrt(dk)
    if visible is not None:
        scores = scores.masked_fill(~visible, -float('inf'))
    attn = torch.softmax(scores, dim=-1)
    if visible is not None:
        attn = attn.masked_fill(~visible, 0.0)
    ctx = (attn @ v).transpose(0, 1).reshape(T, d)
    return ctx @ w[p + '.linear_out.weight'].t() + w[p + '.linear_out.bias']


def _conv_norm(y, w, p, batch_norm):
    if batch_norm:
        g = w[p + '.norm.weight'] / torch.sqrt(w[p + '.norm.running_var'] + 1e-5)
        return (y - w[p + '.norm.running_mean']) * g + w[p + '.norm.bias']
    return F.layer_norm(y, (y.shape[1], ), w[p + '.norm.weight'], w[p + '.norm.bias'], 1e-5)


def conv_module(x, w, p, K, causal, batch_norm):
    """squeezeformer ConvolutionModule.forward on one utterance: the adaptive scale, K - 1 ZERO
    frames in front when causal (behind the scale, in front of pointwise_conv1), GLU, depthwise
    conv (its own zero padding when not causal), norm, swish, pointwise_conv2."""
    T, d = x.shape
    xa = _ada(x, w, p)
    if causal:
        xa = torch.cat([torch.zeros(K - 1, d, dtype=x.dtype), xa], dim=0)
    h = xa @ w[p + '.pointwise_conv1.weight'][:, :, 0].t() + w[p + '.pointwise_conv1.bias']
    g = h[:, :d] * torch.sigmoid(h[:, d:])
    pad = 0 if causal else (K - 1) // 2
    y = F.conv1d(g.t().unsqueeze(0), w[p + '.depthwise_conv.weight'],
                 w[p + '.depthwise_conv.bias'], padding=pad, groups=d)[0].t()
    y = F.silu(_conv_norm(y, w, p, batch_norm))
    return y @ w[p + '.pointwise_conv2.weight'][:, :, 0].t() + w[p + '.pointwise_conv2.bias']


def ffn_module(x, w, p):
    h = F.silu(_ada(x, w, p) @ w[p + '.w_1.weight'].t() + w[p + '.w_1.bias'])
    return h @ w[p + '.w_2.weight'].t() + w[p + '.w_2.bias']


def layer_formulation(x, w, p, ec, pos, visible=None):
    """SqueezeformerEncoderLayer.forward, post-LN, on one utterance x (T, d)."""
    d = x.shape[1]
    ln = lambda t, n: F.layer_norm(t, (d, ), w[f'{p}.{n}.weight'], w[f'{p}.{n}.bias'], 1e-5)
    x = ln(x + attention_module(x, w, p + '.self_attn', ec['attention_heads'], pos,
                                ec.get('do_rel_shift', True), visible), 'layer_norm1')
    x = ln(x + ffn_module(x, w, p + '.ffn1'), 'layer_norm2')
    x = ln(x + conv_module(x, w, p + '.conv_module', ec['cnn_module_kernel'],
                           bool(ec.get('causal', False)),
                           ec.get('cnn_norm_type', 'batch_norm') == 'batch_norm'), 'layer_norm3')
    return ln(x + ffn_module(x, w, p + '.ffn2'), 'layer_norm4')


def time_reduction_module(x, w, p, K):
    """TimeReductionLayer1D (K 5, padding 3) / TimeReductionLayerStream (K 1) on one utterance."""
    T = x.shape[0]
    y = ref_time_reduce(x, w[p + '.dw_conv.weight'], w[p + '.dw_conv.bias'], K, 3 if K == 5 else 0,
                        [(0, T)], [0], (T + 1) // 2, dtype=x.dtype).to(x.dtype)
    return y @ w[p + '.pw_conv.weight'][:, :, 0].t() + w[p + '.pw_conv.bias']


# ---------------------------------------------------------------------------------------------
# the folds of csrc/cabi_model.hip, restated in fp64


def fold_ada(W, b, scale, bias):
    """`W (ada_scale * x + ada_bias) + b` = W' x + b'."""
    W, b = W.double(), b.double()
    return W * scale.double().reshape(1, -1), W @ bias.double().reshape(-1) + b


def folded_layer(x, w, p, ec, pos, visible=None):
    """The block as the library evaluates it (fp64): the adaptive scales folded into Q / K / V,
    w_1 and pointwise_conv1; a causal conv's padded frame = GLU of the UNFOLDED pointwise_conv1
    bias; an eval-mode BatchNorm as a per-channel affine.  x (T, d) fp64."""
    d, H = x.shape[1], ec['attention_heads']
    T = x.shape[0]
    K, causal = ec['cnn_module_kernel'], bool(ec.get('causal', False))
    ln = lambda t, n: F.layer_norm(t, (d, ), w[f'{p}.{n}.weight'], w[f'{p}.{n}.bias'], 1e-5)
    a = p + '.self_attn'
    heads = lambda t: t.view(-1, H, 64).transpose(0, 1)
    qkv = []
    for n in ('linear_q', 'linear_k', 'linear_v'):
        Wf, bf = fold_ada(w[f'{a}.{n}.weight'], w[f'{a}.{n}.bias'], w[a + '.ada_scale'],
                          w[a + '.ada_bias'])
        qkv.append(heads(x @ Wf.t() + bf))
    q, k, v = qkv
    pp = heads(pos[:T].double() @ w[a + '.linear_pos.weight'].t())
    ac = (q + w[a + '.pos_bias_u'].unsqueeze(1)) @ k.transpose(1, 2)
    bd = (q + w[a + '.pos_bias_v'].unsqueeze(1)) @ pp.transpose(1, 2)
    if ec.get('do_rel_shift', True):
        bd = wrapped_shift(bd, T)
    sc = (ac + bd) * 0.125
    if visible is not None:
        sc = sc.masked_fill(~visible, -float('inf'))
    ctx = (torch.softmax(sc, dim=-1) @ v).transpose(0, 1).reshape(T, d)
    x = ln(x + ctx @ w[a + '.linear_out.weight'].t() + w[a + '.linear_out.bias'], 'layer_norm1')

    def ffn(t, f):
        Wf, bf = fold_ada(w[f + '.w_1.weight'], w[f + '.w_1.bias'], w[f + '.ada_scale'],
                          w[f + '.ada_bias'])
        return F.silu(t @ Wf.t() + bf) @ w[f + '.w_2.weight'].t() + w[f + '.w_2.bias']

    x = ln(x + ffn(x, p + '.ffn1'), 'layer_norm2')
    c = p + '.conv_module'
    b1 = w[c + '.pointwise_conv1.bias'].double()
    Wf, bf = fold_ada(w[c + '.pointwise_conv1.weight'][:, :, 0], b1, w[c + '.ada_scale'],
                      w[c + '.ada_bias'])
    h = x @ Wf.t() + bf
    g = h[:, :d] * torch.sigmoid(h[:, d:])
    cpad = b1[:d] * torch.sigmoid(b1[d:])
    left = K - 1 if causal else (K - 1) // 2
    right = 0 if causal else (K - 1) // 2
    front = cpad.expand(left, d) if causal else torch.zeros(left, d, dtype=torch.float64)
    gp = torch.cat([front, g, torch.zeros(right, d, dtype=torch.float64)], dim=0)
    y = F.conv1d(gp.t().unsqueeze(0), w[c + '.depthwise_conv.weight'],
                 w[c + '.depthwise_conv.bias'], groups=d)[0].t()
    if ec.get('cnn_norm_type', 'batch_norm') == 'batch_norm':
        sc_ = w[c + '.norm.weight'] / torch.sqrt(w[c + '.norm.running_var'] + 1e-5)
        y = y * sc_ + (w[c + '.norm.bias'] - w[c + '.norm.running_mean'] * sc_)
    else:
        y = F.layer_norm(y, (d, ), w[c + '.norm.weight'], w[c + '.norm.bias'], 1e-5)
    y = F.silu(y) @ w[c + '.pointwise_conv2.weight'][:, :, 0].t() + w[c + '.pointwise_conv2.bias']
    x = ln(x + y, 'layer_norm3')
    return ln(x + ffn(x, p + '.ffn2'), 'layer_norm4')


def frontend_formulation(feats, sd, d, dtype=torch.float64):
    """GlobalCMVN + DepthwiseConv2dSubsampling4 (no dw_stride) on ONE utterance feats (n, F):
    the Conformer's convs under other names, and input_proj(x * sqrt(d)).  (T', d)."""
    pfx = 'encoder.embed.'
    view = {pfx + 'conv.0.weight': sd[pfx + 'pw_conv.weight'],
            pfx + 'conv.0.bias': sd[pfx + 'pw_conv.bias'],
            pfx + 'conv.2.weight': sd[pfx + 'dw_conv.weight'],
            pfx + 'conv.2.bias': sd[pfx + 'dw_conv.bias'],
            pfx + 'out.0.weight': sd[pfx + 'input_proj.0.weight'],
            # (W x + b / sqrt d) * sqrt d = W (x sqrt d) + b
            pfx + 'out.0.bias': (sd[pfx + 'input_proj.0.bias'].double() / math.sqrt(d)),
            'encoder.global_cmvn.mean': sd['encoder.global_cmvn.mean'],
            'encoder.global_cmvn.istd': sd['encoder.global_cmvn.istd']}
    return KR.ref_frontend_chain(feats.unsqueeze(0), [feats.shape[0]], view, d,
                                 fp32=dtype == torch.float32)[0].to(dtype)


def block_model_formulation(feats, sd, configs, dtype=torch.float64):
    """The encoder of a ONE-block model without a time reduction on one utterance: front end,
    preln, the block."""
    ec = configs['encoder_conf']
    d = ec['encoder_dim']
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = frontend_formulation(feats, sd, d, dtype)
    x = F.layer_norm(x, (d, ), w['encoder.preln.weight'], w['encoder.preln.bias'], 1e-5)
    pos = sd['encoder.embed.pos_enc.pe'].reshape(-1, d).to(dtype)
    return layer_formulation(x, w, 'encoder.encoders.0', ec, pos)


# ---------------------------------------------------------------------------------------------
# the inputs of the fixtures (tools/gen_golden_squeezeformer.py records the reference's outputs)

ATTN_MODULE = dict(d=128, H=2, seed=50, frames=(1, 2, 33))
REDUCE_MODULE = dict(d=64, seed=60, frames=(1, 2, 5, 33, 64))
LAYER_T = 40
FRAMES = [291, 135, 131, 127, 15, 11, 7]          # T' = 72, 33, 32, 31, 3, 2, 1
ENC_LENS = [72, 33, 32, 31, 3, 2, 1]
TINY = {
    'tiny_squeezeformer': dict(frames=FRAMES, fseed=500, reverse_weight=0.0),
    'tiny_squeezeformer_u2pp': dict(frames=FRAMES, fseed=510, reverse_weight=0.3),
}
CHUNK_CASES = ((4, -1), (4, 2))    # (decoding_chunk_size, num_decoding_left_chunks)
CHUNK_FRAMES = (135, 15)
CTC_BEAM = 5
METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring')
# one block at each recipe's real widths (tests/test_gpu_squeezeformer.py), 135 frames: T' = 33
WIDTH_CASES = {
    'd256_ffn1024': dict(d=256, heads=4, factor=4, k=31, reduction='conv1d', shift=True,
                         cnn_norm='layer_norm', causal=False),
    'd256_ffn2048_causal_stream': dict(d=256, heads=4, factor=8, k=31, reduction='stream',
                                       shift=False, cnn_norm='layer_norm', causal=True),
    'd512_batch_norm': dict(d=512, heads=8, factor=4, k=31, reduction='conv1d', shift=True,
                            cnn_norm='batch_norm', causal=False),
}


def width_case_configs(name):
    """A one-block model without a time reduction at the widths of a shipped recipe."""
    from wenet_amd import synthetic as S
    c = WIDTH_CASES[name]
    cfg = S.make_configs('tiny_squeezeformer')
    cfg.update(S._squeezeformer(c['d'], c['heads'], c['factor'], 1, None, None, c['k'],
                                c['reduction'], c['shift'], c['cnn_norm'], c['causal'], False,
                                'transformer', c['heads'], 96, 1, 41))
    return cfg


def attn_module_inputs():
    """(x (33, d) fp64, state dict of RelPositionMultiHeadedAttention(H, d, 0, do_rel_shift=True,
    adaptive_scale=True), pos (33, d) fp64)."""
    from wenet_amd import synthetic as S
    m = ATTN_MODULE
    d, H = m['d'], m['H']
    g = torch.Generator().manual_seed(m['seed'])
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).double()
    sd = {'pos_bias_u': r(H, d // H, std=0.3), 'pos_bias_v': r(H, d // H, std=0.3),
          'ada_scale': 1.0 + r(1, 1, d, std=0.2), 'ada_bias': r(1, 1, d, std=0.3),
          'linear_pos.weight': r(d, d, std=d ** -0.5)}
    for n in ('linear_q', 'linear_k', 'linear_v', 'linear_out'):
        sd[n + '.weight'] = r(d, d, std=d ** -0.5)
        sd[n + '.bias'] = r(d, std=0.1)
    T = max(m['frames'])
    x = r(T, d) * 1.2
    pos = S.positional_table(d).reshape(-1, d)[:T].double()
    return x, sd, pos


def reduce_module_inputs(K):
    """(x (64, d) fp64, state dict of TimeReductionLayer1D (K 5) / ...Stream (K 1))."""
    m = REDUCE_MODULE
    d = m['d']
    g = torch.Generator().manual_seed(m['seed'] + K)
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).double()
    sd = {'dw_conv.weight': r(d, 1, K, std=K ** -0.5), 'dw_conv.bias': r(d, std=0.3),
          'pw_conv.weight': r(d, d, 1, std=d ** -0.5), 'pw_conv.bias': r(d, std=0.1)}
    return r(max(m['frames']), d) * 1.3 + 0.1, sd


def layer_module_inputs(name):
    """(x (40, d) fp64, configs, state dict) of block 0 of the tiny model `name`."""
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, 5)
    d = configs['encoder_conf']['encoder_dim']
    g = torch.Generator().manual_seed(70 + len(name))
    x = (torch.randn(LAYER_T, d, generator=g) * 1.2).double()
    return x, configs, sd


def tiny_features(name):
    """The utterances of a model fixture, one (n, 80) fp32 matrix each."""
    from wenet_amd import synthetic as S
    t = TINY[name]
    return [S.make_features(1, n, seed=t['fseed'] + i)[0][0] for i, n in enumerate(t['frames'])]


def load_fixture(stem):
    """(meta, arrays) of tests/golden/squeezeformer/<stem>.npz and its continuation files
    <stem>_<i>.npz; arrays cut into row blocks (`<name>__part<i>`) are put together again."""
    import json
    import os

    import numpy as np
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'squeezeformer')
    raw, meta, i = {}, None, 0
    while True:
        path = os.path.join(gdir, f'{stem}.npz' if i == 0 else f'{stem}_{i}.npz')
        if not os.path.exists(path):
            break
        with np.load(path) as z:
            for k in z.files:
                if k == 'meta':
                    meta = json.loads(bytes(z[k]).decode())
                else:
                    raw[k] = z[k]
        i += 1
    assert meta is not None, f'{stem}.npz is missing (tools/gen_golden_squeezeformer.py)'
    arrays = {}
    for k in sorted(raw, key=lambda s: (s.split('__part')[0], int(s.split('__part')[1])
                                        if '__part' in s else 0)):
        base = k.split('__part')[0]
        arrays[base] = raw[k] if base not in arrays else np.concatenate([arrays[base], raw[k]])
    return meta, arrays
