"""Plain references of the Efficient Conformer kernels (csrc/efficonformer.hip: the grouped
attention, the strided depthwise conv with its norm and swish, the average-pool residual), of the
modules and of one encoder block, and the cases the tests run them on
(tests/test_efficonformer_host.py on the CPU, tests/test_gpu_efficonformer_ops.py and
tests/test_gpu_efficonformer.py on the GPU).

The grouped view is written from its definition, not from pad4group's transposes
(efficient_conformer/attention.py:83-126): the (T, D) matrix of an utterance, zero frames appended
up to a multiple of g, read FLAT as (ceil(T / g), h, g * d_k).  Every formulation evaluates ONE
utterance alone in fp64; fp32=True / dtype=torch.float32 evaluates the SAME
formula in fp32, the yardstick `e_plain` of the GPU tolerances (tests/kernel_refs.py bound /
cap_ok).  The fixtures of tests/golden/efficonformer/ (tools/gen_golden_efficonformer.py) pin the
formulations to the reference's own modules.

No GPU in here.
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import kernel_refs as KR

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'efficonformer')

# ---------------------------------------------------------------------------------------------
# grouped attention


def grouped_view(x, g, H):
    """x (T, D) -> (H, ceil(T / g), g * D / H): zero frames appended, the flat data re-read."""
    T, D = x.shape
    ng = (T + g - 1) // g
    xp = torch.cat([x, torch.zeros(ng * g - T, D, dtype=x.dtype)], dim=0)
    return xp.reshape(ng, H, g * D // H).transpose(0, 1)


def group_visible(ng, m, chunk, left):
    """(ng, ng) bool: query group r sees key group s.  chunk 0: everything.  Else, in frames of
    the mask's own rate, m frames per group row: m s < ((m r) // chunk + 1) * chunk and, for
    left >= 0, m s >= ((m r) // chunk - left) * chunk."""
    vis = torch.ones(ng, ng, dtype=torch.bool)
    if chunk <= 0:
        return vis
    for r in range(ng):
        qc = (m * r) // chunk
        for s in range(ng):
            ok = m * s < (qc + 1) * chunk
            if left >= 0:
                ok = ok and m * s >= (qc - left) * chunk
            vis[r, s] = ok
    return vis


def ref_attention_grouped(q, k, v, P, bias_u, bias_v, seqs, p_offs, g, H, scale, mask_step=1,
                          chunk=0, left=-1, fp32=False):
    """q / k / v (rows, >= D) and P (p_rows, >= D) packed frames (only the first D columns are
    read), bias_u / bias_v (H, W), seqs = [(off, len)], p_offs the first table row of every
    sequence.  Per sequence, with everything read through grouped_view:
        softmax(((q + u) k^T + (q + v) p^T) * scale, masked by group_visible) v
    written back through the same view, the padded frames dropped.  (rows, D) fp64."""
    dt = torch.float32 if fp32 else torch.float64
    W = bias_u.shape[1]
    D = H * W // g
    out = torch.zeros(q.shape[0], D, dtype=torch.float64)
    for (off, T), po in zip(seqs, p_offs):
        if T == 0:
            continue
        ng = (T + g - 1) // g
        qs = grouped_view(q[off:off + T, :D].to(dt), g, H)
        ks = grouped_view(k[off:off + T, :D].to(dt), g, H)
        vs = grouped_view(v[off:off + T, :D].to(dt), g, H)
        ps = grouped_view(P[po:po + T, :D].to(dt), g, H)
        ac = torch.matmul(qs + bias_u.to(dt).unsqueeze(1), ks.transpose(1, 2))
        bd = torch.matmul(qs + bias_v.to(dt).unsqueeze(1), ps.transpose(1, 2))
        sc = (ac + bd) * scale
        vis = group_visible(ng, mask_step, chunk, left)
        sc = sc.masked_fill(~vis, -float('inf'))
        o = torch.matmul(torch.softmax(sc, dim=-1), vs)             # (H, ng, W)
        out[off:off + T] = o.transpose(0, 1).reshape(ng * g, D)[:T].double()
    return out


GROUPED_LENS = [1, 2, 3, 4, 31, 95, 97, 200]
# (chunk_size, left_chunks, mask_step)
GROUPED_MASKS = [(0, -1, 3), (4, -1, 3), (4, 0, 3), (4, 2, 6), (16, -1, 6), (16, 0, 3), (16, 2, 3),
                 (16, 2, 6)]
GROUPED_HEADS = {96: 4, 192: 2}       # W -> heads at D = 128, g = 3


def make_grouped_case(W, lens=GROUPED_LENS, g=3, seed=0, gap=3, lead=5, pads=(8, 4, 12, 4)):
    """One packed batch at D = H W / g with row strides D + pads (Q, K, V, P).  Rows no sequence
    owns and the pad columns hold +-POISON; the position table is packed like the frames (its own
    gaps, p_offs), so the rows behind a sequence's len are POISON too: frames >= len must read
    as zeros, never as what lies there."""
    gen = torch.Generator().manual_seed(seed)
    H = GROUPED_HEADS[W]
    D = H * W // g
    offs, rows = KR.pack_layout(lens, gap, lead)
    p_offs, p_rows = KR.pack_layout(lens, gap + 2, lead - 3)
    sgn = torch.where(torch.arange(D + max(pads)) % 2 == 0, 1.0, -1.0) * KR.POISON

    def packed(n_rows, layout, pad, flip, std):
        t = (flip * sgn[:D + pad]).expand(n_rows, D + pad).clone()
        for o, n in zip(layout, lens):
            t[o:o + n, :D] = torch.randn(n, D, generator=gen) * std
        return t

    q = packed(rows, offs, pads[0], 1.0, 1.0)
    k = packed(rows, offs, pads[1], -1.0, 1.0)
    v = packed(rows, offs, pads[2], 1.0, 1.0)
    P = packed(p_rows, p_offs, pads[3], -1.0, 1.0)
    bu = torch.randn(H, W, generator=gen) * 0.5
    bv = torch.randn(H, W, generator=gen) * 0.5
    own = torch.zeros(rows, dtype=torch.bool)
    for o, n in zip(offs, lens):
        own[o:o + n] = True
    return dict(q=q, k=k, v=v, P=P, bias_u=bu, bias_v=bv, seqs=list(zip(offs, lens)),
                p_offs=p_offs, g=g, H=H, W=W, D=D, rows=rows, p_rows=p_rows, own=own,
                scale=1.0 / math.sqrt(W))


def grouped_refs(c, chunk=0, left=-1, mask_step=3):
    """(fp64 reference, e_plain, scale)."""
    a = (c['q'], c['k'], c['v'], c['P'], c['bias_u'], c['bias_v'], c['seqs'], c['p_offs'], c['g'],
         c['H'], c['scale'], mask_step, chunk, left)
    ref = ref_attention_grouped(*a)
    plain = ref_attention_grouped(*a, fp32=True)
    scale = max(c['v'][o:o + T, :c['D']].abs().max().item() for o, T in c['seqs'] if T > 0)
    return ref, (plain - ref).abs().max().item(), scale


# ---------------------------------------------------------------------------------------------
# strided depthwise conv + norm + swish, average-pool residual


def ref_stride_dwconv(x, wt, bias, ln_w, ln_b, norm_mode, K, causal, seqs, out_offs, out_rows,
                      cpad=None, stride=2, dtype=torch.float64, eps=1e-5):
    """x (rows, C) packed rows, wt (C, 1, K) / bias (C) as Conv1d(groups=C) holds them.  For
    t < ceil(len / stride): c[t] = bias + sum_k wt[:, 0, k] * x[stride t - pad + k], pad =
    (K - 1) / 2 or K - 1 (causal); frames >= len are zeros, frames < 0 zeros or (causal, cpad
    given) cpad.  y = silu(LayerNorm(c)) (norm_mode 0) or silu(c * ln_w + ln_b) (1).
    (out_rows, C) fp64, zero in unowned rows."""
    C = x.shape[1]
    out = torch.zeros(out_rows, C, dtype=torch.float64)
    w = wt.to(dtype)[:, 0, :]
    pad = K - 1 if causal else (K - 1) // 2
    for (off, T), o2 in zip(seqs, out_offs):
        xs = x[off:off + T].to(dtype)
        for t in range((T + stride - 1) // stride):
            acc = torch.zeros(C, dtype=dtype)
            for kk in range(K):
                s = stride * t - pad + kk
                if 0 <= s < T:
                    acc = acc + w[:, kk] * xs[s]
                elif s < 0 and causal and cpad is not None:
                    acc = acc + w[:, kk] * cpad.to(dtype)
            acc = acc + bias.to(dtype)
            if norm_mode == 0:
                acc = F.layer_norm(acc, (C, ), ln_w.to(dtype), ln_b.to(dtype), eps)
            else:
                acc = acc * ln_w.to(dtype) + ln_b.to(dtype)
            out[o2 + t] = F.silu(acc).double()
    return out


def ref_avgpool_residual(x, z, seqs, out_offs, dtype=torch.float64):
    """y[o2 + t] = z[o2 + t] + mean(x[off + 2 t .. min(2 t + 2, len) - 1]): (a + b) * 0.5 for a
    full window, the last frame itself for the short one.  Zero in unowned rows."""
    out = torch.zeros(z.shape, dtype=torch.float64)
    for (off, T), o2 in zip(seqs, out_offs):
        for t in range((T + 1) // 2):
            a = x[off + 2 * t].to(dtype)
            p = (a + x[off + 2 * t + 1].to(dtype)) * 0.5 if 2 * t + 1 < T else a
            out[o2 + t] = (z[o2 + t].to(dtype) + p).double()
    return out


STRIDE_LENS = [1, 2, 3, 16, 33, 64]


def make_stride_case(C, K, lens=STRIDE_LENS, seed=0, gap=2, lead=3):
    """Packed incoming rows x (POISON in unowned rows), the outgoing layout (its own gaps) with z,
    taps of order 1 / sqrt(K), a norm's weights and a pad frame."""
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
    ln_w = 1.0 + torch.randn(C, generator=g) * 0.1
    ln_b = torch.randn(C, generator=g) * 0.1
    cpad = torch.randn(C, generator=g) * 0.7
    return dict(x=x, z=z, wt=wt, bias=bias, ln_w=ln_w, ln_b=ln_b, cpad=cpad, K=K, C=C,
                seqs=list(zip(offs, lens)), offs2=offs2, lens2=lens2, rows=rows, rows2=rows2)


def stride_dwconv_refs(c, norm_mode, causal, cpad=None):
    a = (c['x'], c['wt'], c['bias'], c['ln_w'], c['ln_b'], norm_mode, c['K'], causal, c['seqs'],
         c['offs2'], c['rows2'], cpad)
    ref = ref_stride_dwconv(*a)
    plain = ref_stride_dwconv(*a, dtype=torch.float32)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# modules, written from the module text


def grouped_attention_module(x, w, p, H, g, pos, visible=None):
    """GroupedRelPositionMultiHeadedAttention.forward on one utterance x (T, d); pos (>= T, d) the
    position rows of the layer's rate; visible (ng, ng) bool or None."""
    T, d = x.shape
    lin = lambda n: x @ w[f'{p}.{n}.weight'].t() + w[f'{p}.{n}.bias']
    q, k, v = (grouped_view(lin(n), g, H) for n in ('linear_q', 'linear_k', 'linear_v'))
    pp = grouped_view(pos[:T].to(x.dtype) @ w[p + '.linear_pos.weight'].t(), g, H)
    ac = (q + w[p + '.pos_bias_u'].unsqueeze(1)) @ k.transpose(1, 2)
    bd = (q + w[p + '.pos_bias_v'].unsqueeze(1)) @ pp.transpose(1, 2)
    sc = (ac + bd) / math.sqrt(g * d // H)
    if visible is not None:
        sc = sc.masked_fill(~visible, -float('inf'))
    ng = q.shape[1]
    ctx = (torch.softmax(sc, dim=-1) @ v).transpose(0, 1).reshape(ng * g, d)[:T]
    return ctx @ w[p + '.linear_out.weight'].t() + w[p + '.linear_out.bias']


def plain_attention_module(x, w, p, H, pos, visible=None):
    """RelPositionMultiHeadedAttention.forward without a shift on one utterance."""
    T, d = x.shape
    dk = d // H
    heads = lambda t: t.view(-1, H, dk).transpose(0, 1)
    lin = lambda n: x @ w[f'{p}.{n}.weight'].t() + w[f'{p}.{n}.bias']
    q, k, v = (heads(lin(n)) for n in ('linear_q', 'linear_k', 'linear_v'))
    pp = heads(pos[:T].to(x.dtype) @ w[p + '.linear_pos.weight'].t())
    ac = (q + w[p + '.pos_bias_u'].unsqueeze(1)) @ k.transpose(1, 2)
    bd = (q + w[p + '.pos_bias_v'].unsqueeze(1)) @ pp.transpose(1, 2)
    sc = (ac + bd) / math.sqrt(dk)
    if visible is not None:
        sc = sc.masked_fill(~visible, -float('inf'))
    # (the reference's MultiHeadedAttention.forward_attention takes this softmax in fp32 whatever
    # the module's dtype, transformer/attention.py:163; the grouped attention has its own,
    # dtype-preserving forward_attention)
    ctx = (torch.softmax(sc.float(), dim=-1).to(x.dtype) @ v).transpose(0, 1).reshape(T, d)
    return ctx @ w[p + '.linear_out.weight'].t() + w[p + '.linear_out.bias']


def conv_module(x, w, p, K, causal, batch_norm, stride=1):
    """efficient_conformer ConvolutionModule.forward on one utterance: K - 1 ZERO frames in front
    when causal (in front of pointwise_conv1), GLU, the depthwise conv with `stride` (its own zero
    padding when not causal), norm, swish, pointwise_conv2.  (ceil(T / stride), d)."""
    T, d = x.shape
    xa = torch.cat([torch.zeros(K - 1, d, dtype=x.dtype), x], dim=0) if causal else x
    h = xa @ w[p + '.pointwise_conv1.weight'][:, :, 0].t() + w[p + '.pointwise_conv1.bias']
    g = h[:, :d] * torch.sigmoid(h[:, d:])
    y = F.conv1d(g.t().unsqueeze(0), w[p + '.depthwise_conv.weight'],
                 w[p + '.depthwise_conv.bias'], stride=stride,
                 padding=0 if causal else (K - 1) // 2, groups=d)[0].t()
    if batch_norm:
        sc = w[p + '.norm.weight'] / torch.sqrt(w[p + '.norm.running_var'] + 1e-5)
        y = (y - w[p + '.norm.running_mean']) * sc + w[p + '.norm.bias']
    else:
        y = F.layer_norm(y, (d, ), w[p + '.norm.weight'], w[p + '.norm.bias'], 1e-5)
    y = F.silu(y)
    return y @ w[p + '.pointwise_conv2.weight'][:, :, 0].t() + w[p + '.pointwise_conv2.bias']


def avgpool_time(x):
    """AvgPool1d(2, 2, ceil_mode=True, count_include_pad=False) over time of x (T, d)."""
    T = x.shape[0]
    rows = [(x[2 * t] + x[2 * t + 1]) * 0.5 if 2 * t + 1 < T else x[2 * t]
            for t in range((T + 1) // 2)]
    return torch.stack(rows)


def ffn_module(x, w, p):
    return F.silu(x @ w[p + '.w_1.weight'].t() + w[p + '.w_1.bias']) @ w[p + '.w_2.weight'].t() \
        + w[p + '.w_2.bias']


def layer_formulation(x, w, p, H, pos, K, causal, batch_norm, grouped, stride, g=3, visible=None):
    """ConformerEncoderLayer / StrideConformerEncoderLayer.forward (pre-LN, macaron) on one
    utterance x (T, d).  `visible`: at the layer's own (group) rate."""
    d = x.shape[1]
    ln = lambda t, n: F.layer_norm(t, (d, ), w[f'{p}.{n}.weight'], w[f'{p}.{n}.bias'], 1e-5)
    x = x + 0.5 * ffn_module(ln(x, 'norm_ff_macaron'), w, p + '.feed_forward_macaron')
    if grouped:
        x = x + grouped_attention_module(ln(x, 'norm_mha'), w, p + '.self_attn', H, g, pos, visible)
    else:
        x = x + plain_attention_module(ln(x, 'norm_mha'), w, p + '.self_attn', H, pos, visible)
    y = conv_module(ln(x, 'norm_conv'), w, p + '.conv_module', K, causal, batch_norm,
                    2 if stride else 1)
    x = (avgpool_time(x) if stride else x) + y
    x = x + 0.5 * ffn_module(ln(x, 'norm_ff'), w, p + '.feed_forward')
    return ln(x, 'norm_final')


def frame_visible(T, chunk, left):
    """subsequent_chunk_mask (utils/mask.py) of T frames: (T, T) bool, or None for chunk <= 0."""
    return None if chunk <= 0 else group_visible(T, 1, chunk, left)


def encoder_formulation(x, sd, plan, chunk=0, left=-1, dtype=torch.float64):
    """The layers + after_norm on the front end's output x (T0, d) of ONE utterance; `plan` as
    wenet_amd.efficonformer.efficonformer_plan returns it."""
    d = x.shape[1]
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    pe = sd['encoder.embed.pos_enc.pe'].reshape(-1, d).to(dtype)
    x = x.to(dtype)
    g = plan['group_size']
    for i in range(plan['blocks']):
        f = plan['rates'][i]
        T = x.shape[0]
        grouped = i in plan['group_layers']
        if chunk <= 0:
            vis = None
        elif grouped:
            vis = group_visible((T + g - 1) // g, f * g, chunk, left)
        else:
            vis = group_visible(T, f, chunk, left)
        x = layer_formulation(x, w, f'encoder.encoders.{i}', plan['heads'], pe[0::f],
                              plan['kernels'][i], plan['causal'],
                              plan['ec'].get('cnn_module_norm', 'batch_norm') == 'batch_norm',
                              grouped, i in plan['stride_layers'], g, vis)
    return F.layer_norm(x, (d, ), w['encoder.after_norm.weight'], w['encoder.after_norm.bias'],
                        1e-5)


def frontend_formulation(feats, sd, d, front_rate, dtype=torch.float64):
    """GlobalCMVN + Conv2dSubsampling4 / Conv2dSubsampling2 + the rel-pos scaling on ONE utterance
    feats (n, F).  (T0, d)."""
    if front_rate == 4:
        return KR.ref_frontend_chain(feats.unsqueeze(0), [feats.shape[0]], sd, d,
                                     fp32=dtype == torch.float32)[0].to(dtype)
    x = feats.to(dtype)
    if 'encoder.global_cmvn.mean' in sd:
        x = (x - sd['encoder.global_cmvn.mean'].to(dtype)) * sd['encoder.global_cmvn.istd'].to(dtype)
    y = F.relu(F.conv2d(x[None, None], sd['encoder.embed.conv.0.weight'].to(dtype),
                        sd['encoder.embed.conv.0.bias'].to(dtype), stride=2))[0]   # (c, t, f)
    c, t, f = y.shape
    y = y.permute(1, 0, 2).reshape(t, c * f)
    y = y @ sd['encoder.embed.out.0.weight'].to(dtype).t() + sd['encoder.embed.out.0.bias'].to(dtype)
    return y * math.sqrt(d)


# ---------------------------------------------------------------------------------------------
# the inputs of the fixtures (tools/gen_golden_efficonformer.py records the reference's outputs)

ATTN_MODULE = {'w96': dict(d=128, H=4, g=3, seed=50, frames=(1, 2, 3, 4, 33)),
               'w192': dict(d=128, H=2, g=3, seed=51, frames=(1, 2, 3, 4, 33))}
CONV_MODULE = {'k15_ln': dict(d=64, K=15, causal=False, norm='layer_norm', seed=60),
               'k7_bn_causal': dict(d=64, K=7, causal=True, norm='batch_norm', seed=61)}
CONV_FRAMES = (1, 2, 3, 16, 33)
ATTN_MASK_T = 21
ATTN_MASK_CASES = [(3, 4, 0), (6, 4, 2), (6, 16, -1), (3, 16, 1)]     # (mask_step, chunk, left)
LAYER_T = 40
MASK_T = 50
MASK_CASES = [(m, c, left) for m in (3, 6) for c in (4, 8, 16) for left in (-1, 0, 2)]
# v1: conv2d, T0 = 72, 33, 32, 31, 3, 2, 1 in front of both grouped layers and the stride layer
# v2: conv2d2, T0 = (n - 1) // 2 = 73, 36, 35, 17, 7, 5, 3, 2, 1 in front of the first grouped
#     stride layer, 37, 18, 18, 9, 4, 3, 2, 1, 1 in front of the second
# (tests/test_efficonformer_host.py checks that both cover T mod 3 = 0, 1, 2, T = 1 and 2, odd and
# even lengths at every grouped / stride layer)
TINY = {
    'tiny_efficonformer_v1': dict(frames=[291, 135, 131, 127, 15, 11, 7], fseed=600,
                                  reverse_weight=0.3, chunk_cases=((4, -1), (4, 2)),
                                  chunk_frames=(135, 15)),
    'tiny_efficonformer_v2': dict(frames=[147, 73, 71, 35, 15, 11, 7, 5, 3], fseed=610,
                                  reverse_weight=0.0, chunk_cases=((8, -1), (8, 1)),
                                  chunk_frames=(147, 35)),
}
CTC_BEAM = 5
METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring')
RECIPES = ('aishell_v1', 'aishell_v1_stream', 'aishell_v2', 'librispeech_v1', 'librispeech_v2')


def attn_module_inputs(name):
    """(x (33, d) fp64, state dict of GroupedRelPositionMultiHeadedAttention(H, d, 0, g),
    pos (33, d) fp64)."""
    from wenet_amd import synthetic as S
    m = ATTN_MODULE[name]
    d, H, g = m['d'], m['H'], m['g']
    gen = torch.Generator().manual_seed(m['seed'])
    r = lambda *s, std=1.0: (torch.randn(*s, generator=gen) * std).double()
    sd = {'pos_bias_u': r(H, g * d // H, std=0.3), 'pos_bias_v': r(H, g * d // H, std=0.3),
          'linear_pos.weight': r(d, d, std=d ** -0.5)}
    for n in ('linear_q', 'linear_k', 'linear_v', 'linear_out'):
        sd[n + '.weight'] = r(d, d, std=d ** -0.5)
        sd[n + '.bias'] = r(d, std=0.1)
    T = max(m['frames'])
    x = r(T, d) * 1.2
    pos = S.positional_table(d).reshape(-1, d)[:T].double()
    return x, sd, pos


def conv_module_inputs(name):
    """(x (33, d) fp64, state dict of ConvolutionModule(d, K, SiLU, norm, causal, True, 2))."""
    m = CONV_MODULE[name]
    d, K = m['d'], m['K']
    gen = torch.Generator().manual_seed(m['seed'])
    r = lambda *s, std=1.0: (torch.randn(*s, generator=gen) * std).double()
    sd = {'pointwise_conv1.weight': r(2 * d, d, 1, std=d ** -0.5),
          'pointwise_conv1.bias': r(2 * d, std=0.3),
          'depthwise_conv.weight': r(d, 1, K, std=K ** -0.5), 'depthwise_conv.bias': r(d, std=0.3),
          'norm.weight': 1.0 + r(d, std=0.1), 'norm.bias': r(d, std=0.1),
          'pointwise_conv2.weight': r(d, d, 1, std=d ** -0.5), 'pointwise_conv2.bias': r(d, std=0.1)}
    if m['norm'] == 'batch_norm':
        sd['norm.running_mean'] = r(d, std=0.3)
        sd['norm.running_var'] = 0.5 + r(d, std=0.5).abs()
        sd['norm.num_batches_tracked'] = torch.tensor(1000)
    return r(max(CONV_FRAMES), d) * 1.3 + 0.1, sd


def layer_module_inputs(name):
    """(x (40, d) fp64, configs, state dict) of the first stride layer of the tiny model `name`
    (a grouped stride layer in both)."""
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, 5)
    d = configs['encoder_conf']['output_size']
    gen = torch.Generator().manual_seed(70 + len(name))
    x = (torch.randn(LAYER_T, d, generator=gen) * 1.2).double()
    return x, configs, sd


def tiny_features(name):
    """The utterances of a model fixture, one (n, 80) fp32 matrix each."""
    from wenet_amd import synthetic as S
    t = TINY[name]
    return [S.make_features(1, n, seed=t['fseed'] + i)[0][0] for i, n in enumerate(t['frames'])]


def width_case_configs():
    """A one-block model at the shipped widths: 256, 8 heads (W = 96), K 15, the block grouped and
    strided (tests/test_gpu_efficonformer.py)."""
    from wenet_amd import synthetic as S
    cfg = S.make_configs('tiny_efficonformer_v1')
    cfg.update(S._efficonformer(256, 8, 2048, 1, 'conv2d', [0], [0], True, 15, 'layer_norm', False,
                                'transformer', 4, 96, 1, 41))
    return cfg


def load_recipe(name):
    import yaml
    with open(os.path.join(GOLDEN_DIR, 'recipes', name + '.yaml')) as f:
        return yaml.safe_load(f)


def load_fixture(stem):
    """(meta, arrays) of tests/golden/efficonformer/<stem>.npz and its continuation files
    <stem>_<i>.npz; arrays cut into row blocks (`<name>__part<i>`) are put together again."""
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
    assert meta is not None, f'{stem}.npz is missing (tools/gen_golden_efficonformer.py)'
    arrays = {}
    for k in sorted(raw, key=lambda s: (s.split('__part')[0], int(s.split('__part')[1])
                                        if '__part' in s else 0)):
        base = k.split('__part')[0]
        arrays[base] = raw[k] if base not in arrays else np.concatenate([arrays[base], raw[k]])
    return meta, arrays
