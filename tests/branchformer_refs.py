"""Plain references of the Branchformer / E-Branchformer kernels (csrc/branchformer.hip: the
cgMLP's gating unit, the merge conv), of the layers and of the whole encoder, and the cases the
tests run them on (tests/test_branchformer_host.py on the CPU, tests/test_gpu_branchformer_ops.py
and tests/test_gpu_branchformer.py on the GPU).

Every formulation is written from the reference's module text (wenet/models/branchformer/
cgmlp.py:86-131, encoder_layer.py:112-206; e_branchformer/encoder_layer.py:94-148) in fp64 torch
and evaluates ONE utterance alone -- the rule of the library: the reference's
cgMLP and merge convs ignore the padding mask, so its batched result depends on the batch.
dtype=float32 evaluates the SAME formula in fp32, the yardstick `e_plain` of the GPU tolerances
(tests/kernel_refs.py bound).  The fixtures of tests/golden/branchformer/
(tools/gen_golden_branchformer.py) pin the formulations to the reference's own modules.

No GPU in here.
"""
import math

import torch
import torch.nn.functional as F

import kernel_refs as KR

# ---------------------------------------------------------------------------------------------
# the two kernels


def dwconv_alone(x, wt, bias, K, causal, pad_row=None):
    """Depthwise conv over time of ONE utterance x (T, C): wt (C, 1, K) and bias (C) as
    torch.nn.Conv1d(groups=C) holds them.  K - 1 padded frames in front when causal, (K - 1) / 2
    on both sides otherwise; a padded frame is `pad_row` (C) or 0."""
    T, C = x.shape
    left = K - 1 if causal else (K - 1) // 2
    right = 0 if causal else (K - 1) // 2
    row = torch.zeros(C, dtype=x.dtype) if pad_row is None else pad_row.to(x.dtype)
    xp = torch.cat([row.expand(left, C), x, row.expand(right, C)], dim=0)
    return F.conv1d(xp.t().unsqueeze(0), wt.to(x.dtype), bias.to(x.dtype), groups=C)[0].t()


def ref_csgu(h, ln_w, ln_b, wt, bias, K, causal, seqs, gate=True, dtype=torch.float64,
             mutate=None):
    """ConvolutionalSpatialGatingUnit.forward (without the optional Linear) on the packed rows
    h (rows, 2 C), seqs = [(off, len)]: r, g = h.chunk(2); g = LayerNorm(g); g = conv(g);
    out = r * g.  causal: the reference pads K - 1 zero frames IN FRONT of the LayerNorm, so a
    padded frame enters the conv as ln_b; otherwise the conv's own zero padding applies behind
    the norm.  Returns (rows, C) fp64, zero in rows no utterance owns.
    mutate: one of the mistakes tests/test_branchformer_host.py shows the fixtures would catch --
    'pad_zero' (causal pad frame 0), 'pad_bias' (non-causal pad frame ln_b), 'drop_tap' (the
    last tap missing), 'neighbours' (the conv runs over the packed buffer, across utterance
    boundaries), 'swap' (r and g exchanged)."""
    C = h.shape[1] // 2
    out = torch.zeros(h.shape[0], C, dtype=torch.float64)
    w = wt.clone()
    if mutate == 'drop_tap':
        w[:, :, K - 1] = 0
    hd = h.to(dtype)
    r_all, g_all = hd[:, :C], hd[:, C:]
    if mutate == 'swap':
        r_all, g_all = g_all, r_all
    norm = lambda t: F.layer_norm(t, (C, ), ln_w.to(dtype), ln_b.to(dtype), 1e-5)
    pad_is_bias = (causal and mutate != 'pad_zero') or (not causal and mutate == 'pad_bias')
    pad_row = ln_b if pad_is_bias else None
    if mutate == 'neighbours':
        lo, hi = seqs[0][0], seqs[-1][0] + seqs[-1][1]
        whole = torch.nan_to_num(norm(g_all[lo:hi]), nan=0.0, posinf=1e6, neginf=-1e6)
        conv_all = dwconv_alone(whole, w, bias, K, causal, pad_row)
    for (off, T) in seqs:
        if T == 0:
            continue
        if mutate == 'neighbours':
            cv = conv_all[off - lo:off - lo + T]
        else:
            cv = dwconv_alone(norm(g_all[off:off + T]), w, bias, K, causal, pad_row)
        out[off:off + T] = ((r_all[off:off + T] * cv) if gate else cv).double()
    return out


def ref_merge(c, wt, bias, K, causal, seqs, dtype=torch.float64):
    """c + depthwise_conv_fusion(c) on packed rows c (rows, 2 d), zero padding
    (e_branchformer/encoder_layer.py:129-137 in front of merge_proj)."""
    out = torch.zeros(c.shape, dtype=torch.float64)
    for (off, T) in seqs:
        if T > 0:
            x = c[off:off + T].to(dtype)
            out[off:off + T] = (x + dwconv_alone(x, wt, bias, K, causal)).double()
    return out


def op_lens(tile):
    """The packed utterances of every operator launch: 1, 5, tile - 1 and tile + 1 frames."""
    return [1, 5, tile - 1, tile + 1]


def make_csgu_case(C, K, causal, lens, seed=0, order=None, gap=2, lead=3):
    """h (rows, 2 C) with the utterances `lens` packed in `order` (a permutation: position ->
    utterance; the content of an utterance does not depend on where it lies), POISON in rows no
    utterance owns; a LayerNorm with a bias of order 0.3, taps of order 1 / sqrt(K)."""
    g = torch.Generator().manual_seed(seed)
    utts = [torch.randn(n, 2 * C, generator=g) * 1.5 + 0.2 for n in lens]
    ln_w = 1.0 + torch.randn(C, generator=g) * 0.1
    ln_b = torch.randn(C, generator=g) * 0.3
    wt = (torch.rand(C, 1, K, generator=g) * 2 - 1) / math.sqrt(K)
    bias = (torch.rand(C, generator=g) * 2 - 1) / math.sqrt(K)
    order = list(range(len(lens))) if order is None else list(order)
    offs, rows = KR.pack_layout([lens[u] for u in order], gap, lead)
    h = torch.full((rows, 2 * C), KR.POISON)
    seq_of = {}
    for pos, u in enumerate(order):
        h[offs[pos]:offs[pos] + lens[u]] = utts[u]
        seq_of[u] = (offs[pos], lens[u])
    seqs = [(offs[pos], lens[u]) for pos, u in enumerate(order)]
    return dict(h=h, ln_w=ln_w, ln_b=ln_b, wt=wt, bias=bias, K=K, causal=causal, C=C, seqs=seqs,
                seq_of=seq_of, rows=rows)


def csgu_refs(c, gate=True):
    """(fp64 reference, e_plain, scale)."""
    a = (c['h'], c['ln_w'], c['ln_b'], c['wt'], c['bias'], c['K'], c['causal'], c['seqs'], gate)
    ref = ref_csgu(*a)
    plain = ref_csgu(*a, dtype=torch.float32)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


def merge_refs(c):
    """The same case read as a merge input: x = the first C columns of h."""
    a = (c['h'][:, :c['C']], c['wt'], c['bias'], c['K'], c['causal'], c['seqs'])
    ref = ref_merge(*a)
    plain = ref_merge(*a, dtype=torch.float32)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# modules


def cgmlp_formulation(x, w, p, K, causal, mutate=None):
    """ConvolutionalGatingMLP.forward on one utterance x (T, d); w: weights by name, p: prefix."""
    dt = x.dtype
    h = F.gelu(x @ w[p + '.channel_proj1.0.weight'].t() + w[p + '.channel_proj1.0.bias'])
    T = x.shape[0]
    lin = p + '.csgu.linear.weight' in w
    g = ref_csgu(h, w[p + '.csgu.norm.weight'], w[p + '.csgu.norm.bias'],
                 w[p + '.csgu.conv.weight'], w[p + '.csgu.conv.bias'], K, causal, [(0, T)],
                 gate=not lin, dtype=dt, mutate=mutate).to(dt)
    if lin:
        g = g @ w[p + '.csgu.linear.weight'].t() + w[p + '.csgu.linear.bias']
        g = h[:, :h.shape[1] // 2] * g
    return g @ w[p + '.channel_proj2.weight'].t() + w[p + '.channel_proj2.bias']


def rel_attention(x, w, p, H, pos, visible, softmax32):
    """RelPositionMultiHeadedAttention.forward (transformer/attention.py:395-428, no rel_shift:
    key j uses position row j) on one utterance x (T, d) with heads of ANY width d / H.
    softmax32: the softmax in fp32 whatever the dtype, as the module runs it."""
    T, d = x.shape
    dk = d // H
    heads = lambda t: t.view(-1, H, dk).transpose(0, 1)
    q = heads(x @ w[p + '.linear_q.weight'].t() + w[p + '.linear_q.bias'])
    k = heads(x @ w[p + '.linear_k.weight'].t() + w[p + '.linear_k.bias'])
    v = heads(x @ w[p + '.linear_v.weight'].t() + w[p + '.linear_v.bias'])
    pp = heads(pos[:T].to(x.dtype) @ w[p + '.linear_pos.weight'].t())
    qu = q + w[p + '.pos_bias_u'].unsqueeze(1)
    qv = q + w[p + '.pos_bias_v'].unsqueeze(1)
    scores = (qu @ k.transpose(1, 2) + qv @ pp.transpose(1, 2)) / math.sqrt(dk)
    scores = scores.masked_fill(~visible, -float('inf'))
    if softmax32:
        attn = torch.softmax(scores.float(), dim=-1).to(x.dtype)
    else:
        attn = torch.softmax(scores, dim=-1)
    attn = attn.masked_fill(~visible, 0.0)
    ctx = (attn @ v).transpose(0, 1).reshape(T, d)
    return ctx @ w[p + '.linear_out.weight'].t() + w[p + '.linear_out.bias']


def layer_formulation(x, w, p, ec, ebf, pos, visible, softmax32=True):
    """BranchformerEncoderLayer (merge_method concat) / EBranchformerEncoderLayer on one
    utterance x (T, d)."""
    d, H = ec['output_size'], ec['attention_heads']
    K, causal = ec['cgmlp_conv_kernel'], bool(ec.get('causal', False))
    eps = ec.get('norm_eps', 1e-5)
    ln = lambda t, n: F.layer_norm(t, (d, ), w[f'{p}.{n}.weight'], w[f'{p}.{n}.bias'], eps)

    def ffn(t, q):
        hh = F.silu(t @ w[q + '.w_1.weight'].t() + w[q + '.w_1.bias'])
        return hh @ w[q + '.w_2.weight'].t() + w[q + '.w_2.bias']

    if ebf:
        x = x + 0.5 * ffn(ln(x, 'norm_ff_macaron'), p + '.feed_forward_macaron')
    x1 = rel_attention(ln(x, 'norm_mha'), w, p + '.attn', H, pos, visible, softmax32)
    x2 = cgmlp_formulation(ln(x, 'norm_mlp'), w, p + '.cgmlp', K, causal)
    c = torch.cat([x1, x2], dim=-1)
    if ebf:
        Km = ec.get('merge_conv_kernel', 3)
        c = ref_merge(c, w[p + '.depthwise_conv_fusion.weight'],
                      w[p + '.depthwise_conv_fusion.bias'], Km, causal, [(0, x.shape[0])],
                      dtype=x.dtype).to(x.dtype)
    x = x + c @ w[p + '.merge_proj.weight'].t() + w[p + '.merge_proj.bias']
    if ebf:
        x = x + 0.5 * ffn(ln(x, 'norm_ff'), p + '.feed_forward')
    return ln(x, 'norm_final')


def encoder_formulation(feats, sd, configs, chunk=-1, left=-1, softmax32=True,
                        dtype=torch.float64, n_layers=None):
    """BranchformerEncoder / EBranchformerEncoder.forward on ONE utterance feats (n, F): CMVN,
    Conv2dSubsampling4 and the sqrt(d) scale (tests/kernel_refs.ref_frontend_chain), the layers,
    after_norm.  chunk > 0 on a use_dynamic_chunk model: the chunk mask of mask.py:126-198 with
    `left` chunks of history (< 0: all)."""
    ec = configs['encoder_conf']
    d = ec['output_size']
    ebf = configs['encoder'] == 'e_branchformer'
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = KR.ref_frontend_chain(feats.unsqueeze(0), [feats.shape[0]], sd, d,
                              fp32=dtype == torch.float32)[0].to(dtype)
    T = x.shape[0]
    mode = 2 if (ec.get('use_dynamic_chunk', False) and chunk > 0) else 0
    visible = KR.chunk_window(T, T, mode, chunk, left)
    pos = sd['encoder.embed.pos_enc.pe'].reshape(-1, d)
    nl = ec['num_blocks'] if n_layers is None else n_layers
    for i in range(nl):
        x = layer_formulation(x, w, f'encoder.encoders.{i}', ec, ebf, pos, visible, softmax32)
    return F.layer_norm(x, (d, ), w['encoder.after_norm.weight'], w['encoder.after_norm.bias'],
                        ec.get('norm_eps', 1e-5))


# ---------------------------------------------------------------------------------------------
# zero-padded heads (head width 32 on the d_k = 64 attention kernel), in numpy for the host test


def pad_heads_rows(w, H, hd):
    """(H * hd, ...) -> (H * 64, ...): head h's hd rows, then 64 - hd zero rows."""
    import numpy as np
    out = np.zeros((H * 64, ) + w.shape[1:], dtype=w.dtype)
    for h in range(H):
        out[h * 64:h * 64 + hd] = w[h * hd:(h + 1) * hd]
    return out


# ---------------------------------------------------------------------------------------------
# the inputs of the fixtures (tools/gen_golden_branchformer.py records the reference's outputs)

MODULE_T = (40, 5)             # frames of the module inputs (5: shorter than any conv's history)
CGMLP_MODULE = dict(d=64, U=256, K=15, seed=30)
TINY = {
    'tiny_ebranchformer': dict(frames=[291, 135, 131, 127, 15], fseed=400, reverse_weight=0.0),
    'tiny_branchformer': dict(frames=[291, 135, 131, 127, 15], fseed=410, reverse_weight=0.3),
}
CHUNK_CASES = ((4, -1), (4, 2))    # (decoding_chunk_size, num_decoding_left_chunks)
CTC_BEAM = 5
METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring')


def load_fixture(stem):
    """(meta, arrays) of tests/golden/branchformer/<stem>.npz and its continuation files
    <stem>_<i>.npz; arrays cut into row blocks (`<name>__part<i>`) are put together again."""
    import json
    import os

    import numpy as np
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'branchformer')
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
    assert meta is not None, f'{stem}.npz is missing (tools/gen_golden_branchformer.py)'
    arrays = {}
    for k in sorted(raw, key=lambda s: (s.split('__part')[0], int(s.split('__part')[1])
                                        if '__part' in s else 0)):
        base = k.split('__part')[0]
        arrays[base] = raw[k] if base not in arrays else np.concatenate([arrays[base], raw[k]])
    return meta, arrays


def cgmlp_module_inputs(causal, linear):
    """(x (40, d) fp64, state dict of ConvolutionalGatingMLP(d, U, K, 0, linear, 'identity',
    causal)) -- not the ESPnet initialisation: taps 1 / sqrt(K), norm bias 0.3."""
    m = CGMLP_MODULE
    d, U, K = m['d'], m['U'], m['K']
    C = U // 2
    g = torch.Generator().manual_seed(m['seed'] + 2 * int(causal) + int(linear))
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).double()
    sd = {'channel_proj1.0.weight': r(U, d, std=d ** -0.5), 'channel_proj1.0.bias': r(U, std=0.1),
          'csgu.norm.weight': 1.0 + r(C, std=0.1), 'csgu.norm.bias': r(C, std=0.3),
          'csgu.conv.weight': r(C, 1, K, std=K ** -0.5), 'csgu.conv.bias': r(C, std=0.2),
          'channel_proj2.weight': r(d, C, std=C ** -0.5), 'channel_proj2.bias': r(d, std=0.1)}
    if linear:
        sd['csgu.linear.weight'] = r(C, C, std=C ** -0.5)
        sd['csgu.linear.bias'] = r(C, std=0.2)
    x = r(MODULE_T[0], d) * 1.5 + 0.2
    return x, sd


def layer_module_inputs(name):
    """(x (40, d) fp64, configs, state dict) of layer 0 of the tiny model `name`: the layer
    fixtures run the reference's own layer class on it."""
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, 5)
    d = configs['encoder_conf']['output_size']
    g = torch.Generator().manual_seed(40 + len(name))
    x = (torch.randn(MODULE_T[0], d, generator=g) * 1.2).double()
    return x, configs, sd


def tiny_features(name):
    """The utterances of a model fixture, one (n, 80) fp32 matrix each: 291, 135, 131, 127 and 15
    frames give T' = 72, 33, 32, 31 and 3."""
    from wenet_amd import synthetic as S
    t = TINY[name]
    return [S.make_features(1, n, seed=t['fseed'] + i)[0][0] for i, n in enumerate(t['frames'])]
