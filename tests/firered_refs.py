"""Plain references of the FireRedASR-AED encoder kernels (csrc/firered.hip) -- the relative-
position attention WITH the relative shift and the 32-channel conv2d4 front end -- and the cases
the operator tests run them on (tests/test_firered_host.py on the CPU,
tests/test_gpu_firered_ops.py on the GPU).

Every `ref_*` is written from the reference's module text (wenet/models/firered/attention.py:
86-105, 134-165; firered/subsampling.py:57-75) in fp64; `fp32=True` evaluates the SAME plain
formula in fp32, the yardstick `e_plain` of the GPU tolerances (tests/kernel_refs.py bound /
cap_ok).

The module fixtures of tests/golden/firered/firered_modules.npz (tools/gen_golden_firered.py) are
recorded from the reference's own modules on the inputs `attn_module_inputs` /
`frontend_module_inputs` rebuild here from their seeds.

No GPU in here.
"""
import math

import torch
import torch.nn.functional as F

import kernel_refs as KR

# ---------------------------------------------------------------------------------------------
# rel-shift attention


def rel_positions(T, d_model, dtype=torch.float64):
    """The (2T - 1, d_model) sinusoid rows FireRedRelPositionalEncoding.forward hands a T-frame
    input (firered/attention.py:27-56): row c is the sinusoid of the relative position
    T - 1 - c.  Evaluated like the module: fp32 table, then cast."""
    rel = torch.arange(T - 1, -T, -1, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2).float() *
                    -(torch.log(torch.tensor(10000.0)).item() / d_model))
    pe = torch.zeros(2 * T - 1, d_model)
    pe[:, 0::2] = torch.sin(rel * div)
    pe[:, 1::2] = torch.cos(rel * div)
    return pe.to(dtype)


def ref_attention_relshift(q, k, v, P, p_center, bias_u, bias_v, seqs, scale=0.125, fp32=False,
                           want_weights=False, softmax32=False):
    """q / k / v (rows, H * 64); P (p_rows, H * 64) with the projected position row of DISTANCE
    r = i - j in row p_center - r; bias_u / bias_v (H, 64); seqs = [(off, len)].  Per (sequence,
    head), attention.py:134-165:
        matrix_ac = (q + u) k^T                       (T, T)
        matrix_bd = rel_shift((q + v) p^T)            p = the 2T - 1 rows of distances T-1 .. -(T-1)
        softmax((matrix_ac + matrix_bd) * scale) v
    rel_shift(raw)[i, j] = raw[i, T - 1 - i + j], written here as that index (the module's
    pad-and-view trick is checked against it in tests/test_firered_host.py).  Returns (rows,
    H * 64) fp64, zero in rows no sequence owns.
    softmax32: the softmax alone in fp32 on fp64 scores, as the module runs it whatever its own
    dtype (transformer/attention.py forward_attention: torch.softmax(scores.float())) -- only
    for the pin against the module's recorded .double() output; the fp64 reference of the GPU
    tests keeps the softmax in fp64."""
    dt = torch.float32 if fp32 else torch.float64
    H = q.shape[1] // 64
    out = torch.zeros(q.shape[0], H * 64, dtype=torch.float64)
    wmax = []
    for (off, T) in seqs:
        if T == 0:
            continue
        qs = q[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)        # (H, T, 64)
        ks = k[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)
        vs = v[off:off + T].to(dt).view(T, H, 64).transpose(0, 1)
        ps = P[p_center - (T - 1):p_center + T].to(dt).view(2 * T - 1, H, 64).transpose(0, 1)
        qu = qs + bias_u.to(dt).unsqueeze(1)
        qv = qs + bias_v.to(dt).unsqueeze(1)
        ac = torch.matmul(qu, ks.transpose(1, 2))
        raw = torch.matmul(qv, ps.transpose(1, 2))                        # (H, T, 2T - 1)
        i = torch.arange(T).unsqueeze(1)
        j = torch.arange(T).unsqueeze(0)
        idx = (T - 1 - i + j).unsqueeze(0).expand(H, T, T)
        bd = torch.gather(raw, 2, idx)
        if softmax32:
            attn = torch.softmax(((ac + bd) * scale).float(), dim=-1).to(dt)
        else:
            attn = torch.softmax((ac + bd) * scale, dim=-1)
        if want_weights:
            wmax.append(attn.max(dim=-1).values.reshape(-1).double())
        o = torch.matmul(attn, vs)
        out[off:off + T] = o.transpose(0, 1).reshape(T, H * 64).double()
    if want_weights:
        return out, torch.cat(wmax)
    return out


def module_rel_shift(x):
    """The pad-and-view form of FiredRelPositionMultiHeadedAttention.rel_shift, restated for a
    (H, T, 2T - 1) tensor: the CPU test pins ref_attention_relshift's index against it."""
    H, T, W = x.shape
    xp = torch.cat([torch.zeros(H, T, 1, dtype=x.dtype), x], dim=-1).view(H, W + 1, T)
    return xp[:, 1:].reshape(H, T, W)[:, :, :W // 2 + 1]


def make_relshift_case(H, lens, seed=0, gap=3, lead=5, t_table=None, regime='unit', param=None,
                       neg_only=False):
    """One packed self-attention batch.  P is a table for t_table >= max(lens) frames
    (2 t_table - 1 rows, distance 0 in row t_table - 1).  Rows of Q / K / V no sequence owns hold
    +-POISON.  regime 'peaked': (q, u, v) scaled so that the scores have the standard deviation
    `param`.  neg_only: the position rows are 40 times larger for distances r < 0 than for
    r >= 0, so a wrong sign of the distance or a band row off by one moves the scores by many
    standard deviations."""
    g = torch.Generator().manual_seed(seed)
    offs, rows = KR.pack_layout(lens, gap, lead)
    d = H * 64
    t_table = t_table or max(lens)
    q = torch.randn(rows, d, generator=g)
    k = torch.randn(rows, d, generator=g)
    v = torch.randn(rows, d, generator=g)
    P = torch.randn(2 * t_table - 1, d, generator=g)
    bu = torch.randn(H, 64, generator=g) * 0.5
    bv = torch.randn(H, 64, generator=g) * 0.5
    pc = t_table - 1
    if neg_only:
        # row pc - r: r < 0 are the rows behind the centre
        P[:pc + 1] *= 0.05
        P[pc + 1:] *= 2.0
    seqs = [(offs[s], lens[s]) for s in range(len(lens))]
    if regime == 'peaked':
        ref, _ = _scores(q, k, P, pc, bu, bv, seqs)
        c = float(param) / ref
        q *= c
        bu *= c
        bv *= c
    own = torch.zeros(rows, dtype=torch.bool)
    for (o, T) in seqs:
        own[o:o + T] = True
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0) * KR.POISON
    q[~own] = sign
    k[~own] = -sign
    v[~own] = sign
    return dict(q=q, k=k, v=v, P=P, p_center=pc, bias_u=bu, bias_v=bv, seqs=seqs, H=H,
                scale=0.125, rows=rows, own=own)


def _scores(q, k, P, pc, bu, bv, seqs, scale=0.125):
    """(standard deviation of all scores, list of score tensors)."""
    H = q.shape[1] // 64
    vals = []
    for (off, T) in seqs:
        if T == 0:
            continue
        qs = q[off:off + T].double().view(T, H, 64).transpose(0, 1)
        ks = k[off:off + T].double().view(T, H, 64).transpose(0, 1)
        for i in range(T):
            # position rows of query i: distance i - j for j = 0 .. T - 1 -> rows pc - i + j
            pi = P[pc - i:pc - i + T].double().view(T, H, 64).transpose(0, 1)
            s = (torch.einsum('hd,hjd->hj', qs[:, i] + bu.double(), ks) +
                 torch.einsum('hd,hjd->hj', qs[:, i] + bv.double(), pi)) * scale
            vals.append(s.reshape(-1))
    allv = torch.cat(vals)
    return (allv.std().item() if allv.numel() > 1 else 1.0), vals


def ref_attention_relshift_loops(case):
    """The same attention written query by query with explicit position rows (no shift index at
    all): an independent statement of "score (i, j) uses the row of distance i - j"."""
    q, k, v, P, pc = case['q'], case['k'], case['v'], case['P'], case['p_center']
    H = case['H']
    out = torch.zeros(q.shape[0], H * 64, dtype=torch.float64)
    for (off, T) in case['seqs']:
        if T == 0:
            continue
        qs = q[off:off + T].double().view(T, H, 64).transpose(0, 1)
        ks = k[off:off + T].double().view(T, H, 64).transpose(0, 1)
        vs = v[off:off + T].double().view(T, H, 64).transpose(0, 1)
        for i in range(T):
            pi = P[pc - i:pc - i + T].double().view(T, H, 64).transpose(0, 1)
            s = (torch.einsum('hd,hjd->hj', qs[:, i] + case['bias_u'].double(), ks) +
                 torch.einsum('hd,hjd->hj', qs[:, i] + case['bias_v'].double(), pi))
            w = torch.softmax(s * case['scale'], dim=-1)
            out[off + i] = torch.einsum('hj,hjd->hd', w, vs).reshape(-1)
    return out


def relshift_refs(case):
    """(fp64 reference, e_plain, scale, largest weight per (row, head)) of a case."""
    args = (case['q'], case['k'], case['v'], case['P'], case['p_center'], case['bias_u'],
            case['bias_v'], case['seqs'], case['scale'])
    ref, w = ref_attention_relshift(*args, want_weights=True)
    plain = ref_attention_relshift(*args, fp32=True)
    scale = max(case['v'][o:o + T].abs().max().item() for (o, T) in case['seqs'] if T > 0)
    return ref, (plain - ref).abs().max().item(), scale, w


# the cases of tests/test_gpu_firered_ops.py; test_firered_host.py asserts cap_ok for each here
RAGGED = [1, 31, 32, 33, 65, 100]
RELSHIFT_CASES = {
    # name: kwargs of make_relshift_case
    'ragged-h2': dict(H=2, lens=RAGGED, seed=1),
    'ragged-h20': dict(H=20, lens=RAGGED, seed=2),
    'ragged-h2-peaked': dict(H=2, lens=RAGGED, seed=3, regime='peaked', param=10.0),
    'ragged-h20-peaked': dict(H=20, lens=RAGGED, seed=4, regime='peaked', param=10.0),
    'one-h2': dict(H=2, lens=[1], seed=5, gap=0, lead=0),
    'one-h20': dict(H=20, lens=[1], seed=6),
    'sign-h2': dict(H=2, lens=[33, 97, 64], seed=7, neg_only=True),
    'sign-h20': dict(H=20, lens=[33, 97, 64], seed=8, neg_only=True),
    # a table sized for more frames than any sequence has (the encoder's cap on T')
    'table-h2': dict(H=2, lens=[70, 5], seed=9, t_table=300),
}


# ---------------------------------------------------------------------------------------------
# front end


def firered_out_len(n):
    """Frames FireRedConv2dSubsampling4 gives an utterance of n frames decoded ALONE: six zero
    frames behind it, two 3-wide stride-2 convolutions (subsampling.py:64-74)."""
    return ((n + 6 - 3) // 2 + 1 - 3) // 2 + 1 if n > 0 else 0


def ref_firered_frontend(feats, lens, mean, istd, w1, b1, w2, b2, fp32=False):
    """feats (B, T, F), lens [B]; w1 (C, 1, 3, 3), w2 (C, C, 3, 3) in torch's layout.  Per
    utterance, alone: CMVN, six zero frames appended, conv + ReLU twice, then
    x.transpose(1, 2).view(t, c * f) (subsampling.py:67-72).  Returns the list of (T', C * F2)
    fp64 matrices."""
    dt = torch.float32 if fp32 else torch.float64
    outs = []
    for b, n in enumerate(lens):
        n = int(n)
        if n == 0:
            outs.append(torch.zeros(0, 0, dtype=torch.float64))
            continue
        x = feats[b, :n].to(dt)
        if mean is not None:
            x = (x - mean.to(dt)) * istd.to(dt)
        x = F.pad(x, (0, 0, 0, 6))
        h = F.relu(F.conv2d(x.view(1, 1, n + 6, -1), w1.to(dt), b1.to(dt), stride=2))
        h = F.relu(F.conv2d(h, w2.to(dt), b2.to(dt), stride=2))
        _, c, t, f = h.shape
        outs.append(h.transpose(1, 2).reshape(t, c * f).double())
    return outs


def make_frontend_case(lens, F_in=80, C=32, seed=0, T=None, cmvn=True):
    g = torch.Generator().manual_seed(seed)
    T = T or max(lens)
    feats = torch.randn(len(lens), T, F_in, generator=g) * 3.0 + 1.0
    for b, n in enumerate(lens):
        feats[b, n:] = KR.POISON * (1.0 if b % 2 == 0 else -1.0)
    mean = torch.randn(F_in, generator=g) if cmvn else None
    istd = (torch.rand(F_in, generator=g) * 0.5 + 0.25) if cmvn else None
    w1 = torch.randn(C, 1, 3, 3, generator=g) / 3.0
    b1 = torch.randn(C, generator=g) * 0.1
    w2 = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9.0 * C)
    b2 = torch.randn(C, generator=g) * 0.1
    return dict(feats=feats, lens=list(lens), mean=mean, istd=istd, w1=w1, b1=b1, w2=w2, b2=b2,
                C=C, F=F_in, T=T)


def frontend_refs(c):
    """(list of fp64 references, e_plain, scale)."""
    args = (c['feats'], c['lens'], c['mean'], c['istd'], c['w1'], c['b1'], c['w2'], c['b2'])
    ref = ref_firered_frontend(*args)
    plain = ref_firered_frontend(*args, fp32=True)
    e = max((p - r).abs().max().item() for p, r in zip(plain, ref) if r.numel())
    scale = max(r.abs().max().item() for r in ref if r.numel())
    return ref, e, scale


FRONTEND_LENS = [7, 61, 97, 290, 1]


# ---------------------------------------------------------------------------------------------
# the inputs of the module fixtures (tools/gen_golden_firered.py records the reference's outputs)

ATTN_MODULE = dict(T=40, d=128, H=2, seed=20)
FRONT_MODULE = dict(lens=[97, 61], F=80, d=64, C=32, seed=21)
POS_ROWS = [0, 1, 2, 38, 39, 40, 41, 77, 78]     # rows of pos_emb the fixture keeps (T = 40)


def attn_module_inputs():
    """(x (T, d) fp64, state dict of FiredRelPositionMultiHeadedAttention(H, d, no q/k/v bias))."""
    T, d, H = ATTN_MODULE['T'], ATTN_MODULE['d'], ATTN_MODULE['H']
    g = torch.Generator().manual_seed(ATTN_MODULE['seed'])
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).double()
    sd = {}
    for n in ('q', 'k', 'v'):
        sd[f'layer_norm_{n}.weight'] = 1.0 + r(d, std=0.2)
        sd[f'layer_norm_{n}.bias'] = r(d, std=0.2)
        sd[f'linear_{n}.weight'] = r(d, d, std=d ** -0.5)
    sd['linear_pos.weight'] = r(d, d, std=d ** -0.5)
    sd['linear_out.weight'] = r(d, d, std=d ** -0.5)
    sd['pos_bias_u'] = r(H, d // H, std=0.5)
    sd['pos_bias_v'] = r(H, d // H, std=0.5)
    x = r(T, d) * 2.0 + 0.3
    return x, sd


def attention_module_formulation(x, sd, H, eps=1e-5, fold=False, softmax32=False, fp32=False):
    """FiredRelPositionMultiHeadedAttention.forward on one unpadded utterance x (T, d), restated
    on ref_attention_relshift.  fold: the three LayerNorms folded into the QKV weights (one
    plain normalisation, W' = W diag(g), b' = W b) -- the form the encoder path runs."""
    T, d = x.shape
    if fold:
        xn = F.layer_norm(x, (d, ), None, None, eps)
        q, k, v = (xn @ (sd[f'linear_{n}.weight'] * sd[f'layer_norm_{n}.weight']).t() +
                   sd[f'linear_{n}.weight'] @ sd[f'layer_norm_{n}.bias'] for n in 'qkv')
    else:
        q, k, v = (F.layer_norm(x, (d, ), sd[f'layer_norm_{n}.weight'],
                                sd[f'layer_norm_{n}.bias'], eps) @ sd[f'linear_{n}.weight'].t()
                   for n in 'qkv')
    P = rel_positions(T, d, x.dtype) @ sd['linear_pos.weight'].t()
    ctx = ref_attention_relshift(q, k, v, P, T - 1, sd['pos_bias_u'], sd['pos_bias_v'],
                                 [(0, T)], scale=1.0 / math.sqrt(d // H), softmax32=softmax32,
                                 fp32=fp32)
    # (linear_out carries a bias only with query_bias, transformer/attention.py:77: none here)
    return ctx.to(x.dtype) @ sd['linear_out.weight'].t(), (q, k, v)


def frontend_module_inputs():
    """(make_frontend_case without CMVN, Linear(C * F2 -> d) weight, bias) of
    FireRedConv2dSubsampling4(F, d, odim=C)."""
    m = FRONT_MODULE
    c = make_frontend_case(m['lens'], m['F'], m['C'], seed=m['seed'], cmvn=False)
    c['feats'] = torch.where(c['feats'].abs() > 1e17, torch.zeros(()), c['feats'])
    g = torch.Generator().manual_seed(m['seed'] + 1)
    F2 = ((m['F'] - 1) // 2 - 1) // 2
    w = torch.randn(m['d'], m['C'] * F2, generator=g) / math.sqrt(m['C'] * F2)
    b = torch.randn(m['d'], generator=g) * 0.1
    return c, w, b


# ---------------------------------------------------------------------------------------------
# the whole encoder, restated (tests/golden/firered/firered_tiny.npz pins it to the reference)

TINY = dict(config='tiny_firered', frames=[290, 131, 127, 121], fseed=300)
RECORDED_ENC = (131, 121)      # utterances whose fp64 encoder output the fixture carries
RECORDED_ENC_3TILE = 290       # ... and the one firered_tiny_enc3.npz carries


def tiny_features():
    """The utterances of the model fixture, one (n, 80) fp32 matrix each: 290, 131, 127 and 121
    frames give T' = 73 (three key tiles), 33, 32 and 31 (one tile)."""
    from wenet_amd import synthetic as S
    return [S.make_features(1, n, seed=TINY['fseed'] + i)[0][0]
            for i, n in enumerate(TINY['frames'])]


def firered_encoder_formulation(feats, sd, configs, softmax32=True, dtype=torch.float64):
    """FireRedConformerEncoder.forward on ONE utterance `feats` (n, F), in fp64 torch, in the form
    the library runs: CMVN, six zero frames, the two convolutions, the output projection (no
    xscale; the positional encoding returns x unchanged), then per layer the macaron FFN, the
    attention with layer_norm_q / k / v FOLDED into the QKV weights, the conv module at inner
    factor 4 (GLU, depthwise conv with zero padding, LayerNorm over 2 d, swish), the FFN and
    norm_final; no after_norm.  softmax32: the attention softmax in fp32, as the reference's
    forward_attention runs it even in a .double() model -- the form the recorded output has."""
    ec = configs['encoder_conf']
    d, H, K = ec['output_size'], ec['attention_heads'], ec['cnn_module_kernel']
    eps = ec.get('norm_eps', 1e-5)
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    fp32 = dtype == torch.float32
    x = ref_firered_frontend(feats.unsqueeze(0), [feats.shape[0]],
                             w.get('encoder.global_cmvn.mean'), w.get('encoder.global_cmvn.istd'),
                             w['encoder.embed.conv.0.weight'], w['encoder.embed.conv.0.bias'],
                             w['encoder.embed.conv.2.weight'], w['encoder.embed.conv.2.bias'],
                             fp32=fp32)[0].to(dtype)
    x = x @ w['encoder.embed.out.0.weight'].t() + w['encoder.embed.out.0.bias']
    ln = lambda t, p, n=d: F.layer_norm(t, (n, ), w[p + '.weight'], w[p + '.bias'], eps)

    def ffn(t, p):
        h = F.silu(t @ w[p + '.w_1.weight'].t() + w[p + '.w_1.bias'])
        return h @ w[p + '.w_2.weight'].t() + w[p + '.w_2.bias']

    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        x = x + 0.5 * ffn(ln(x, p + '.norm_ff_macaron'), p + '.feed_forward_macaron')
        asd = {k[len(p) + 11:]: v for k, v in w.items() if k.startswith(p + '.self_attn.')}
        att, _ = attention_module_formulation(x, asd, H, fold=True, softmax32=softmax32,
                                              fp32=fp32)
        x = x + att
        y = ln(x, p + '.norm_conv')
        y = y @ w[p + '.conv_module.pointwise_conv1.weight'][:, :, 0].t()
        y = y[:, :2 * d] * torch.sigmoid(y[:, 2 * d:])                       # GLU over channels
        y = F.conv1d(y.t().unsqueeze(0), w[p + '.conv_module.depthwise_conv.weight'],
                     padding=(K - 1) // 2, groups=2 * d)[0].t()
        y = F.silu(ln(y, p + '.conv_module.norm', 2 * d))
        x = x + y @ w[p + '.conv_module.pointwise_conv2.weight'][:, :, 0].t()
        x = x + 0.5 * ffn(ln(x, p + '.norm_ff'), p + '.feed_forward')
        x = ln(x, p + '.norm_final')
    return x
