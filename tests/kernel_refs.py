"""Plain references of the four kernel families that are not GEMMs -- attention, depthwise conv +
norm + SiLU, CMVN + conv1 + ReLU, CTC log-softmax + top-k -- and the input regimes the operator
tests run them on (tests/test_kernel_refs.py on the CPU, tests/test_gpu_kernels.py on the GPU).

Every `ref_*` is written from the reference's module text (the citations of
oracle/wenet_oracle.py), at the level of loops, einsum-like matmuls and torch.nn.functional
convolutions, in fp64.  `fp32=True` evaluates the SAME plain formula in fp32 (`bf16=True`, attention
only: Q (+ bias), K, V, P and the probabilities rounded to bf16, fp32 accumulation): the distance
of that evaluation from the fp64 one is the yardstick `e_plain` of the GPU tolerances.

Further down: the kernels of the `attention` decode mode (csrc/attn_search.hip; CPU checks in
tests/test_kernel_refs.py, GPU tests in tests/test_gpu_attn_search.py) -- the self-attention step
as ref_attention on the rows gathered through the paths, the beam state kernels restated in NumPy.

Behind conv1: the rest of the Conformer front end (conv2, the output projection) and the Whisper
front end, for tests/test_gpu_frontend.py; their whole-chain references call the oracle's own
functions (imported inside those functions only).

At the end: the kernels that own a complete row -- LayerNorm, the FFN slice reduce, the row-LN GEMM
-- as written-out formulas, a decoder of the plane image (csrc/x6.h) and the row regimes, for
tests/test_gpu_rows.py.

Last: the fp32 and bf16-on-the-fly matrix-core GEMMs with every argument of GemmArgs -- strides,
epilogues, GLU, gathered rows, the implicit 3x3 / stride-2 operand -- as `ref_gemm`, and the list
of cases GEMM_CASES that tests/test_gpu_gemm_ops.py runs and tests/test_kernel_refs.py checks.

After them: the stored-operand GEMMs (csrc/gemm_bf16s.hip, gemm_bf16p.hip) and the MXFP8 quantiser
-- `mx_encode` / `mx_decode` from the OCP MX rule, `ref_gemm_lowp` on the decoded operands and the
cases GEMM_LOWP_CASES of tests/test_gpu_gemm_lowp_ops.py.

No GPU in here.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

ULP32 = 2.0 ** -23


def _r16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_representable(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------
# attention


def chunk_window(n_q, n_kv, mask_mode, chunk, left):
    """Visible keys as a (n_q, n_kv) bool matrix: mode 0 every key, mode 1 subsequent_mask
    (mask.py:51-85: key j <= query i), mode 2 subsequent_chunk_mask (mask.py:88-123: keys from
    `left` chunks back -- `left` < 0: from the start -- to the end of the query's own chunk)."""
    vis = torch.zeros(n_q, n_kv, dtype=torch.bool)
    for i in range(n_q):
        if mask_mode == 0:
            lo, hi = 0, n_kv
        elif mask_mode == 1:
            lo, hi = 0, min(i + 1, n_kv)
        else:
            lo = 0 if left < 0 else max((i // chunk - left) * chunk, 0)
            hi = min((i // chunk + 1) * chunk, n_kv)
        vis[i, lo:hi] = True
    return vis


def ref_attention(q, k, v, pos, bias_u, bias_v, seqs, mask_mode=0, chunk=0, left=-1,
                  scale=0.125, fp32=False, bf16=False, want_weights=False):
    """q (q_rows, H * 64), k / v (kv_rows, H * 64), pos (p_rows, H * 64) or None, bias_u / bias_v
    (H, 64); seqs = [(q_off, q_len, kv_off, kv_len, p_off)].  Per (sequence, head):
    softmax(mask(((q + u) k^T + (q + v) p^T) * scale)) v  (attention.py:133-178, 410-428; no
    rel_shift: key j uses position row p_off + j).  Returns (q_rows, H * 64) fp64, zero in rows no
    sequence owns; with want_weights also the largest weight of every owned (row, head)."""
    dt = torch.float32 if (fp32 or bf16) else torch.float64
    rnd = _r16 if bf16 else (lambda t: t)
    H = q.shape[1] // 64
    out = torch.zeros(q.shape[0], H * 64, dtype=torch.float64)
    wmax = []
    for (qo, ql, ko, kl, po) in seqs:
        if ql == 0:
            continue
        qs = q[qo:qo + ql].to(dt).view(ql, H, 64).transpose(0, 1)       # (H, ql, 64)
        ks = rnd(k[ko:ko + kl].to(dt)).view(kl, H, 64).transpose(0, 1)
        vs = rnd(v[ko:ko + kl].to(dt)).view(kl, H, 64).transpose(0, 1)
        if pos is not None:
            ps = rnd(pos[po:po + kl].to(dt)).view(kl, H, 64).transpose(0, 1)
            qu = rnd(qs + bias_u.to(dt).unsqueeze(1))
            qv = rnd(qs + bias_v.to(dt).unsqueeze(1))
            scores = (torch.matmul(qu, ks.transpose(1, 2)) +
                      torch.matmul(qv, ps.transpose(1, 2))) * scale
        else:
            scores = torch.matmul(rnd(qs), ks.transpose(1, 2)) * scale
        hidden = ~chunk_window(ql, kl, mask_mode, chunk, left)
        scores = scores.masked_fill(hidden, -float('inf'))
        attn = torch.softmax(scores, dim=-1).masked_fill(hidden, 0.0)
        if want_weights:
            wmax.append(attn.max(dim=-1).values.reshape(-1).double())
        o = torch.matmul(rnd(attn), vs)                                  # (H, ql, 64)
        out[qo:qo + ql] = o.transpose(0, 1).reshape(ql, H * 64).double()
    if want_weights:
        return out, torch.cat(wmax)
    return out


def visible_v_scale(v, seqs):
    """max |v| over the keys of the sequences: the scale of an attention output (a convex
    combination of them)."""
    m = 0.0
    for (_, ql, ko, kl, _) in seqs:
        if ql > 0:
            m = max(m, v[ko:ko + kl].abs().max().item())
    return m


POISON = 1e18


def pack_layout(lens, gap, lead):
    """Offsets of a packed ragged batch: `lead` unowned rows in front, `gap` unowned rows behind
    every sequence.  Returns (offsets, total rows)."""
    offs, at = [], lead
    for n in lens:
        offs.append(at)
        at += n + gap
    return offs, max(at, 1)


def make_attention_case(regime, H, q_lens, kv_lens=None, relpos=False, mask_mode=0, chunk=0,
                        left=-1, seed=0, gap=3, lead=5, bf16=False, needle='first', param=None):
    """Inputs of one attention case.  kv_lens None: self attention (one layout for Q and K / V).
    Rows of K / V / Q no sequence owns hold +-POISON.  Regimes: see test_gpu_kernels.py."""
    g = torch.Generator().manual_seed(seed)
    self_attn = kv_lens is None
    q_off, q_rows = pack_layout(q_lens, gap, lead)
    if self_attn:
        kv_lens, kv_off, kv_rows = list(q_lens), list(q_off), q_rows
    else:
        kv_off, kv_rows = pack_layout(kv_lens, gap + 1, lead + 2)
    d = H * 64
    scale = 0.125
    q = torch.randn(q_rows, d, generator=g)
    k = torch.randn(kv_rows, d, generator=g)
    v = torch.randn(kv_rows, d, generator=g)
    p_rows = max(kv_lens) + 7
    p_off = [(3 * s) % 7 for s in range(len(q_lens))] if relpos else [0] * len(q_lens)
    pos = torch.randn(p_rows, d, generator=g) if relpos else None
    bu = torch.randn(H, 64, generator=g) * 0.5 if relpos else None
    bv = torch.randn(H, 64, generator=g) * 0.5 if relpos else None
    steer = regime in ('ascending', 'descending', 'shifted', 'needle')
    if steer:
        # coordinate 0 of every head steers the scores: keep the rel-pos term out of it
        q.view(q_rows, H, 64)[:, :, 0] = 0
        k.view(kv_rows, H, 64)[:, :, 0] = 0
        if relpos:
            pos.view(p_rows, H, 64)[:, :, 0] = 0
            bu[:, 0] = 0
            bv[:, 0] = 0
    seqs = [(q_off[s], q_lens[s], kv_off[s], kv_lens[s], p_off[s]) for s in range(len(q_lens))]
    q3, k3 = q.view(q_rows, H, 64), k.view(kv_rows, H, 64)
    if regime == 'unit':
        pass
    elif regime == 'peaked':
        # scale (q, u, v) together: the scores are linear in them
        sd0 = _score_std(q, k, pos, bu, bv, seqs, scale)
        c = float(param) / sd0
        q *= c
        if relpos:
            bu *= c
            bv *= c
    elif regime in ('ascending', 'descending'):
        step = float(param) * (1.0 if regime == 'ascending' else -1.0)
        q3[:, :, 0] = 1.0 / scale
        for (_, _, ko, kl, _) in seqs:
            k3[ko:ko + kl, :, 0] = (torch.arange(kl, dtype=torch.float32) * step).unsqueeze(1)
    elif regime == 'needle':
        q3[:, :, 0] = 1.0 / scale
        for (_, _, ko, kl, _) in seqs:
            if kl == 0:
                continue
            if needle == 'last_visible':
                # 40 more per key: under every mask the last visible key leads by 40
                k3[ko:ko + kl, :, 0] = (torch.arange(kl, dtype=torch.float32) * 40.0).unsqueeze(1)
                continue
            tiles = (kl + 31) // 32
            j = {'first': 0, '31': 31, '32': 32, '63': 63, '64': 64, 'last': kl - 1,
                 'second_half': ((tiles + 1) // 2) * 32}[needle]
            j = min(j, kl - 1)
            # the other 63 coordinates give scores of a standard deviation near 1 (1.6 with the
            # rel-pos term), at most ~8 over 1500 keys: 60 clears them by more than 40
            k3[ko + j, :, 0] = 60.0
    elif regime == 'shifted':
        q3[:, :, 0] = float(param) / scale
        k3[:, :, 0] = 1.0
        v += 100.0
    elif regime == 'tied':
        q.zero_()
        if relpos:
            bu.zero_()
            bv.zero_()
    else:
        raise ValueError(regime)
    # unowned rows: large finite poison (the reference never reads them)
    own_q = torch.zeros(q_rows, dtype=torch.bool)
    own_k = torch.zeros(kv_rows, dtype=torch.bool)
    for (qo, ql, ko, kl, _) in seqs:
        own_q[qo:qo + ql] = True
        own_k[ko:ko + kl] = True
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0) * POISON
    q[~own_q] = sign
    k[~own_k] = -sign
    v[~own_k] = sign
    if bf16:
        if relpos:
            # The bf16 kernel rounds q + bias_u / q + bias_v: with free q and biases that rounding
            # alone moves a score of standard deviation 10 by 0.04 and the plain bf16 evaluation
            # breaks its cap (1.4e-2 of the scale at `peaked` 10).  So q and the biases go on a
            # common grid of 256 steps per binade of their largest sum: q + u is then exact in
            # bf16 and the rounding that is left is the one of the probabilities.  (The steering
            # coordinate has zero biases and keeps its value.)
            sl = slice(1, None) if steer else slice(None)
            qq = q.view(q_rows, H, 64)
            top = qq[own_q][:, :, sl].abs().max().item() + \
                max(bu[:, sl].abs().max().item(), bv[:, sl].abs().max().item())
            if top > 0:
                grid = 2.0 ** math.ceil(math.log2(top)) / 256
                qq[:, :, sl] = torch.round(qq[:, :, sl] / grid) * grid
                bu[:, sl] = torch.round(bu[:, sl] / grid) * grid
                bv[:, sl] = torch.round(bv[:, sl] / grid) * grid
        q, k, v = bf16_representable(q), bf16_representable(k), bf16_representable(v)
        if relpos:
            pos, bu, bv = bf16_representable(pos), bf16_representable(bu), bf16_representable(bv)
    return dict(q=q, k=k, v=v, pos=pos, bias_u=bu, bias_v=bv, seqs=seqs, H=H, scale=scale,
                mask_mode=mask_mode, chunk=chunk, left=left, self_attn=self_attn,
                q_rows=q_rows, kv_rows=kv_rows, own_q=own_q)


def _score_std(q, k, pos, bu, bv, seqs, scale):
    H = q.shape[1] // 64
    vals = []
    for (qo, ql, ko, kl, po) in seqs:
        if ql == 0:
            continue
        qs = q[qo:qo + ql].double().view(ql, H, 64).transpose(0, 1)
        ks = k[ko:ko + kl].double().view(kl, H, 64).transpose(0, 1)
        if pos is not None:
            ps = pos[po:po + kl].double().view(kl, H, 64).transpose(0, 1)
            s = torch.matmul(qs + bu.double().unsqueeze(1), ks.transpose(1, 2)) + \
                torch.matmul(qs + bv.double().unsqueeze(1), ps.transpose(1, 2))
        else:
            s = torch.matmul(qs, ks.transpose(1, 2))
        vals.append((s * scale).reshape(-1))
    return torch.cat(vals).std().item()


def attention_refs(case, bf16=False):
    """(fp64 reference, e_plain, scale, largest weight per (row, head)) of a case."""
    args = (case['q'], case['k'], case['v'], case['pos'], case['bias_u'], case['bias_v'],
            case['seqs'], case['mask_mode'], case['chunk'], case['left'], case['scale'])
    ref, w = ref_attention(*args, want_weights=True)
    plain = ref_attention(*args, fp32=not bf16, bf16=bf16)
    return ref, (plain - ref).abs().max().item(), visible_v_scale(case['v'], case['seqs']), w


# ---------------------------------------------------------------------------------------------
# depthwise conv + LayerNorm / affine + SiLU


def ref_dwconv(x, wt, bias, cpad, ln_w, ln_b, norm_mode, off, lens, K, causal, t_max, eps,
               fp32=False):
    """x (M, D) packed rows, wt (K, D) tap-major.  Per utterance the (t_max, D) tensor whose rows
    >= len are `cpad` (masked_fill before pointwise_conv1, convolution.py:115-117, seen behind
    it), causal: K - 1 rows of `cpad` in front (:122-124), symmetric: (K - 1) / 2 zero rows on
    both sides (Conv1d padding); depthwise conv, LayerNorm over channels (mode 0) or the
    per-channel affine of eval-mode BatchNorm1d (mode 1), SiLU (:132-146).  Returns (M, D) fp64,
    zero in rows no utterance owns."""
    dt = torch.float32 if fp32 else torch.float64
    M, D = x.shape
    out = torch.zeros(M, D, dtype=torch.float64)
    w = wt.to(dt).t().contiguous().unsqueeze(1)            # (D, 1, K)
    for o, n in zip(off, lens):
        if n == 0:
            continue
        X = cpad.to(dt).unsqueeze(0).repeat(t_max, 1)
        X[:n] = x[o:o + n].to(dt)
        if causal:
            X = torch.cat([cpad.to(dt).unsqueeze(0).repeat(K - 1, 1), X], 0)
        else:
            z = torch.zeros((K - 1) // 2, D, dtype=dt)
            X = torch.cat([z, X, z], 0)
        y = F.conv1d(X.t().unsqueeze(0), w, bias.to(dt), groups=D)[0].t()   # (t_max, D)
        if norm_mode == 0:
            y = F.layer_norm(y, (D, ), ln_w.to(dt), ln_b.to(dt), eps)
        else:
            y = y * ln_w.to(dt) + ln_b.to(dt)
        y = y * torch.sigmoid(y)
        out[o:o + n] = y[:n].double()
    return out


def make_dwconv_case(D, K, causal, norm_mode, lens, seed=0, gap=1, lead=0, t_extra=0, pad_ld=0,
                     offset=0.0, tail=3):
    g = torch.Generator().manual_seed(seed)
    off, M = pack_layout(lens, gap, lead)
    M += tail
    x = torch.randn(M, D, generator=g)
    if offset:
        x += offset * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).unsqueeze(1)
    own = torch.zeros(M, dtype=torch.bool)
    for o, n in zip(off, lens):
        own[o:o + n] = True
    x[~own] = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0) * POISON
    wt = torch.randn(K, D, generator=g) / math.sqrt(K)
    return dict(x=x, wt=wt, bias=torch.randn(D, generator=g) * 0.3,
                cpad=torch.randn(D, generator=g),
                ln_w=1.0 + 0.2 * torch.randn(D, generator=g), ln_b=0.2 * torch.randn(D, generator=g),
                norm_mode=norm_mode, off=off, lens=list(lens), K=K, causal=causal,
                t_max=max(lens) + t_extra, eps=1e-5, M=M, D=D, own=own, pad_ld=pad_ld)


def dwconv_refs(c):
    args = (c['x'], c['wt'], c['bias'], c['cpad'], c['ln_w'], c['ln_b'], c['norm_mode'], c['off'],
            c['lens'], c['K'], c['causal'], c['t_max'], c['eps'])
    ref = ref_dwconv(*args)
    plain = ref_dwconv(*args, fp32=True)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# CMVN + Conv2d(1, C, 3, stride 2) + ReLU


def ref_conv1(feats, mean, istd, w, bias, t1_lens, fp32=False):
    """feats (B, T, F), w (C, 1, 3, 3).  (x - mean) * istd (cmvn.py:36-47), Conv2d stride 2 +
    ReLU (subsampling.py:188-190), channels last; utterance b keeps its first t1_lens[b] frames.
    Returns a list of (t1_len, F1, C) fp64 tensors."""
    dt = torch.float32 if fp32 else torch.float64
    outs = []
    for b, n in enumerate(t1_lens):
        x = feats[b].to(dt)
        if mean is not None:
            x = (x - mean.to(dt)) * istd.to(dt)
        y = F.relu(F.conv2d(x.unsqueeze(0).unsqueeze(0), w.to(dt), bias.to(dt), stride=2))[0]
        outs.append(y.permute(1, 2, 0)[:n].double())
    return outs


def make_conv1_case(Fdim, C, t1_lens, cmvn=True, seed=0, gap=1, lead=2):
    g = torch.Generator().manual_seed(seed)
    B = len(t1_lens)
    T = 2 * max(max(t1_lens), 1) + 1 + 2
    feats = torch.randn(B, T, Fdim, generator=g) * 3.0 + (11.0 if cmvn else 0.0)
    # frames behind an utterance's last window: finite poison
    for b, n in enumerate(t1_lens):
        feats[b, 2 * n + 1:] = POISON
    mean = istd = None
    if cmvn:
        mean = 11.0 + torch.randn(Fdim, generator=g)
        istd = 0.3 + 0.05 * torch.rand(Fdim, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
    bias = torch.randn(C, generator=g) * 0.2
    off, rows = pack_layout(t1_lens, gap, lead)
    return dict(feats=feats, mean=mean, istd=istd, w=w, bias=bias, t1_lens=list(t1_lens), off=off,
                rows=rows, F=Fdim, F1=(Fdim - 1) // 2, C=C, T=T, B=B)


def conv1_refs(c):
    args = (c['feats'], c['mean'], c['istd'], c['w'], c['bias'], c['t1_lens'])
    ref = ref_conv1(*args)
    plain = ref_conv1(*args, fp32=True)
    e = max([(p - r).abs().max().item() for p, r in zip(plain, ref) if r.numel()] + [0.0])
    s = max([r.abs().max().item() for r in ref if r.numel()] + [0.0])
    return ref, e, s


# ---------------------------------------------------------------------------------------------
# the rest of Conv2dSubsampling4: conv2 + ReLU, Linear(d * F2 -> d) * sqrt(d)


def ref_conv2(c1_b, w, bias, fp32=False):
    """c1_b (t1_len, F1, C): ONE utterance's conv1 activations, channels last; w (C, C, 3, 3), the
    reference's weight.  relu(Conv2d(C, C, 3, stride 2)) (subsampling.py:191-192) -> (t2_len, F2,
    C) fp64, t2_len = (t1_len - 3) // 2 + 1."""
    dt = torch.float32 if fp32 else torch.float64
    x = c1_b.to(dt).permute(2, 0, 1).unsqueeze(0)                      # (1, C, t1, F1)
    y = F.relu(F.conv2d(x, w.to(dt), bias.to(dt), stride=2))[0]        # (C, t2, F2)
    return y.permute(1, 2, 0).double()


def ref_sub_out(c2_b, w_out, b_out, d, fp32=False):
    """c2_b (t2_len, F2, C) -> sqrt(d) * Linear(C * F2 -> d) over the reference's column order
    c * F2 + f (x.transpose(1, 2).view(b, t, c * f), subsampling.py:225-226; xscale,
    embedding.py:144).  Returns (t2_len, d) fp64."""
    dt = torch.float32 if fp32 else torch.float64
    t2, F2, C = c2_b.shape
    x = c2_b.to(dt).permute(0, 2, 1).reshape(t2, C * F2)
    return (F.linear(x, w_out.to(dt), b_out.to(dt)) * math.sqrt(d)).double()


def sub4_lens(lens):
    """Output frames of Conv2dSubsampling4 for utterances of `lens` feature frames: the mask
    [:, :, 2::2][:, :, 2::2] (subsampling.py:228) keeps the frames 6 + 4 k < L."""
    return [(int(n) - 7) // 4 + 1 if int(n) > 6 else 0 for n in lens]


def ref_frontend_chain(feats, lens, sd, d, fp32=False):
    """GlobalCMVN + Conv2dSubsampling4 + xscale through the oracle's own functions, one utterance
    at a time on its first 4 l2 + 3 frames (everything its l2 kept output frames read).  Returns
    a list of (l2, d) fp64 tensors."""
    from oracle import wenet_oracle as O
    dt = torch.float32 if fp32 else torch.float64
    pfx = 'encoder.embed.'
    sdd = {k: v.to(dt) for k, v in sd.items()
           if k.startswith(pfx + 'conv.') or k.startswith(pfx + 'out.')}
    sdd[pfx + 'pos_enc.pe'] = torch.zeros(1, 1, d, dtype=dt)     # (the table is not used here)
    mean, istd = sd.get('encoder.global_cmvn.mean'), sd.get('encoder.global_cmvn.istd')
    outs = []
    for b, l2 in enumerate(sub4_lens(lens)):
        if l2 == 0:
            outs.append(torch.zeros(0, d, dtype=torch.float64))
            continue
        n = 4 * l2 + 3
        x = feats[b, :n].to(dt).unsqueeze(0)
        if mean is not None:
            x = O.global_cmvn(x, mean.to(dt), istd.to(dt))
        y, _, m = O.conv2d_subsampling4(x, torch.ones(1, 1, n, dtype=torch.bool), sdd, pfx, d)
        assert y.shape[1] == l2 and int(m.sum()) == l2
        outs.append(y[0].double())
    return outs


def _err_scale(plain, ref):
    e = max([(p - r).abs().max().item() for p, r in zip(plain, ref) if r.numel()] + [0.0])
    s = max([r.abs().max().item() for r in ref if r.numel()] + [0.0])
    return e, s


def frontend_refs(feats, lens, sd, d, c1, c2, utts=None):
    """The three comparisons of the front-end tests.  c1 / c2: the GPU's own conv1 / conv2
    activations as lists per utterance ((2 l2 + 1, F1, d) and (l2, F2, d) fp32); utts: the
    utterances to evaluate (None: all).  Returns {'c2': ..., 'x_proj': ..., 'x_chain': ...}, each
    (list of fp64 references per evaluated utterance, e_plain, scale):
      c2       ref_conv2 of the GPU's c1                   -- conv2 alone
      x_proj   ref_sub_out of the GPU's c2                 -- the projection alone
      x_chain  ref_frontend_chain of the features          -- everything from the features on
    e_plain: the fp32 CPU evaluation of the same step on the same inputs against the fp64 one."""
    pfx = 'encoder.embed.'
    w2, b2 = sd[pfx + 'conv.2.weight'], sd[pfx + 'conv.2.bias']
    wo, bo = sd[pfx + 'out.0.weight'], sd[pfx + 'out.0.bias']
    l2 = sub4_lens(lens)
    utts = [b for b in (range(len(l2)) if utts is None else utts) if l2[b] > 0]
    out = {}
    ref = [ref_conv2(c1[b], w2, b2) for b in utts]
    plain = [ref_conv2(c1[b], w2, b2, fp32=True) for b in utts]
    out['c2'] = (ref, ) + _err_scale(plain, ref)
    ref = [ref_sub_out(c2[b], wo, bo, d) for b in utts]
    plain = [ref_sub_out(c2[b], wo, bo, d, fp32=True) for b in utts]
    out['x_proj'] = (ref, ) + _err_scale(plain, ref)
    sub_f = torch.stack([feats[b] for b in utts]) if utts else feats[:0]
    sub_l = [lens[b] for b in utts]
    ref = ref_frontend_chain(sub_f, sub_l, sd, d)
    plain = ref_frontend_chain(sub_f, sub_l, sd, d, fp32=True)
    out['x_chain'] = (ref, ) + _err_scale(plain, ref)
    return out, utts


def frontend_model_parts(F_in, d, whisper=False, seed=0):
    """(configs, state dict) of a one-block model with `F_in` feature bins and width `d`: a copy
    of the synthetic configuration tiny_lite (whisper: whisper_tiny_like), d / 64 heads."""
    from wenet_amd import synthetic as S
    configs = S.make_configs('whisper_tiny_like' if whisper else 'tiny_lite')
    configs['input_dim'] = F_in
    ec = configs['encoder_conf']
    ec['output_size'], ec['attention_heads'], ec['num_blocks'] = d, d // 64, 1
    if configs.get('decoder_conf'):
        configs['decoder_conf']['attention_heads'] = d // 64
    return configs, S.make_state_dict(configs, seed)


def make_frontend_feats(lens, F_in, seed=0, T=None, poison=True):
    """(B, T, F_in) fbank-like features (mean 11, std 3) for utterances of `lens` frames, T =
    max(lens) unless given.  poison: the frames at and beyond 4 l2 + 3 of every utterance -- what
    none of its l2 kept output frames reads -- hold POISON; else the frames beyond the length are
    zeros, as the reference's padding() leaves them."""
    g = torch.Generator().manual_seed(seed)
    T = max(lens) if T is None else T
    feats = torch.randn(len(lens), T, F_in, generator=g) * 3.0 + 11.0
    for b, (n, l2) in enumerate(zip(lens, sub4_lens(lens))):
        if poison:
            feats[b, (4 * l2 + 3 if l2 else 0):] = POISON
        else:
            feats[b, n:] = 0.0
    return feats


# ---------------------------------------------------------------------------------------------
# Conv1dSubsampling2 + WhisperPositionalEncoding (the Whisper front end)


def sub2_lens(lens, T):
    """Output frames of Conv1dSubsampling2 on a (B, T, F) batch: the mask [:, :, (T + 1) % 2::2]
    (subsampling.py:171) keeps t' with 2 t' + (T + 1) % 2 < L."""
    par = (T + 1) % 2
    return [(int(n) - par + 1) // 2 if int(n) > par else 0 for n in lens]


def ref_whisper_frontend(feats, lens, sd, fp32=False):
    """The oracle's conv1d_subsampling2 on the whole zero-padded batch (the reference reads the
    padding frames: they stay zeros, processor.py:526-577), cut to the frames its mask keeps.
    Returns a list of (l2, d) fp64 tensors."""
    from oracle import wenet_oracle as O
    dt = torch.float32 if fp32 else torch.float64
    pfx = 'encoder.embed.'
    sdd = {k: v.to(dt) for k, v in sd.items() if k.startswith(pfx)}
    T = feats.shape[1]
    mask = ~O.make_pad_mask(torch.as_tensor(lens), T).unsqueeze(1)
    y, _, m = O.conv1d_subsampling2(feats.to(dt), mask, sdd, pfx)
    keep = m.squeeze(1).sum(1).tolist()
    assert keep == sub2_lens(lens, T), (keep, sub2_lens(lens, T))
    return [y[b, :n].double() for b, n in enumerate(keep)]


def whisper_frontend_refs(feats, lens, sd):
    ref = ref_whisper_frontend(feats, lens, sd)
    plain = ref_whisper_frontend(feats, lens, sd, fp32=True)
    return (ref, ) + _err_scale(plain, ref)


# ---------------------------------------------------------------------------------------------
# CTC rows


def ref_ctc_rows(logits, blank, penalty, k, fp32=False):
    """logits (M, V): blank penalty (asr_model.py:258-259), log_softmax (ctc.py:73-81), topk
    (search.py:158).  Returns (logp, topk_val, topk_idx)."""
    dt = torch.float32 if fp32 else torch.float64
    x = logits.to(dt).clone()
    x[:, blank] -= penalty
    logp = x.log_softmax(dim=1)
    val, idx = logp.topk(k, dim=1)
    return logp.double(), val.double(), idx


def make_ctc_case(regime, M, V, blank=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, V, generator=g) * 3.0
    x[:, blank] += 4.0                                   # the blank boost of a CTC head
    if regime == 'randn':
        pass
    elif regime == 'shift_up':
        x = (x.double() + 1e4).float()                   # shifted before the fp32 rounding
    elif regime == 'shift_down':
        x = (x.double() - 1e4).float()
    elif regime == 'spread':
        x = torch.rand(M, V, generator=g) * 300.0
    elif regime == 'ties':
        # few distinct values: exact ties among the leaders of every row
        x = torch.randint(0, 3, (M, V), generator=g).float() * 2.0
    else:
        raise ValueError(regime)
    return x


def ctc_refs(x, blank, penalty, k):
    logp, val, idx = ref_ctc_rows(x, blank, penalty, k)
    logp32, _, _ = ref_ctc_rows(x, blank, penalty, k, fp32=True)
    return logp, val, idx, (logp32 - logp).abs().max().item(), logp.abs().max().item()


# (regime, param) of every attention data regime; the operator tests run each of them
ATTENTION_REGIMES = [('unit', None), ('peaked', 10.0), ('peaked', 30.0), ('ascending', 1.0),
                     ('ascending', 0.375), ('descending', 1.0), ('descending', 0.375),
                     ('needle', 'first'), ('needle', '31'), ('needle', '32'), ('needle', 'last'),
                     ('needle', 'second_half'), ('needle', 'last_visible'), ('shifted', 80.0),
                     ('shifted', -80.0), ('tied', None)]
# regimes whose reference weights must be peaked: (smallest share of (row, head) pairs whose
# largest weight exceeds 0.5; a noiseless 1-per-key ramp puts 0.63 on its leader, the unit noise
# of the other 63 coordinates takes some rows below one half).  The 0.375-per-key ramps move the maximum in every tile but
# spread the weight over ~3 keys; they are not in this list.
NON_FLAT = {('peaked', 10.0): 0.5, ('peaked', 30.0): 0.8, ('ascending', 1.0): 0.5,
            ('descending', 1.0): 0.5, ('needle', 'first'): 0.95, ('needle', '31'): 0.9,
            ('needle', '32'): 0.9, ('needle', 'last'): 0.95, ('needle', 'second_half'): 0.9,
            ('needle', 'last_visible'): 0.95}


def regime_case(regime, param, **kw):
    if regime == 'needle':
        return make_attention_case('needle', needle=param, **kw)
    return make_attention_case(regime, param=param, **kw)


# ---------------------------------------------------------------------------------------------
# the `attention` decode mode: one self-attention step over the per-hypothesis paths

# the attention regimes with the needle at the edges of the step kernel's 64-key blocks
SELF_STEP_REGIMES = [('unit', None), ('peaked', 10.0), ('peaked', 30.0), ('ascending', 1.0),
                     ('ascending', 0.375), ('descending', 1.0), ('descending', 0.375),
                     ('needle', 'first'), ('needle', '63'), ('needle', '64'), ('needle', 'last'),
                     ('shifted', 80.0), ('shifted', -80.0), ('tied', None)]
SELF_STEP_NON_FLAT = {**NON_FLAT, ('needle', '63'): 0.9, ('needle', '64'): 0.9}


def make_self_step_case(regime, param, H, n, length, seed=0, beam=0, prompt=0):
    """One decoder step of n hypothesis rows that attend over `length` positions (the newest
    included): qkv (n, 3d) = this step's Q | K | V, cache (max_len, n, 2d) = K | V of the earlier
    positions, path (n, max_len): position j of row r lives in cache[j][path[r][j]], the newest
    one in the row's own slot.  beam = 0: every ancestor is a random slot; beam = N > 0 with
    prompt = P: rows are B x N hypotheses whose first P positions live in their utterance's
    first slot and the later ones in random slots of the utterance.

    The data is the cross-attention case of make_attention_case with n sequences of one query
    and `length` keys (its regimes shape the scores by the key's POSITION, so they survive the
    gather): slot s holds sequence s's key / value row of every position.  Cache rows no path
    names, and every row of steps >= length, hold +-POISON (cache[length - 1] is what the step
    itself stores).  `q`, `kg`, `vg`, `seqs` are the gathered rows ref_attention runs on."""
    base = regime_case(regime, param, H=H, q_lens=[1] * n, kv_lens=[length] * n, seed=seed)
    d, step, max_len = H * 64, length - 1, length + 2
    g = torch.Generator().manual_seed(seed + 1000)
    if beam:
        assert n % beam == 0 and prompt < length
        first = (torch.arange(n) // beam * beam).unsqueeze(1)
        path = first + torch.randint(0, beam, (n, max_len), generator=g)
        path[:, :prompt] = first
    else:
        path = torch.randint(0, n, (n, max_len), generator=g)
    path[:, step] = torch.arange(n)
    q = torch.stack([base['q'][s[0]] for s in base['seqs']])                    # (n, d)
    ks = torch.stack([base['k'][s[2]:s[2] + length] for s in base['seqs']])     # (slot, pos, d)
    vs = torch.stack([base['v'][s[2]:s[2] + length] for s in base['seqs']])
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0) * POISON
    cache = torch.cat([-sign, sign]).repeat(max_len, n, 1)
    named = torch.zeros(max_len, n, dtype=torch.bool)
    pos = torch.arange(step)
    for r in range(n):
        named[pos, path[r, :step]] = True
    cache[:step][named[:step]] = torch.cat([ks, vs], 2).transpose(0, 1)[:step][named[:step]]
    qkv = torch.cat([q, ks[:, step], vs[:, step]], 1)
    # row r's keys: position j from slot path[r][j]
    idx = path[:, :length].long()
    kg = ks[idx, torch.arange(length).unsqueeze(0)].reshape(n * length, d)
    vg = vs[idx, torch.arange(length).unsqueeze(0)].reshape(n * length, d)
    seqs = [(r, 1, r * length, length, 0) for r in range(n)]
    return dict(qkv=qkv.contiguous(), cache=cache.contiguous(), path=path.to(torch.int32),
                named=named, n=n, H=H, d=d, step=step, length=length, max_len=max_len, q=q,
                kg=kg, vg=vg, seqs=seqs, scale=base['scale'])


def self_step_refs(case):
    """(fp64 reference (n, d), e_plain, scale, largest weight per (row, head)) of a step case:
    ref_attention on the gathered rows, one sequence of one query per hypothesis row."""
    args = (case['q'], case['kg'], case['vg'], None, None, None, case['seqs'], 0, 0, -1,
            case['scale'])
    ref, w = ref_attention(*args, want_weights=True)
    plain = ref_attention(*args, fp32=True)
    return ref, (plain - ref).abs().max().item(), visible_v_scale(case['vg'], case['seqs']), w


# ---------------------------------------------------------------------------------------------
# the `attention` decode mode: the beam state kernels, restated in NumPy.  Scores are fp32 (one
# fp32 add per step is bit-reproducible); token / path rows have max_len columns, and a column no
# kernel writes keeps `fill`.

FILL = 0x7fc0dead


def ref_beam_init(B, N, max_len, sos=0, prompt=None, fill=FILL):
    """The start state (search.py:287-294): slot 0 of every utterance alive, the others -inf;
    every row <sos>, or (prompt (B, P)) its utterance's prompt, whose positions live in the
    utterance's first slot."""
    BN = B * N
    st = dict(score=np.where(np.arange(BN) % N == 0, 0.0, -np.inf).astype(np.float32),
              end=np.zeros(BN, np.int32), tok=np.full((BN, max_len), fill, np.int32),
              path=np.full((BN, max_len), fill, np.int32))
    if prompt is None:
        st['tok'][:, 0] = sos
        st['path'][:, 0] = np.arange(BN)
        st['last_tok'] = np.full(BN, sos, np.int32)
    else:
        prompt = np.asarray(prompt, np.int32)
        P = prompt.shape[1]
        st['tok'][:, :P] = np.repeat(prompt, N, axis=0)
        st['path'][:, :P] = (np.arange(BN) // N * N)[:, None]
        st['last_tok'] = np.repeat(prompt[:, P - 1], N).astype(np.int32)
    return st


def beam_rank(cand, N):
    """Flat indices of the N best of a row of candidates: NaN counts as -inf, then value
    descending, flat index ascending (a stable sort)."""
    c = np.where(np.isnan(cand), -np.inf, cand)
    return np.argsort(-c, kind='stable')[:N]


def ref_beam_update(st, topv, topi, B, N, step, eos, V, shared_row=False, fill=FILL):
    """One pruning step (search.py:315-354) on parents of `step` tokens.  topv / topi (B * N, N):
    the step's top-k log-probs (fp32) and tokens.  Returns (state, number of ended children)."""
    BN, max_len = st['tok'].shape
    topv = np.asarray(topv, np.float32).reshape(BN, N)
    topi = np.asarray(topi, np.int32).reshape(BN, N)
    ended = st['end'] != 0
    lp = topv.copy()
    lp[ended, 1:] = -np.inf                                  # mask_finished_scores
    lp[ended, 0] = 0.0
    with np.errstate(invalid='ignore'):
        cand = (st['score'][:, None] + lp).astype(np.float32)
    cand = np.where(np.isnan(cand), np.float32(-np.inf), cand)
    pred = np.where(ended[:, None], eos, topi)               # mask_finished_preds
    pred = np.where((pred < 0) | (pred >= V), eos, pred)     # the token clamp
    out = dict(score=np.empty(BN, np.float32), end=np.empty(BN, np.int32),
               tok=np.full((BN, max_len), fill, np.int32),
               path=np.full((BN, max_len), fill, np.int32), last_tok=np.empty(BN, np.int32))
    for b in range(B):
        flat = cand[b * N:(b + 1) * N].reshape(-1)
        for c, f in enumerate(beam_rank(flat, N)):
            parent, child = b * N + f // N, b * N + c
            t = pred[parent, f % N]
            out['score'][child] = flat[f]
            out['tok'][child, :step] = st['tok'][parent, :step]
            out['tok'][child, step] = t
            out['path'][child, :step - 1] = st['path'][parent, :step - 1]
            out['path'][child, step - 1] = b * N if shared_row else parent
            out['path'][child, step] = child
            out['last_tok'][child] = t
            out['end'][child] = int(t == eos)
    return out, int(out['end'].sum())


def beam_finish_scores(score, tok, B, N, length, eos, length_penalty):
    """(B, N) fp64 penalised scores score / count(tokens != eos) ** length_penalty
    (search.py:357-359)."""
    cnt = (np.asarray(tok)[:, :length] != eos).sum(1).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (np.asarray(score, np.float64) / cnt ** float(length_penalty)).reshape(B, N)


def ref_beam_finish(score, tok, B, N, length, eos, length_penalty, prefix=1, fill=FILL):
    """search.py:357-370: the first maximum of the penalised scores (a NaN never wins), its row
    without the first `prefix` tokens and without <eos>.  Returns (out_tok (B, max_len), out_len
    (B), best (B))."""
    tok = np.asarray(tok)
    max_len = tok.shape[1]
    s = beam_finish_scores(score, tok, B, N, length, eos, length_penalty)
    out_tok = np.full((B, max_len), fill, np.int32)
    out_len, best = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        top = -np.inf
        for n in range(N):
            if s[b, n] > top:
                top, best[b] = s[b, n], n
        row = tok[b * N + best[b], prefix:length]
        row = row[row != eos]
        out_tok[b, :len(row)] = row
        out_len[b] = len(row)
    return out_tok, out_len, best


def make_beam_finish_case(B, N, prefix, seed=0, V=50, eos=2):
    """Token rows of prefix + 9 tokens (some ended early, row 0 empty behind its prefix, columns
    behind the length garbage) and negative fp32 scores.  Returns (score, tok, length)."""
    rng = np.random.default_rng(seed)
    length = prefix + 9
    tok = rng.integers(3, V, (B * N, length + 2)).astype(np.int32)
    for r in range(B * N):
        if rng.random() < 0.6:
            tok[r, rng.integers(prefix, length):length] = eos
    tok[0, prefix:length] = eos
    score = (-rng.uniform(0.5, 30.0, B * N)).astype(np.float32)
    return score, tok, length


def beam_finish_margin_ok(s_row, same=()):
    """True when the winner of a row of fp64 penalised scores leads every other entry (those in
    `same`, rows with the winner's score and count and so its fp32 quotient, excepted) by more than 4 fp32 ulps of its size:
    powf may differ from the fp64 power in the last place, the division rounds once more."""
    s_row = np.asarray(s_row, np.float64)
    w = int(np.argmax(s_row))
    if not np.isfinite(s_row[w]):
        return bool(np.all(np.isneginf(s_row)))           # every row -inf: the first wins
    others = [s_row[i] for i in range(len(s_row)) if i != w and i not in same]
    return all(s_row[w] - o > 4 * ULP32 * abs(s_row[w]) for o in others)


# ---------------------------------------------------------------------------------------------
# the kernels that own a complete row: the LayerNorm family (csrc/encoder_kernels.hip), the FFN
# reduce (csrc/ffn_fused.hip), the row-LN GEMM (csrc/gemm_rowln.hip); GPU tests in
# tests/test_gpu_rows.py


def ref_layernorm(x, w, b, eps, fp32=False):
    """torch.nn.LayerNorm over the last dim, written out: mean, centred second moment (biased),
    (x - mean) / sqrt(var + eps) * w + b.  Returns fp64."""
    dt = torch.float32 if fp32 else torch.float64
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / D
    return (d / torch.sqrt(var + eps) * w + b).double()


def ref_ffn_reduce(x, P, b2, alpha, w, b, w2, bb2, eps, mode, fp32=False):
    """x (M, D), P (S, M, D).  x_new = x + alpha * (sum_s P[s] + b2), the slices added one by one.
    mode 0: (x_new, LN(x_new; w, b)); mode 1: (x1 = LN(x_new; w, b), LN(x1; w2, bb2)); mode 2:
    (LN(x_new; w, b), None).  Returns (new x, y) in fp64."""
    dt = torch.float32 if fp32 else torch.float64
    acc = torch.zeros(P.shape[1:], dtype=dt)
    for s in range(P.shape[0]):
        acc = acc + P[s].to(dt)
    x_new = (x.to(dt) + alpha * (acc + b2.to(dt))).double()
    if mode == 0:
        return x_new, ref_layernorm(x_new, w, b, eps, fp32)
    x1 = ref_layernorm(x_new, w, b, eps, fp32)
    if mode == 1:
        return x1, ref_layernorm(x1, w2, bb2, eps, fp32)
    return x1, None


def ref_gemm_rowln(A, W, bias, resid, alpha, ln_w, ln_b, eps, fp32=False):
    """A (M, K), W (256, K); bias / resid may be None.  x_out = resid + alpha * (A W^T + bias),
    y = LN(x_out; ln_w, ln_b).  Returns (x_out, y) in fp64."""
    dt = torch.float32 if fp32 else torch.float64
    acc = A.to(dt) @ W.to(dt).t()
    if bias is not None:
        acc = acc + bias.to(dt)
    x_out = alpha * acc
    if resid is not None:
        x_out = resid.to(dt) + x_out
    x_out = x_out.double()
    return x_out, ref_layernorm(x_out, ln_w, ln_b, eps, fp32)


def x3_offsets(M, D):
    """Byte offsets (3, M, D) of the bf16 elements of a plane image of M rows x D columns
    (csrc/x6.h): for plane pl, k block kb, half h and row, the 16 bytes at
    ((kb * tiles + (row >> 5)) * 3072 + pl * 1024 + h * 512 + (row & 31) * 16 hold the columns
    16 kb + 8 h .. + 7; tiles = ceil(M / 32)."""
    tiles = (M + 31) // 32
    pl = np.arange(3).reshape(3, 1, 1)
    row = np.arange(M).reshape(1, M, 1)
    col = np.arange(D).reshape(1, 1, D)
    kb, h, e = col // 16, (col // 8) % 2, col % 8
    return ((kb * tiles + (row >> 5)) * 3072 + pl * 1024 + h * 512 + (row & 31) * 16) + 2 * e


def x3_image_bytes(M, D):
    return (D // 16) * ((M + 31) // 32) * 3072


def x3_decode(buf, M, D):
    """buf: the bytes of a plane image (uint8, at least x3_image_bytes(M, D)).  Returns the three
    bf16 planes as a (3, M, D) float32 array."""
    buf = np.asarray(buf, dtype=np.uint8)
    off = x3_offsets(M, D)
    u16 = buf[off].astype(np.uint32) | (buf[off + 1].astype(np.uint32) << 8)
    return (u16 << 16).view(np.float32)


ROW_REGIMES = ('unit', 'offset', 'cols', 'small', 'outlier')
ROWS_EPS = 1e-5


def make_rows_case(regime, M, D, seed=0):
    """Rows for the LayerNorm family.  unit: 3 randn + 1; offset: 30 + randn (a one-pass variance
    cancels); cols: randn times a per-column logspace(-3, 3); small: 1e-4 randn, variance far below
    eps (eps outside the root shows); outlier: randn with the last column at 1e4.  w, b (and w2,
    b2 of a second norm) distinct per column."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    if regime == 'unit':
        x = 3.0 * x + 1.0
    elif regime == 'offset':
        x = 30.0 + x
    elif regime == 'cols':
        x = x * torch.logspace(-3, 3, D)
    elif regime == 'small':
        x = 1e-4 * x
    elif regime == 'outlier':
        x[:, -1] = 1e4
    else:
        raise ValueError(regime)
    return dict(x=x.contiguous(), w=1.0 + 0.2 * torch.randn(D, generator=g),
                b=0.1 * torch.randn(D, generator=g), w2=1.0 + 0.2 * torch.randn(D, generator=g),
                b2=0.1 * torch.randn(D, generator=g), eps=ROWS_EPS, M=M, D=D)


def rows_refs(c):
    """(fp64 LN(x), e_plain, scale) of a make_rows_case."""
    ref = ref_layernorm(c['x'], c['w'], c['b'], c['eps'])
    plain = ref_layernorm(c['x'], c['w'], c['b'], c['eps'], fp32=True)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


def rows2_refs(c):
    """(fp64 LN(LN(x; w, b); w2, b2), e_plain, scale) of a make_rows_case."""
    def two(fp32):
        y1 = ref_layernorm(c['x'], c['w'], c['b'], c['eps'], fp32)
        return ref_layernorm(y1, c['w2'], c['b2'], c['eps'], fp32)
    ref, plain = two(False), two(True)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


def make_ffn_reduce_case(M, D, S, alpha, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = make_rows_case('unit', M, D, seed + 1)
    c.update(P=torch.randn(S, M, D, generator=g), fb2=0.3 * torch.randn(D, generator=g),
             alpha=alpha, S=S)
    return c


def ffn_reduce_refs(c, mode):
    """((x, y) fp64, (e_plain, scale) of x, (e_plain, scale) of y or None)."""
    args = (c['x'], c['P'], c['fb2'], c['alpha'], c['w'], c['b'], c['w2'], c['b2'], c['eps'], mode)
    ref = ref_ffn_reduce(*args)
    plain = ref_ffn_reduce(*args, fp32=True)
    out = [ref]
    for r, p in zip(ref, plain):
        out.append(None if r is None else ((p - r).abs().max().item(), r.abs().max().item()))
    return tuple(out)


def make_gemm_rowln_case(M, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(A=torch.randn(M, K, generator=g), W=torch.randn(256, K, generator=g) / math.sqrt(K),
                bias=0.3 * torch.randn(256, generator=g), resid=torch.randn(M, 256, generator=g),
                ln_w=1.0 + 0.2 * torch.randn(256, generator=g),
                ln_b=0.1 * torch.randn(256, generator=g), eps=ROWS_EPS, M=M, K=K)


def gemm_rowln_refs(c, bias=True, resid=True, alpha=1.0):
    """((x_out, y) fp64, (e_plain, scale) of x_out, (e_plain, scale) of y)."""
    args = (c['A'], c['W'], c['bias'] if bias else None, c['resid'] if resid else None, alpha,
            c['ln_w'], c['ln_b'], c['eps'])
    ref = ref_gemm_rowln(*args)
    plain = ref_gemm_rowln(*args, fp32=True)
    return (ref, ) + tuple(((p - r).abs().max().item(), r.abs().max().item())
                           for r, p in zip(ref, plain))


# ---------------------------------------------------------------------------------------------
# the tolerance of the issue: err <= margin * e_plain + floor, and the cap on the yardstick

MARGIN_F32, MARGIN_BF16 = 8.0, 4.0
CAP_F32, CAP_BF16 = 1e-3, 1e-2


def bound(e_plain, scale, bf16=False):
    if bf16:
        return MARGIN_BF16 * e_plain + 2.0 ** -9 * scale
    return MARGIN_F32 * e_plain + 16 * ULP32 * scale


def cap_ok(e_plain, scale, bf16=False):
    return e_plain <= (CAP_BF16 if bf16 else CAP_F32) * scale


# ---------------------------------------------------------------------------------------------
# the fp32 and bf16-on-the-fly matrix-core GEMMs (csrc/gemm.hip, gemm_bf16.hip) through
# wn_op_gemm_ex; GPU tests in tests/test_gpu_gemm_ops.py


def glu_perm(d):
    """Rows of a (2 d, K) GLU weight [values | gates] in the order the GLU epilogue reads them:
    per 64 rows [32 values | 32 gates] (what wn_model_create gives pointwise_conv1)."""
    return torch.cat([torch.cat([torch.arange(32) + 32 * u, torch.arange(32) + 32 * u + d])
                      for u in range(d // 32)])


def gemm_route_code(bm, bn, wgm, wgn, bk, pf, glu=False, conv=False, prec=0, act=0, resid=False):
    """The instantiation code wn_op_gemm_ex reports (csrc/common.h gemm_route_code)."""
    return (bm // 64 | (bn // 64) << 4 | wgm << 8 | wgn << 12 | (bk // 32) << 16 | pf << 20 |
            int(glu) << 22 | int(conv) << 23 | prec << 24 | act << 25 | int(resid) << 27)


# pre-activations / gates of the `wide` regime: exp overflow and underflow of x * rcp(1 + exp(-x))
GEMM_WIDE = (0.0, 20.0, -20.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0)
GATE_ON, GATE_OFF = 40.0, -200.0      # sigmoid == 1.0f / a product that rounds to 0.0f


def gemm_act(z, act):
    """0 none, 1 SiLU (x * sigmoid(x)), 2 ReLU, 3 exact GELU (erf)."""
    if act == 1:
        return z * torch.sigmoid(z)
    if act == 2:
        return F.relu(z)
    if act == 3:
        return F.gelu(z)
    return z


def _coded_w(N, K):
    """W[n][k] = (37 n + 11 k) mod 251 - 125: integers of at most 8 bits (exact in bf16) that
    differ between neighbouring rows, columns, 32- / 64- / 128-wide tiles and K tiles."""
    n = torch.arange(N, dtype=torch.int32).unsqueeze(1)
    k = torch.arange(K, dtype=torch.int32).unsqueeze(0)
    return ((37 * n + 11 * k) % 251 - 125).float()


def _gemm_spec(kind, M, N, K, route, **kw):
    s = dict(kind=kind, M=M, N=N, K=K, route=route, act=0, resid=0, glu=False, prec=0,
             regime='unit', alpha=1.0, lens=None, F1=0, conv_C=0, stride=2, taps=3,
             tile1_route=None, seed=0)
    s.update(kw)
    return s


def gemm_case_id(s):
    bm, bn, wgm, wgn, bk, pf = s['route']
    t = ['bf16' if s['prec'] else 'f32', s['kind'], f'{bm}x{bn}w{wgm}x{wgn}k{bk}pf{pf}',
         f"{s['M']}x{s['N']}x{s['K']}", f"act{s['act']}", ('r0', 'r1', 'rC')[s['resid']], s['regime']]
    if s['glu']:
        t.insert(2, 'glu')
    return '-'.join(t)


def rows_layout(lens, taps, stride, gap=1, lead=1):
    """Packed utterances of `lens` frames with `gap` unowned frames between them: (first frame of
    every output row, total frames).  Output t of an utterance reads frames stride * t .. + taps."""
    first, at = [], lead
    for n in lens:
        first += [at + stride * t for t in range((n - taps) // stride + 1)]
        at += n + gap
    return first, at


def conv3_layout(t1_lens, F1, gap=1, lead=1):
    """Packed channels-last images of t1_lens[u] x F1 pixels: (first pixel of every output row of
    the 3x3 / stride-2 conv, image offsets in frames, total frames)."""
    first, offs, at = [], [], lead
    F2 = (F1 - 3) // 2 + 1
    for n in t1_lens:
        offs.append(at)
        for t2 in range((n - 3) // 2 + 1):
            first += [(at + 2 * t2) * F1 + 2 * f2 for f2 in range(F2)]
        at += n + gap
    return first, offs, at


def gemm_rows(s):
    """M of a spec (gathered kinds: the output rows their layout gives)."""
    if s['kind'] == 'rows':
        return len(rows_layout(s['lens'], s['taps'], s['stride'])[0])
    if s['kind'] == 'conv3':
        return len(conv3_layout(s['lens'], s['F1'])[0])
    return s['M']


def make_gemm_case(s):
    """The tensors of a spec of GEMM_CASES.  kind plain: A (M, K).  kind rows: `buf`, packed frames
    of d = K / taps channels; output row r is `taps` consecutive frames from frame first[r] on
    (a_row_off = first * d, conv_C = K).  kind conv3: `buf`, packed channels-last images of F1
    pixels x conv_C channels per frame; a_row_off = first pixel * conv_C, conv_sy = F1 * conv_C,
    conv_sx = conv_C, K = 9 conv_C.  Every float of `buf` that no (row, k) reads holds POISON.
    `W` is what the kernel gets ((N, K); GLU: rows permuted); `W_un` / `b_un` the un-permuted GLU
    weight [values | gates]; `w_t` the torch-layout conv weight."""
    g = torch.Generator().manual_seed(1000 + s['seed'])
    kind, N, K, regime, glu = s['kind'], s['N'], s['K'], s['regime'], s['glu']
    M = gemm_rows(s)
    assert M == s['M'], (M, s['M'])
    coded = regime == 'coded'
    c = dict(spec=s, M=M, N=N, K=K)
    # ---- the A operand
    if kind == 'plain':
        if coded:
            A = torch.zeros(M, K)
            A[torch.arange(M), (13 * torch.arange(M) + 5) % K] = 1.0
        else:
            A = torch.randn(M, K, generator=g)
        c['A'] = A
    else:
        if kind == 'rows':
            d = K // s['taps']
            first, frames = rows_layout(s['lens'], s['taps'], s['stride'])
            px, reach = frames, [t * d + e for t in range(s['taps']) for e in range(d)]
            c.update(conv_C=K, conv_sy=0, conv_sx=0)
        else:
            d, F1 = s['conv_C'], s['F1']
            first, offs, frames = conv3_layout(s['lens'], F1)
            px = frames * F1
            reach = [(ky * F1 + kx) * d + e for ky in range(3) for kx in range(3) for e in range(d)]
            c.update(conv_C=d, conv_sy=F1 * d, conv_sx=d, img_off=offs)
        if coded:
            buf = torch.zeros(px, d)
            buf[torch.arange(px), (5 * torch.arange(px) + 1) % d] = 1.0
        else:
            buf = torch.randn(px, d, generator=g)
        buf = buf.reshape(-1)
        off = torch.tensor(first, dtype=torch.int64) * d
        own = torch.zeros(buf.numel(), dtype=torch.bool)
        own[(off.unsqueeze(1) + torch.tensor(reach).unsqueeze(0)).reshape(-1)] = True
        buf[~own] = POISON
        c.update(buf=buf, a_row_off=off, d=d, own=own)
    # ---- W, bias
    W = _coded_w(N, K) if coded else torch.randn(N, K, generator=g) / math.sqrt(K)
    if coded:
        bias = (torch.arange(N) % 7 - 3).float()
    else:
        bias = 0.3 * torch.randn(N, generator=g)
    if regime == 'wide':
        wide = torch.tensor(GEMM_WIDE)[torch.arange(N) % len(GEMM_WIDE)]
    if glu:
        h = N // 2
        if coded:
            # value rows coded, gate rows zero with a bias that opens (1.0f) or shuts the gate
            W[h:] = 0.0
            bias[h:] = torch.where((5 * torch.arange(h) + torch.arange(h) // 32) % 3 != 0,
                                   GATE_ON, GATE_OFF)
        elif regime == 'wide':
            bias[h:] = wide[:h]
        perm = glu_perm(h)
        c.update(W_un=W, b_un=bias, W=W[perm].contiguous(), bias=bias[perm].contiguous())
    else:
        if regime == 'wide':
            bias = wide
        c.update(W=W, bias=bias)
        if kind == 'rows':      # the Conv1d weight (N, d, taps) this (N, taps * d) matrix is
            c['w_t'] = W.view(N, s['taps'], d).permute(0, 2, 1).contiguous()
        if kind == 'conv3':     # the Conv2d weight (N, C, 3, 3)
            c['w_t'] = W.view(N, 3, 3, d).permute(0, 3, 1, 2).contiguous()
    if s['resid']:
        if coded:
            r = torch.arange(M, dtype=torch.int32).unsqueeze(1)
            n = torch.arange(N, dtype=torch.int32).unsqueeze(0)
            c['resid'] = ((3 * r + 5 * n) % 17 - 8).float()
        else:
            c['resid'] = torch.randn(M, N, generator=g)
    return c


def gemm_operand(c):
    """The (M, K) operand of a gathered case by explicit indexing of the flat buffer:
    element (r, k) = buf[a_row_off[r] + (tap / 3) * conv_sy + (tap % 3) * conv_sx + k % conv_C]."""
    k = torch.arange(c['K'])
    tap = k // c['conv_C']
    koff = (tap // 3) * c['conv_sy'] + (tap % 3) * c['conv_sx'] + k % c['conv_C']
    return c['buf'][c['a_row_off'].unsqueeze(1) + koff.unsqueeze(0)]


def ref_gemm(c, fp32=False):
    """resid + alpha * act(X W^T + bias) in fp64 (fp32: the same statement evaluated in fp32, the
    yardstick).  precision 1: both operands rounded to bf16 first.  GLU: F.glu over the
    UN-permuted weight [values | gates].  rows: X by explicit indexing of the flat buffer.
    conv3: F.conv2d (stride 2) on every utterance's channels-last image with the Conv2d-layout
    weight.  Returns (M, N) -- (M, N / 2) with GLU -- fp64."""
    s = c['spec']
    dt = torch.float32 if fp32 else torch.float64
    rnd = _r16 if s['prec'] == 1 else (lambda t: t)
    if s['kind'] == 'conv3':
        d, F1 = c['d'], s['F1']
        img = c['buf'].view(-1, F1, d)
        w = rnd(c['w_t']).to(dt)
        zs = []
        for o, n in zip(c['img_off'], s['lens']):
            x = rnd(img[o:o + n]).to(dt).permute(2, 0, 1).unsqueeze(0)        # (1, C, t1, F1)
            y = F.conv2d(x, w, stride=2)[0]                                    # (N, t2, F2)
            zs.append(y.permute(1, 2, 0).reshape(-1, c['N']))
        z = torch.cat(zs)
    else:
        X = c['A'] if s['kind'] == 'plain' else gemm_operand(c)
        Wm = c['W_un'] if s['glu'] else c['W']
        z = rnd(X).to(dt) @ rnd(Wm).to(dt).t()
    z = z + (c['b_un'] if s['glu'] else c['bias']).to(dt)
    y = F.glu(z, dim=-1) if s['glu'] else gemm_act(z, s['act'])
    y = y * s['alpha']
    if s['resid']:
        y = c['resid'].to(dt) + y
    return y.double()


def gemm_refs(c):
    """(fp64 reference, e_plain, scale = max |ref|) of a case."""
    ref = ref_gemm(c)
    plain = ref_gemm(c, fp32=True)
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item()


def _gemm_cases():
    S = _gemm_spec
    out = []

    def epis(kind, M, N, K, route, combos, **kw):
        for regime, act, resid in combos:
            alpha = 0.5 if resid == 1 else 1.0
            out.append(S(kind, M, N, K, route, regime=regime, act=act, resid=resid, alpha=alpha,
                         seed=len(out), **kw))

    every = [('unit', a, r) for a in range(4) for r in (0, 1)]
    coded = [('coded', 0, 0), ('coded', 2, 1), ('coded', 0, 2)]
    wide = [('wide', 1, 0), ('wide', 3, 0)]
    few = [('unit', 0, 0), ('unit', 2, 1), ('coded', 0, 0)]
    for prec in (0, 1):
        P = dict(prec=prec)
        ks = (32, ) if prec == 0 else (64, 96)
        bk = lambda K: 32 if prec == 0 else (64 if K % 64 == 0 else 32)
        # ---- plain rows, the 128x128 / 2x4 block (fp32: 384 tiles, bf16: 224)
        Nw = 24571 if prec == 0 else 14331
        for K in ks:
            r = (128, 128, 2, 4, bk(K), 1)
            epis('plain', 200, Nw, K, r, (every + [('unit', 0, 2)] + coded + wide) if K == ks[0]
                 else every + few[2:], **P)
        if prec == 0:
            # tall: the XCD block order over 96 M panels
            epis('plain', 12285, 500, 32, (128, 128, 2, 4, 32, 1), [('unit', 0, 0), ('coded', 0, 0)])
            # t128 = 192, t64x128 = 384; ragged in M and N
            epis('plain', 100, 24570, 32, (64, 128, 2, 4, 32, 1), every + coded[:2])
        # ---- the 64x64 / 2x2 block
        for K in ks:
            r = (64, 64, 2, 2, bk(K), 1)
            epis('plain', 333, 200, K, r, (every + coded + wide) if K == ks[0]
                 else every + few[2:], **P)
            epis('plain', 1, 1, K, r, few, **P)
            epis('plain', 65, 67, K, r, few + wide + [('unit', 0, 2)], **P)
        if prec == 0:
            # PF = 2 (K >= 1024; act 0 and ReLU only): 32, 33 (the tail) and 34 K tiles
            for K in (1024, 1056, 1088):
                epis('plain', 65, 67, K, (64, 64, 2, 2, 32, 2),
                     [('unit', 0, 0), ('unit', 0, 1), ('unit', 2, 0), ('unit', 2, 1),
                      ('coded', 0, 0), ('coded', 2, 1)])
            big2 = (128, 128, 2, 4, 32, 2)
            epis('plain', 200, 24571, 1024, big2, [('unit', 2, 1)])
            epis('plain', 200, 24571, 1056, big2, [('unit', 0, 0), ('unit', 2, 0)])
            epis('plain', 200, 24571, 1088, big2, [('coded', 0, 1)])
            epis('plain', 100, 24570, 1024, (64, 128, 2, 4, 32, 2), [('unit', 2, 0)])
            epis('plain', 100, 24570, 1056, (64, 128, 2, 4, 32, 2), [('unit', 0, 1)])
        # ---- GLU
        glu3 = [('unit', 0, 0), ('coded', 0, 0), ('wide', 0, 0)]
        for K in ks:
            for N in (64, 128, 192):
                for M in (1, 63, 130):
                    if K == ks[0] or (N, M) == (192, 130):
                        epis('plain', M, N, K, (64, 128, 2, 2, bk(K), 1),
                             glu3 if M == 63 or N == 192 else glu3[:2], glu=True, **P)
            epis('plain', 129, 14272, K, (128, 128, 4, 2, bk(K), 1),
                 glu3 if K == ks[0] else glu3[:1], glu=True, **P)
        # ---- gathered rows: a 3-tap stride-2 Conv1d over packed utterances
        gath = [('unit', 0, 0), ('unit', 0, 1), ('unit', 2, 0), ('unit', 2, 1), ('unit', 3, 0),
                ('unit', 3, 1), ('coded', 0, 0), ('coded', 2, 1)]
        big = (128, 128, 2, 2) if prec == 0 else (128, 128, 2, 4)
        for K in ((96, ) if prec == 0 else (96, 192)):
            epis('rows', 66, 200, K, (64, 128, 2, 2, bk(K), 1), gath, lens=[37, 3, 95], **P)
            epis('rows', 129, Nw, K, big + (bk(K), 1), gath, lens=[150, 111], **P)
        # ---- the implicit 3x3 / stride-2 operand: two images, F1 = 7
        for C in (32, 64):
            conv = [('unit', 2, 0), ('coded', 2, 0)]
            epis('conv3', 69, 70, 9 * C, (64, 128, 2, 2, bk(C), 1), conv, lens=[31, 17], F1=7,
                 conv_C=C, **P)
            epis('conv3', 138, Nw, 9 * C, big + (bk(C), 1), conv if C == 32 else conv[:1],
                 lens=[61, 33], F1=7, conv_C=C, **P)
    # ---- bf16 256x256 / 4x2: t256 = 2 * 513 = 1026; under gemm_tile_bf16 = 1 the 128x128 block
    t1 = (128, 128, 2, 4, 64, 1)
    epis('plain', 257, 131069, 64, (256, 256, 4, 2, 64, 1),
         [('unit', 0, 0), ('coded', 2, 1), ('wide', 1, 0), ('unit', 3, 1)], prec=1, tile1_route=t1)
    # K >= 2048 with t256 = 2 * 128 = 256
    epis('plain', 257, 32765, 2048, (256, 256, 4, 2, 64, 1), [('unit', 0, 0)], prec=1,
         tile1_route=t1)
    return out


GEMM_CASES = _gemm_cases()


# ---------------------------------------------------------------------------------------------
# the stored-operand GEMMs (csrc/gemm_bf16s.hip, gemm_bf16p.hip) through wn_op_gemm_lowp_ex and the
# MXFP8 quantiser through wn_op_mx_quantize_ex; GPU tests in tests/test_gpu_gemm_lowp_ops.py


def e4m3_encode(v):
    """fp64 values -> OCP e4m3 bytes (1 sign, 4 exponent bits of bias 7, 3 mantissa bits, no
    infinity, largest finite value 448): round to nearest even, saturating; a zero keeps its sign.
    Normal numbers have the quantum 2^(floor(log2 |v|) - 3), everything below 2^-6 the subnormal
    quantum 2^-9."""
    v = v.double()
    a = v.abs()
    ex = torch.frexp(a)[1] - 1                                   # floor(log2 a); a = 0: anything
    quantum = torch.exp2(torch.where(a < 2.0 ** -6, torch.full_like(ex, -9), ex - 3).double())
    q = torch.clamp(torch.round(a / quantum) * quantum, max=448.0)        # torch.round: ties to even
    ex = torch.frexp(q)[1] - 1                                   # the rounding may have carried
    sub = q < 2.0 ** -6
    field = torch.where(sub, torch.zeros_like(ex), ex + 7)
    man = torch.where(sub, q * 2.0 ** 9, (q / torch.exp2(ex.double()) - 1.0) * 8.0)
    byte = field.long() * 8 + man.long() + torch.signbit(v).long() * 128
    return byte.to(torch.uint8)


def e4m3_decode(b):
    b = b.long()
    field, man = (b >> 3) & 15, (b & 7).double()
    mag = torch.where(field == 0, man * 2.0 ** -9, (1.0 + man / 8.0) * torch.exp2(field.double() - 7.0))
    return torch.where((b & 128) != 0, -mag, mag)


def mx_encode(x):
    """(rows, K) fp32, K % 32 == 0 -> (e4m3 bytes (rows, K), E8M0 bytes (rows, K / 32)), the OCP
    MX rule with the block scale csrc/mxfp8.h states: one scale 2^e per 32 consecutive k, the
    smallest power of two with amax <= 448 * 2^e, stored as E = e + 127 clamped to [0, 253];
    elements = e4m3(v * 2^-e), round to nearest even, saturating."""
    rows, K = x.shape
    xb = x.double().reshape(rows, K // 32, 32)
    amax = xb.abs().amax(-1)
    e = torch.frexp(amax)[1] - 1 - 8                             # amax < 2 * 256 * 2^e
    e = e + (amax > 448.0 * torch.exp2(e.double())).to(e.dtype)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)      # every power of two will do
    E = torch.clamp(e + 127, 0, 253)
    q = e4m3_encode(xb * torch.exp2(127.0 - E.double()).unsqueeze(-1))
    return q.reshape(rows, K), E.to(torch.uint8)


def mx_decode(q, E):
    """The fp64 values an MXFP8 image stands for: e4m3 element x 2^(E - 127) of its 32-block."""
    rows, K = q.shape
    v = e4m3_decode(q).reshape(rows, K // 32, 32)
    return (v * torch.exp2(E.double() - 127.0).unsqueeze(-1)).reshape(rows, K)


def mx_scale_dwords(E, pitch, fill=0xfe):
    """E bytes (rows, nblk) -> the dword array [ceil(nblk / 4)][pitch] the kernels read (byte b of
    dword [kt][row] = block 4 kt + b), as int32; every byte no (row, block) owns holds `fill`."""
    rows, nblk = E.shape
    nk = (nblk + 3) // 4
    by = torch.full((nk, pitch, 4), fill, dtype=torch.uint8)
    for kb in range(nblk):
        by[kb // 4, :rows, kb % 4] = E[:, kb]
    return by.view(torch.int32).reshape(nk, pitch)


def mx_scale_bytes(dw, rows, nblk):
    """The inverse: int32 [nk][pitch] -> E bytes (rows, nblk)."""
    by = dw.contiguous().view(torch.uint8).reshape(dw.shape[0], dw.shape[1], 4)
    return torch.stack([by[kb // 4, :rows, kb % 4] for kb in range(nblk)], dim=1)


def bf16_tie_share(v, b):
    """The share of the elements of v (fp64) that lie within b of a bf16 rounding boundary: v - b
    and v + b round to different bf16 numbers.  (elementwise mask, share)"""
    near = (v - b).float().to(torch.bfloat16) != (v + b).float().to(torch.bfloat16)
    return near, near.float().mean().item()


GELU_E5_ABS = 4.7e-6       # |gelu_e5 - gelu| (csrc/gemm_bf16p.hip; tests/test_gelu_form.py)
FAM_STORED, FAM_PIPELINED = 1, 2


def lowp_route_code(s):
    """The code wn_op_gemm_lowp_ex reports for a spec (csrc/common.h gemm_route_code): the fields
    of gemm_route_code | MXFP8 << 19 | family << 28 | C mode << 30, as an int32."""
    bm, bn, wgm, wgn, bk = s['route']
    pipe = s['fam'] == FAM_PIPELINED
    code = gemm_route_code(bm, bn, wgm, wgn, bk, 1 if pipe else 2, glu=s['glu'],
                           prec=0 if s['et'] else 1, act=s['act'], resid=bool(s['resid']))
    code |= s['et'] << 19 | s['fam'] << 28 | s['cm'] << 30
    return code - (1 << 32) if code >> 31 else code


def _lowp_spec(fam, et, M, N, K, route, **kw):
    s = dict(fam=fam, et=et, M=M, N=N, K=K, route=route, cm=0, act=0, resid=0, glu=False,
             regime='unit', alpha=1.0, tile=8 if fam == FAM_PIPELINED and not et else 0,
             model_pitch=True, w_pad=0, seed=0)
    s.update(kw)
    return s


def gemm_lowp_case_id(s):
    bm, bn, wgm, wgn, bk = s['route']
    t = ['mx' if s['et'] else 'bf16', ('stored', 'pipe')[s['fam'] - 1],
         f'{bm}x{bn}w{wgm}x{wgn}k{bk}', f"{s['M']}x{s['N']}x{s['K']}", f"act{s['act']}",
         f"r{s['resid']}", ('c32', 'c16', 'cmx')[s['cm']], s['regime']]
    if s['glu']:
        t.insert(2, 'glu')
    if s['fam'] == FAM_PIPELINED and not s['et'] and s['tile'] != 8:
        t.insert(2, f"tile{s['tile']}")
    return '-'.join(t)


def _coded_hot_k(M, K):
    return (13 * torch.arange(M) + 5) % K


def make_gemm_lowp_case(s):
    """The tensors of a spec of GEMM_LOWP_CASES.  `A` (M, K) / `W` (N, K) hold, as fp32, exactly
    the values of the storage type (bf16, or e4m3 x block scale); MXFP8 cases also carry the
    images Aq / AE and Wq / WE (element bytes, E8M0 bytes (rows, K / 32)).  `W` is what the kernel
    gets (GLU: rows permuted), `W_un` / `b_un` the un-permuted GLU weight [values | gates].
    Regimes: see the docstring of tests/test_gpu_gemm_lowp_ops.py."""
    g = torch.Generator().manual_seed(7000 + s['seed'])
    M, N, K, et, regime, glu = s['M'], s['N'], s['K'], s['et'], s['regime'], s['glu']
    nb = K // 32
    c = dict(spec=s, M=M, N=N, K=K)
    mi = torch.arange(M).unsqueeze(1)
    ni = torch.arange(N).unsqueeze(1)
    ki = torch.arange(K).unsqueeze(0)
    kb = torch.arange(nb).unsqueeze(0)
    if regime in ('coded-hot', 'coded-dense'):
        w_int = ((37 * ni + 11 * ki) % 17 - 8).double()
        if regime == 'coded-hot':
            # one product per output: 2^s(m) at k = h(m) against w_int 2^t(n, k / 32)
            hot = _coded_hot_k(M, K)
            a_int = torch.zeros(M, K, dtype=torch.float64)
            a_int[torch.arange(M), hot] = 1.0
            a_e = (5 * mi + 3 * kb) % 11 - 5                     # the blocks that hold only zeros
            a_e[torch.arange(M), hot // 32] = torch.arange(M) % 9 - 4
            w_e = (3 * ni + 5 * kb) % 9 - 4
        else:
            # dense small integers, one power of two per row: every k-step's products are integers
            a_int = ((7 * mi + 3 * ki + (mi * ki) % 5) % 5 - 2).double()
            a_e = ((mi % 7) - 3).expand(M, nb)
            w_e = ((ni % 5) - 2).expand(N, nb)
        if et:
            c['Aq'], c['AE'] = e4m3_encode(a_int), (a_e + 127).to(torch.uint8)
            c['Wq'], c['WE'] = e4m3_encode(w_int), (w_e + 127).to(torch.uint8)
        A = a_int * torch.exp2(a_e.double()).repeat_interleave(32, dim=1)
        W = w_int * torch.exp2(w_e.double()).repeat_interleave(32, dim=1)
        bias = (torch.arange(N) % 7 - 3).float()
    else:
        if et:
            if regime == 'unit':
                A0 = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
                A0 = A0 * torch.exp2(torch.randint(-6, 6, (1, nb), generator=g).float()
                                     ).repeat_interleave(32, dim=1)
                W0 = torch.randn(N, K, generator=g) * 0.2
            else:
                A0 = torch.randn(M, K, generator=g)
                W0 = torch.randn(N, K, generator=g) / math.sqrt(K)
            c['Aq'], c['AE'] = mx_encode(A0)
            c['Wq'], c['WE'] = mx_encode(W0)
            A, W = mx_decode(c['Aq'], c['AE']), mx_decode(c['Wq'], c['WE'])
        else:
            A = _r16(torch.randn(M, K, generator=g)).double()
            W = _r16(torch.randn(N, K, generator=g) / math.sqrt(K)).double()
        bias = 0.3 * torch.randn(N, generator=g)
        if s['cm'] == 1:
            # bf16 C: keep the outputs off zero, where every absolute bound spans many bf16
            # rounding boundaries (the tie share of the test)
            bias = bias + 4.0
    A, W = A.float(), W.float()
    assert torch.isfinite(A).all() and torch.isfinite(W).all()
    if not et:
        assert torch.equal(_r16(A), A) and torch.equal(_r16(W), W)
    else:
        assert torch.equal(mx_decode(c['Aq'], c['AE']).float(), A)
        assert torch.equal(mx_decode(c['Wq'], c['WE']).float(), W)
    if regime == 'wide':
        wide = torch.tensor(GEMM_WIDE)[torch.arange(N) % len(GEMM_WIDE)]
    if glu:
        h = N // 2
        if regime.startswith('coded'):
            W[h:] = 0.0
            bias[h:] = torch.where((5 * torch.arange(h) + torch.arange(h) // 32) % 3 != 0,
                                   GATE_ON, GATE_OFF)
        elif regime == 'wide':
            bias[h:] = wide[:h]
        perm = glu_perm(h)
        c.update(W_un=W, b_un=bias, W=W[perm].contiguous(), bias=bias[perm].contiguous())
    else:
        if regime == 'wide':
            bias = wide
        c.update(W=W, bias=bias)
    c['A'] = A
    if s['resid']:
        if regime.startswith('coded'):
            c['resid'] = ((3 * mi + 5 * torch.arange(N).unsqueeze(0)) % 17 - 8).float()
        else:
            c['resid'] = torch.randn(M, N, generator=g)
    return c


def ref_gemm_lowp(c, fp32=False):
    """resid + alpha * act(A W^T + bias) on the DECODED operands, in fp64 (fp32: the same formula
    in torch fp32, the yardstick).  GLU: F.glu over the un-permuted weight.  A bf16 or MXFP8 C is
    not rounded here: the GPU test compares it with the rounding of the kernel's own fp32 C."""
    s = c['spec']
    dt = torch.float32 if fp32 else torch.float64
    Wm = c['W_un'] if s['glu'] else c['W']
    z = c['A'].to(dt) @ Wm.to(dt).t() + (c['b_un'] if s['glu'] else c['bias']).to(dt)
    y = F.glu(z, dim=-1) if s['glu'] else gemm_act(z, s['act'])
    y = y * s['alpha']
    if s['resid']:
        y = c['resid'].to(dt) + y
    return y.double()


def gemm_lowp_refs(c):
    """(fp64 reference, e_plain, scale = max |ref|, S = max sum_k |a||w|) of a case."""
    ref = ref_gemm_lowp(c)
    plain = ref_gemm_lowp(c, fp32=True)
    S = (c['A'].double().abs() @ c['W'].double().abs().t()).max().item()
    return ref, (plain - ref).abs().max().item(), ref.abs().max().item(), S


def _gemm_lowp_cases():
    S = _lowp_spec
    out = []

    def add(fam, et, M, N, K, route, regime, act, resid, cm=0, **kw):
        alpha = 0.5 if resid else 1.0
        n = len(out)
        out.append(S(fam, et, M, N, K, route, regime=regime, act=act, resid=resid, cm=cm,
                     alpha=alpha, seed=n, model_pitch=n % 2 == 0, **kw))

    # ---- the pipelined kernel: bf16 under gemm_tile_bf16 = 8, MXFP8 always; K tiles 2 3 4 5
    for et in (0, 1):
        P = FAM_PIPELINED
        r = (256, 256, 2, 4, 128 if et else 64)
        k2, k3, k4, k5 = [t * (128 if et else 64) for t in (2, 3, 4, 5)]
        # every activation x residual form with fp32 C; every M, N, tile count
        add(P, et, 1, 8, k2, r, 'unit', 0, 0)
        add(P, et, 255, 256, k3, r, 'unit', 0, 1, w_pad=5)
        add(P, et, 256, 264, k4, r, 'unit', 1, 0)
        add(P, et, 257, 520, k5, r, 'unit', 1, 1)
        add(P, et, 300, 8, k3, r, 'unit', 2, 0)
        add(P, et, 1030, 264, k2, r, 'unit', 2, 1)        # 5 M panels: the last group has 1
        add(P, et, 1281, 256, k4, r, 'unit', 3, 0)        # 6 M panels: the last group has 2
        add(P, et, 257, 264, k5, r, 'unit', 3, 1)
        # exact: one product per output (M >= K: every k is some row's hot k)
        add(P, et, 257, 264, k2 if et else k4, r, 'coded-hot', 0, 0, w_pad=5)
        add(P, et, 1030, 264, k5, r, 'coded-hot', 2, 1)
        add(P, et, 1281, 520, k3, r, 'coded-hot', 0, 1)
        # exact: dense integers, every K tile count
        add(P, et, 300, 264, k5, r, 'coded-dense', 0, 0)
        add(P, et, 1030, 264, k4, r, 'coded-dense', 2, 1, w_pad=5)
        add(P, et, 255, 520, k2, r, 'coded-dense', 0, 0)
        add(P, et, 257, 256, k3, r, 'coded-dense', 0, 1)
        add(P, et, 257, 264, k2, r, 'wide', 1, 0)
        add(P, et, 300, 520, k3, r, 'wide', 3, 0)
        if not et:
            # bf16 C: every activation
            add(P, 0, 255, 520, k2, r, 'unit', 0, 0, cm=1)
            add(P, 0, 1030, 264, k3, r, 'unit', 1, 0, cm=1)
            add(P, 0, 257, 8, k4, r, 'unit', 2, 0, cm=1)
            add(P, 0, 1281, 256, k5, r, 'unit', 3, 0, cm=1)
            add(P, 0, 1, 264, k2, r, 'unit', 0, 0, cm=1)
            add(P, 0, 300, 264, k4, r, 'coded-hot', 0, 0, cm=1)
            add(P, 0, 256, 520, k5, r, 'coded-dense', 2, 0, cm=1)
        else:
            # MXFP8 C: every activation; N = 288 leaves one used byte in the last scale dword
            add(P, 1, 255, 32, k2, r, 'unit', 0, 0, cm=2)
            add(P, 1, 1030, 288, k3, r, 'unit', 1, 0, cm=2)
            add(P, 1, 257, 544, k4, r, 'unit', 2, 0, cm=2, w_pad=5)
            add(P, 1, 1281, 288, k5, r, 'unit', 3, 0, cm=2)
            add(P, 1, 1, 288, k2, r, 'unit', 0, 0, cm=2)
            add(P, 1, 256, 544, k3, r, 'unit', 3, 0, cm=2)
            add(P, 1, 300, 288, k2, r, 'coded-hot', 0, 0, cm=2)
            add(P, 1, 257, 288, k2, r, 'wide', 1, 0, cm=2)
    # ---- the natural dispatch: t256 = 2 * 97 = 194 >= 192
    add(FAM_PIPELINED, 0, 257, 24584, 128, (256, 256, 2, 4, 64), 'unit', 0, 0, tile=0)
    add(FAM_PIPELINED, 0, 257, 24584, 128, (256, 256, 2, 4, 64), 'coded-hot', 2, 1, tile=0)

    # ---- gemm_bf16s_kernel (t256 < 192: the dispatch of gemm_bf16_stored stays in its file)
    T = FAM_STORED
    every = [(a, r) for a in range(4) for r in (0, 1)]
    bk = lambda K: 64 if K % 64 == 0 else 32
    for K in (64, 96):
        small, big = (64, 64, 2, 2, bk(K)), (128, 128, 2, 4, bk(K))
        for act, resid in every:
            add(T, 0, 333, 200, K, small, 'unit', act, resid)
            add(T, 0, 200, 14332, K, big, 'unit', act, resid)        # t128 = 2 * 112 = 224
        for act in range(4):
            add(T, 0, 333, 200, K, small, 'unit', act, 0, cm=1)
            add(T, 0, 200, 14336, K, big, 'unit', act, 0, cm=1)
        add(T, 0, 200, 14332, K, big, 'coded-hot', 2, 1)
        add(T, 0, 200, 14332, K, big, 'coded-dense', 0, 0)
    # 1, 2, 3 and 5 K tiles of both widths; a single row
    for K in (32, 64, 128, 192, 96, 160, 320):
        small = (64, 64, 2, 2, bk(K))
        add(T, 0, 65, 68, K, small, 'coded-dense', 2, 1)
        add(T, 0, 333, 200, K, small, 'coded-hot', 0, 0)
        add(T, 0, 1, 4, K, small, 'unit', 0, 0)
    add(T, 0, 65, 68, 64, (64, 64, 2, 2, 64), 'wide', 1, 0)
    add(T, 0, 65, 68, 96, (64, 64, 2, 2, 32), 'wide', 3, 0)
    add(T, 0, 65, 72, 64, (64, 64, 2, 2, 64), 'coded-dense', 2, 0, cm=1)
    add(T, 0, 333, 200, 160, (64, 64, 2, 2, 32), 'coded-hot', 0, 0, cm=1)
    # GLU
    for K in (64, 96):
        for N in (64, 128, 192):
            for M in (1, 63, 130):
                if K == 64 or (N, M) == (192, 130):
                    for regime in (('unit', 'coded-hot', 'wide') if M == 63 or N == 192
                                   else ('unit', 'coded-hot')):
                        add(T, 0, M, N, K, (64, 128, 2, 2, bk(K)), regime, 0, 0, glu=True)
        for regime in (('unit', 'coded-hot', 'wide') if K == 64 else ('unit', )):
            add(T, 0, 129, 14272, K, (128, 128, 4, 2, bk(K)), regime, 0, 0, glu=True)
    # the 256x256 stored block: t256 = 2 * 128 = 256 with K >= 2048, and N % 8 != 0, which the
    # pipelined kernel does not take
    add(T, 0, 257, 32764, 2048, (256, 256, 4, 2, 64), 'unit', 0, 0)
    return out


GEMM_LOWP_CASES = _gemm_lowp_cases()


def mx_quantize_case(rows, K, seed=5):
    """x (rows, K): rows scaled over e^+-3, the first min(rows, 6) of them the special rows of
    test_mx_quantize_matches_oracle_bit_for_bit (tests/test_gpu_fp8.py)."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + K)
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 3)
    sp = [x[0].clone() for _ in range(6)]
    sp[0][:32] = 1e-4
    sp[0][0] = 448.0 * 2.0 ** -5                                 # amax on a block-scale boundary
    sp[1][:32] = 1e-4
    sp[1][0] = 449.0 * 2.0 ** 3                                  # just above it
    sp[2][:32] = torch.linspace(-1, 1, 32) * 2.0 ** -12          # e4m3 subnormals after scaling
    sp[2][0] = 1.0
    sp[3][:32] = 0.0                                             # one all-zero block
    sp[4] = torch.randn(K, generator=g) * 1e-30                  # tiny values
    sp[5] = torch.zeros(K)                                       # all-zero blocks
    for r in range(min(rows, 6)):
        x[r] = sp[r]
    return x
