"""CPU checks of tests/kernel_refs.py: every plain fp64 reference against the oracle's module
(oracle/wenet_oracle.py, itself pinned to the unmodified reference) reduced to the bare operator
-- identity projections, zero biases -- to 1e-12 relative, the mask builder against the oracle's
chunk masks, and the cap on the yardstick `e_plain` for every data regime of every operator, so
that all of it is settled before any GPU time is spent."""
import math

import pytest
import torch

import kernel_refs as KR
from oracle import wenet_oracle as O

REL = 1e-12

# every (mask_mode, chunk, left) the GPU tests use
MASKS = [(0, 0, -1), (1, 0, -1)] + [(2, c, l) for c in (1, 4, 16) for l in (-1, 0, 1, 3)]


def _close(a, b):
    s = b.abs().max().item()
    assert (a - b).abs().max().item() <= REL * max(s, 1.0), (a - b).abs().max().item()


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('T', [1, 5, 33, 70])
def test_mask_builder_matches_oracle(mask, T):
    mode, chunk, left = mask
    got = KR.chunk_window(T, T, mode, chunk, left)
    if mode == 0:
        want = torch.ones(T, T, dtype=torch.bool)
    elif mode == 1:
        want = O.subsequent_mask(T)
    else:
        want = O.subsequent_chunk_mask(T, chunk, left)
    assert torch.equal(got, want)


def _identity_attn_sd(d, H, relpos, g):
    eye = torch.eye(d, dtype=torch.float64)
    sd = {}
    for n in ('linear_q', 'linear_k', 'linear_v', 'linear_out'):
        sd['a.' + n + '.weight'] = eye
        sd['a.' + n + '.bias'] = torch.zeros(d, dtype=torch.float64)
    if relpos:
        sd['a.linear_pos.weight'] = eye
        sd['a.pos_bias_u'] = torch.randn(H, 64, generator=g, dtype=torch.float64)
        sd['a.pos_bias_v'] = torch.randn(H, 64, generator=g, dtype=torch.float64)
    return sd


@pytest.mark.parametrize('mask', [(0, 0, -1), (1, 0, -1), (2, 4, 1), (2, 16, -1), (2, 1, 0)])
def test_ref_attention_matches_rel_pos_mha(mask):
    """rel_pos_mha with identity projections: q = k = v = x, P = pos_emb."""
    mode, chunk, left = mask
    g = torch.Generator().manual_seed(1)
    H, T, Tp = 4, 37, 40
    d = H * 64
    x = torch.randn(2, Tp, d, generator=g, dtype=torch.float64)
    pos = torch.randn(1, Tp, d, generator=g, dtype=torch.float64)
    lens = [T, Tp]
    sd = _identity_attn_sd(d, H, True, g)
    pad = ~O.make_pad_mask(torch.tensor(lens), Tp).unsqueeze(1)             # (B, 1, Tp)
    m = pad & KR.chunk_window(Tp, Tp, mode, chunk, left).unsqueeze(0)
    want = O.rel_pos_mha(x, m, pos, sd, 'a.', H)
    rows = x.reshape(2 * Tp, d)
    seqs = [(0, T, 0, T, 0), (Tp, Tp, Tp, Tp, 0)]
    got = KR.ref_attention(rows, rows, rows, pos[0], sd['a.pos_bias_u'], sd['a.pos_bias_v'], seqs,
                           mode, chunk, left, 1.0 / math.sqrt(64))
    for b, n in enumerate(lens):
        _close(got[b * Tp:b * Tp + n], want[b, :n])


def test_ref_attention_matches_mha_cross():
    """mha with identity projections, q_len != kv_len, padded memory."""
    g = torch.Generator().manual_seed(2)
    H, Tq, Tk = 2, 9, 50
    d = H * 64
    qx = torch.randn(2, Tq, d, generator=g, dtype=torch.float64)
    mem = torch.randn(2, Tk, d, generator=g, dtype=torch.float64)
    vmem = mem                      # the module projects key and value from the same tensor
    klens = [Tk, 31]
    sd = _identity_attn_sd(d, H, False, g)
    m = ~O.make_pad_mask(torch.tensor(klens), Tk).unsqueeze(1)
    want = O.mha(qx, mem, vmem, m, sd, 'a.', H)
    seqs = [(0, Tq, 0, Tk, 0), (Tq, Tq, Tk, 31, 0)]
    got = KR.ref_attention(qx.reshape(2 * Tq, d), mem.reshape(2 * Tk, d), mem.reshape(2 * Tk, d),
                           None, None, None, seqs, 0, 0, -1, 1.0 / math.sqrt(64))
    _close(got, want.reshape(2 * Tq, d))


@pytest.mark.parametrize('K,causal', [(8, True), (2, True), (15, False), (3, False), (33, False)])
@pytest.mark.parametrize('norm', ['layer_norm', 'batch_norm'])
def test_ref_dwconv_matches_conv_module(K, causal, norm):
    """conv_module with pointwise_conv1 = [identity | gate 50] (GLU(a, 50) == a in fp64, so a
    masked / left-pad frame becomes the bias of the value half: that is `cpad`) and an identity
    pointwise_conv2: what is left is the kernel's operator."""
    g = torch.Generator().manual_seed(K)
    D, Tp = 64, 40
    lens = [Tp, 7, 1, K]
    B = len(lens)
    dd = dict(generator=g, dtype=torch.float64)
    x = torch.randn(B, Tp, D, **dd)
    ca = torch.randn(D, **dd)
    wt = torch.randn(K, D, **dd)
    bias = torch.randn(D, **dd)
    ln_w, ln_b = torch.randn(D, **dd), torch.randn(D, **dd)
    sd = {'c.pointwise_conv1.weight': torch.cat([torch.eye(D, dtype=torch.float64),
                                                 torch.zeros(D, D, dtype=torch.float64)]).unsqueeze(-1),
          'c.pointwise_conv1.bias': torch.cat([ca, torch.full((D, ), 50.0, dtype=torch.float64)]),
          'c.depthwise_conv.weight': wt.t().contiguous().unsqueeze(1),
          'c.depthwise_conv.bias': bias,
          'c.norm.weight': ln_w, 'c.norm.bias': ln_b,
          'c.pointwise_conv2.weight': torch.eye(D, dtype=torch.float64).unsqueeze(-1),
          'c.pointwise_conv2.bias': torch.zeros(D, dtype=torch.float64)}
    if norm == 'batch_norm':
        rm, rv = torch.randn(D, **dd), torch.rand(D, **dd) + 0.5
        sd['c.norm.running_mean'], sd['c.norm.running_var'] = rm, rv
        # eval-mode BatchNorm1d as the per-channel affine the model folds it into
        a = ln_w / torch.sqrt(rv + 1e-5)
        kw, kb, mode = a, ln_b - rm * a, 1
    else:
        kw, kb, mode = ln_w, ln_b, 0
    assert torch.sigmoid(torch.tensor(50.0, dtype=torch.float64)).item() == 1.0
    mask_pad = ~O.make_pad_mask(torch.tensor(lens), Tp).unsqueeze(1)
    want = O.conv_module(x, mask_pad, sd, 'c.', K, causal, torch.nn.functional.silu)
    rows = (x + ca).reshape(B * Tp, D)           # GLU output of a real frame
    off = [b * Tp for b in range(B)]
    got = KR.ref_dwconv(rows, wt, bias, ca, kw, kb, mode, off, lens, K, causal, Tp, 1e-5)
    for b, n in enumerate(lens):
        _close(got[off[b]:off[b] + n], want[b, :n])


@pytest.mark.parametrize('Fdim,cmvn', [(80, True), (7, True), (23, False)])
def test_ref_conv1_matches_subsampling(Fdim, cmvn):
    """global_cmvn + the first Conv2d + ReLU of conv2d_subsampling4."""
    g = torch.Generator().manual_seed(Fdim)
    C, T = 8, 21
    dd = dict(generator=g, dtype=torch.float64)
    feats = torch.randn(2, T, Fdim, **dd) + 11
    mean, istd = torch.randn(Fdim, **dd) + 11, torch.rand(Fdim, **dd) + 0.2
    w, bias = torch.randn(C, 1, 3, 3, **dd), torch.randn(C, **dd)
    x = O.global_cmvn(feats, mean, istd) if cmvn else feats
    want = torch.relu(torch.nn.functional.conv2d(x.unsqueeze(1), w, bias, stride=2))
    # (conv2d_subsampling4 itself goes on into conv.2 / out.0; its first two lines are these)
    got = KR.ref_conv1(feats, mean if cmvn else None, istd if cmvn else None, w, bias, [10, 4])
    _close(got[0], want[0].permute(1, 2, 0)[:10])
    _close(got[1], want[1].permute(1, 2, 0)[:4])


@pytest.mark.parametrize('penalty,blank', [(0.0, 0), (1.5, 0), (1.5, 5)])
def test_ref_ctc_rows_matches_ctc_logprobs(penalty, blank):
    g = torch.Generator().manual_seed(3)
    V = 37
    x = torch.randn(2, 11, V, generator=g, dtype=torch.float64) * 3
    sd = {'ctc.ctc_lo.weight': torch.eye(V, dtype=torch.float64),
          'ctc.ctc_lo.bias': torch.zeros(V, dtype=torch.float64)}
    want = O.ctc_logprobs(sd, x, penalty, blank)
    logp, val, idx = KR.ref_ctc_rows(x.reshape(22, V), blank, penalty, 4)
    _close(logp, want.reshape(22, V))
    wv, wi = want.reshape(22, V).topk(4, dim=1)
    assert torch.equal(idx, wi)
    _close(val, wv)


# ---- the yardstick's cap, regime by regime ----------------------------------------------------


def _attn_kw(shape):
    if shape == 'plain_129':
        return dict(H=1, q_lens=[129])
    if shape == 'relpos_packed':
        return dict(H=4, q_lens=[65, 0, 129, 33], relpos=True)
    if shape == 'relpos_chunk':
        return dict(H=2, q_lens=[130, 31], relpos=True, mask_mode=2, chunk=16, left=1)
    if shape == 'causal':
        return dict(H=2, q_lens=[100, 2], mask_mode=1)
    if shape == 'cross':
        return dict(H=2, q_lens=[1, 40], kv_lens=[300, 77])
    raise ValueError(shape)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape', ['plain_129', 'relpos_packed', 'relpos_chunk', 'causal', 'cross'])
@pytest.mark.parametrize('regime', KR.ATTENTION_REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_attention_regime_caps(regime, shape, bf16):
    case = KR.regime_case(regime[0], regime[1], bf16=bf16, seed=11, **_attn_kw(shape))
    ref, e, scale, w = KR.attention_refs(case, bf16)
    assert torch.isfinite(ref).all()
    assert KR.cap_ok(e, scale, bf16), (e / scale)
    masked_needle = regime[0] == 'needle' and regime[1] != 'last_visible' and \
        (case['mask_mode'] != 0 or not case['self_attn'])
    if regime in KR.NON_FLAT and not masked_needle and not bf16:
        share = (w > 0.5).double().mean().item()
        assert share >= KR.NON_FLAT[regime], share
    if regime[0] == 'unit':
        assert (w > 0.5).double().mean().item() < 0.2     # today's regime: flat softmaxes
    if regime[0] == 'tied':
        # the one regime whose answer needs no softmax: the mean of the visible value rows
        for (qo, ql, ko, kl, _) in case['seqs']:
            if ql == 0:
                continue
            vis = KR.chunk_window(ql, kl, case['mask_mode'], case['chunk'], case['left']).double()
            mean = (vis / vis.sum(1, keepdim=True)) @ case['v'][ko:ko + kl].double()
            assert (ref[qo:qo + ql] - mean).abs().max().item() <= 1e-12 * scale


@pytest.mark.parametrize('T', [1500])
@pytest.mark.parametrize('regime', [('peaked', 30.0), ('ascending', 1.0), ('descending', 0.375),
                                    ('shifted', 80.0), ('needle', 'second_half')],
                         ids=lambda r: f'{r[0]}-{r[1]}')
def test_attention_regime_caps_long(regime, T):
    for bf16 in (False, True):
        case = KR.regime_case(regime[0], regime[1], bf16=bf16, seed=5, H=1, q_lens=[T], relpos=True)
        ref, e, scale, _ = KR.attention_refs(case, bf16)
        assert KR.cap_ok(e, scale, bf16), (bf16, e / scale)


@pytest.mark.parametrize('D,K,causal', [(256, 8, True), (1280, 33, False), (64, 2, True),
                                        (768, 17, False)])
@pytest.mark.parametrize('norm_mode', [0, 1])
@pytest.mark.parametrize('offset', [0.0, 50.0])
def test_dwconv_regime_caps(D, K, causal, norm_mode, offset):
    c = KR.make_dwconv_case(D, K, causal, norm_mode, [1, 2, 3, 4, 5, max(K - 1, 1), K, K + 1, 100],
                            seed=D + K, t_extra=3, offset=offset)
    ref, e, scale = KR.dwconv_refs(c)
    assert torch.isfinite(ref).all() and KR.cap_ok(e, scale), e / scale


@pytest.mark.parametrize('Fdim', [7, 23, 80, 127, 128])
@pytest.mark.parametrize('cmvn', [True, False])
def test_conv1_regime_caps(Fdim, cmvn):
    c = KR.make_conv1_case(Fdim, 64, [17, 0, 1, 16], cmvn=cmvn, seed=Fdim)
    ref, e, scale = KR.conv1_refs(c)
    assert KR.cap_ok(e, scale), e / scale


@pytest.mark.parametrize('V', [1, 2, 65, 4233, 30720])
@pytest.mark.parametrize('regime', ['randn', 'shift_up', 'shift_down', 'spread', 'ties'])
def test_ctc_regime_caps(regime, V):
    x = KR.make_ctc_case(regime, 5, V, blank=0, seed=V)
    logp, val, idx, e, scale = KR.ctc_refs(x, 0, 1.5, min(4, V))
    assert torch.isfinite(logp).all()
    if V > 1:                        # (V = 1: the row is exactly 0, nothing to scale by)
        assert KR.cap_ok(e, scale), e / scale
    else:
        assert e == 0.0
