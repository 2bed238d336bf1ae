"""CPU checks of tests/kernel_refs.py: every plain fp64 reference against the oracle's module
(oracle/wenet_oracle.py, itself pinned to the unmodified reference) reduced to the bare operator
-- identity projections, zero biases -- to 1e-12 relative, the mask builder against the oracle's
chunk masks, and the cap on the yardstick `e_plain` for every data regime of every operator, so
that all of it is settled before any GPU time is spent.  At the end: the NumPy statements of the
attention search's beam kernels against the reference's step and final selection, restated in
torch from its text, and the invariant of the path rows."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

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


# ---- the `attention` decode mode (csrc/attn_search.hip) ----------------------------------------
# The torch functions below restate the reference's step and its final selection line by line
# (wenet/models/transformer/search.py and wenet/utils/mask.py at the cited lines), as the oracle
# restates its modules; `logp.topk` is replaced by the top-k tables the caller hands in.


def _mask_finished_scores(score, flag):                      # mask.py:258-285
    beam_size = score.size(-1)
    zero_mask = torch.zeros_like(flag, dtype=torch.bool)
    if beam_size > 1:
        unfinished = torch.cat((zero_mask, flag.repeat([1, beam_size - 1])), dim=1)
        finished = torch.cat((flag, zero_mask.repeat([1, beam_size - 1])), dim=1)
    else:
        unfinished = zero_mask
        finished = flag
    score.masked_fill_(unfinished, -float('inf'))
    score.masked_fill_(finished, 0)
    return score


def _mask_finished_preds(pred, flag, eos):                   # mask.py:288-304
    return pred.masked_fill_(flag.repeat([1, pred.size(-1)]), eos)


def _search_step(hyps, scores, end_flag, top_k_logp, top_k_index, batch_size, beam_size, eos):
    """search.py:315-354 (the cache re-gather of :323-331 left out: it has no output here)."""
    top_k_logp = _mask_finished_scores(top_k_logp.clone(), end_flag)
    top_k_index = _mask_finished_preds(top_k_index.clone(), end_flag, eos)
    scores = scores + top_k_logp
    scores = scores.view(batch_size, beam_size * beam_size)
    scores, offset_k_index = scores.topk(k=beam_size)
    scores = scores.view(-1, 1)
    base_k_index = torch.arange(batch_size).view(-1, 1).repeat([1, beam_size])
    base_k_index = base_k_index * beam_size * beam_size
    best_k_index = base_k_index.view(-1) + offset_k_index.view(-1)
    best_k_pred = torch.index_select(top_k_index.view(-1), dim=-1, index=best_k_index)
    best_hyps_index = best_k_index // beam_size
    last_best_k_hyps = torch.index_select(hyps, dim=0, index=best_hyps_index)
    hyps = torch.cat((last_best_k_hyps, best_k_pred.view(-1, 1)), dim=1)
    end_flag = torch.eq(hyps[:, -1], eos).view(-1, 1)
    return hyps, scores, end_flag


def _search_finish(hyps, scores, batch_size, beam_size, eos, length_penalty, prefix_len):
    """search.py:357-370."""
    scores = scores.view(batch_size, beam_size)
    lengths = hyps.ne(eos).sum(dim=1).view(batch_size, beam_size).float()
    scores = scores / lengths.pow(length_penalty)
    best_scores, best_index = scores.max(dim=-1)
    best_hyps_index = best_index + torch.arange(batch_size, dtype=torch.long) * beam_size
    best_hyps = torch.index_select(hyps, dim=0, index=best_hyps_index)
    best_hyps = best_hyps[:, prefix_len:]
    return [h[h != eos].tolist() for h in best_hyps]


def _topk_tables(rng, BN, N, V, eos, p_eos=0.15):
    """Top-k tables of one step: descending log-probs without repeated values, distinct tokens
    per row, <eos> among them now and then."""
    topv = -np.sort(rng.uniform(0.05, 9.0, (BN, N)), axis=1).astype(np.float32)
    topi = np.stack([rng.choice(V, N, replace=False) for _ in range(BN)]).astype(np.int32)
    for r in range(BN):
        if rng.random() < p_eos and eos not in topi[r]:
            topi[r, rng.integers(N)] = eos
    return topv, topi


def _untied(st, topv, N):
    """No two of the N + 1 best candidates of any utterance are equal (the reference's topk
    leaves the order of equal values open)."""
    ended = st['end'] != 0
    lp = topv.copy()
    lp[ended, 1:] = -np.inf
    lp[ended, 0] = 0.0
    cand = (st['score'][:, None] + lp).reshape(-1, N * N)
    top = -np.sort(-cand, axis=1)[:, :N + 1]
    return bool(np.all(top[:, :-1] > top[:, 1:])) if N * N > 1 else True


@pytest.mark.parametrize('B,N,prompt_len', [(1, 1, 0), (2, 2, 0), (3, 3, 0), (2, 10, 0), (1, 33, 0),
                                            (2, 4, 3), (1, 10, 4)])
def test_ref_beam_update_matches_reference_step(B, N, prompt_len):
    """init + 9 steps: scores bit for bit, token rows, end flags against the reference's step."""
    rng = np.random.default_rng(100 * B + N)
    V, eos, sos, steps = max(2 * N, 11), 2, 1, 9
    BN = B * N
    prompt = rng.integers(3, V, (B, prompt_len)).astype(np.int32) if prompt_len else None
    first = prompt_len if prompt_len else 1
    max_len = first + steps + 2
    st = KR.ref_beam_init(B, N, max_len, sos=sos, prompt=prompt)
    if prompt_len:
        hyps = torch.from_numpy(np.repeat(prompt, N, axis=0)).long()
    else:
        hyps = torch.ones([BN, 1], dtype=torch.long).fill_(sos)                  # search.py:287
    scores = torch.tensor([0.0] + [-float('inf')] * (N - 1),
                          dtype=torch.float).repeat([B]).unsqueeze(1)            # :290-293
    end_flag = torch.zeros_like(scores, dtype=torch.bool)
    assert np.array_equal(st['score'], scores.view(-1).numpy())
    assert np.array_equal(st['tok'][:, :first], hyps.numpy())
    n_ended = 0
    for i in range(first, first + steps):
        topv, topi = _topk_tables(rng, BN, N, V, eos)
        assert _untied(st, topv, N)
        st, done = KR.ref_beam_update(st, topv, topi, B, N, i, eos, V, shared_row=i == prompt_len)
        hyps, scores, end_flag = _search_step(hyps, scores, end_flag, torch.from_numpy(topv),
                                              torch.from_numpy(topi).long(), B, N, eos)
        assert np.array_equal(st['score'].view(np.int32), scores.view(-1).numpy().view(np.int32))
        assert np.array_equal(st['tok'][:, :i + 1], hyps.numpy())
        assert np.array_equal(st['end'] != 0, end_flag.view(-1).numpy())
        assert np.array_equal(st['last_tok'], hyps[:, -1].numpy())
        assert done == int(end_flag.sum())
        assert bool((st['tok'][:, i + 1:] == KR.FILL).all())
        assert bool((st['path'][:, i + 1:] == KR.FILL).all())
        n_ended = max(n_ended, done)
    assert n_ended > 0 or N == 1                 # the masks of finished hypotheses were in play


def test_ref_beam_update_ties_by_hand():
    """The rule on exact ties and on NaN, the winners spelled out."""
    eos, V = 2, 9
    ti = np.array([[5, 6], [7, 8]], np.int32)

    def run(score, end, topv, topi=ti):
        st = dict(score=np.array(score, np.float32), end=np.array(end, np.int32),
                  tok=np.array([[1, 3, 0], [1, 4, 0]], np.int32),
                  path=np.array([[0, 0, 0], [1, 0, 0]], np.int32))
        out, done = KR.ref_beam_update(st, np.array(topv, np.float32), topi, 1, 2, 2, eos, V)
        return out, done

    inf, nan = float('inf'), float('nan')
    # the first step: slot 1 is -inf; flat 0, 1 win (parent 0 twice)
    out, done = run([0, -inf], [0, 0], [[-1, -2], [-1, -2]])
    assert out['score'].tolist() == [-1, -2] and out['last_tok'].tolist() == [5, 6]
    assert out['tok'].tolist() == [[1, 3, 5], [1, 3, 6]] and done == 0
    assert out['path'].tolist() == [[0, 0, 0], [0, 0, 1]]
    # duplicated candidates across parents: -2 (flat 0), -2 (flat 2); the lower flat index first
    out, _ = run([-1, -1], [0, 0], [[-1, -2], [-1, -2]])
    assert out['score'].tolist() == [-2, -2] and out['last_tok'].tolist() == [5, 7]
    assert out['tok'].tolist() == [[1, 3, 5], [1, 4, 7]]
    assert out['path'].tolist() == [[0, 0, 0], [1, 1, 1]]
    # three equal candidates: flat 0, 1 win over flat 2
    out, _ = run([-1, -1.5], [0, 0], [[-1, -1], [-0.5, -3]])
    assert out['score'].tolist() == [-2, -2] and out['last_tok'].tolist() == [5, 6]
    # both parents ended, equal scores: each keeps its one live branch, in slot order
    out, done = run([-3, -3], [1, 1], [[-1, -2], [-1, -2]])
    assert out['score'].tolist() == [-3, -3] and out['last_tok'].tolist() == [eos, eos]
    assert out['tok'].tolist() == [[1, 3, eos], [1, 4, eos]] and done == 2
    # one parent ended and better than every live candidate; its dead branch (-inf) loses
    out, done = run([-0.5, -1], [1, 0], [[-1, -2], [-1, -2]])
    assert out['score'].tolist() == [-0.5, -2] and out['last_tok'].tolist() == [eos, 7]
    assert done == 1
    # tokens outside [0, V) end the hypothesis
    out, done = run([0, -1], [0, 0], [[-1, -2], [-9, -9]],
                    np.array([[-1, 0x7fffffff], [7, 8]], np.int32))
    assert out['last_tok'].tolist() == [eos, eos] and done == 2
    out, _ = run([0, -1], [0, 0], [[-1, -9], [-9, -9]], np.array([[V, 3], [7, 8]], np.int32))
    assert out['last_tok'].tolist()[0] == eos
    # one parent's row NaN: its candidates count as -inf, the clean parent takes both slots
    out, _ = run([-1, -1], [0, 0], [[nan, nan], [-1, -2]])
    assert out['score'].tolist() == [-2, -3] and out['last_tok'].tolist() == [7, 8]
    # every candidate NaN: flat 0, 1 with -inf
    out, done = run([-1, -1], [0, 0], [[nan, nan], [nan, nan]],
                    np.full((2, 2), 0x7fffffff, np.int32))
    assert out['score'].tolist() == [-inf, -inf] and out['last_tok'].tolist() == [eos, eos]
    assert out['tok'].tolist() == [[1, 3, eos], [1, 3, eos]] and done == 2


@pytest.mark.parametrize('nn', [1, 4, 9, 100, 4096])
def test_beam_rank_is_a_permutation_for_every_input(nn):
    """With NaN -> -inf the counting rule of beam_update_kernel (rank = number of candidates that
    are larger, or equal with a lower flat index) is a permutation; without it every NaN gets
    rank 0."""
    rng = np.random.default_rng(nn)
    for kind in ('random', 'nan_some', 'nan_all', 'inf_all', 'dup'):
        c = rng.standard_normal(nn).astype(np.float32)
        if kind == 'nan_some':
            c[rng.random(nn) < 0.4] = np.nan
        elif kind == 'nan_all':
            c[:] = np.nan
        elif kind == 'inf_all':
            c[:] = -np.inf
        elif kind == 'dup':
            c = np.round(c)
        v = np.where(np.isnan(c), np.float32(-np.inf), c)
        idx = np.arange(nn)
        rank = ((v[None, :] > v[:, None]) |
                ((v[None, :] == v[:, None]) & (idx[None, :] < idx[:, None]))).sum(1)
        assert sorted(rank.tolist()) == list(range(nn)), kind
        N = int(round(nn ** 0.5))
        assert np.array_equal(np.argsort(rank)[:N], KR.beam_rank(c, N)), kind
    c = np.full(nn, np.nan, np.float32)
    raw = ((c[None, :] > c[:, None]) | ((c[None, :] == c[:, None]))).sum(1)
    assert (raw == 0).all()


@pytest.mark.parametrize('B,N,prompt_len', [(2, 3, 0), (3, 10, 0), (2, 4, 3), (1, 33, 5)])
def test_beam_paths_name_the_slot_that_held_the_prefix(B, N, prompt_len):
    """After init (both kinds) and a chain of updates: for every row c and position j, the slot
    path[c][j] held, when position j was computed (the decoder step on rows of j + 1 tokens, or
    the prompt prefill in the utterance's first slot), exactly tok[c][:j + 1]."""
    rng = np.random.default_rng(7 * B + N)
    V, eos, sos, steps = 2 * N + 5, 2, 1, 12
    BN = B * N
    prompt = rng.integers(3, V, (B, prompt_len)).astype(np.int32) if prompt_len else None
    first = prompt_len if prompt_len else 1
    max_len = first + steps + 2
    st = KR.ref_beam_init(B, N, max_len, sos=sos, prompt=prompt)
    held = {}                                   # (position, slot) -> the token prefix it computed
    for b in range(B):
        for j in range(prompt_len):             # the prefill: utterance b's first slot
            held[(j, b * N)] = tuple(prompt[b, :j + 1])

    def check(st, n_tok):
        for c in range(BN):
            for j in range(n_tok):
                assert held[(j, int(st['path'][c, j]))] == tuple(st['tok'][c, :j + 1]), (c, j)

    check(st, prompt_len)
    for i in range(first, first + steps):
        if i != prompt_len:                     # the step on rows of i tokens computes position i - 1
            for r in range(BN):
                assert st['path'][r, i - 1] == r
                held[(i - 1, r)] = tuple(st['tok'][r, :i])
        topv, topi = _topk_tables(rng, BN, N, V, eos)
        st, _ = KR.ref_beam_update(st, topv, topi, B, N, i, eos, V, shared_row=i == prompt_len)
        check(st, i)
        assert np.array_equal(st['path'][:, i], np.arange(BN))


@pytest.mark.parametrize('length_penalty', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('prefix', [1, 4])
@pytest.mark.parametrize('B,N', [(3, 1), (3, 10), (3, 64)])
def test_ref_beam_finish_matches_reference(B, N, prefix, length_penalty):
    """Every draw the GPU test uses: the margin that makes fp32 powf irrelevant holds for all of
    them (none is rejected), and the NumPy statement gives the reference's answer."""
    eos = 2
    score, tok, length = KR.make_beam_finish_case(B, N, prefix, seed=N + prefix, eos=eos)
    s = KR.beam_finish_scores(score, tok, B, N, length, eos, length_penalty)
    assert all(KR.beam_finish_margin_ok(s[b]) for b in range(B))
    out_tok, out_len, best = KR.ref_beam_finish(score, tok, B, N, length, eos, length_penalty,
                                                prefix)
    want = _search_finish(torch.from_numpy(tok[:, :length]).long(), torch.from_numpy(score), B, N,
                          eos, length_penalty, prefix)
    for b in range(B):
        assert out_tok[b, :out_len[b]].tolist() == want[b]
        assert bool((out_tok[b, out_len[b]:] == KR.FILL).all())


def test_ref_beam_finish_edges():
    """sos == eos (WeNet models): the count of [sos, eos] is 0, the penalised score -x / 0 = -inf
    for a positive penalty; every row like that: row 0, length 0, as the reference's max gives.
    Two best rows of equal score and count: the first."""
    eos = 2
    tok = np.array([[eos, eos, 0], [eos, eos, 0], [eos, eos, 0]], np.int32)
    score = np.array([-3, -1, -2], np.float32)
    for lp in (0.3, 1.0):
        out_tok, out_len, best = KR.ref_beam_finish(score, tok, 1, 3, 2, eos, lp, 1)
        assert best.tolist() == [0] and out_len.tolist() == [0]
        assert _search_finish(torch.from_numpy(tok[:, :2]).long(), torch.from_numpy(score), 1, 3,
                              eos, lp, 1) == [[]]
    # penalty 0: 0 ** 0 = 1, the scores decide; the answer is empty either way
    out_tok, out_len, best = KR.ref_beam_finish(score, tok, 1, 3, 2, eos, 0.0, 1)
    assert best.tolist() == [1] and out_len.tolist() == [0]
    tok = np.array([[eos, 5, eos], [eos, 7, 8], [eos, 8, 7], [eos, 9, 9]], np.int32)
    score = np.array([-4, -2, -2, -2.5], np.float32)
    for lp in (0.0, 0.3, 1.0):
        out_tok, out_len, best = KR.ref_beam_finish(score, tok, 1, 4, 3, eos, lp, 1)
        assert best.tolist() == [1] and out_tok[0, :2].tolist() == [7, 8]
        assert _search_finish(torch.from_numpy(tok).long(), torch.from_numpy(score), 1, 4, eos,
                              lp, 1) == [[7, 8]]


@pytest.mark.parametrize('length', [129, 200])
@pytest.mark.parametrize('regime', KR.SELF_STEP_REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_self_step_regime_caps(regime, length):
    """The cap on the yardstick and the weight shares of the step cases the GPU test runs, and the
    case's own layout: named cache rows hold the sequence data, every other row the poison."""
    case = KR.make_self_step_case(regime[0], regime[1], H=4, n=5, length=length, seed=51)
    ref, e, scale, w = KR.self_step_refs(case)
    assert torch.isfinite(ref).all() and KR.cap_ok(e, scale), e / scale
    if regime in KR.SELF_STEP_NON_FLAT:
        assert (w > 0.5).double().mean().item() >= KR.SELF_STEP_NON_FLAT[regime]
    if regime[0] == 'unit':
        assert (w > 0.5).double().mean().item() < 0.2
    cache, named, step = case['cache'], case['named'], case['step']
    assert bool((cache[~named].abs() == KR.POISON).all()) and not bool(named[step:].any())
    assert bool((cache[named].abs() < 1e3).all())
    for r in range(case['n']):
        for j in range(step):
            row = cache[j, case['path'][r, j]]
            assert torch.equal(row[:case['d']], case['kg'][r * length + j])
            assert torch.equal(row[case['d']:], case['vg'][r * length + j])
        assert torch.equal(case['qkv'][r, case['d']:2 * case['d']], case['kg'][r * length + step])
    if regime[0] == 'tied':
        mean = case['vg'].double().view(case['n'], length, -1).mean(1)
        assert (ref - mean).abs().max().item() <= 1e-12 * scale


# ---------------------------------------------------------------------------------------------
# the front ends behind conv1 (tests/test_gpu_frontend.py)


@pytest.mark.parametrize('F_in,d', [(23, 64), (81, 64), (80, 128)])
def test_frontend_steps_compose_to_the_oracle_chain(F_in, d):
    """ref_conv1 -> ref_conv2 -> ref_sub_out, the three plain steps, against the oracle's
    global_cmvn + conv2d_subsampling4 on the same utterances."""
    _, sd = KR.frontend_model_parts(F_in, d)
    lens = [7, 6, 10, 11, 0, 75, 40]
    feats = KR.make_frontend_feats(lens, F_in, seed=3)
    l2 = KR.sub4_lens(lens)
    pfx = 'encoder.embed.'
    c1 = KR.ref_conv1(feats, sd['encoder.global_cmvn.mean'], sd['encoder.global_cmvn.istd'],
                      sd[pfx + 'conv.0.weight'], sd[pfx + 'conv.0.bias'],
                      [2 * n + 1 if n else 0 for n in l2])
    want = KR.ref_frontend_chain(feats, lens, sd, d)
    for b, n in enumerate(l2):
        assert want[b].shape == (n, d)
        if n == 0:
            continue
        c2 = KR.ref_conv2(c1[b], sd[pfx + 'conv.2.weight'], sd[pfx + 'conv.2.bias'])
        assert c2.shape == (n, ((F_in - 1) // 2 - 1) // 2, d)
        _close(KR.ref_sub_out(c2, sd[pfx + 'out.0.weight'], sd[pfx + 'out.0.bias'], d), want[b])


@pytest.mark.parametrize('F_in,d', [(23, 64), (80, 64)])
def test_frontend_chain_per_utterance_equals_the_padded_batch(F_in, d):
    """The per-utterance evaluation on the first 4 l2 + 3 frames against conv2d_subsampling4 on
    the whole batch, padded as the reference pads it (sorted by length, zeros behind), at the
    frames its mask keeps: the kept frames read nothing at or beyond frame 4 l2 + 3."""
    _, sd = KR.frontend_model_parts(F_in, d)
    g = torch.Generator().manual_seed(5)
    raw = [(torch.randn(n, F_in, generator=g) * 3.0 + 11.0).numpy()
           for n in (7, 9, 10, 11, 12, 30, 61, 8)]
    padded, lens, _ = O.padding(raw)
    T = padded.shape[1]
    sd64 = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    mask = ~O.make_pad_mask(lens, T).unsqueeze(1)
    x = O.global_cmvn(padded.double(), sd64['encoder.global_cmvn.mean'],
                      sd64['encoder.global_cmvn.istd'])
    want, _, m = O.conv2d_subsampling4(x, mask, sd64, 'encoder.embed.', d)
    keep = m.squeeze(1).sum(1).tolist()
    assert keep == KR.sub4_lens(lens.tolist())
    got = KR.ref_frontend_chain(padded, lens.tolist(), sd, d)
    # ... and the frames behind 4 l2 + 3 may hold anything
    poisoned = padded.clone()
    for b, n in enumerate(keep):
        poisoned[b, 4 * n + 3:] = KR.POISON
    got_p = KR.ref_frontend_chain(poisoned, lens.tolist(), sd, d)
    for b, n in enumerate(keep):
        _close(got[b], want[b, :n])
        assert torch.equal(got[b], got_p[b])


def test_sub4_lens_is_the_reference_mask():
    lens = torch.arange(0, 40)
    m = ~O.make_pad_mask(lens, 40).unsqueeze(1)
    assert m[:, :, 2::2][:, :, 2::2].squeeze(1).sum(1).tolist() == KR.sub4_lens(lens.tolist())


@pytest.mark.parametrize('F_in,d', [(23, 64), (80, 256)])
def test_frontend_yardstick_is_inside_the_cap(F_in, d):
    """frontend_refs on CPU stand-ins for the GPU's c1 / c2 (the fp32 evaluation of the previous
    step): e_plain of all three comparisons inside the cap, and far inside (< 1e-5 of the
    scale: what makes these tests three orders tighter than the whole-encoder ones)."""
    _, sd = KR.frontend_model_parts(F_in, d)
    lens = [7, 6, 10, 11, 0, 75, 120]
    feats = KR.make_frontend_feats(lens, F_in, seed=4)
    l2 = KR.sub4_lens(lens)
    pfx = 'encoder.embed.'
    c1 = KR.ref_conv1(feats, sd['encoder.global_cmvn.mean'], sd['encoder.global_cmvn.istd'],
                      sd[pfx + 'conv.0.weight'], sd[pfx + 'conv.0.bias'],
                      [2 * n + 1 if n else 0 for n in l2], fp32=True)
    c1 = [t.float() for t in c1]
    c2 = [KR.ref_conv2(t, sd[pfx + 'conv.2.weight'], sd[pfx + 'conv.2.bias'], fp32=True).float()
          if t.numel() else torch.zeros(0) for t in c1]
    refs, utts = KR.frontend_refs(feats, lens, sd, d, c1, c2)
    assert utts == [0, 2, 3, 5, 6]
    for name in ('c2', 'x_proj', 'x_chain'):
        ref, e, s = refs[name]
        assert [r.shape[0] for r in ref] == [l2[b] for b in utts]
        assert s > 0 and KR.cap_ok(e, s) and 0 < e < 1e-5 * s, (name, e, s)


@pytest.mark.parametrize('F_in,T', [(80, 12), (128, 13)])
def test_whisper_frontend_reference(F_in, T):
    """sub2_lens against the reference's mask (asserted inside ref_whisper_frontend), the shapes
    and the cap on the yardstick."""
    _, sd = KR.frontend_model_parts(F_in, 384, whisper=True)
    lens = [T, 0, 1, 2, 3, T - 1, 7]
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(len(lens), T, F_in, generator=g)
    for b, n in enumerate(lens):
        feats[b, n:] = 0.0
    ref, e, s = KR.whisper_frontend_refs(feats, lens, sd)
    assert [r.shape[0] for r in ref] == KR.sub2_lens(lens, T)
    assert s > 0 and KR.cap_ok(e, s)


# ---- the kernels that own a complete row (tests/test_gpu_rows.py) ------------------------------

# every width of the layernorm launcher; the GPU tests run all five regimes at 192, 256, 640
LN_WIDTHS = [64, 128, 192, 256, 384, 512, 640, 768, 1024, 1280]


def _ln_f32(x, w, b, eps, form):
    """fp32 restatements of a LayerNorm row kernel.  'recip': the kernel's own arithmetic (sum
    times 1.0f / D, 1.0f / sqrtf); 'one_pass': variance as E[x^2] - mean^2; 'eps_outside': eps
    added to the standard deviation instead of the variance."""
    x, w, b = x.float(), w.float(), b.float()
    D = x.shape[-1]
    inv = torch.tensor(1.0 / D, dtype=torch.float32)
    mean = x.sum(-1, keepdim=True) * inv
    d = x - mean
    if form == 'one_pass':
        var = (x * x).sum(-1, keepdim=True) * inv - mean * mean
    else:
        var = (d * d).sum(-1, keepdim=True) * inv
    if form == 'eps_outside':
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    return (d * rstd * w + b).double()


def test_ref_layernorm_is_torch_layer_norm():
    c = KR.make_rows_case('unit', 9, 192, seed=3)
    want = torch.nn.functional.layer_norm(c['x'].double(), (192, ), c['w'].double(),
                                          c['b'].double(), c['eps'])
    _close(KR.ref_layernorm(c['x'], c['w'], c['b'], c['eps']), want)


@pytest.mark.parametrize('D', LN_WIDTHS)
@pytest.mark.parametrize('regime', KR.ROW_REGIMES)
def test_rows_regime_caps_and_reciprocal_form(regime, D):
    """The yardstick is inside its cap for every regime, width and row count of the GPU tests,
    and a correct fp32 kernel -- the reciprocal form the kernels use -- is inside the bound."""
    for M in (1, 4, 5, 37):
        c = KR.make_rows_case(regime, M, D, seed=D + M)
        ref, e, scale = KR.rows_refs(c)
        assert torch.isfinite(ref).all() and scale > 0 and KR.cap_ok(e, scale), (M, e / scale)
        err = (_ln_f32(c['x'], c['w'], c['b'], c['eps'], 'recip') - ref).abs().max().item()
        assert err <= KR.bound(e, scale), (M, err, KR.bound(e, scale))
        ref2, e2, scale2 = KR.rows2_refs(c)
        assert KR.cap_ok(e2, scale2), (M, e2 / scale2)


@pytest.mark.parametrize('D', [64, 192, 256, 640, 1280])
def test_rows_offset_regime_catches_a_one_pass_variance(D):
    c = KR.make_rows_case('offset', 37, D, seed=D)
    ref, e, scale = KR.rows_refs(c)
    err = (_ln_f32(c['x'], c['w'], c['b'], c['eps'], 'one_pass') - ref).abs().max().item()
    assert not err <= KR.bound(e, scale), (err, KR.bound(e, scale))


@pytest.mark.parametrize('D', [64, 192, 256, 640, 1280])
def test_rows_small_regime_catches_eps_outside_the_root(D):
    c = KR.make_rows_case('small', 37, D, seed=D)
    ref, e, scale = KR.rows_refs(c)
    err = (_ln_f32(c['x'], c['w'], c['b'], c['eps'], 'eps_outside') - ref).abs().max().item()
    assert not err <= KR.bound(e, scale), (err, KR.bound(e, scale))


@pytest.mark.parametrize('D', [256, 512])
def test_x3_decode_returns_the_planes_of_an_image(D):
    """An image laid out record by record from the layout's text (csrc/x6.h: records of 32 rows x
    16 k per (k block, row tile, plane), halves of 8 k, 16 bytes per row and half), filled with
    the oracle's planes."""
    M = 37
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * 3.0
    planes = [p.numpy() for p in O.x6_planes(x)]
    tiles = (M + 31) // 32
    img = np.full(KR.x3_image_bytes(M, D), 0xA5, np.uint8)
    assert img.size == (D // 16) * tiles * 3 * 1024
    for kb in range(D // 16):
        for tile in range(tiles):
            for pl in range(3):
                rec = ((kb * tiles + tile) * 3 + pl) * 1024
                for h in range(2):
                    for r in range(32):
                        row = tile * 32 + r
                        if row >= M:
                            continue
                        v = planes[pl][row, 16 * kb + 8 * h:16 * kb + 8 * h + 8]
                        u16 = (v.view(np.uint32) >> 16).astype(np.uint16)
                        assert ((v.view(np.uint32) & 0xffff) == 0).all()     # bf16 values
                        at = rec + h * 512 + r * 16
                        img[at:at + 16] = u16.view(np.uint8)
    got = KR.x3_decode(img, M, D)
    for pl in range(3):
        np.testing.assert_array_equal(got[pl].view(np.uint32), planes[pl].view(np.uint32))
    # the offsets name every byte of the rows < M once and nothing else
    off = KR.x3_offsets(M, D)
    owned = np.zeros(img.size, np.int32)
    np.add.at(owned, off.reshape(-1), 1)
    np.add.at(owned, off.reshape(-1) + 1, 1)
    assert owned.max() == 1 and owned.sum() == 3 * M * D * 2
    assert (img[owned == 0] == 0xA5).all()


@pytest.mark.parametrize('D', [256, 512])
def test_ref_ffn_reduce_modes(D):
    c = KR.make_ffn_reduce_case(5, D, 9, 0.5, seed=D)
    args = (c['x'], c['P'], c['fb2'], c['alpha'], c['w'], c['b'], c['w2'], c['b2'], c['eps'])
    x_new = c['x'].double() + 0.5 * (c['P'].double().sum(0) + c['fb2'].double())
    x0, y0 = KR.ref_ffn_reduce(*args, 0)
    _close(x0, x_new)
    _close(y0, KR.ref_layernorm(x_new, c['w'], c['b'], c['eps']))
    x1, y1 = KR.ref_ffn_reduce(*args, 1)
    assert torch.equal(x1, KR.ref_layernorm(x0, c['w'], c['b'], c['eps']))
    assert torch.equal(y1, KR.ref_layernorm(KR.ref_layernorm(x0, c['w'], c['b'], c['eps']),
                                            c['w2'], c['b2'], c['eps']))
    x2, y2 = KR.ref_ffn_reduce(*args, 2)
    assert torch.equal(x2, x1) and y2 is None


@pytest.mark.parametrize('D', [256, 512])
@pytest.mark.parametrize('alpha', [0.5, 16.0])
def test_ffn_reduce_caps(D, alpha):
    for S in (1, 9, 32):
        c = KR.make_ffn_reduce_case(9, D, S, alpha, seed=D + S)
        for mode in (0, 1, 2):
            _, ex, ey = KR.ffn_reduce_refs(c, mode)
            assert KR.cap_ok(*ex) and (ey is None or KR.cap_ok(*ey)), (S, mode, ex, ey)


@pytest.mark.parametrize('K', [96, 128, 256, 512])
def test_gemm_rowln_caps(K):
    c = KR.make_gemm_rowln_case(95, K, seed=K)
    for bias, resid, alpha in ((True, True, 0.5), (False, True, 1.0), (True, False, 1.0),
                               (False, False, 0.5)):
        (x, y), ex, ey = KR.gemm_rowln_refs(c, bias, resid, alpha)
        assert x.shape == y.shape == (95, 256)
        assert KR.cap_ok(*ex) and KR.cap_ok(*ey), (bias, resid, alpha, ex, ey)
    want = c['resid'].double() + 0.5 * (c['A'].double() @ c['W'].double().t() + c['bias'].double())
    (x, y), _, _ = KR.gemm_rowln_refs(c, True, True, 0.5)
    _close(x, want)
    _close(y, KR.ref_layernorm(want, c['ln_w'], c['ln_b'], c['eps']))


def test_oracle_defines_the_scale_of_an_all_zero_mx_block():
    """What test_gpu_rows.py's zero-block case of layernorm_mx relies on: amax = 0 gives the scale
    byte 0 and zero elements."""
    x = torch.randn(3, 256)
    x[:, 64:96] = 0.0
    q, E = O.mx_quantize(x)
    assert (E[:, 2] == 0).all() and (q.view(torch.uint8)[:, 64:96] == 0).all()
    assert (E[:, [0, 1, 3]] > 0).all()


# ---------------------------------------------------------------------------------------------
# the GEMM references (tests/test_gpu_gemm_ops.py): every statement of ref_gemm against a second
# one, and the yardstick of every GPU case


def _gemm_spec_of(kind, prec=0, glu=False, regime='unit', **match):
    for s in KR.GEMM_CASES:
        if (s['kind'], s['prec'], s['glu'], s['regime']) == (kind, prec, glu, regime) and \
                all(s[k] == v for k, v in match.items()):
            return s
    raise KeyError((kind, prec, glu, regime, match))


@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('prec', [0, 1])
def test_ref_gemm_plain_is_linear(prec, act):
    """torch.nn.Linear + the torch.nn activation module, alpha and the residual by hand."""
    c = KR.make_gemm_case(_gemm_spec_of('plain', prec, M=333, act=act, resid=1))
    s = c['spec']
    lin = torch.nn.Linear(c['K'], c['N']).double()
    rnd = KR._r16 if prec else (lambda t: t)
    with torch.no_grad():
        lin.weight.copy_(rnd(c['W']).double())
        lin.bias.copy_(c['bias'].double())
        mod = [torch.nn.Identity(), torch.nn.SiLU(), torch.nn.ReLU(), torch.nn.GELU()][act]
        want = c['resid'].double() + s['alpha'] * mod(lin(rnd(c['A']).double()))
    assert s['alpha'] == 0.5
    _close(KR.ref_gemm(c), want)


@pytest.mark.parametrize('N,M', [(64, 1), (192, 130), (14272, 129)])
def test_ref_gemm_glu_is_the_epilogue_over_the_permuted_weight(N, M):
    """F.glu over [values | gates] == per 64 permuted columns, value j (0..31) times the sigmoid
    of gate 32 + j, at output column 32 * block + j -- the GLU epilogue's own column rule, on the
    weight the kernel gets."""
    c = KR.make_gemm_case(_gemm_spec_of('plain', glu=True, N=N, M=M))
    z = c['A'].double() @ c['W'].double().t() + c['bias'].double()          # permuted columns
    z = z.view(M, N // 64, 2, 32)
    want = (z[:, :, 0] * torch.sigmoid(z[:, :, 1])).reshape(M, N // 2)
    _close(KR.ref_gemm(c), want)
    assert sorted(KR.glu_perm(N // 2).tolist()) == list(range(N))


@pytest.mark.parametrize('prec', [0, 1])
def test_ref_gemm_rows_is_conv1d(prec):
    """The gathered-rows operand == Conv1d(d, N, 3, stride 2) over every utterance's frames."""
    c = KR.make_gemm_case(_gemm_spec_of('rows', prec, M=66, act=0, resid=0))
    s, d = c['spec'], c['d']
    rnd = KR._r16 if prec else (lambda t: t)
    frames = c['buf'].view(-1, d)
    outs, at = [], 1
    for n in s['lens']:
        x = rnd(frames[at:at + n]).double().t().unsqueeze(0)                  # (1, d, n)
        outs.append(F.conv1d(x, rnd(c['w_t']).double(), c['bias'].double(), stride=s['stride'])[0].t())
        at += n + 1
    _close(KR.ref_gemm(c), torch.cat(outs))


@pytest.mark.parametrize('C', [32, 64])
@pytest.mark.parametrize('prec', [0, 1])
def test_ref_gemm_conv3_is_the_gathered_operand(prec, C):
    """F.conv2d on the channels-last images == the operand indexed tap by tap out of the flat
    buffer (GemmArgs' address rule) times the (N, (ky * 3 + kx) * C + c) weight."""
    c = KR.make_gemm_case(_gemm_spec_of('conv3', prec, M=69, conv_C=C))
    rnd = KR._r16 if prec else (lambda t: t)
    X = KR.gemm_operand(c)
    assert X.shape == (69, 9 * C) and X.abs().max() < KR.POISON
    want = F.relu(rnd(X).double() @ rnd(c['W']).double().t() + c['bias'].double())
    _close(KR.ref_gemm(c), want)


def test_gemm_cases_yardstick_and_coded_values():
    """Every case of the GPU file: its id is unique, its reference is finite (no POISON reaches
    it), the cap on e_plain holds from the reference alone; a coded case's reference rounds to a
    matrix of (half-)integers that the fp32 evaluation reproduces to the bit, with more than one
    value per row and per column (a misplaced row or column is then a different number); a wide
    case's pre-activations reach past +-88 and +-104."""
    ids = [KR.gemm_case_id(s) for s in KR.GEMM_CASES]
    assert len(set(ids)) == len(ids)
    for s, name in zip(KR.GEMM_CASES, ids):
        c = KR.make_gemm_case(s)
        ref, e_plain, scale = KR.gemm_refs(c)
        n_out = s['N'] // 2 if s['glu'] else s['N']
        assert ref.shape == (s['M'], n_out), name
        assert torch.isfinite(ref).all() and scale < 1e6, name
        assert KR.cap_ok(e_plain, scale), (name, e_plain, scale)
        if 'buf' in c:
            assert (c['buf'][c['own']].abs() < KR.POISON).all() and \
                (c['buf'][~c['own']] == KR.POISON).all() and not c['own'].all(), name
        if s['regime'] == 'coded':
            # (a shut GLU gate leaves 1e-85 of its value in fp64: 0.0f once rounded to fp32)
            r32 = ref.float()
            assert e_plain < 1e-80 and torch.equal(KR.ref_gemm(c, fp32=True).float(), r32), name
            assert torch.equal(2 * r32, torch.round(2 * r32)) and (ref - r32).abs().max() < 1e-80, \
                name
            if s['M'] > 1 and n_out > 1:
                assert (ref.max(0).values > ref.min(0).values).float().mean() > 0.9, name
                assert (ref.max(1).values > ref.min(1).values).float().mean() > 0.9, name
        if s['regime'] == 'wide':
            bias = c['b_un'][s['N'] // 2:] if s['glu'] else c['bias']
            assert bias.max() >= 104.0 and bias.min() <= -104.0 or s['N'] < 9, name


# ---------------------------------------------------------------------------------------------
# the stored-operand GEMMs and the MXFP8 quantiser (tests/test_gpu_gemm_lowp_ops.py): mx_encode /
# mx_decode against the oracle and against torch.float8_e4m3fn, the cases of GEMM_LOWP_CASES


def _mx_edge_rows():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(40, 256, generator=g) * torch.exp(torch.randn(40, 1, generator=g) * 3)
    x[0] = 0.0                                                   # zero blocks
    x[1, :32] = 0.0
    x[1, 40] = -0.0
    for j, e in enumerate(range(-20, 20, 5)):                    # amax on / just above a boundary
        x[2, 32 * j:32 * j + 32] = 1e-4 * 2.0 ** e
        x[2, 32 * j] = 448.0 * 2.0 ** e
        x[3, 32 * j:32 * j + 32] = 1e-4 * 2.0 ** e
        x[3, 32 * j + 5] = -448.0 * 2.0 ** e * (1 + 2.0 ** -23)
    x[4, 0] = 449.0 * 2.0 ** 3
    x[5, :64] = torch.randn(64, generator=g) * 1e-30             # tiny values
    x[5, 64:96] = torch.randn(32, generator=g) * 1e-41           # fp32 subnormals: E clamps at 0
    x[6, :32] = torch.linspace(-1, 1, 32) * 2.0 ** -9            # e4m3 subnormals after scaling
    x[6, 0] = 1.0
    x[7, :32] = torch.arange(32) * 2.0 ** -10                    # ties between subnormals
    x[7, 31] = 256.0
    x[8, :32] = torch.finfo(torch.float32).max                   # the largest finite value
    x[8, 32:64] = torch.finfo(torch.float32).max * torch.linspace(-1, 1, 32)
    x[9, :32] = (16.0 + torch.arange(32)) * 2.0 ** 4             # ties between normals (17 -> 16)
    return x


def test_mx_encode_is_the_oracle_and_float8():
    """mx_encode against oracle.mx_quantize (bytes and scales) and, element by element, against
    the cast to torch.float8_e4m3fn of the scaled values; mx_decode against oracle.mx_round."""
    x = _mx_edge_rows()
    q, E = KR.mx_encode(x)
    oq, oE = O.mx_quantize(x)
    assert torch.equal(E, oE) and torch.equal(q, oq.view(torch.uint8))
    assert torch.equal(KR.mx_decode(q, E).float(), O.mx_round(x))
    # second statement: the scale by a search over powers of two, the elements by float8
    xb = x.double().view(40, 8, 32)
    amax = xb.abs().amax(-1)
    for r in range(40):
        for b in range(8):
            e = -127
            while amax[r, b] > 448.0 * 2.0 ** e and e < 126:
                e += 1
            assert int(E[r, b]) == e + 127, (r, b)
            v = (xb[r, b] * 2.0 ** (127 - int(E[r, b]))).float()
            assert v.abs().max() <= 448.0
            assert torch.equal(v.to(torch.float8_e4m3fn).view(torch.uint8), q[r, 32 * b:32 * b + 32])
    assert E[0].max() == 0 and q[0].max() == 0 and q[1, 40] == 0x80
    assert (E[5, 2] == 0) and E[8, 0] == 127 + 120 and q[8, 0] == 0x78   # rounds to 2^8 * 2^120
    # every byte but the two NaNs decodes to what float8 says and encodes back to itself
    by = torch.arange(256, dtype=torch.uint8)
    ok = (by & 0x7f) != 0x7f
    assert torch.equal(KR.e4m3_decode(by)[ok].float(), by.view(torch.float8_e4m3fn).float()[ok])
    assert torch.equal(KR.e4m3_encode(KR.e4m3_decode(by))[ok], by[ok])
    # scale dwords: there and back, unowned bytes keep the fill
    dw = KR.mx_scale_dwords(E[:, :5], 43)
    assert dw.shape == (2, 43) and torch.equal(KR.mx_scale_bytes(dw, 40, 5), E[:, :5])
    assert (dw.view(torch.uint8).view(2, 43, 4)[1, :, 1:] == 0xfe).all() and (dw[:, 40:] == -0x01010102).all()


def test_gemm_lowp_route_codes_extend_the_old_ones():
    assert KR.gemm_route_code(128, 128, 2, 4, 64, 1, prec=1, act=3, resid=True) == \
        2 | 2 << 4 | 2 << 8 | 4 << 12 | 2 << 16 | 1 << 20 | 1 << 24 | 3 << 25 | 1 << 27
    codes = [KR.lowp_route_code(s) for s in KR.GEMM_LOWP_CASES]
    old = {KR.gemm_route_code(*s['route'], glu=s['glu'], conv=s['kind'] != 'plain', prec=s['prec'],
                              act=s['act'], resid=s['resid'] != 0) for s in KR.GEMM_CASES}
    assert not old & set(codes) and all(-2 ** 31 <= c < 2 ** 31 for c in codes)
    assert len({(c, s['tile'] == 0) for c, s in zip(codes, KR.GEMM_LOWP_CASES)}) >= 60


def _lowp_small():
    return [s for s in KR.GEMM_LOWP_CASES if s['M'] * s['N'] * s['K'] < 2e9]


def test_gemm_lowp_cases_cover_what_the_issue_lists():
    cases = KR.GEMM_LOWP_CASES
    ids = [KR.gemm_lowp_case_id(s) for s in cases]
    assert len(set(ids)) == len(ids)
    for et in (0, 1):
        P = [s for s in cases if s['fam'] == KR.FAM_PIPELINED and s['et'] == et and s['N'] < 20000]
        kt = 128 if et else 64
        assert {s['M'] for s in P} == {1, 255, 256, 257, 300, 1030, 1281}
        assert {s['K'] // kt for s in P} == {2, 3, 4, 5}
        assert {(s['act'], s['resid']) for s in P if s['cm'] == 0} == \
            {(a, r) for a in range(4) for r in (0, 1)}
        assert {s['N'] for s in P if s['cm'] == 0} == {8, 256, 264, 520}
        lp = [s for s in P if s['cm'] != 0]
        assert {s['act'] for s in lp} == {0, 1, 2, 3}
        assert {s['N'] for s in lp} == ({32, 288, 544} if et else {8, 256, 264, 520})
        assert any((s['M'], s['N']) == (1030, 264) and s['regime'] == r for s in P
                   for r in ('coded-hot', )) and {s['regime'] for s in P} == \
            {'unit', 'coded-hot', 'coded-dense', 'wide'}
        assert sum(s['w_pad'] == 5 for s in P) >= 2
    mx = [s for s in cases if s['et']]
    assert abs(sum(s['model_pitch'] for s in mx) - len(mx) / 2) <= 1
    T = [s for s in cases if s['fam'] == KR.FAM_STORED]
    for r in {(64, 64, 2, 2), (128, 128, 2, 4)}:
        for bk in (32, 64):
            B = [s for s in T if s['route'] == r + (bk, )]
            assert {(s['act'], s['resid']) for s in B if s['cm'] == 0} >= \
                {(a, q) for a in range(4) for q in (0, 1)}
            assert {s['act'] for s in B if s['cm'] == 1} == {0, 1, 2, 3}
    assert {(s['route'][:4], s['route'][4]) for s in T if s['glu']} == \
        {((64, 128, 2, 2), 64), ((64, 128, 2, 2), 32), ((128, 128, 4, 2), 64), ((128, 128, 4, 2), 32)}
    assert any(s['route'] == (256, 256, 4, 2, 64) for s in T)
    # the dispatch rules the routes were written from
    cd = lambda a, b: -(-a // b)
    for s in cases:
        t128, t256 = cd(s['M'], 128) * cd(s['N'], 128), cd(s['M'], 256) * cd(s['N'], 256)
        if s['fam'] == KR.FAM_PIPELINED:
            assert s['et'] or s['tile'] == 8 or (s['tile'] == 0 and t256 >= 192)
            continue
        pipe_ok = s['K'] % 64 == 0 and s['K'] >= 128 and s['N'] % 8 == 0 and not s['glu']
        assert s['tile'] == 0 and (t256 < 192 or not pipe_ok)
        bk = 64 if s['K'] % 64 == 0 else 32
        if s['glu']:
            want = (128, 128, 4, 2) if t128 >= 224 else (64, 128, 2, 2)
        elif bk == 64 and t256 >= 256 and (t256 >= 1024 or s['K'] >= 2048):
            want = (256, 256, 4, 2)
        else:
            want = (128, 128, 2, 4) if t128 >= 224 else (64, 64, 2, 2)
        assert s['route'] == want + (bk, ), KR.gemm_lowp_case_id(s)


@pytest.mark.parametrize('which', ['pipe-bf16', 'pipe-mx', 'stored', 'stored-glu'])
def test_gemm_lowp_cases_yardstick_exactness_and_tie_share(which):
    """Every case but the two whose reference is large (they run on the GPU machine only): the
    reference is finite, e_plain is under the cap; a coded case is exact in fp32, every k is some
    row's hot k when the rows allow it, and the scale bytes of neighbouring blocks and rows differ;
    a bf16-C case has less than 2 % of its reference within the fp32 bound of a bf16 rounding
    boundary."""
    sel = dict([('pipe-bf16', lambda s: s['fam'] == 2 and not s['et']),
                ('pipe-mx', lambda s: s['fam'] == 2 and s['et']),
                ('stored', lambda s: s['fam'] == 1 and not s['glu']),
                ('stored-glu', lambda s: s['glu'])])[which]
    n = 0
    for s in _lowp_small():
        if not sel(s):
            continue
        n += 1
        name = KR.gemm_lowp_case_id(s)
        c = KR.make_gemm_lowp_case(s)
        ref, e_plain, scale, S = KR.gemm_lowp_refs(c)
        n_out = s['N'] // 2 if s['glu'] else s['N']
        assert ref.shape == (s['M'], n_out) and torch.isfinite(ref).all() and scale < 1e6, name
        assert KR.cap_ok(e_plain, scale), (name, e_plain, scale)
        if s['regime'].startswith('coded'):
            r32 = ref.float()
            assert e_plain < 1e-80 and (ref - r32).abs().max() < 1e-80, name
            assert torch.equal(KR.ref_gemm_lowp(c, fp32=True).float(), r32), name
            assert torch.equal(r32 * 1024, torch.round(r32 * 1024)), name
            if s['M'] > 1:
                assert (ref.max(0).values > ref.min(0).values).float().mean() > 0.9, name
                assert (ref.max(1).values > ref.min(1).values).float().mean() > 0.9, name
        if s['regime'] == 'coded-hot':
            hot = KR._coded_hot_k(s['M'], s['K'])
            assert (c['A'] != 0).sum(1).eq(1).all() and len(set(c['A'][c['A'] != 0].tolist())) >= \
                min(8, s['M']), name
            if s['M'] >= s['K']:
                assert len(set(hot.tolist())) == s['K'], name
            if s['et']:
                WE = c['WE'].int()
                assert len(set(WE.flatten().tolist())) >= 8
                assert (WE[:, 1:] != WE[:, :-1]).all() and (WE[1:] != WE[:-1]).all(), name
        if s['regime'] == 'coded-dense':
            assert c['A'].abs().max() <= 2 * 8 and (c['A'] != 0).float().mean() > 0.7, name
            if s['et']:
                assert (c['AE'] == c['AE'][:, :1]).all() and (c['WE'] == c['WE'][:, :1]).all()
                assert KR.e4m3_decode(c['Aq']).abs().max() == 2 and \
                    KR.e4m3_decode(c['Wq']).abs().max() == 8, name
        if s['regime'] == 'wide':
            bias = c['b_un'][s['N'] // 2:] if s['glu'] else c['bias']
            assert bias.max() >= 104.0 and bias.min() <= -104.0, name
        if s['cm'] == 1 and s['regime'] == 'unit':
            b = KR.bound(e_plain, scale) + (KR.GELU_E5_ABS * abs(s['alpha']) if s['act'] == 3 and
                                           s['fam'] == KR.FAM_PIPELINED else 0.0)
            assert KR.bf16_tie_share(ref, b)[1] < 0.02, name
    assert n >= 15


def test_mx_quantize_cases_have_their_special_rows():
    for rows in (1, 4, 5, 300):
        for K in (32, 160, 256, 544):
            x = KR.mx_quantize_case(rows, K)
            q, E = KR.mx_encode(x)
            assert x[0, 0] == 14.0 and E[0, 0] == 127 - 5 and q[0, 0] == 0x7e
            if rows >= 4:
                assert E[1, 0] == 127 + 4 and (q[2, 12:20] & 0x78).eq(0).all() and (q[2, 12:20] & 7).ne(0).all() and E[3, 0] == 0
            if rows >= 6:
                assert 0 < E[4].max() < 40 and (q[5] == 0).all() and (E[5] == 0).all()
