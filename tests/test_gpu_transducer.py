"""The hybrid transducer on the GPU (csrc/transducer.hip, csrc/cabi_transducer.hip):
 (a) wn_op_lstm_step and (b) wn_op_joint_argmax against fp64 NumPy
     (tests/transducer_formulation.py);
 (c) basic_greedy_search on the reference's recorded encoder output and (d) Transducer end to
     end against the reference's recorded token lists (tests/golden/rnnt/rnnt_tiny.npz,
     tools/gen_golden_transducer.py).

Error bars of (a) / (b): the kernel's max-abs error against fp64 may be 4 x the error of the same
computation by torch in fp32 on the CPU (the reference's own operations) against fp64, plus 1e-6;
the 4 covers another summation order.  The measured ratios are printed.  Arg-max indices must
equal the fp64 arg-max wherever the fp64 top-two gap exceeds the fp32 dot-product bound
(transducer_formulation.dot_bound)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import transducer_formulation as TF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from wenet_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- (a) the predictor step -----------------------------------------------------------------
def _lstm_case(B, E, H, P, seed):
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.LSTM(E, H, num_layers=2, batch_first=True)
    proj = torch.nn.Linear(H, P)
    with torch.no_grad():
        for p in list(rnn.parameters()) + list(proj.parameters()):
            std = 3.0 / math.sqrt(p.shape[1]) if p.dim() == 2 else 0.1
            p.copy_(torch.randn(p.shape, generator=g) * std)
    x = torch.randn(B, E, generator=g)
    h = torch.randn(2, B, H, generator=g) * 0.5
    c = torch.randn(2, B, H, generator=g)
    adv = (torch.rand(B, generator=g) < 0.6).to(torch.int32)
    adv[0], adv[B - 1] = 1, 0
    return rnn, proj, x, h, c, adv


def _torch_step(rnn, proj, x, h, c, dtype):
    rnn, proj = rnn.to(dtype), proj.to(dtype)
    with torch.no_grad():
        out, (h2, c2) = rnn(x.to(dtype).unsqueeze(1), (h.to(dtype), c.to(dtype)))
        out = proj(out[:, 0])
    rnn.float(), proj.float()
    return out.double().numpy(), h2.double().numpy(), c2.double().numpy()


@pytest.mark.parametrize('B,E,H,P', [(3, 64, 80, 96), (33, 64, 80, 96), (33, 256, 256, 256)])
def test_lstm_step_against_fp64(B, E, H, P):
    Lm, L = _lib()
    rnn, proj, x, h, c, adv = _lstm_case(B, E, H, P, seed=B * 1000 + H)
    ref = _torch_step(rnn, proj, x, h, c, torch.float64)
    plain = _torch_step(rnn, proj, x, h, c, torch.float32)
    # the formulation the search is checked against is the same function
    W = dict(rnn=[tuple(getattr(rnn, f'{n}_l{l}').detach().double().numpy()
                        for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
                  for l in range(2)])
    top, fh, fc = TF.lstm_step(x.double().numpy(), h.double().numpy(), c.double().numpy(), W['rnn'])
    assert np.abs(fh - ref[1]).max() < 1e-12 and np.abs(fc - ref[2]).max() < 1e-12
    dev = [getattr(rnn, f'{n}_l{l}').detach().cuda().contiguous()
           for l in range(2) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    ptrs = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in dev])
    pw, pb = proj.weight.detach().cuda().contiguous(), proj.bias.detach().cuda().contiguous()
    xd, hd, cd, ad = x.cuda(), h.cuda().contiguous(), c.cuda().contiguous(), adv.cuda()
    SENT = 123.25
    od = torch.full((B, P), SENT, device='cuda')
    st = L.wn_op_lstm_step(xd.data_ptr(), ptrs, 2, pw.data_ptr(), pb.data_ptr(), hd.data_ptr(),
                           cd.data_ptr(), ad.data_ptr(), od.data_ptr(), B, E, H, P, _stream())
    assert st == 0, L.wn_last_error()
    torch.cuda.synchronize()
    got = (od.cpu(), hd.cpu(), cd.cpu())
    on = adv.bool().numpy()
    # rows without `advance`: state and output untouched, bit for bit
    assert torch.equal(got[1][:, ~adv.bool()], h[:, ~adv.bool()])
    assert torch.equal(got[2][:, ~adv.bool()], c[:, ~adv.bool()])
    assert (got[0][~adv.bool()] == SENT).all()
    for name, g_, r_, p_ in (('out', got[0].double().numpy()[on], ref[0][on], plain[0][on]),
                             ('h', got[1].double().numpy()[:, on], ref[1][:, on], plain[1][:, on]),
                             ('c', got[2].double().numpy()[:, on], ref[2][:, on], plain[2][:, on])):
        err, e_plain = np.abs(g_ - r_).max(), np.abs(p_ - r_).max()
        print(f'lstm_step B={B} E={E} H={H} {name}: err {err:.3e}, torch fp32 {e_plain:.3e}, '
              f'ratio {err / max(e_plain, 1e-30):.2f}')
        assert err <= 4 * e_plain + 1e-6, (name, err, e_plain)


# ---- (b) joint + arg-max ----------------------------------------------------------------------
def _joint_case(J, V, seed):
    g = torch.Generator().manual_seed(seed)
    enc_proj = torch.randn(40, J, generator=g)
    pred_proj = torch.randn(5, J, generator=g)
    W = torch.randn(V, J, generator=g) * (3.0 / math.sqrt(J))
    bias = torch.randn(V, generator=g) * 0.1
    # two identical weight rows that win now and then: in one wave's 32 columns, in two waves of
    # a block and (V > 128) in two column blocks
    pairs = [(5, 9), (3, 40)] + ([(7, V - 100)] if V > 256 else [])
    if V > 64 * 128:
        pairs.append((130, 64 * 128 + 2))      # column blocks 1 and 64: both lane 0's partials
    for n, (i, j) in enumerate(pairs):
        W[j] = W[i]
        bias[i] = bias[j] = 2.0 + n
    return enc_proj, pred_proj, W, bias, pairs


def _joint_run(L, dev, row_enc, row_pred, J, V):
    enc_proj, pred_proj, W, bias = dev
    M = len(row_enc)
    re_ = np.ascontiguousarray(row_enc, dtype=np.int32)
    rp_ = np.ascontiguousarray(row_pred, dtype=np.int32)
    idx = np.full((M, ), -7, dtype=np.int32)
    mx = np.zeros((M, ), dtype=np.float32)
    Lm, _ = _lib()
    st = L.wn_op_joint_argmax(enc_proj.data_ptr(), enc_proj.shape[0], pred_proj.data_ptr(),
                              pred_proj.shape[0], Lm.i32p(re_), Lm.i32p(rp_), W.data_ptr(),
                              bias.data_ptr(), M, J, V, Lm.i32p(idx), Lm.f32p(mx), _stream())
    assert st == 0, L.wn_last_error()
    return idx, mx


@pytest.mark.parametrize('M', [3, 48, 130])
@pytest.mark.parametrize('J,V', [(160, 67), (512, 4233), (32, 8329)])
def test_joint_argmax_against_fp64(J, V, M):
    _, L = _lib()
    enc_proj, pred_proj, W, bias, pairs = _joint_case(J, V, seed=J + V)
    rng = np.random.default_rng(M * 7 + J)
    row_enc = rng.integers(0, 40, size=M)
    row_pred = rng.integers(0, 5, size=M)
    row_enc[rng.random(M) < 0.2] = -1          # rows past an utterance's end
    row_enc[0], row_enc[M - 1] = 11, -1
    dev = tuple(t.cuda().contiguous() for t in (enc_proj, pred_proj, W, bias))
    idx, mx = _joint_run(L, dev, row_enc, row_pred, J, V)
    live = row_enc >= 0
    assert (idx[~live] == -1).all() and np.isneginf(mx[~live]).all()
    e64, p64 = enc_proj.double().numpy(), pred_proj.double().numpy()
    W64, b64 = W.double().numpy(), bias.double().numpy()
    hrows = np.tanh(e64[row_enc[live]] + p64[row_pred[live]])
    logits = hrows @ W64.T + b64
    with torch.no_grad():
        plain = (torch.tanh(enc_proj[row_enc[live]] + pred_proj[row_pred[live]]) @ W.T + bias)
    e_plain = np.abs(plain.double().numpy().max(axis=1) - logits.max(axis=1)).max()
    err = np.abs(mx[live].astype(np.float64) - logits.max(axis=1)).max()
    print(f'joint_argmax J={J} V={V} M={M}: max-logit err {err:.3e}, torch fp32 {e_plain:.3e}, '
          f'ratio {err / max(e_plain, 1e-30):.2f}')
    assert err <= 4 * e_plain + 1e-6
    best = logits.argmax(axis=1)                 # lowest index on ties
    lower = {j: i for i, j in pairs}
    checked = ties = 0
    for r in range(len(best)):
        gap, bound = TF.dot_bound(hrows[r], logits[r], W64, J)
        if int(best[r]) in [i for i, _ in pairs]:
            # the top two are the identical rows: an exact tie, the lower index must win
            assert idx[live][r] == best[r], (r, idx[live][r], best[r])
            ties += 1
        elif gap > bound:
            assert idx[live][r] == best[r], (r, idx[live][r], best[r], gap, bound)
            checked += 1
        assert idx[live][r] not in lower, 'the higher of two identical rows was returned'
    assert checked + ties >= len(best) // 2
    if M >= 48:
        assert ties >= 1
    # permuted rows and each row alone (M = 1): the same bits for that row
    perm = rng.permutation(M)
    idx_p, mx_p = _joint_run(L, dev, row_enc[perm], row_pred[perm], J, V)
    assert np.array_equal(idx_p, idx[perm]) and np.array_equal(mx_p.view(np.int32),
                                                               mx[perm].view(np.int32))
    for m in (0, M // 2, M - 2):
        i1, m1 = _joint_run(L, dev, row_enc[m:m + 1], row_pred[m:m + 1], J, V)
        assert i1[0] == idx[m] and m1.view(np.int32)[0] == mx.view(np.int32)[m], m


# ---- (c), (d) the search ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, torch.from_numpy(z['enc']).cuda(), meta['enc_lens']


def _model(meta, bias=None):
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    sd = S.make_state_dict(configs, meta['wseed'],
                           rnnt_blank_bias=meta['blank_bias'] if bias is None else bias)
    return Transducer(configs, sd, device='cuda')


@pytest.fixture(scope='module')
def model(gold):
    return _model(gold[0])


@pytest.mark.parametrize('lookahead', [1, 4, 8, 16])
@pytest.mark.parametrize('n_steps', [64, 3, 1])
def test_search_on_the_recorded_encoder_output(gold, model, n_steps, lookahead):
    from wenet_amd.transducer import basic_greedy_search
    meta, enc, lens = gold
    want = meta['tokens'][str(n_steps)]
    assert model.tune('rnnt_lookahead', lookahead) == lookahead
    try:
        got = basic_greedy_search(model, enc, lens, n_steps=n_steps)
        assert got == want
        assert all(len(u) <= n * n_steps for u, n in zip(got, lens))
        # each utterance alone, and the batch in another order
        for b in range(len(lens)):
            assert basic_greedy_search(model, enc[b:b + 1], lens[b:b + 1], n_steps) == [want[b]]
        order = [2, 0, 1]
        got = basic_greedy_search(model, enc[order].contiguous(), [lens[b] for b in order], n_steps)
        assert got == [want[b] for b in order]
    finally:
        model.tune('rnnt_lookahead', 'inherit')


def test_lookahead_takes_fewer_steps(gold, model):
    from wenet_amd.transducer import basic_greedy_search
    meta, enc, lens = gold
    steps = {}
    try:
        for F in (1, 8):
            model.tune('rnnt_lookahead', F)
            assert basic_greedy_search(model, enc, lens, n_steps=3) == meta['tokens']['3']
            steps[F] = model.last_rnnt_steps
    finally:
        model.tune('rnnt_lookahead', 'inherit')
    print('lock-step steps at lookahead 1 / 8:', steps)
    assert 0 < steps[8] < steps[1]
    # the formulation takes exactly as many
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    sd = S.make_state_dict(configs, meta['wseed'])
    W = TF.weights64({k: v.numpy() for k, v in sd.items()}, 2)
    for F in (1, 8):
        assert TF.lookahead_greedy_search(enc.cpu().numpy(), lens, W, meta['blank'], 3, F)[1] == \
            steps[F]


# The host loop issues steps in groups of 8 up to the bound longest x (n_steps + 1) + 1 and looks
# at n_active one group late.  The recorded utterances (29 / 16 / 15 frames) have bounds of 59
# and more; here are the two edges they leave out, on their first frames (the decisions are a
# prefix of the recorded searches', so the fp64 formulation is a reference as it is there):
# a bound of 7, below one group, and a search whose last step is the 6th of its second group.
@pytest.mark.parametrize('lens,n_steps,bound,steps1', [([1, 3], 1, 7, 3), ([4, 6], 3, 25, 14)])
def test_poll_loop_edges(gold, model, lens, n_steps, bound, steps1):
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import basic_greedy_search
    meta, enc, _ = gold
    assert max(lens) * (n_steps + 1) + 1 == bound
    enc = enc[:len(lens), :max(lens)].contiguous()
    configs = S.make_configs(meta['config'])
    sd = S.make_state_dict(configs, meta['wseed'], rnnt_blank_bias=meta['blank_bias'])
    W = TF.weights64({k: v.numpy() for k, v in sd.items()}, 2)
    form = {F: TF.lookahead_greedy_search(enc.cpu().numpy(), lens, W, meta['blank'], n_steps, F)
            for F in (1, 16)}
    assert form[1][1] == steps1 and form[1][0] == form[16][0] and any(form[1][0])
    try:
        for F in (1, 16):
            model.tune('rnnt_lookahead', F)
            assert basic_greedy_search(model, enc, lens, n_steps=n_steps) == form[F][0]
            assert model.last_rnnt_steps == form[F][1]
            for b, n in enumerate(lens):
                assert basic_greedy_search(model, enc[b:b + 1, :n].contiguous(), [n],
                                           n_steps) == [form[F][0][b]]
    finally:
        model.tune('rnnt_lookahead', 'inherit')


# A vocabulary of 65 x 128 + 9: the joint kernel leaves 66 column-block partials per row, so the
# advance kernel's own reduction runs (lane-strided merge with a second round for lane 0 and 1,
# butterfly, the m * ncb pitch), which the 67-token golden model (one column block) never
# reaches.  There is no recorded reference at this size; the fp64 formulation is the reference,
# and it is one only where fp32 cannot flip a decision: every joint row that takes part in one
# must have a top-two gap of at least 4 x the fp32 dot-product bound (the fixture's condition 4),
# which the weight seed below was searched for and the test asserts on the fp64 side.
# ffn_out rows are duplicated across column blocks (an exact tie in every row: the lower index
# must win) and some tokens of the last two blocks are favoured so that they are emitted.
WIDE_SEED = 4      # of seeds 0..15, the one with the widest margin that also emits both kinds of tie
WIDE_TIES = [(5, 8200), (7, 4000), (70, 8300)]     # (kept, duplicate): blocks 0 / 64, 0 / 31, 0 / 64
WIDE_LENS = [21, 8, 16]


def _wide_case(wseed):
    """(configs, state dict, enc (3, 21, d), lens, fp64 tokens {F: lists}, facts)."""
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_rnnt_wide')
    V = configs['output_dim']
    sd = S.make_state_dict(configs, wseed)
    w, bias = sd['joint.ffn_out.weight'], sd['joint.ffn_out.bias']
    bias[V - 130:] += 1.5                    # the last two column blocks (64 and 65)
    for n, (i, j) in enumerate(WIDE_TIES):
        bias[i] += 3.0
        w[j], bias[j] = w[i], bias[i]
    d = configs['encoder_conf']['output_size']
    rng = np.random.default_rng(1234)
    enc = rng.standard_normal((len(WIDE_LENS), max(WIDE_LENS), d)).astype(np.float32)
    W = TF.weights64({k: v.numpy() for k, v in sd.items()}, 2)
    keep = np.ones(V, dtype=bool)
    keep[[j for _, j in WIDE_TIES]] = False
    w_keep = W['ffn_out'][0][keep]
    facts = dict(rows=0, min_ratio=float('inf'), tie_rows=0)

    def on_row(b, t, hrow, logits):
        gap, bound = TF.dot_bound(hrow, logits[keep], w_keep, w_keep.shape[1])
        facts['rows'] += 1
        facts['min_ratio'] = min(facts['min_ratio'], gap / bound)
        facts['tie_rows'] += int(logits.argmax()) in [i for i, _ in WIDE_TIES]

    tokens = {}
    for F in (1, 5, 16):
        tokens[F], _ = TF.lookahead_greedy_search(enc, WIDE_LENS, W, 0, 3, F,
                                                  on_row if F == 1 else None)
    return configs, sd, enc, WIDE_LENS, tokens, facts


@pytest.fixture(scope='module')
def wide():
    from wenet_amd import Transducer
    configs, sd, enc, lens, tokens, facts = _wide_case(WIDE_SEED)
    print('wide vocabulary case:', facts, [len(u) for u in tokens[1]])
    # conditions on the inputs (fp64 only): the reference is unambiguous and the case bites
    assert facts['min_ratio'] >= 4.0, facts
    assert tokens[1] == tokens[5] == tokens[16]
    flat = [t for u in tokens[1] for t in u]
    assert facts['tie_rows'] >= 1 and any(t >= 64 * 128 for t in flat)
    assert 5 in flat and 7 in flat          # ties between blocks 0 / 64 (one lane) and 0 / 31
    assert not {j for _, j in WIDE_TIES} & set(flat)
    return Transducer(configs, sd, device='cuda'), torch.from_numpy(enc).cuda(), lens, tokens[1]


@pytest.mark.parametrize('lookahead', [1, 5, 16])
def test_search_reduces_many_column_blocks(wide, lookahead):
    from wenet_amd.transducer import basic_greedy_search
    model, enc, lens, want = wide
    model.tune('rnnt_lookahead', lookahead)
    try:
        assert basic_greedy_search(model, enc, lens, n_steps=3) == want
        order = [1, 2, 0]
        got = basic_greedy_search(model, enc[order].contiguous(), [lens[b] for b in order], 3)
        assert got == [want[b] for b in order]
    finally:
        model.tune('rnnt_lookahead', 'inherit')


def test_blank_heavy_model_gives_empty_results(gold):
    from wenet_amd.transducer import basic_greedy_search
    meta, enc, lens = gold
    heavy = _model(meta, meta['heavy']['bias'])
    got = basic_greedy_search(heavy, enc, lens, n_steps=64)
    assert got == meta['heavy']['tokens'] and any(len(u) == 0 for u in got)


def test_end_to_end(gold, model):
    from wenet_amd import synthetic as S
    meta, _, lens = gold
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    want = meta['tokens']['64']
    assert model.greedy_search(feats.cuda(), flens) == want
    assert model.greedy_search(feats.cuda(), flens, n_steps=3) == meta['tokens']['3']
    res = model.decode(['rnnt_greedy_search', 'ctc_greedy_search'], feats.cuda(), flens)
    assert [r.tokens for r in res['rnnt_greedy_search']] == want
    assert [list(r.tokens) for r in res['ctc_greedy_search']] == meta['ctc_greedy']
    other = model.clone()
    assert type(other) is type(model)
    assert other.greedy_search(feats.cuda(), flens) == want
    # the hybrid's other modes run on the same handle
    res = model.decode(['attention_rescoring'], feats.cuda(), flens, beam_size=4, ctc_weight=0.5)
    assert len(res['attention_rescoring']) == meta['batch']


def test_a_model_without_transducer_weights_is_refused():
    from gpu_util import cached_model
    Lm, L = _lib()
    _, _, asr = cached_model('tiny_causal', 0)
    feats = torch.zeros(1, 40, 80, device='cuda')
    asr._forward_encoder(feats, torch.tensor([40]))
    tok = np.zeros((1, 8), dtype=np.int32)
    ln = np.zeros((1, ), dtype=np.int32)
    st = L.wn_transducer_greedy_search(asr._h, 64, Lm.i32p(tok), Lm.i32p(ln), 8, None, _stream())
    assert st == -1
    assert b'no transducer weights' in L.wn_last_error()
    assert b'wn_model_create_transducer' in L.wn_last_error()
