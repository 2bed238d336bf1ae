"""The stateless predictors on the GPU (csrc/transducer_stateless.hip and its five call sites):
 (a) wn_op_stateless_step against fp64 NumPy (tests/transducer_stateless_formulation.py) and its
     row invariance, bit for bit;
 (b) the greedy search, (c) the prefix beam search, (d) the transducer score and the rescoring on
     the reference's recorded encoder output (tests/golden/rnnt/rnnt_stateless_tiny.npz,
     tools/gen_golden_transducer_stateless.py), both models;
 (e) the resumable greedy and beam sessions against the one-shot searches, bit for bit, and the
     two recognizers end to end.

Error bar of (a): the kernel's max-abs error against fp64 may be 4 x the error of the
reference's own fp32 forward_step + joint.pred_ffn against fp64 -- recorded in the fixture for
its steps (e_step), computed here by a torch fp32 restatement of the reference's operations for
the other shapes; the 4 covers another summation order.  The measured ratios are printed.
(c) and (d) follow tests/test_gpu_transducer_beam.py and tests/test_gpu_transducer_score.py:
the reference's lists, scores within 4 x the fixture's measured fp32 error + 1e-6."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import transducer_stateless_formulation as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('tiny_rnnt_embed', 'tiny_rnnt_conv')
SENT = 123.25
V_OP = 50


def _lib():
    from wenet_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- (a) the operator ---------------------------------------------------------------------------
def _op_weights(kind, E, C, heads, J, bias, seed):
    """A random predictor + joint.pred_ffn as a state dict (torch fp32) and its configuration."""
    g = torch.Generator().manual_seed(seed)

    def mat(o, i):
        return torch.randn(o, i, generator=g) * (3.0 / math.sqrt(i))

    def vec(n):
        return torch.randn(n, generator=g) * 0.1
    sd = {'predictor.embed.weight': torch.randn(V_OP, E, generator=g),
          'predictor.norm.weight': 1.0 + vec(E), 'predictor.norm.bias': vec(E),
          'joint.pred_ffn.weight': mat(J, E), 'joint.pred_ffn.bias': vec(J),
          'joint.enc_ffn.weight': torch.zeros(1, 1), 'joint.enc_ffn.bias': torch.zeros(1),
          'joint.ffn_out.weight': torch.zeros(1, 1), 'joint.ffn_out.bias': torch.zeros(1)}
    pc = dict(embed_size=E, output_size=E, history_size=C - 1, bias=bias)
    if kind == 'embedding':
        pc['n_head'] = heads
        sd['predictor.pos_embed.weight'] = mat(heads, E * C)
        sd['predictor.ffn.weight'], sd['predictor.ffn.bias'] = mat(E, E), vec(E)
    else:
        sd['predictor.conv.weight'] = torch.randn(E, 1, C, generator=g) * (3.0 / math.sqrt(C))
        if bias:
            sd['predictor.conv.bias'] = vec(E)
    return sd, dict(predictor=kind, predictor_conf=pc)


def _torch_pred_proj(ctx, sd, configs, dtype):
    """forward_step + joint.pred_ffn with the reference's own torch operations
    (predictor.py:344-376, :482-495) in `dtype`."""
    pc = configs['predictor_conf']
    E, C = pc['embed_size'], pc['history_size'] + 1
    t = {k: v.to(dtype) for k, v in sd.items()}
    ids = torch.as_tensor(ctx, dtype=torch.long)
    x = t['predictor.embed.weight'][ids.clamp(min=0)] * (ids >= 0).unsqueeze(-1).to(dtype)
    with torch.no_grad():
        if configs['predictor'] == 'embedding':
            H = pc['n_head']
            pos = t['predictor.pos_embed.weight'].view(H, E, C).permute(0, 2, 1)
            inp = x.unsqueeze(1).unsqueeze(2)                        # [bs, 1, 1, C, E]
            weight = (inp * pos).sum(dim=-1).unsqueeze(3)           # [bs, 1, H, 1, C]
            out = weight.matmul(inp).squeeze(dim=3).sum(dim=2) / (H * C)
            out = torch.nn.functional.linear(out, t['predictor.ffn.weight'], t['predictor.ffn.bias'])
            act = torch.nn.functional.silu
        else:
            out = torch.nn.functional.conv1d(x.permute(0, 2, 1), t['predictor.conv.weight'],
                                             t.get('predictor.conv.bias'), groups=E).permute(0, 2, 1)
            act = torch.relu
        out = act(torch.nn.functional.layer_norm(out, (E, ), t['predictor.norm.weight'],
                                                 t['predictor.norm.bias'], 1e-5))
        out = torch.nn.functional.linear(out, t['joint.pred_ffn.weight'], t['joint.pred_ffn.bias'])
    return out[:, 0].double().numpy()


class _Op:
    """wn_op_stateless_step on one set of device weights."""

    def __init__(self, sd, configs, V):
        Lm, self.L = _lib()
        pc = configs['predictor_conf']
        emb = configs['predictor'] == 'embedding'
        names = ['predictor.embed.weight'] + (
            ['predictor.pos_embed.weight', 'predictor.ffn.weight', 'predictor.ffn.bias'] if emb
            else ['predictor.conv.weight', 'predictor.conv.bias'])
        names += ['predictor.norm.weight', 'predictor.norm.bias', 'joint.pred_ffn.weight',
                  'joint.pred_ffn.bias']
        self.dev = [sd[n].float().cuda().contiguous() if n in sd else None for n in names]
        self.ptrs = (ctypes.c_void_p * len(names))(*[t.data_ptr() if t is not None else None
                                                     for t in self.dev])
        self.sc = Lm.WnStatelessPredictorConfig()
        self.sc.kind = 1 if emb else 2
        self.sc.context = pc['history_size'] + 1
        self.sc.heads = pc.get('n_head', 1)
        self.sc.activation = 0 if emb else 1
        self.sc.conv_bias = int('predictor.conv.bias' in sd)
        self.sc.norm_eps = 1e-5
        self.V, self.E, self.J = V, pc['embed_size'], sd['joint.pred_ffn.weight'].shape[0]

    def __call__(self, ctx, adv=None):
        Lm, _ = _lib()
        ctx = np.ascontiguousarray(ctx, dtype=np.int32)
        M = ctx.shape[0]
        out = torch.full((M, self.J), SENT, device='cuda')
        a = None if adv is None else Lm.i32p(np.ascontiguousarray(adv, dtype=np.int32))
        st = self.L.wn_op_stateless_step(ctypes.byref(self.sc), Lm.i32p(ctx), self.ptrs, a,
                                         out.data_ptr(), M, self.V, self.E, self.J, _stream())
        assert st == 0, self.L.wn_last_error()
        return out.cpu().numpy()


def _windows(M, C, seed):
    """M windows, some with leading -1 entries (never a -1 behind an id, as in a search)."""
    rng = np.random.default_rng(seed)
    ctx = rng.integers(0, V_OP, size=(M, C))
    for m in range(M):
        ctx[m, :int(rng.integers(0, C + 1)) if m % 3 == 0 else 0] = -1
    ctx[0, :C - 1] = -1                       # [-1, ..., blank]: the first step of a search
    ctx[0, C - 1] = 0
    ctx[M - 1] = -1                           # all zero vectors: LayerNorm of a constant row
    return ctx


OP_SHAPES = [('embedding', 80, 4, 4, 160, False), ('embedding', 320, 6, 4, 320, False),
             ('embedding', 33, 1, 1, 32, False), ('conv', 96, 3, 1, 160, True),
             ('conv', 96, 3, 1, 160, False), ('conv', 80, 1, 1, 96, True),
             ('conv', 80, 1, 1, 96, False)]


@pytest.mark.parametrize('kind,E,C,heads,J,bias', OP_SHAPES)
def test_stateless_step_against_fp64_and_row_invariance(kind, E, C, heads, J, bias):
    sd, configs = _op_weights(kind, E, C, heads, J, bias, seed=E * 100 + C)
    op = _Op(sd, configs, V_OP)
    W = SF.weights64({k: v.numpy() for k, v in sd.items()}, configs)
    ctx = _windows(37, C, seed=E + J)
    ref = SF.pred_proj(ctx, W)
    assert np.abs(_torch_pred_proj(ctx, sd, configs, torch.float64) - ref).max() < 1e-11
    e_plain = np.abs(_torch_pred_proj(ctx, sd, configs, torch.float32) - ref).max()
    base = op(ctx)                            # M = 37, every row
    err = np.abs(base.astype(np.float64) - ref).max()
    print(f'stateless_step {kind} E={E} C={C} heads={heads} J={J} bias={bias}: err {err:.3e}, '
          f'torch fp32 {e_plain:.3e}, ratio {err / e_plain:.2f}')
    assert err <= 4 * e_plain, (err, e_plain)
    bits = base.view(np.int32)
    rng = np.random.default_rng(C)
    for M in (1, 5, 37):
        # other places, other companions, mixed masks over a sentinel-filled output
        for trial in range(3):
            rows = rng.permutation(37)[:M] if trial else np.arange(M)
            adv = (rng.random(M) < 0.6).astype(np.int32) if trial else np.ones(M, np.int32)
            if trial == 1:
                adv[0] = 1
            if trial == 2:
                adv[:] = 0
                adv[M - 1] = 1
            got = op(ctx[rows], adv if trial else None)
            on = adv.astype(bool)
            assert np.array_equal(got.view(np.int32)[on], bits[rows[on]]), (M, trial)
            assert (got[~on] == SENT).all(), (M, trial)


# ---- the fixture ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_stateless_tiny.npz'))
    return json.loads(bytes(z['meta']).decode()), z


_MODELS = {}


def _case(gold, name):
    """(meta of the model, Transducer, state dict, configs, enc on the device, lens)."""
    if name not in _MODELS:
        from wenet_amd import Transducer
        from wenet_amd import synthetic as S
        meta, z = gold
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, meta[name]['wseed'])
        _MODELS[name] = (meta[name], Transducer(configs, sd, device='cuda'), sd, configs,
                         torch.from_numpy(z[f'{name}_enc']).cuda(), meta[name]['enc_lens'])
    return _MODELS[name]


@pytest.mark.parametrize('name', CONFIGS)
def test_stateless_step_on_the_recorded_steps(gold, name):
    meta, z = gold
    m, _, sd, configs, _, _ = _case(gold, name)
    W = SF.weights64({k: v.numpy() for k, v in sd.items()
                      if k.startswith(('predictor.', 'joint.'))}, configs)
    op = _Op(sd, configs, configs['output_dim'])
    steps = m['greedy']['step_at']
    ctx = np.stack([z[f'{name}_step{k}_ctx'] for k in steps])
    out = np.stack([z[f'{name}_step{k}_out'] for k in steps])
    ref = out @ W['pred_ffn'][0].T + W['pred_ffn'][1]         # of the reference's fp64 output
    err = np.abs(op(ctx).astype(np.float64) - ref).max()
    print(f"stateless_step {name} recorded steps: err {err:.3e}, reference fp32 "
          f"{m['greedy']['e_step']:.3e}, ratio {err / m['greedy']['e_step']:.2f}")
    assert err <= 4 * m['greedy']['e_step'], (err, m['greedy']['e_step'])


# ---- (b) greedy -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CONFIGS)
@pytest.mark.parametrize('n_steps', [64, 3, 1])
def test_greedy_search_on_the_recorded_encoder_output(gold, name, n_steps):
    from wenet_amd.transducer import basic_greedy_search
    m, model, _, _, enc, lens = _case(gold, name)
    want = m['greedy']['tokens'][str(n_steps)]
    try:
        for lookahead in (1, 4, 16):
            assert model.tune('rnnt_lookahead', lookahead) == lookahead
            assert basic_greedy_search(model, enc, lens, n_steps=n_steps) == want, lookahead
            for b in range(len(lens)):
                assert basic_greedy_search(model, enc[b:b + 1], lens[b:b + 1], n_steps) == [want[b]]
        order = [2, 0, 1]
        got = basic_greedy_search(model, enc[order].contiguous(), [lens[b] for b in order], n_steps)
        assert got == [want[b] for b in order]
    finally:
        model.tune('rnnt_lookahead', 'inherit')


# ---- (c) beam ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CONFIGS)
def test_beam_search_on_the_recorded_encoder_output(gold, name):
    from wenet_amd.transducer import prefix_beam_search
    m, model, _, _, enc, lens = _case(gold, name)
    bar = 4 * m['beam']['e_score'] + 1e-6
    for key, run in m['beam']['runs'].items():
        cw, tw, beam = run['ctc_weight'], run['transducer_weight'], run['beam']
        want = run['fp64']
        got = prefix_beam_search(model, enc, lens, beam, cw, tw)
        assert [[t for t, _ in u] for u in got] == [[t for t, _ in u] for u in want], key
        err = max(abs(s - r) for g, w in zip(got, want) for (_, s), (_, r) in zip(g, w))
        print(f"{name} search ({cw}, {tw}) beam {beam}: score err {err:.3e}, e_score "
              f"{m['beam']['e_score']:.3e}, ratio {err / m['beam']['e_score']:.2f}")
        assert err <= bar, (key, err, bar)
        # each utterance alone, and the batch in another order: the same lists and bits
        for b in range(len(lens)):
            assert prefix_beam_search(model, enc[b:b + 1], lens[b:b + 1], beam, cw, tw) == [got[b]]
        order = [2, 0, 1]
        again = prefix_beam_search(model, enc[order].contiguous(), [lens[b] for b in order], beam,
                                   cw, tw)
        assert again == [got[b] for b in order]


# ---- (d) transducer score and rescoring ---------------------------------------------------------
@pytest.mark.parametrize('name', CONFIGS)
def test_transducer_score_and_rescoring_on_the_recorded_encoder_output(gold, name):
    from wenet_amd.transducer import attention_rescoring, transducer_score
    m, model, _, _, enc, lens = _case(gold, name)
    r = m['rescore']
    sw = r['search_weights']
    for key, run in r['runs'].items():
        w, beam = run['weights'], run['beam']
        want = run['fp64']
        if w == r['rescore_weights'][1]:        # the transducer scores, once per n-best
            hyps = [[t for t, _ in u['nbest']] for u in want]
            got = transducer_score(model, enc, lens, hyps)
            err = max(abs(a - c) for g, u in zip(got, want) for a, c in zip(g, u['td']))
            print(f"{name} transducer score beam {beam}: err {err:.3e}, e_td {r['e_td']:.3e}, "
                  f"ratio {err / r['e_td']:.2f}")
            assert err <= 4 * r['e_td'] + 1e-6, (key, err)
            for b in range(len(lens)):
                assert transducer_score(model, enc[b:b + 1], lens[b:b + 1], [hyps[b]]) == [got[b]]
            assert transducer_score(model, enc, lens, [h[::-1] for h in hyps]) == \
                [g[::-1] for g in got]
        for res in (attention_rescoring(model, enc, lens, beam, reverse_weight=w[3],
                                        ctc_weight=w[0], attn_weight=w[1], transducer_weight=w[2],
                                        search_ctc_weight=sw[0], search_transducer_weight=sw[1]),
                    [attention_rescoring(model, enc[b:b + 1], lens[b:b + 1], beam,
                                         reverse_weight=w[3], ctc_weight=w[0], attn_weight=w[1],
                                         transducer_weight=w[2], search_ctc_weight=sw[0],
                                         search_transducer_weight=sw[1])[0]
                     for b in range(len(lens))]):
            for b, (g, u) in enumerate(zip(res, want)):
                assert g.nbest == [t for t, _ in u['nbest']], (key, b)
                assert list(g.tokens) == u['tokens'], (key, b)
                assert abs(g.score - u['score']) <= 4 * r['e_score'] + 1e-6, (key, b)
                assert max(abs(a - c) for a, c in zip(g.nbest_scores, u['final'])) \
                    <= 4 * r['e_score'] + 1e-6


# ---- (e) sessions -----------------------------------------------------------------------------------
def _pieces(n, split):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(split[i % len(split)], n - sum(out)))
        i += 1
    return out


def _feed(rs, enc, lens, split, slots, utts):
    """Sessions slots[i] <- utterance utts[i], fed with `split` in the same calls (a session that
    is through gets n_t = 0).  Returns the last result of every session."""
    plans = [_pieces(lens[u], split) for u in utts]
    chunk = max(split)
    at, last = [0] * len(slots), [None] * len(slots)
    for call in range(max(len(p) for p in plans)):
        nt = [p[call] if call < len(p) else 0 for p in plans]
        x = torch.zeros((len(slots), chunk, enc.size(2)), device='cuda')
        for i, u in enumerate(utts):
            x[i, :nt[i]] = enc[u, at[i]:at[i] + nt[i]]
            at[i] += nt[i]
        res = rs.advance_encoded(slots, x, nt)
        for i in range(len(slots)):
            if call < len(plans[i]):
                last[i] = res[i]
    return last


def _bits(st):
    if isinstance(st, tuple):
        st = dict(h=st[0], c=st[1], pred_proj=st[2], **st[3])
    return tuple((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(st.items()))


# every split into calls of 1, 3, 7 and all frames; other slots, another order, companions or none
PLANS = (((1, ), [0, 1, 2], [0, 1, 2]), ((3, ), [5, 3, 4], [0, 1, 2]), ((7, ), [1, 2, 0], [2, 0, 1]),
         ((29, ), [4, 0, 5], [1, 2, 0]), ((7, 3), [3], [0]), ((3, ), [2], [1]), ((1, ), [0], [2]))


@pytest.mark.parametrize('name', CONFIGS)
@pytest.mark.parametrize('n_steps', [64, 3])
def test_greedy_sessions_equal_the_one_shot_search(gold, name, n_steps):
    from wenet_amd.streaming import RnntStreamSearch
    from wenet_amd.transducer import basic_greedy_search
    m, model, _, _, enc, lens = _case(gold, name)
    one = basic_greedy_search(model, enc, lens, n_steps=n_steps)
    assert one == m['greedy']['tokens'][str(n_steps)]
    rs = RnntStreamSearch(model._h, model.device, 6, 32, 32 * n_steps, n_steps,
                          dims=(0, 0, model._tcfg.join_dim))
    try:
        want = {}
        for split, slots, utts in PLANS:
            rs.reset(slots)
            last = _feed(rs, enc, lens, split, slots, utts)
            for s, u, r in zip(slots, utts, last):
                assert list(r.tokens) == one[u], (split, s, u)
                assert r.frames_decoded == lens[u]
                h, c, pp, sc = st = rs.state(s)
                assert h.size == 0 and c.size == 0 and sc['n_tok'] == len(one[u])
                assert want.setdefault(u, _bits(st)) == _bits(st), (split, s, u)
    finally:
        rs.close()


@pytest.mark.parametrize('name', CONFIGS)
@pytest.mark.parametrize('beam,cw,tw', [(5, 0.3, 0.7), (3, 0.0, 1.0), (1, 1.0, 0.0)])
def test_beam_sessions_equal_the_one_shot_search(gold, name, beam, cw, tw):
    from wenet_amd.streaming import RnntBeamStreamSearch
    from wenet_amd.transducer import prefix_beam_search
    m, model, _, _, enc, lens = _case(gold, name)
    one = prefix_beam_search(model, enc, lens, beam, cw, tw)
    rs = RnntBeamStreamSearch(model._h, model.device, 6, beam, 32, cw, tw,
                              dims=(0, 0, model._tcfg.join_dim))
    try:
        want = {}
        for split, slots, utts in PLANS:
            rs.reset(slots)
            last = _feed(rs, enc, lens, split, slots, utts)
            for s, u, r in zip(slots, utts, last):
                # tokens and scores, bit for bit
                assert list(zip([list(t) for t in r.nbest], r.nbest_scores)) == one[u], (split, s, u)
                st = rs.state(s)
                assert st['h'].size == 0 and st['c'].size == 0
                assert want.setdefault(u, _bits(st)) == _bits(st), (split, s, u)
    finally:
        rs.close()


def _stream_all(rec, utts, piece_sizes, finish):
    """The utterances through `rec` in uneven pieces; session i opens at round i."""
    sids, fed, final = {}, {}, {}
    rnd = 0
    while len(final) < len(utts):
        if rnd < len(utts):
            sids[rnd] = rec.open()
            fed[rnd] = 0
        for i, sid in sids.items():
            if i in final:
                continue
            k = piece_sizes[(rnd + i) % len(piece_sizes)]
            rec.accept(sid, utts[i][fed[i]:fed[i] + k])
            fed[i] = min(fed[i] + k, utts[i].size(0))
        while rec.step():
            pass
        for i, sid in sids.items():
            if i not in final and fed[i] >= utts[i].size(0):
                final[i] = finish(sid)
        rnd += 1
    for sid in sids.values():
        rec.close(sid)
    return final


@pytest.mark.parametrize('name', CONFIGS)
def test_recognizers_finish_with_the_one_shot_results(gold, name):
    """Both recognizers from features: finish() equals the one-shot search on the session's own
    encoder_out(sid); and the model's own modes from features agree with each other."""
    from wenet_amd import RnntBeamStreamingRecognizer
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import StreamingRecognizer
    from wenet_amd.transducer import basic_greedy_search, prefix_beam_search
    meta, _ = gold
    m, model, _, _, enc, lens = _case(gold, name)
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    utts = [feats[b, :int(flens[b])].cuda() for b in range(meta['batch'])]
    rec = StreamingRecognizer(model, 3, 4, -1, max_seconds=2.0, search='rnnt_greedy_search',
                              n_steps=3, max_tokens=64 * 3)
    final = _stream_all(rec, utts, [23, 50, 7, 64], lambda sid: (rec.finish(sid), rec.encoder_out(sid)))
    for b in range(3):
        r, e = final[b]
        assert [list(r.tokens)] == basic_greedy_search(model, e, [e.size(1)], n_steps=3), b
    rec.search.close()
    brec = RnntBeamStreamingRecognizer(model, 3, 4, -1, beam_size=5, search_ctc_weight=0.3,
                                       search_transducer_weight=0.7, max_seconds=2.0)
    final = _stream_all(brec, utts, [23, 50, 7, 64],
                        lambda sid: (brec.finish(sid, rescoring=False), brec.encoder_out(sid)))
    for b in range(3):
        r, e = final[b]
        one = prefix_beam_search(model, e, [e.size(1)], 5, 0.3, 0.7)[0]
        assert list(zip([list(t) for t in r.nbest], r.nbest_scores)) == one, b
    brec.search.close()
    # full-context decoding from features: the recorded lists, and decode() serves all three modes
    want = m['greedy']['tokens']['64']
    assert model.greedy_search(feats.cuda(), flens) == want
    res = model.decode(['rnnt_greedy_search', 'rnnt_beam_search', 'rnnt_beam_attn_rescoring'],
                       feats.cuda(), flens, beam_size=5, attn_weight=0.4, ctc_weight=0.3,
                       transducer_weight=0.3)
    assert [r.tokens for r in res['rnnt_greedy_search']] == want
    toks, _ = model.beam_search(feats.cuda(), flens, beam_size=5)
    assert [list(r.tokens) for r in res['rnnt_beam_search']] == toks
    assert toks == [u[0][0] for u in m['beam']['runs']['0.3_0.7_5']['fp64']]
    assert len(res['rnnt_beam_attn_rescoring']) == 3
    assert type(model.clone()) is type(model)
    assert model.clone().greedy_search(feats.cuda(), flens) == want
