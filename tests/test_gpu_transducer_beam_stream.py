"""Streaming transducer beam sessions on the GPU (csrc/transducer_beam_stream.hip, the carry mode
of csrc/transducer_beam.hip's beam step, csrc/cabi_transducer_beam_stream.hip,
wenet_amd/streaming.py): the resumable RNN-T prefix beam search on the recorded encoder output of
tests/golden/rnnt/rnnt_beam_tiny.npz, three sessions at once with their own lengths, against the
fp64 session formulation (tests/transducer_beam_stream_formulation.py) after every call and the
reference's recorded beams at the end; bit for bit against the one-shot search and across splits,
slots and batches; empty calls and resets; the carry step alone; RnntBeamStreamingRecognizer end
to end against the reference's chunk-masked beams (tests/golden/rnnt/rnnt_beam_stream_tiny.npz);
the refusals.  The formulation is a reference here because every gap that decides a beam of the
fixtures is at least 8 e + 2e-6 (their generators' condition); scores are held to 4 e_score +
1e-6, e_score being the reference's own fp32-against-fp64 error in the fixture's meta."""
import json
import os

import numpy as np
import pytest
import torch

import transducer_beam_formulation as BF
import transducer_beam_stream_formulation as SF
import transducer_formulation as TF
from transducer_stream_formulation import pieces

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = [(1, ), (4, ), (7, 3), (2, 0, 5), (29, )]
WEIGHTS = [(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)]      # of tests/test_gpu_transducer_beam.py


def _load(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', name))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, {k: z[k] for k in z.files if k != 'meta'}


def _state_dict(meta):
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    return configs, S.make_state_dict(configs, meta['wseed'])


def _model(meta):
    from wenet_amd import Transducer
    configs, sd = _state_dict(meta)
    return Transducer(configs, sd, device='cuda')


def _search(model, n_slots, beam, cw, tw, max_frames=32):
    from wenet_amd.streaming import RnntBeamStreamSearch
    tc = model._tcfg
    return RnntBeamStreamSearch(model._h, model.device, n_slots, beam, max_frames, cw, tw,
                                dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))


@pytest.fixture(scope='module')
def gold():
    meta, arr = _load('rnnt_beam_tiny.npz')
    return meta, arr['enc'], torch.from_numpy(arr['enc']).cuda(), meta['enc_lens']


@pytest.fixture(scope='module')
def model(gold):
    return _model(gold[0])


@pytest.fixture(scope='module')
def weights(gold):
    configs, sd = _state_dict(gold[0])
    sd = {k: v.numpy() for k, v in sd.items()}
    W = TF.weights64(sd, configs['predictor_conf']['num_layers'])
    x = gold[1].astype(np.float64) @ sd['ctc.ctc_lo.weight'].astype(np.float64).T \
        + sd['ctc.ctc_lo.bias'].astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return W, x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


_FORM = {}


def _formulation(gold, weights, cw, tw, beam, split):
    """Per utterance (the fp64 session at the end, its beam after every call of `split`);
    computed once and shared."""
    k = (cw, tw, beam, split)
    if k not in _FORM:
        meta, enc, _, lens = gold
        W, ctc = weights
        out = []
        for b, n in enumerate(lens):
            after = []
            s = SF.run_splits(enc[b, :n], ctc[b, :n], split, W, meta['blank'], beam, cw, tw,
                              after=lambda s, t: after.append((s.result(), s.trailing_blank())))
            out.append((s, after))
        _FORM[k] = out
    return _FORM[k]


def _feed(rs, enc_dev, lens, split, slots, utts=None, after_call=None):
    """Sessions `slots[i]` <- utterance utts[i], all fed with `split` in the same calls (a session
    that is through gets n_t = 0).  Returns the last result of every session."""
    utts = list(range(len(slots))) if utts is None else utts
    plans = [pieces(lens[u], split) for u in utts]
    chunk = max(split)
    at = [0] * len(slots)
    last = [None] * len(slots)
    for call in range(max(len(p) for p in plans)):
        nt = [p[call] if call < len(p) else 0 for p in plans]
        x = torch.zeros((len(slots), chunk, enc_dev.size(2)), device='cuda')
        for i, u in enumerate(utts):
            x[i, :nt[i]] = enc_dev[u, at[i]:at[i] + nt[i]]
            at[i] += nt[i]
        res = rs.advance_encoded(slots, x, nt)
        for i in range(len(slots)):
            if call < len(plans[i]):
                last[i] = res[i]
                if after_call is not None:
                    after_call(i, call, res[i])
            assert res[i].frames_decoded == at[i]
    return last


def _pairs(r):
    return list(zip([list(t) for t in r.nbest], r.nbest_scores))


def _close(got, want, bar):
    assert [t for t, _ in got] == [t for t, _ in want]
    err = max(abs(a - c) for (_, a), (_, c) in zip(got, want))
    assert err <= bar, (err, bar)
    return err


# ---- 1. per call -------------------------------------------------------------------------------
@pytest.mark.parametrize('split', SPLITS, ids=str)
@pytest.mark.parametrize('beam', [1, 5])
@pytest.mark.parametrize('cw,tw', WEIGHTS)
def test_beams_after_every_call(gold, model, weights, cw, tw, beam, split):
    meta, enc, enc_dev, lens = gold
    bar = 4 * meta['e_score'] + 1e-6
    form = _formulation(gold, weights, cw, tw, beam, split)
    rs = _search(model, 4, beam, cw, tw)
    calls, worst = [0], [0.0]

    def after_call(i, call, r):
        want, trailing = form[i][1][call]       # (run_splits makes the same calls, empty ones too)
        worst[0] = max(worst[0], _close(_pairs(r), want, bar))
        assert list(r.tokens) == want[0][0] and r.score == r.nbest_scores[0]
        assert r.trailing_blank == trailing and 0 <= r.trailing_blank <= r.frames_decoded
        calls[0] += 1
    try:
        last = _feed(rs, enc_dev, lens, split, [2, 0, 3], after_call=after_call)
    finally:
        rs.close()
    assert calls[0] == sum(len(f[1]) for f in form)
    print(f'({cw}, {tw}) beam {beam} split {split}: worst score err {worst[0]:.3e}, bar {bar:.3e}')
    run = meta['runs'][f'{cw}_{tw}_{beam}']
    for b, r in enumerate(last):
        _close(_pairs(r), run['fp64'][b], bar)
        assert r.frames_decoded == lens[b]


# ---- 2. bitwise --------------------------------------------------------------------------------
def _bits(st):
    return tuple((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(st.items()))


@pytest.mark.parametrize('beam', [1, 5])
@pytest.mark.parametrize('cw,tw', WEIGHTS)
def test_bitwise_against_the_one_shot_search_and_across_splits(gold, model, weights, cw, tw, beam):
    from wenet_amd.transducer import prefix_beam_search
    meta, enc, enc_dev, lens = gold
    one = prefix_beam_search(model, enc_dev, lens, beam, cw, tw)
    rs = _search(model, 6, beam, cw, tw)
    try:
        want = None
        # (7, 3) and (29, ) hold calls in which a session's n_t is 1, 2, 13 and 14 frames below
        # another's (both buffer parities) and sessions with n_t = 0 beside advancing ones;
        # (2, 0, 5) holds calls in which no session has a frame
        for split, slots, utts in (((4, ), [0, 1, 2], [0, 1, 2]), ((1, ), [0, 1, 2], [0, 1, 2]),
                                   ((7, 3), [5, 3, 4], [0, 1, 2]), ((2, 0, 5), [1, 2, 0], [2, 0, 1]),
                                   ((29, ), [4, 0, 5], [1, 2, 0])):
            rs.reset(slots)
            last = _feed(rs, enc_dev, lens, split, slots, utts)
            for r, u in zip(last, utts):
                assert _pairs(r) == one[u], (split, u)          # lists and score bits
            got = {u: rs.state(s) for s, u in zip(slots, utts)}
            if want is None:
                want = {u: _bits(st) for u, st in got.items()}
                form = _formulation(gold, weights, cw, tw, beam, (4, ))
                for u, st in got.items():
                    s = form[u][0]
                    n = st['n_live']
                    assert n == len(s.hyps) and st['frames'] == lens[u]
                    assert st['tok_len'][:n].tolist() == [len(h) for h, _ in s.hyps]
                    assert st['last_tok'][:n].tolist() == s.last_tok
                    assert st['pending'][:n].tolist() == s.pending
                    assert st['last_time'][:n].tolist() == s.last_time
                    for j, (h, _) in enumerate(s.hyps):
                        assert st['tokens'][j, :len(h)].tolist() == h
                        assert (st['tokens'][j, len(h):lens[u]] == -1).all()
                    # the slots beyond n_live: one fixed form
                    assert np.isneginf(st['score'][n:]).all() and not st['h'][n:].any()
                    assert (st['last_tok'][n:] == meta['blank']).all() and not st['pending'][n:].any()
            for u, st in got.items():
                assert _bits(st) == want[u], (split, u)
        # each session alone
        for u in range(3):
            rs.reset([3])
            _feed(rs, enc_dev, lens, (7, 3), [3], [u])
            assert _bits(rs.state(3)) == want[u], u
    finally:
        rs.close()


# ---- 3. n_t = 0 and reset ----------------------------------------------------------------------
def test_empty_calls_resets_and_reuse(gold, model):
    meta, enc, enc_dev, lens = gold
    rs = _search(model, 3, 5, 0.3, 0.7)
    try:
        fresh = _bits(rs.state(2))
        x = enc_dev[:2, :8].contiguous()
        first = rs.advance_encoded([0, 1], x, [8, 5])
        a, b = _bits(rs.state(0)), _bits(rs.state(1))
        # n_t = 0 leaves a slot bit for bit and returns its beam, alone and beside a session
        # that advances
        r = rs.advance_encoded([0], x[:1], [0])
        assert _bits(rs.state(0)) == a and r[0].frames_decoded == 8
        assert _pairs(r[0]) == _pairs(first[0]) and r[0].trailing_blank == first[0].trailing_blank
        r = rs.advance_encoded([1, 0], enc_dev[[1, 0], 5:9].contiguous(), [4, 0])
        assert _bits(rs.state(0)) == a and _bits(rs.state(1)) != b
        assert _pairs(r[1]) == _pairs(first[0])
        assert r[1].frames_decoded == 8 and r[0].frames_decoded == 9
        b = _bits(rs.state(1))
        # resetting slot 0 leaves slot 1 bit for bit; the reset slot is a fresh one
        rs.reset([0])
        assert _bits(rs.state(1)) == b and _bits(rs.state(0)) == fresh
        st = rs.state(0)
        assert st['n_live'] == 1 and st['frames'] == 0 and st['score'][0] == 0.0
        assert np.isneginf(st['score'][1:]).all() and not st['tok_len'].any()
        assert (st['last_tok'] == meta['blank']).all() and st['pending'].tolist() == [1, 0, 0, 0, 0]
        assert (st['last_time'] == -1).all() and (st['tokens'] == -1).all()
        assert not st['h'].any() and not st['c'].any() and not st['pred_proj'].any()
        r0 = rs.advance_encoded([0], x[:1], [8])
        r2 = rs.advance_encoded([2], x[:1], [8])
        assert _pairs(r0[0]) == _pairs(r2[0]) == _pairs(first[0])
        assert _bits(rs.state(0)) == _bits(rs.state(2)) == a
    finally:
        rs.close()


# ---- 4. the carry step alone -------------------------------------------------------------------
def _carry_run(slots, top_val, top_idx, frame, lens, blank, beam, V, max_tok, frame0, last_time,
               pending, last_tok):
    from wenet_amd import _lib as Lm
    from test_gpu_transducer_beam import _pack, _pack_top
    L = Lm.lib()
    B = len(slots)
    n_live, scores, tok_lens, tokens = _pack(slots, beam, max_tok)
    tv, ti = _pack_top(top_val, top_idx, B, beam)
    ln = np.array(lens, dtype=np.int32)
    o_n = np.full((B, ), -7, dtype=np.int32)
    o_sc = np.zeros((B, beam), dtype=np.float64)
    o_len = np.full((B, beam), -7, dtype=np.int32)
    o_tok = np.full((B, beam, max_tok), -7, dtype=np.int32)
    maps = [np.full((B, beam), -7, dtype=np.int32) for _ in range(6)]
    ins = [np.ascontiguousarray(v, dtype=np.int32) for v in (frame0, last_time, pending, last_tok)]
    st = L.wn_op_rnnt_beam_step_carry(
        B, beam, blank, V, frame, Lm.i32p(ln), max_tok, Lm.i32p(n_live), Lm.f64p(scores),
        Lm.i32p(tok_lens), Lm.i32p(tokens), Lm.f32p(tv), Lm.i32p(ti), *[Lm.i32p(v) for v in ins],
        Lm.i32p(o_n), Lm.f64p(o_sc), Lm.i32p(o_len), Lm.i32p(o_tok), *[Lm.i32p(m) for m in maps],
        torch.cuda.current_stream().cuda_stream)
    assert st == 0, L.wn_last_error()
    out = [[(o_tok[b, j, :o_len[b, j]].tolist(), float(o_sc[b, j])) for j in range(o_n[b])]
           for b in range(B)]
    return (out, *maps)       # src, tok, advance, row_enc, pending, last_time


@pytest.mark.parametrize('last_of_call', [True, False])
@pytest.mark.parametrize('case', BF.hand_cases(), ids=lambda c: c['name'])
def test_carry_step_hand_cases(case, last_of_call):
    """The hand cases with the frame set to the last of the call (and, where the case has a later
    frame, in the middle of one): the slots are the one-shot step's; src is written as usual,
    the owed step goes to `pending`, row_enc stays -1; a finished utterance moves on with an
    identity src and keeps last_tok / pending; last_time follows the hypotheses."""
    from test_gpu_transducer_beam import _same_step
    beam, blank, B = case['beam'], 0, len(case['lens'])
    slots = case['slots']
    for i, f in enumerate(case['frames']):
        frame = case['frame0'] + i
        lens = [min(n, frame + 1) for n in case['lens']] if last_of_call else case['lens']
        # what follows a frame as usual: one frame more than the call has (the formulation's rule)
        more = [n + 1 if frame < n else n for n in lens]
        want, src, tok, adv, row_enc = BF.ref_beam_step(slots, f['top_val'], f['top_idx'], frame,
                                                        more, blank, beam, np.float32)
        assert [[h for h, _ in u] for u in want] == [[h for h, _ in u] for u in f['want']]
        frame0 = [100 * (b + 1) for b in range(B)]
        lt_in = np.array([[10 * b + j - 1 for j in range(beam)] for b in range(B)])
        pend_in = np.ones((B, beam), dtype=np.int64)
        tok_in = np.array([[3 + j for j in range(beam)] for b in range(B)])
        pending = np.zeros((B, beam), dtype=np.int64)
        lt = np.full((B, beam), -1, dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
        for b in range(B):
            n_new = len(want[b])
            if frame >= lens[b]:          # finished: identity, everything kept
                src[b, :n_new] = b * beam + np.arange(n_new)
                tok[b], pending[b], lt[b, :n_new] = tok_in[b], pend_in[b], lt_in[b, :n_new]
                adv[b], row_enc[b] = 0, -1
                continue
            last = frame + 1 == lens[b]
            for s in range(n_new):
                lt[b, s] = frame0[b] + frame if adv[b, s] else lt_in[b, src[b, s] - b * beam]
                if last:
                    pending[b, s], adv[b, s] = adv[b, s], 0
            row_enc[b, :n_new] = -1 if last else off[b] + frame + 1
        got = _carry_run(slots, f['top_val'], f['top_idx'], frame, lens, blank, beam, 16, 6,
                         frame0, lt_in, pend_in, tok_in)
        _same_step(got, (f['want'], src, tok, adv, row_enc, pending, lt))
        if not last_of_call:
            # in the middle of a call the maps are the one-shot step's
            assert [np.asarray(g).tolist() for g in got[1:5]] == [f['src'], f['tok'], f['advance'],
                                                                  f['row_enc']] \
                or any(frame + 1 >= n for n in case['lens'])
        slots = f['want']


# ---- 5. end to end -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sgold():
    return _load('rnnt_beam_stream_tiny.npz')


@pytest.fixture(scope='module')
def smodel(sgold, gold, model):
    same = all(sgold[0][k] == gold[0][k] for k in ('config', 'wseed'))
    return model if same else _model(sgold[0])


def _features(meta):
    from wenet_amd import synthetic as S
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    assert [int(v) for v in flens] == meta['feat_lens']
    return [feats[b, :int(flens[b])].cuda() for b in range(meta['batch'])]


def _stream_all(rec, utts, piece_sizes, finish):
    """The utterances through `rec` in uneven pieces; session i opens at round i.  Returns
    ({i: finish(sid)}, {i: [partials]})."""
    sids, fed, partials, final = {}, {}, {}, {}
    rnd = 0
    while len(final) < len(utts):
        if rnd < len(utts):
            sids[rnd] = rec.open()
            fed[rnd] = 0
            partials[rnd] = []
        for i, sid in sids.items():
            if i in final:
                continue
            k = piece_sizes[(rnd + i) % len(piece_sizes)]
            rec.accept(sid, utts[i][fed[i]:fed[i] + k])
            fed[i] = min(fed[i] + k, utts[i].size(0))
        while True:
            out = rec.step()
            if not out:
                break
            for i, sid in sids.items():
                if sid in out:
                    partials[i].append(out[sid])
        for i, sid in sids.items():
            if i not in final and fed[i] >= utts[i].size(0):
                final[i] = finish(sid)
        rnd += 1
    for sid in sids.values():
        rec.close(sid)
    return final, partials


@pytest.mark.parametrize('cw,tw', [(0.3, 0.7), (0.0, 1.0)])
@pytest.mark.parametrize('c,l', [(4, -1), (3, 2)])
def test_recognizer_end_to_end(sgold, smodel, c, l, cw, tw):
    from wenet_amd import RnntBeamStreamingRecognizer
    from wenet_amd.streaming import RnntBeamStreamSearch
    from wenet_amd.transducer import attention_rescoring
    meta, _ = sgold
    bar = 4 * meta['e_score'] + 1e-6
    utts = _features(meta)
    assert smodel._cfg.dec_layers > 0
    rw = 0.3 if smodel._cfg.dec_r_layers > 0 else 0.0
    kw = dict(attn_weight=0.5, transducer_weight=0.3, ctc_weight=0.2, reverse_weight=rw)
    for beam in (1, 5):
        want = meta['runs'][f'c{c}_l{l}_{cw}_{tw}_{beam}']['fp64']
        rec = RnntBeamStreamingRecognizer(smodel, 3, c, l, beam_size=beam, search_ctc_weight=cw,
                                          search_transducer_weight=tw, max_seconds=2.0)
        assert isinstance(rec.search, RnntBeamStreamSearch)

        def finish(sid):
            plain = rec.finish(sid, rescoring=False)
            again = rec.finish(sid, rescoring=False)        # nothing left: the same beam
            assert _pairs(again) == _pairs(plain)
            enc = rec.encoder_out(sid)
            return plain, rec.finish(sid, rescoring=True, **kw), enc
        final, partials = _stream_all(rec, utts, [23, 50, 7, 64], finish)
        for b in range(3):
            plain, rescored, enc = final[b]
            err = _close(_pairs(plain), want[b], bar)
            print(f'c{c} l{l} ({cw}, {tw}) beam {beam} utt {b}: score err {err:.3e}, bar {bar:.3e}')
            assert plain.frames_decoded == meta['enc_lens'][b] == enc.size(1)
            assert plain.is_endpoint in (None, 'rule1', 'rule2', 'rule3')
            assert partials[b], b
            for p in partials[b]:
                assert p.frames_decoded % c == 0 and 0 <= p.trailing_blank <= p.frames_decoded
                assert 1 <= len(p.nbest) <= beam and list(p.tokens) == list(p.nbest[0])
            # the third transducer mode on the session's final beam, without a second search
            one = attention_rescoring(smodel, enc, [enc.size(1)], beam, rw, kw['ctc_weight'],
                                      kw['attn_weight'], kw['transducer_weight'], cw, tw)[0]
            assert [list(t) for t in rescored.nbest] == [list(t) for t in one.nbest]
            assert list(rescored.tokens) == list(one.tokens)
            assert rescored.nbest_scores == one.nbest_scores and rescored.score == one.score
            assert rescored.frames_decoded == plain.frames_decoded
        rec.search.close()


def test_recognizer_refuses_a_model_without_transducer_weights():
    from gpu_util import cached_model
    from wenet_amd import RnntBeamStreamingRecognizer
    _, _, asr = cached_model('tiny_causal', 0)
    with pytest.raises(TypeError, match='Transducer'):
        RnntBeamStreamingRecognizer(asr, 1, 4)


# ---- 6. refusals -------------------------------------------------------------------------------
def test_refusals_change_no_state(gold, model):
    from gpu_util import cached_model, refusal_text
    from wenet_amd.streaming import RnntBeamStreamSearch
    meta, enc, enc_dev, lens = gold
    _, _, asr = cached_model('tiny_causal', 0)
    with pytest.raises(RuntimeError, match='no transducer weights'):
        RnntBeamStreamSearch(asr._h, asr.device, 2, 5, 32)
    for n_slots in (0, 257):
        with pytest.raises(RuntimeError, match='n_slots'):
            RnntBeamStreamSearch(model._h, model.device, n_slots, 5, 32)
    for beam in (0, 17):
        with pytest.raises(RuntimeError, match=r'beam must be in \[1, 16\]'):
            RnntBeamStreamSearch(model._h, model.device, 2, beam, 32)
    with pytest.raises(RuntimeError, match='max_frames'):
        RnntBeamStreamSearch(model._h, model.device, 2, 5, 0)
    for cw, tw, what in ((-0.1, 0.7, 'must be >= 0'), (0.3, -0.7, 'must be >= 0'),
                         (0.0, 0.0, 'both 0')):
        with pytest.raises(RuntimeError, match=what):
            RnntBeamStreamSearch(model._h, model.device, 2, 5, 32, cw, tw)
    rs = _search(model, 3, 5, 0.3, 0.7, max_frames=12)
    try:
        x = enc_dev[:3, :8].contiguous()
        rs.advance_encoded([0, 1], x[:2], [8, 6])
        before = [_bits(rs.state(s)) for s in range(3)]
        mirror = list(rs.frames)
        who = 'wn_rnnt_beam_stream_advance_encoded'
        for slots, xs, nt, kw, what in (
                ([0, 1, 2, 0], torch.cat([x, x[:1]]), [1, 1, 1, 1], {},
                 ': n must be in [1, n_slots]'),
                ([0, 3], x[:2], [1, 1], {}, ': slot_ids: slot id out of range'),
                ([0, -1], x[:2], [1, 1], {}, ': slot_ids: slot id out of range'),
                ([1, 1], x[:2], [1, 1], {}, ': slot_ids: a slot is named twice in one call (two '
                                            'rows would write one state)'),
                ([0, 1], x[:2], [1, 9], {}, ': n_t: need 0 <= n_t <= chunk'),
                ([0, 1], x[:2], [-1, 1], {}, ': n_t: need 0 <= n_t <= chunk'),
                ([2, 0], x[:2], [1, 5], {},
                 ': the session in slot 0 has 8 frames and would pass max_frames = 12 with 5 '
                 'more; no session was advanced'),
                ([2, 1], x[:2], [4, 1], dict(max_len=6),
                 ': max_len is smaller than a hypothesis may become (7 tokens); no session was '
                 'advanced')):
            with pytest.raises(RuntimeError) as e:
                rs.advance_encoded(slots, xs, nt, **kw)
            assert refusal_text(e.value) == who + what
            assert [_bits(rs.state(s)) for s in range(3)] == before, what
            assert rs.frames == mirror
        with pytest.raises(RuntimeError) as e:
            rs.reset([3])
        assert refusal_text(e.value) == 'wn_rnnt_beam_stream_reset: slot_ids: slot id out of range'
        assert [_bits(rs.state(s)) for s in range(3)] == before
        # the sessions go on as if nothing had happened
        r = rs.advance_encoded([1, 0], enc_dev[[1, 0], 6:10].contiguous(), [2, 4])
        assert [q.frames_decoded for q in r] == [8, 12]
    finally:
        rs.close()
