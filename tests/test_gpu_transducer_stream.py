"""Streaming transducer sessions on the GPU (csrc/transducer_stream.hip,
csrc/cabi_transducer_stream.hip, wenet_amd/streaming.py): the resumable RNN-T greedy search on
the recorded encoder output of tests/golden/rnnt/rnnt_tiny.npz, three sessions at once with
their own lengths, against the fp64 session formulation (tests/transducer_stream_formulation.py)
after every call and the reference's recorded token lists at the end; the bitwise invariance of
a session's state; the blank-heavy and the wide-vocabulary model; StreamingRecognizer end to end
against the reference's chunk-masked results (tests/golden/rnnt/rnnt_stream_tiny.npz); the
refusals.  The formulation is a reference here because the fixtures' deciding joint rows have a
top-two gap of at least 4 x the fp32 dot-product bound (their generators' condition)."""
import json
import os

import numpy as np
import pytest
import torch

import transducer_formulation as TF
import transducer_stream_formulation as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = [(1, ), (4, ), (7, 3), (2, 0, 5), (29, )]


def _load(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', name))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, {k: z[k] for k in z.files if k != 'meta'}


def _state_dict(meta, bias=None):
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    return configs, S.make_state_dict(
        configs, meta['wseed'], rnnt_blank_bias=meta['blank_bias'] if bias is None else bias)


def _model(meta, bias=None):
    from wenet_amd import Transducer
    configs, sd = _state_dict(meta, bias)
    return Transducer(configs, sd, device='cuda')


def _weights(meta, bias=None):
    configs, sd = _state_dict(meta, bias)
    return TF.weights64({k: v.numpy() for k, v in sd.items()},
                        configs['predictor_conf']['num_layers'])


def _search(model, n_slots, max_frames=32, max_tokens=None, n_steps=64):
    from wenet_amd.streaming import RnntStreamSearch
    tc = model._tcfg
    return RnntStreamSearch(model._h, model.device, n_slots, max_frames,
                            max_tokens or max_frames * n_steps, n_steps,
                            dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))


@pytest.fixture(scope='module')
def gold():
    meta, arr = _load('rnnt_tiny.npz')
    return meta, arr['enc'], torch.from_numpy(arr['enc']).cuda(), meta['enc_lens']


@pytest.fixture(scope='module')
def model(gold):
    return _model(gold[0])


@pytest.fixture(scope='module')
def weights(gold):
    return _weights(gold[0])


_FORM = {}


def _formulation(key, enc, lens, W, blank, n_steps, split):
    """Per utterance the fp64 sessions' token lists after every call of `split` (computed once:
    the lists do not depend on the window, tests/test_transducer_stream_formulation.py)."""
    k = (key, n_steps, split)
    if k not in _FORM:
        _FORM[k] = [SF.run_session(enc[b], n, W, blank, n_steps, 4, split)
                    for b, n in enumerate(lens)]
    return _FORM[k]


def _feed(rs, enc_dev, lens, split, slots, utts=None, after_call=None):
    """Sessions `slots[i]` <- utterance utts[i], all fed with `split` in the same calls (a session
    that is through gets n_t = 0).  Returns the last result of every session."""
    utts = list(range(len(slots))) if utts is None else utts
    plans = [SF.pieces(lens[u], split) for u in utts]
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


# ---- token parity per call ---------------------------------------------------------------------
@pytest.mark.parametrize('split', SPLITS, ids=str)
@pytest.mark.parametrize('lookahead', [1, 4, 16])
@pytest.mark.parametrize('n_steps', [64, 3, 1])
def test_tokens_after_every_call(gold, model, weights, n_steps, lookahead, split):
    meta, enc, enc_dev, lens = gold
    form = _formulation('tiny', enc, lens, weights, meta['blank'], n_steps, split)
    rs = _search(model, 4, n_steps=n_steps)
    assert model.tune('rnnt_lookahead', lookahead) == lookahead
    calls = [0]

    def after_call(i, call, r):
        want = form[i][1][call]
        assert list(r.tokens) == want, (i, call)
        assert len(r.times) == len(want)
        calls[0] += 1
    try:
        last = _feed(rs, enc_dev, lens, split, [2, 0, 3], after_call=after_call)
    finally:
        model.tune('rnnt_lookahead', 'inherit')
        rs.close()
    assert calls[0] == sum(len(f[1]) for f in form)
    for b, r in enumerate(last):
        s = form[b][0]
        assert list(r.tokens) == meta['tokens'][str(n_steps)][b]
        assert r.times == s.times
        assert r.frames_decoded == lens[b] and r.trailing_blank == s.trailing_blank
        assert all(a <= c for a, c in zip(r.times, r.times[1:]))
        if r.times:
            assert np.bincount(r.times).max() <= n_steps


# ---- bitwise state -----------------------------------------------------------------------------
def _bits(state):
    h, c, pp, sc = state
    return h.tobytes(), c.tobytes(), pp.tobytes(), tuple(sorted(sc.items()))


def test_state_is_bitwise_independent_of_split_slot_batch_and_window(gold, model, weights):
    meta, enc, enc_dev, lens = gold
    n_steps = 3
    form = _formulation('tiny', enc, lens, weights, meta['blank'], n_steps, (4, ))
    rs = _search(model, 6, n_steps=n_steps)
    try:
        _feed(rs, enc_dev, lens, (4, ), [0, 1, 2])
        ref = [rs.state(s) for s in (0, 1, 2)]
        for b, (h, c, pp, sc) in enumerate(ref):
            s = form[b][0]
            assert sc == dict(last_tok=s.last_tok, stale=s.stale, n_tok=len(s.tokens),
                              frames=lens[b], trailing_blank=s.trailing_blank)
        want = [_bits(r) for r in ref]
        # other splits, other slots, a permuted call order
        for split, slots, utts in (((1, ), [0, 1, 2], [0, 1, 2]), ((7, 3), [5, 3, 4], [0, 1, 2]),
                                   ((2, 0, 5), [1, 2, 0], [2, 0, 1]), ((29, ), [4, 0, 5], [1, 2, 0])):
            rs.reset(slots)
            _feed(rs, enc_dev, lens, split, slots, utts)
            for s, u in zip(slots, utts):
                assert _bits(rs.state(s)) == want[u], (split, s, u)
        # each session alone, with another window
        model.tune('rnnt_lookahead', 16)
        for u in range(3):
            rs.reset([3])
            _feed(rs, enc_dev, lens, (7, 3), [3], [u])
            assert _bits(rs.state(3)) == want[u], u
    finally:
        model.tune('rnnt_lookahead', 'inherit')
        rs.close()


def test_empty_calls_resets_and_reuse(gold, model):
    meta, enc, enc_dev, lens = gold
    rs = _search(model, 3, n_steps=3)
    try:
        x = enc_dev[:2, :8].contiguous()
        rs.advance_encoded([0, 1], x, [8, 5])
        a, b = _bits(rs.state(0)), _bits(rs.state(1))
        # n_t = 0 leaves a slot bit for bit, alone and beside a session that advances
        r = rs.advance_encoded([0], x[:1], [0])
        assert _bits(rs.state(0)) == a and r[0].frames_decoded == 8
        r = rs.advance_encoded([1, 0], enc_dev[[1, 0], 5:9].contiguous(), [4, 0])
        assert _bits(rs.state(0)) == a and _bits(rs.state(1)) != b
        assert r[1].frames_decoded == 8 and r[0].frames_decoded == 9
        b = _bits(rs.state(1))
        # resetting slot 0 leaves slot 1 bit for bit; the reset slot is a fresh one
        fresh = _bits(rs.state(2))
        rs.reset([0])
        assert _bits(rs.state(1)) == b and _bits(rs.state(0)) == fresh
        h, c, pp, sc = rs.state(0)
        assert not h.any() and not c.any() and not pp.any()
        assert sc == dict(last_tok=meta['blank'], stale=1, n_tok=0, frames=0, trailing_blank=0)
        r0 = rs.advance_encoded([0], x[:1], [8])
        r2 = rs.advance_encoded([2], x[:1], [8])
        assert list(r0[0].tokens) == list(r2[0].tokens) and r0[0].times == r2[0].times
        assert _bits(rs.state(0)) == _bits(rs.state(2)) == a
    finally:
        rs.close()


# ---- other models ------------------------------------------------------------------------------
def test_blank_heavy_model_gives_empty_results(gold):
    meta, enc, enc_dev, lens = gold
    heavy = _model(meta, meta['heavy']['bias'])
    rs = _search(heavy, 3)
    try:
        last = _feed(rs, enc_dev, lens, (7, 3), [0, 1, 2])
    finally:
        rs.close()
    assert [list(r.tokens) for r in last] == meta['heavy']['tokens']
    assert any(len(r.tokens) == 0 for r in last)
    for r, n in zip(last, lens):
        if not r.tokens:
            assert r.trailing_blank == r.frames_decoded == n and r.times == []


def test_wide_vocabulary(gold):
    """65 x 128 + 9 tokens: 66 column-block partials per joint row, reduced by the advance
    kernel's wave (tests/test_gpu_transducer.py builds the case and states its conditions)."""
    from test_gpu_transducer import WIDE_SEED, _wide_case
    from wenet_amd import Transducer
    configs, sd, enc, lens, tokens, facts = _wide_case(WIDE_SEED)
    assert facts['min_ratio'] >= 4.0 and tokens[1] == tokens[5] == tokens[16]
    W = TF.weights64({k: v.numpy() for k, v in sd.items()}, 2)
    form = [SF.run_session(enc[b], n, W, 0, 3, 5, (5, )) for b, n in enumerate(lens)]
    assert [f[0].tokens for f in form] == tokens[1]
    assert any(t >= 64 * 128 for u in tokens[1] for t in u)
    wide = Transducer(configs, sd, device='cuda')
    rs = _search(wide, 3, n_steps=3)
    wide.tune('rnnt_lookahead', 5)

    def after_call(i, call, r):
        assert list(r.tokens) == form[i][1][call], (i, call)
    try:
        last = _feed(rs, torch.from_numpy(enc).cuda(), lens, (5, ), [1, 2, 0],
                     after_call=after_call)
    finally:
        wide.tune('rnnt_lookahead', 'inherit')
        rs.close()
    assert [list(r.tokens) for r in last] == tokens[1]
    assert [r.times for r in last] == [f[0].times for f in form]


# ---- end to end --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sgold():
    return _load('rnnt_stream_tiny.npz')


@pytest.fixture(scope='module')
def smodel(sgold, gold, model):
    same = all(sgold[0][k] == gold[0][k] for k in ('config', 'wseed', 'blank_bias'))
    return model if same else _model(sgold[0])


def _features(meta):
    from wenet_amd import synthetic as S
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    assert [int(v) for v in flens] == meta['feat_lens']
    return [feats[b, :int(flens[b])].cuda() for b in range(meta['batch'])]


def _stream_all(rec, utts, piece_sizes):
    """The utterances through `rec` in uneven pieces; session i opens at round i.  Returns
    ({i: final result}, {i: [partials]})."""
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
                final[i] = rec.finish(sid)
        rnd += 1
    for sid in sids.values():
        rec.close(sid)
    return final, partials


@pytest.mark.parametrize('n_steps', [64, 3])
@pytest.mark.parametrize('c,l', [(4, -1), (3, 2)])
def test_recognizer_end_to_end(sgold, smodel, c, l, n_steps):
    from wenet_amd.streaming import RnntStreamSearch, StreamingRecognizer
    meta, _ = sgold
    want = meta['tokens'][f'c{c}_l{l}'][str(n_steps)]
    utts = _features(meta)
    rec = StreamingRecognizer(smodel, 3, c, l, max_seconds=2.0, search='rnnt_greedy_search',
                              n_steps=n_steps, max_tokens=64 * 64)
    assert isinstance(rec.search, RnntStreamSearch)
    final, partials = _stream_all(rec, utts, [23, 50, 7, 64])
    for b in range(3):
        r = final[b]
        assert list(r.tokens) == want[b], b
        assert r.frames_decoded == meta['enc_lens'][b] and len(r.times) == len(want[b])
        assert r.is_endpoint in (None, 'rule1', 'rule2', 'rule3')
        assert partials[b], b
        for p in partials[b]:
            assert list(p.tokens) == want[b][:len(p.tokens)]
            assert p.frames_decoded % c == 0 and 0 <= p.trailing_blank <= p.frames_decoded
            assert p.is_endpoint in (None, 'rule1', 'rule2', 'rule3')
    rec.search.close()


def test_recognizer_modes(sgold, smodel):
    """The default search is the CTC prefix beam search as before; the RNN-T mode refuses a model
    without transducer weights and an unknown mode is an error."""
    from gpu_util import cached_model
    from wenet_amd.streaming import StreamingRecognizer, StreamSearch
    meta, _ = sgold
    utts = _features(meta)
    got = []
    for kw in ({}, dict(search='ctc_prefix_beam_search')):
        rec = StreamingRecognizer(smodel, 3, 4, -1, max_seconds=2.0, **kw)
        assert type(rec.search) is StreamSearch and not rec.rnnt
        final, _ = _stream_all(rec, utts, [23, 50, 7, 64])
        got.append([(list(final[b].tokens), final[b].score) for b in range(3)])
        rec.search.close()
    assert got[0] == got[1]
    # ... the result of the one-shot chunk-masked decode of the same utterances
    for b, f in enumerate(utts):
        one = smodel.decode(['attention_rescoring'], f[None], torch.tensor([f.size(0)]),
                            beam_size=10, decoding_chunk_size=4, num_decoding_left_chunks=-1,
                            ctc_weight=0.5)['attention_rescoring'][0]
        assert got[0][b][0] == list(one.tokens), b
    _, _, asr = cached_model('tiny_causal', 0)
    with pytest.raises(TypeError, match='Transducer'):
        StreamingRecognizer(asr, 1, 4, search='rnnt_greedy_search')
    with pytest.raises(ValueError, match='rnnt_beam_search'):
        StreamingRecognizer(smodel, 1, 4, search='rnnt_beam_search')


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals_change_no_state(gold, model):
    from gpu_util import cached_model, refusal_text
    from wenet_amd.streaming import RnntStreamSearch
    meta, enc, enc_dev, lens = gold
    _, _, asr = cached_model('tiny_causal', 0)
    with pytest.raises(RuntimeError, match='no transducer weights'):
        RnntStreamSearch(asr._h, asr.device, 2, 32, 64)
    for n_slots in (0, 257):
        with pytest.raises(RuntimeError, match='n_slots'):
            RnntStreamSearch(model._h, model.device, n_slots, 32, 64)
    rs = _search(model, 3, max_frames=12, max_tokens=40, n_steps=3)
    try:
        x = enc_dev[:3, :8].contiguous()
        rs.advance_encoded([0, 1], x[:2], [8, 6])
        before = [_bits(rs.state(s)) for s in range(3)]
        mirrors = (list(rs.frames), list(rs.n_tok))
        who = 'wn_rnnt_stream_advance_encoded'
        # the last case: what slots 2 / 1 may hold after 4 / 1 more frames of 3 tokens each
        need = max(min(mirrors[1][2] + 4 * 3, 40), min(mirrors[1][1] + 1 * 3, 40))
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
                ([2, 1], x[:2], [4, 1], dict(max_len=5),
                 ": max_len is smaller than a session's token count may become (%d tokens); no "
                 'session was advanced' % need)):
            with pytest.raises(RuntimeError) as e:
                rs.advance_encoded(slots, xs, nt, **kw)
            assert refusal_text(e.value) == who + what
            assert [_bits(rs.state(s)) for s in range(3)] == before, what
            rs.frames, rs.n_tok = list(mirrors[0]), list(mirrors[1])
        with pytest.raises(RuntimeError) as e:
            rs.reset([3])
        assert refusal_text(e.value) == 'wn_rnnt_stream_reset: slot_ids: slot id out of range'
        assert [_bits(rs.state(s)) for s in range(3)] == before
        # the sessions go on as if nothing had happened
        r = rs.advance_encoded([1, 0], enc_dev[[1, 0], 6:10].contiguous(), [2, 4])
        assert [q.frames_decoded for q in r] == [8, 12]
    finally:
        rs.close()


def test_token_buffer_overflow(gold, model):
    """A session whose tokens pass max_tokens keeps counting and stops storing; the call says so;
    after a reset the slot is a fresh one."""
    meta, enc, enc_dev, lens = gold
    full = meta['tokens']['64'][0]
    assert len(full) > 3
    rs = _search(model, 2, max_tokens=3, n_steps=64)
    try:
        x = enc_dev[:2, :lens[0]].contiguous()
        with pytest.raises(RuntimeError, match='token buffer overflow'):
            rs.advance_encoded([0, 1], x, [lens[0], 0])
        sc = rs.state(0)[3]
        assert sc['n_tok'] == len(full) and sc['frames'] == lens[0]
        assert rs.state(1)[3] == dict(last_tok=meta['blank'], stale=1, n_tok=0, frames=0,
                                      trailing_blank=0)
        rs.reset([0])
        r = rs.advance_encoded([0], x[:1, :1].contiguous(), [1])
        assert r[0].frames_decoded == 1 and list(r[0].tokens) == full[:len(r[0].tokens)]
    finally:
        rs.close()
