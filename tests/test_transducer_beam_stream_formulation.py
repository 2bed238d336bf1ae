"""CPU checks of the resumable RNN-T prefix beam search's fp64 formulation
(tests/transducer_beam_stream_formulation.py):
 * a BeamSession fed the one-shot fixture's encoder output (tests/golden/rnnt/rnnt_beam_tiny.npz)
   in pieces equals transducer_beam_formulation.prefix_beam_search on the frames so far after
   EVERY call -- tokens, order, scores within 1e-9 -- and the reference's recorded fp64 beams at
   the end;
 * the new fixture (tests/golden/rnnt/rnnt_beam_stream_tiny.npz,
   tools/gen_golden_transducer_beam_stream.py: the real reference behind its chunk-masked
   encoder): what its seed was accepted on, its recorded beams, and that the variant that drops
   `pending` decodes another beam on it."""
import functools
import json
import os

import numpy as np
import pytest

import transducer_beam_formulation as BF
import transducer_beam_stream_formulation as SF
import transducer_formulation as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = [(1, ), (4, ), (7, 3), (2, 0, 5), (29, )]
WEIGHTS = [(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)]


def _load(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', name))
    return json.loads(bytes(z['meta']).decode()), z


def _weights(meta):
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    sd = {k: v.numpy() for k, v in S.make_state_dict(configs, meta['wseed']).items()}
    return TF.weights64(sd, configs['predictor_conf']['num_layers']), sd


def _ctc64(enc, sd):
    """The CTC head in fp64 (ctc.py: log_softmax of ctc_lo)."""
    x = enc.astype(np.float64) @ sd['ctc.ctc_lo.weight'].astype(np.float64).T \
        + sd['ctc.ctc_lo.bias'].astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


@pytest.fixture(scope='module')
def gold():
    meta, z = _load('rnnt_beam_tiny.npz')
    W, sd = _weights(meta)
    enc = z['enc']
    return meta, enc, _ctc64(enc, sd), W


@pytest.fixture(scope='module')
def sgold():
    meta, z = _load('rnnt_beam_stream_tiny.npz')
    W, sd = _weights(meta)
    encs = {k[4:]: z[k] for k in z.files if k.startswith('enc_')}
    return meta, encs, {k: _ctc64(e, sd) for k, e in encs.items()}, W


def _same(got, want, tol):
    assert [t for t, _ in got] == [t for t, _ in want]
    assert max(abs(a - c) for (_, a), (_, c) in zip(got, want)) <= tol


@pytest.mark.parametrize('cw,tw', WEIGHTS)
@pytest.mark.parametrize('beam', [1, 5])
def test_session_equals_the_search_on_the_prefix(gold, cw, tw, beam):
    meta, enc, ctc, W = gold
    blank = meta['blank']

    @functools.lru_cache(maxsize=None)
    def on_prefix(b, t):
        return BF.prefix_beam_search(enc[b:b + 1, :t], [t], ctc[b:b + 1, :t], W, blank, beam, cw,
                                     tw)[0]
    run = meta['runs'][f'{cw}_{tw}_{beam}']
    for split in SPLITS:
        for b, n in enumerate(meta['enc_lens']):
            calls = []

            def after(s, t):
                calls.append(t)
                _same(s.result(), on_prefix(b, t), 1e-9)
                assert s.frames == t and 0 <= s.trailing_blank() <= t
            s = SF.run_splits(enc[b, :n], ctc[b, :n], split, W, blank, beam, cw, tw, after=after)
            assert calls[-1] == n and s.frames == n
            _same(s.result(), run['fp64'][b], 1e-9)
            # an empty call changes nothing
            before = (s.result(), list(s.pending), list(s.last_time), s.frames)
            s.advance(enc[b, :0], ctc[b, :0])
            assert (s.result(), list(s.pending), list(s.last_time), s.frames) == before


def test_stream_fixture_meta(sgold):
    meta, encs, _, _ = sgold
    assert meta['enc_lens'] == [29, 16, 15]
    assert [tuple(c) for c in meta['chunks']] == [(4, -1), (3, 2)]
    assert sorted(encs) == ['c3_l2', 'c4_l-1'] and all(e.shape[:2] == (3, 29) for e in encs.values())
    assert [tuple(w) for w in meta['weights']] == [(0.3, 0.7), (0.0, 1.0)]
    assert meta['beams'] == [1, 5] and len(meta['runs']) == 2 * 2 * 2
    # what the seed was accepted on
    assert meta['min_member_gap'] >= 8 * meta['e_row'] + 2e-6
    assert min(meta['min_cut_gap'], meta['min_final_gap']) >= 8 * meta['e_score'] + 2e-6
    assert meta['n_pending_at'] >= 1 and meta['n_fusion_at'] >= 1
    for kk, cw, tw, beam, b, t in meta['pending_at'] + meta['fusion_at']:
        c = int(kk[1:kk.index('_')])
        assert (t + 1) % c == 0 and t + 1 < meta['enc_lens'][b]
    for k, run in meta['runs'].items():
        # beam 1 never fuses: those runs are the unmodified reference's
        assert run['unmodified'] or run['beam'] > 1, k
        assert [[t for t, _ in u] for u in run['fp32']] == [[t for t, _ in u] for u in run['fp64']]


def test_sessions_on_the_stream_fixture(sgold):
    """Chunk by chunk on the reference's chunk-masked encoder output: the recorded beams; the
    variant that forgets the owed predictor step decodes something else."""
    meta, encs, ctcs, W = sgold
    tol32 = 4 * meta['e_score'] + 1e-6
    for k, run in meta['runs'].items():
        kk = f"c{run['chunk']}_l{run['left']}"
        cw, tw, beam, c = run['ctc_weight'], run['transducer_weight'], run['beam'], run['chunk']
        differs = 0
        for b, n in enumerate(meta['enc_lens']):
            rows, crow = encs[kk][b, :n], ctcs[kk][b, :n]
            s = SF.run_splits(rows, crow, (c, ), W, meta['blank'], beam, cw, tw)
            _same(s.result(), run['fp64'][b], 1e-9)
            _same(s.result(), run['fp32'][b], tol32)
            # the fixture's rule: a token lands on the last frame of a chunk inside an utterance
            assert [e['frame'] for e in s.events] == list(range(n))
            d = SF.run_splits(rows, crow, (c, ), W, meta['blank'], beam, cw, tw, drop_pending=True)
            same_lists = [t for t, _ in d.result()] == [t for t, _ in s.result()]
            if not same_lists or max(abs(a - e) for (_, a), (_, e)
                                     in zip(d.result(), s.result())) > tol32:
                differs += 1
        assert differs >= 1, k
