"""CPU checks of the RNN-T prefix beam search:
 * the fp64 restatement (tests/transducer_beam_formulation.py) against the reference's recorded
   final beams (tests/golden/rnnt/rnnt_beam_tiny.npz, tools/gen_golden_transducer_beam.py):
   the token lists in order, scores within 1e-9 of the fp64 reference and within
   4 e_score + 1e-6 of the fp32 one (e_score: the fixture's measured fp32 score error);
 * ref_beam_step on the hand-written cases; ref_fuse_topk's order;
 * the C ABI without a device: the symbols, a null handle, beam and weights out of range;
 * Transducer.decode knows 'rnnt_beam_search'."""
import inspect
import json
import os

import numpy as np
import pytest

import transducer_beam_formulation as BF
import transducer_formulation as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_beam_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, z['enc'], z['ctc_logp']


@pytest.fixture(scope='module')
def weights(gold):
    from wenet_amd import synthetic as S
    meta = gold[0]
    configs = S.make_configs(meta['config'])
    sd = {k: v.numpy() for k, v in S.make_state_dict(configs, meta['wseed']).items()}
    W = TF.weights64(sd, configs['predictor_conf']['num_layers'])
    # the CTC head in fp64 (ctc.py: log_softmax of ctc_lo)
    x = gold[1].astype(np.float64) @ sd['ctc.ctc_lo.weight'].astype(np.float64).T \
        + sd['ctc.ctc_lo.bias'].astype(np.float64)
    # the fp32 dot-product bound of a logit, twice for the row's log-sum-exp on top
    d = gold[1].shape[-1]
    bound = 2 * (d + 2) * 2.0 ** -24 * (
        np.abs(gold[1]).astype(np.float64) @ np.abs(sd['ctc.ctc_lo.weight']).astype(np.float64).T
        + np.abs(x).max(axis=-1, keepdims=True))
    x = x - x.max(axis=-1, keepdims=True)
    return W, x - np.log(np.exp(x).sum(axis=-1, keepdims=True)), bound


def test_fixture_meta(gold, weights):
    meta, enc, ctc = gold
    assert meta['enc_lens'] == [29, 16, 15] and enc.shape[:2] == (3, 29)
    assert [tuple(w) for w in meta['weights']] == [(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)]
    assert meta['beams'][:3] == [1, 3, 5] and len(meta['runs']) == 3 * len(meta['beams'])
    # what the seed was accepted on
    assert meta['min_member_gap'] >= 8 * meta['e_row'] + 2e-6
    assert min(meta['min_cut_gap'], meta['min_final_gap']) >= 8 * meta['e_score'] + 2e-6
    assert meta['most_fusion_frames'] >= 5
    for key, run in meta['runs'].items():
        # beam 1 never fuses: those runs are the unmodified reference's; a run that fused is the
        # reference with its log_add call mended
        assert run['unmodified'] == (run['beam'] == 1), key
        assert [[t for t, _ in u] for u in run['fp32']] == [[t for t, _ in u] for u in run['fp64']]
    assert any(t == [] for r in meta['runs'].values() for u in r['fp64'] for t, _ in u)
    assert any(meta['runs'][f'{cw}_{tw}_1']['fp64'][b][0][0] != meta['runs'][f'{cw}_{tw}_5']['fp64'][b][0][0]
               for cw, tw in meta['weights'] for b in range(3))
    for b, n in enumerate(meta['enc_lens']):
        # the recorded fp32 log-probs are the CTC head's, up to the fp32 dot-product bound
        assert (np.abs(ctc[b, :n] - weights[1][b, :n]) <= weights[2][b, :n]).all()


@pytest.mark.parametrize('cw,tw', [(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)])
def test_restatement_gives_the_reference_beams(gold, weights, cw, tw):
    meta, enc, _ = gold
    W, ctc64, _ = weights
    tol32 = 4 * meta['e_score'] + 1e-6
    for beam in meta['beams']:
        run = meta['runs'][f'{cw}_{tw}_{beam}']
        got = BF.prefix_beam_search(enc, meta['enc_lens'], ctc64, W, meta['blank'], beam, cw, tw)
        for b in range(meta['batch']):
            assert [t for t, _ in got[b]] == [t for t, _ in run['fp64'][b]], (beam, b)
            assert all(len(t) <= meta['enc_lens'][b] for t, _ in got[b])
            e64 = max(abs(s - r) for (_, s), (_, r) in zip(got[b], run['fp64'][b]))
            e32 = max(abs(s - r) for (_, s), (_, r) in zip(got[b], run['fp32'][b]))
            assert e64 <= 1e-9 and e32 <= tol32, (beam, b, e64, e32)


def _check_frame(out, src, tok, advance, row_enc, f, ulps=0):
    assert len(out) == len(f['want'])
    for o, w in zip(out, f['want']):
        assert [h for h, _ in o] == [h for h, _ in w]
        assert all(BF.same_score(a, c, ulps) for (_, a), (_, c) in zip(o, w)), (o, w)
    assert np.asarray(src).tolist() == f['src'] and np.asarray(tok).tolist() == f['tok']
    assert np.asarray(advance).tolist() == f['advance']
    assert np.asarray(row_enc).tolist() == f['row_enc']


@pytest.mark.parametrize('case', BF.hand_cases(), ids=lambda c: c['name'])
def test_beam_step_hand_cases(case):
    slots = case['slots']
    for i, f in enumerate(case['frames']):
        slots, *maps = BF.ref_beam_step(slots, f['top_val'], f['top_idx'], case['frame0'] + i,
                                        case['lens'], 0, case['beam'])
        _check_frame(slots, *maps, f)


def test_recreated_prefix_needs_the_token_sequence():
    """The case bites: keeping the two [5, 7] candidates of its last frame apart (what an
    identity by creation id does) gives another beam."""
    case = [c for c in BF.hand_cases() if c['name'] == 'recreated_prefix'][0]
    f = case['frames'][2]
    start = case['frames'][1]['want'][0]
    unfused = sorted([BF.add32(start[0][1], f['top_val'][0][0][0]),
                      BF.add32(start[1][1], f['top_val'][0][1][0])], reverse=True)
    assert [h for h, _ in f['want'][0]] == [[5, 7], [5]]
    assert unfused[1] > f['want'][0][1][1]        # the duplicate would have pushed [5] out


def test_fuse_topk_order():
    logits = np.array([0.0, 2.0, 2.0, 0.5, -np.inf, 1.0])
    ctc = np.log(np.full(6, 1.0 / 6))
    ctc[3] = np.nan
    ctc[4] = -np.inf
    f, val, idx = BF.ref_fuse_topk(logits, ctc, 0.5, 0.5, 6)
    assert idx.tolist() == [1, 2, 5, 0, 3, 4]          # ties: lower index; NaN as -inf, in place
    assert np.isnan(f[3]) and np.isneginf(val[4:]).all()
    # a NaN logit poisons the row's sum: every value ranks as -inf, the indices stay columns
    logits[0] = np.nan
    assert BF.ref_fuse_topk(logits, None, 0.0, 1.0, 3)[2].tolist() == [0, 1, 2]
    # the fusion formula as written: log(tw exp(logp) + cw exp(ctc))
    logits = np.array([1.0, 0.5, -0.25, 0.0])
    ctc = np.log(np.array([0.1, 0.2, 0.3, 0.4]))
    p = np.exp(logits) / np.exp(logits).sum()
    f, val, idx = BF.ref_fuse_topk(logits, ctc, 0.3, 0.7, 2)
    assert np.allclose(f, np.log(0.7 * p + 0.3 * np.exp(ctc)), rtol=0, atol=1e-14)
    assert idx.tolist() == np.argsort(-f)[:2].tolist() and np.array_equal(val, f[idx])
    f32, _, _ = BF.ref_fuse_topk(logits.astype(np.float32), ctc, 0.3, 0.7, 2)
    assert f32.dtype == np.float32


def test_log_add2():
    import math
    assert BF.log_add2(-1.0, -1.0) == -1.0 + math.log(2.0)
    assert BF.log_add2(-float('inf'), -2.5) == -2.5
    assert BF.log_add2(-float('inf'), -float('inf')) == -float('inf')
    assert math.isnan(BF.log_add2(float('nan'), 0.0))
    assert BF.log_add2(-3.0, -1.0) == BF.log_add2(-1.0, -3.0)


def test_library_exports_the_beam_search_symbols():
    import ctypes
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    for name in ('wn_transducer_beam_search', 'wn_op_joint_fuse_topk', 'wn_op_rnnt_beam_step'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.wn_transducer_beam_search(None, 5, 0.3, 0.7, None, None, None, None, 0, None) == -1
    assert b'null' in L.wn_last_error()
    # refusals that need no device: the hooks check k / beam and the weights before anything else
    one = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    f4 = (ctypes.c_float * 4)()
    d4 = (ctypes.c_double * 4)()
    dummy = ctypes.cast(f4, ctypes.c_void_p)

    def fuse(k, cw, tw, V=4):
        return L.wn_op_joint_fuse_topk(dummy, 1, dummy, 1, one, one, dummy, dummy, 1, 32, V,
                                       None, 0, None, cw, tw, k, f4, one, None, None)
    for k in (0, 17):
        assert fuse(k, 0.3, 0.7, V=64) == -1 and b'k must be in [1, 16]' in L.wn_last_error()
    assert fuse(5, 0.3, 0.7) == -1 and b'larger than the vocabulary' in L.wn_last_error()
    assert fuse(2, -0.1, 0.7) == -1 and b'must be >= 0' in L.wn_last_error()
    assert fuse(2, 0.3, -1.0) == -1 and b'must be >= 0' in L.wn_last_error()
    assert fuse(2, 0.0, 0.0) == -1 and b'both 0' in L.wn_last_error()
    assert fuse(2, 0.3, 0.7) == -1 and b'without CTC log-probs' in L.wn_last_error()

    def step(beam, n_live=1, idx=0):
        nl = (ctypes.c_int32 * 1)(n_live)
        ti = (ctypes.c_int32 * 256)(*([idx] * 256))
        tv = (ctypes.c_float * 256)()
        z = (ctypes.c_int32 * 64)()
        return L.wn_op_rnnt_beam_step(1, beam, 0, 4, 0, (ctypes.c_int32 * 1)(2), 2, nl, d4, z, z,
                                      tv, ti, z, d4, z, z, z, z, z, z, None)
    for beam in (0, 17):
        assert step(beam) == -1 and b'beam must be in [1, 16]' in L.wn_last_error()
    assert step(2, n_live=3) == -1 and b'live count' in L.wn_last_error()
    assert step(2, idx=4) == -1 and b'outside the vocabulary' in L.wn_last_error()
    assert step(2, idx=-1) == -1 and b'outside the vocabulary' in L.wn_last_error()


def test_decode_knows_the_mode():
    from wenet_amd import transducer as T
    assert T.RNNT_BEAM_METHOD == 'rnnt_beam_search'
    sig = inspect.signature(T.Transducer.decode).parameters
    assert sig['search_ctc_weight'].default == 0.3
    assert sig['search_transducer_weight'].default == 0.7
    sig = inspect.signature(T.Transducer.beam_search).parameters
    assert list(sig)[1:] == ['speech', 'speech_lengths', 'decoding_chunk_size', 'beam_size',
                             'num_decoding_left_chunks', 'simulate_streaming', 'ctc_weight',
                             'transducer_weight']
    assert (sig['beam_size'].default, sig['ctc_weight'].default,
            sig['transducer_weight'].default) == (5, 0.3, 0.7)
    src = inspect.getsource(T.Transducer.decode)
    assert 'RNNT_BEAM_METHOD in methods' in src
    assert inspect.signature(T.prefix_beam_search).parameters['beam_size'].default == 5
