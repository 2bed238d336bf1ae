"""The fp64 restatement of the stateless predictors (tests/transducer_stateless_formulation.py)
against what the REAL reference recorded (tests/golden/rnnt/rnnt_stateless_tiny.npz,
tools/gen_golden_transducer_stateless.py): the recorded forward_step calls, and -- driven through
the existing formulation searches -- the greedy token lists, the final beams and the transducer
scores of both models.  No GPU."""
import json
import os

import numpy as np
import pytest

import transducer_beam_formulation as BF
import transducer_formulation as TF
import transducer_score_formulation as SCF
import transducer_stateless_formulation as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('tiny_rnnt_embed', 'tiny_rnnt_conv')


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_stateless_tiny.npz'))
    return json.loads(bytes(z['meta']).decode()), z


@pytest.fixture(scope='module')
def cases(gold):
    from wenet_amd import synthetic as S
    meta, z = gold
    out = {}
    for name in CONFIGS:
        configs = S.make_configs(name)
        sd = {k: v.numpy() for k, v in S.make_state_dict(configs, meta[name]['wseed']).items()}
        W = SF.weights64(sd, configs)
        enc = z[f'{name}_enc'].astype(np.float64)
        ctc = enc @ sd['ctc.ctc_lo.weight'].astype(np.float64).T + sd['ctc.ctc_lo.bias']
        ctc = ctc - np.log(np.exp(ctc - ctc.max(-1, keepdims=True)).sum(-1, keepdims=True)) \
            - ctc.max(-1, keepdims=True)
        out[name] = (meta[name], W, enc, ctc)
    return out


def test_windows_are_preceded_by_the_blank_then_by_zeros():
    assert SF.windows([[], [5], [5, 6, 7], [5, 6, 7, 8, 9]], 4, 0).tolist() == \
        [[-1, -1, -1, 0], [-1, -1, 0, 5], [0, 5, 6, 7], [6, 7, 8, 9]]
    assert SF.windows([[], [5, 6]], 1, 2).tolist() == [[2], [6]]


def test_the_lstm_step_is_still_the_lstm_step():
    """Importing the stateless formulation leaves an LSTM weight dict on the LSTM step."""
    rng = np.random.default_rng(0)
    E, H, P = 5, 4, 3
    W = dict(embed=rng.standard_normal((7, E)),
             rnn=[(rng.standard_normal((4 * H, E)), rng.standard_normal((4 * H, H)),
                   rng.standard_normal(4 * H), rng.standard_normal(4 * H))],
             proj=(rng.standard_normal((P, H)), rng.standard_normal(P)))
    h, c = rng.standard_normal((1, 2, H)), rng.standard_normal((1, 2, H))
    out, h2, c2 = TF.predictor_step([1, 3], h, c, W)
    top, h3, c3 = TF.lstm_step(W['embed'][[1, 3]], h, c, W['rnn'])
    assert np.array_equal(out, top @ W['proj'][0].T + W['proj'][1])
    assert np.array_equal(h2, h3) and np.array_equal(c2, c3)


@pytest.mark.parametrize('name', CONFIGS)
def test_recorded_steps(gold, cases, name):
    _, z = gold
    m, W, enc, _ = cases[name]
    C = m['greedy']['context']
    seq = m['greedy']['tokens']['64'][0]
    enc_proj = enc[0] @ W['enc_ffn'][0].T + W['enc_ffn'][1]
    assert len(m['greedy']['step_at']) == 6
    pre_start = slid = False
    for k in m['greedy']['step_at']:
        ctx = z[f'{name}_step{k}_ctx']
        assert ctx.tolist() == SF.windows([seq[:k]], C, m['blank'])[0].tolist()
        pre_start = pre_start or (ctx < 0).any()
        slid = slid or k >= C
        out = SF.predictor_out(ctx[None], W)[0]
        assert np.abs(out - z[f'{name}_step{k}_out']).max() < 1e-12, k
        logits = TF.joint_logits(enc_proj[k], SF.pred_proj(ctx[None], W)[0], W)
        assert np.abs(logits - z[f'{name}_step{k}_logits']).max() < 1e-10, k
    assert slid and (pre_start or C == 1)


@pytest.mark.parametrize('name', CONFIGS)
@pytest.mark.parametrize('n_steps', [64, 3, 1])
def test_greedy_tokens(cases, name, n_steps):
    m, W, enc, _ = cases[name]
    want = m['greedy']['tokens'][str(n_steps)]
    for lookahead in (1, 4, 16):
        got, _ = TF.lookahead_greedy_search(enc, m['enc_lens'], W, m['blank'], n_steps, lookahead)
        assert got == want, lookahead
    C = m['greedy']['context']
    if n_steps == 64:
        assert any(len(u) > C for u in want)        # the window slides off the leading blank
        assert m['greedy']['min_gap_over_bound'] >= 4.0


@pytest.mark.parametrize('name', CONFIGS)
def test_final_beams(cases, name):
    m, W, enc, ctc = cases[name]
    for key, run in m['beam']['runs'].items():
        cw, tw, beam = run['ctc_weight'], run['transducer_weight'], run['beam']
        got = BF.prefix_beam_search(enc, m['enc_lens'], ctc if cw else None, W, m['blank'], beam,
                                    cw, tw, score_dtype=np.float64)
        for g, w in zip(got, run['fp64']):
            assert [t for t, _ in g] == [t for t, _ in w], key
            assert max(abs(a - c) for (_, a), (_, c) in zip(g, w)) < 1e-9, key
    assert m['beam']['min_member_gap'] >= 8 * m['beam']['e_row'] + 2e-6
    assert min(m['beam']['min_cut_gap'], m['beam']['min_final_gap']) >= \
        8 * m['beam']['e_score'] + 2e-6


@pytest.mark.parametrize('name', CONFIGS)
def test_transducer_scores(cases, name):
    m, W, enc, _ = cases[name]
    for key, run in m['rescore']['runs'].items():
        if run['weights'] != m['rescore']['rescore_weights'][1]:
            continue
        for b, u in enumerate(run['fp64']):
            n = m['enc_lens'][b]
            mine = SCF.transducer_scores(enc[b, :n], [t for t, _ in u['nbest']], W, m['blank'])
            assert max(abs(a - c) for a, c in zip(mine, u['td'])) < 1e-9, (key, b)
            best, scores = SCF.combine(u['attn'], [s for _, s in u['nbest']], u['td'],
                                       *[run['weights'][i] for i in (1, 0, 2)])
            assert best == u['winner']
            assert max(abs(a - c) for a, c in zip(scores, u['final'])) < 1e-9
