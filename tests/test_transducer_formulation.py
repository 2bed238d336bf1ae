"""The lock-step lookahead formulation of the RNN-T greedy search (tests/transducer_formulation.py,
what csrc/transducer.hip implements) against the REAL reference's recorded results
(tests/golden/rnnt/rnnt_tiny.npz, tools/gen_golden_transducer.py): token lists for every n_steps and
lookahead, the blank-heavy model, and four predictor / joint steps."""
import json
import os

import numpy as np
import pytest

import transducer_formulation as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, {k: z[k] for k in z.files if k != 'meta'}


def _weights(meta, bias=None):
    from wenet_amd import synthetic as S
    configs = S.make_configs(meta['config'])
    sd = S.make_state_dict(configs, meta['wseed'],
                           rnnt_blank_bias=meta['blank_bias'] if bias is None else bias)
    return TF.weights64({k: v.numpy() for k, v in sd.items()},
                        configs['predictor_conf']['num_layers'])


@pytest.fixture(scope='module')
def weights(gold):
    return _weights(gold[0])


def test_fixture_meets_its_conditions(gold):
    meta, _ = gold
    assert meta['enc_lens'] == [29, 16, 15]
    assert meta['min_gap_over_bound'] >= 4.0 and meta['heavy']['ratio'] >= 4.0
    assert any(len(u) == 0 for u in meta['heavy']['tokens'])
    assert any(len(u) > 0 for u in meta['tokens']['64'])


@pytest.mark.parametrize('lookahead', [1, 4, 8, 16])
@pytest.mark.parametrize('n_steps', [64, 3, 1])
def test_tokens_equal_the_reference(gold, weights, n_steps, lookahead):
    meta, arr = gold
    toks, steps = TF.lookahead_greedy_search(arr['enc'], meta['enc_lens'], weights, meta['blank'],
                                             n_steps, lookahead)
    assert toks == meta['tokens'][str(n_steps)]
    assert all(len(u) <= n * n_steps for u, n in zip(toks, meta['enc_lens']))
    # about U + T' / F steps for the longest-running utterance
    assert steps <= max(len(u) + -(-n // lookahead) for u, n in zip(toks, meta['enc_lens']))


def test_lookahead_saves_steps(gold, weights):
    meta, arr = gold
    s1 = TF.lookahead_greedy_search(arr['enc'], meta['enc_lens'], weights, meta['blank'], 3, 1)[1]
    s8 = TF.lookahead_greedy_search(arr['enc'], meta['enc_lens'], weights, meta['blank'], 3, 8)[1]
    assert s8 < s1


@pytest.mark.parametrize('lookahead', [1, 4, 16])
def test_blank_heavy_model(gold, lookahead):
    meta, arr = gold
    W = _weights(meta, meta['heavy']['bias'])
    toks, _ = TF.lookahead_greedy_search(arr['enc'], meta['enc_lens'], W, meta['blank'], 64,
                                         lookahead)
    assert toks == meta['heavy']['tokens']


def test_each_utterance_alone_and_reordered(gold, weights):
    meta, arr = gold
    want = meta['tokens']['3']
    for b in range(3):
        got, _ = TF.lookahead_greedy_search(arr['enc'][b:b + 1], meta['enc_lens'][b:b + 1],
                                            weights, meta['blank'], 3, 4)
        assert got == [want[b]]
    order = [2, 0, 1]
    got, _ = TF.lookahead_greedy_search(arr['enc'][order], [meta['enc_lens'][b] for b in order],
                                        weights, meta['blank'], 3, 4)
    assert got == [want[b] for b in order]


def test_recorded_predictor_and_joint_steps(gold, weights):
    """fp64 against the reference's fp32: 1e-5 relative to the largest entry of each tensor."""
    meta, arr = gold
    W = weights
    for k, tok in zip(meta['step_at'], meta['step_tokens']):
        h = arr[f'step{k}_h_in'].astype(np.float64)[:, None]
        c = arr[f'step{k}_c_in'].astype(np.float64)[:, None]
        out, h2, c2 = TF.predictor_step([tok], h, c, W)
        enc_proj = arr['enc'][0, k].astype(np.float64) @ W['enc_ffn'][0].T + W['enc_ffn'][1]
        pred_proj = out[0] @ W['pred_ffn'][0].T + W['pred_ffn'][1]
        logits = TF.joint_logits(enc_proj[None], pred_proj[None], W)[0]
        for name, got in (('out', out[0]), ('h', h2[:, 0]), ('c', c2[:, 0]), ('logits', logits)):
            ref = arr[f'step{k}_{name}'].astype(np.float64)
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
            assert err <= 1e-5, (k, name, err)


def test_argmax_rule_is_torch_argmax_and_stays_inside_the_vocabulary():
    """Lowest index on ties; a NaN beats every number and the first NaN wins, so whatever a joint
    row holds the index is a column in [0, V) (the next embedding row).  The kernels' merge
    (csrc/transducer.hip: argmax_merge, rnnt_reduce_row) implements this rule."""
    import torch
    nan, inf = float('nan'), float('inf')
    rows = np.array([[0.5, 2.0, 2.0, -1.0, 2.0],
                     [nan, nan, nan, nan, nan],
                     [1.0, inf, nan, 3.0, nan],
                     [-inf, -inf, -inf, -inf, -inf],
                     [0.0, -0.0, 0.0, -1.0, -2.0],
                     [inf, 1.0, inf, 2.0, 0.0]])
    got = TF.argmax_rows(rows)
    assert got.tolist() == [1, 0, 2, 0, 0, 0]
    assert got.tolist() == torch.argmax(torch.from_numpy(rows), dim=1).tolist()
    assert got.tolist() == torch.argmax(torch.from_numpy(rows).float(), dim=1).tolist()
    rng = np.random.default_rng(5)
    big = rng.standard_normal((64, 300))
    big[rng.random(big.shape) < 0.01] = nan
    big[:, 17] = big[:, 250]
    got = TF.argmax_rows(big)
    assert got.tolist() == torch.argmax(torch.from_numpy(big), dim=1).tolist()
    assert ((got >= 0) & (got < 300)).all()


def test_a_nan_frame_decodes_as_blank_and_the_search_ends(gold, weights):
    """A NaN in an encoder frame makes every logit of its joint rows NaN: index 0, the blank, so
    the frame emits nothing and every token stays inside the vocabulary."""
    meta, z = gold
    assert meta['blank'] == 0
    enc = z['enc'].copy()
    enc[0, 3, 5] = np.nan
    V = weights['ffn_out'][0].shape[0]
    for F in (1, 8):
        toks, steps = TF.lookahead_greedy_search(enc, meta['enc_lens'], weights, meta['blank'], 3, F)
        assert all(0 <= t < V for u in toks for t in u)
        assert toks[1:] == meta['tokens']['3'][1:]
        assert steps <= max(meta['enc_lens']) * 4 + 1
