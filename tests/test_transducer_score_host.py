"""CPU checks of the transducer score's host side, no device:
 * wn_op_rnnt_trie (csrc/rnnt_trie.h) on hand cases and on 200 random n-bests against the
   restatement's trie (tests/transducer_score_formulation.py), word for word;
 * the new symbols are exported and declared;
 * wn_transducer_score / wn_op_* refuse bad arguments before any HIP call;
 * transducer_attention_rescoring / decode reject an unknown beam_search_type."""
import ctypes
import os

import numpy as np
import pytest
import torch

import transducer_score_formulation as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('wn_transducer_score', 'wn_transducer_score_stats', 'wn_op_rnnt_trie',
       'wn_op_joint_logp_gather', 'wn_op_rnnt_lattice')


def op_trie(hyps, blank, max_len=None):
    """wn_op_rnnt_trie -> the restatement's dict (without `slot`)."""
    from wenet_amd import _lib
    L = _lib.lib()
    n = len(hyps)
    max_len = max([len(h) for h in hyps] + [1]) if max_len is None else max_len
    lens = np.array([len(h) for h in hyps], dtype=np.int32)
    toks = np.full((n, max_len), -7, dtype=np.int32)       # (the padding is never read)
    for k, h in enumerate(hyps):
        toks[k, :len(h)] = h
    cap = 1 + n * max_len
    n_nodes = ctypes.c_int32(0)
    parent, token, depth = (np.full((cap, ), -9, dtype=np.int32) for _ in range(3))
    path = np.full((n, max_len + 1), -9, dtype=np.int32)
    col_off = np.full((cap + 1, ), -9, dtype=np.int32)
    cols = np.full((2 * cap, ), -9, dtype=np.int32)
    _lib.check(L.wn_op_rnnt_trie(n, _lib.i32p(lens), _lib.i32p(toks), max_len, blank,
                                 ctypes.byref(n_nodes), _lib.i32p(parent), _lib.i32p(token),
                                 _lib.i32p(depth), _lib.i32p(path), _lib.i32p(col_off),
                                 _lib.i32p(cols)), 'wn_op_rnnt_trie')
    N = n_nodes.value
    assert (parent[N:] == -9).all() and (col_off[N + 1:] == -9).all()
    assert col_off[N] == 2 * N - 1 and (cols[2 * N - 1:] == -9).all()
    for k, h in enumerate(hyps):
        assert (path[k, len(h) + 1:] == -1).all()
    return dict(parent=parent[:N].tolist(), token=token[:N].tolist(), depth=depth[:N].tolist(),
                paths=[path[k, :len(h) + 1].tolist() for k, h in enumerate(hyps)],
                col_off=col_off[:N + 1].tolist(), cols=cols[:2 * N - 1].tolist())


def same(got, want):
    for k in ('parent', 'token', 'depth', 'paths', 'col_off', 'cols'):
        assert got[k] == want[k], k


def test_trie_hand_cases():
    # identical hypotheses share every node
    t = op_trie([[5, 6], [5, 6]], 0)
    assert t['parent'] == [-1, 0, 1] and t['token'] == [0, 5, 6] and t['depth'] == [0, 1, 2]
    assert t['paths'] == [[0, 1, 2], [0, 1, 2]]
    assert t['col_off'] == [0, 2, 4, 5] and t['cols'] == [0, 5, 0, 6, 0]
    # one a prefix of another, and the empty one
    t = op_trie([[5, 6, 7], [5, 6], []], 2)
    assert t['parent'] == [-1, 0, 1, 2] and t['token'] == [2, 5, 6, 7]
    assert t['paths'] == [[0, 1, 2, 3], [0, 1, 2], [0]]
    assert t['cols'] == [2, 5, 2, 6, 2, 7, 2]
    # no shared prefix: level order, first appearance within a level
    t = op_trie([[3, 4], [9], [8, 4]], 0)
    assert t['token'] == [0, 3, 9, 8, 4, 4] and t['parent'] == [-1, 0, 0, 0, 1, 3]
    assert t['depth'] == [0, 1, 1, 1, 2, 2]
    assert t['paths'] == [[0, 1, 4], [0, 2], [0, 3, 5]]
    assert t['col_off'] == [0, 4, 6, 7, 9, 10, 11] and t['cols'][:4] == [0, 3, 9, 8]
    # only the empty hypothesis
    t = op_trie([[]], 0)
    assert t['parent'] == [-1] and t['paths'] == [[0]] and t['cols'] == [0]
    for case in ([[5, 6], [5, 6]], [[5, 6, 7], [5, 6], []], [[3, 4], [9], [8, 4]], [[]]):
        same(op_trie(case, 1), SF.build_trie(case, 1))


def test_trie_sixteen_hypotheses_of_length_70():
    rng = np.random.default_rng(5)
    stem = rng.integers(1, 50, size=70).tolist()
    hyps = []
    for k in range(16):          # they leave the common stem at 4 k and never meet again
        hyps.append(stem[:4 * k] + rng.integers(50 + 10 * k, 60 + 10 * k, size=70 - 4 * k).tolist())
    t = op_trie(hyps, 0)
    same(t, SF.build_trie(hyps, 0))
    assert len(t['parent']) == 1 + sum(70 - 4 * k for k in range(16)) + 60
    assert max(np.diff(t['col_off'])) == 3 and t['depth'][-1] == 70
    # a node with 16 children: 17 columns
    t = op_trie([[k + 1] for k in range(16)], 0)
    assert t['col_off'][:2] == [0, 17] and t['cols'][:17] == list(range(17))


def test_trie_random_nbests_against_the_restatement():
    rng = np.random.default_rng(11)
    for it in range(200):
        n = int(rng.integers(1, 17))
        vocab = int(rng.choice([2, 3, 6, 40]))
        blank = int(rng.integers(0, vocab))
        hyps = [rng.integers(0, vocab, size=int(rng.integers(0, 9))).tolist() for _ in range(n)]
        got, want = op_trie(hyps, blank, max_len=8 + it % 3), SF.build_trie(hyps, blank)
        same(got, want)
        # parents precede children; a path follows parents; a child's slot names its column
        for i, p in enumerate(want['parent'][1:], start=1):
            assert p < i and want['depth'][i] == want['depth'][p] + 1
            assert want['cols'][want['col_off'][p] + want['slot'][i]] == want['token'][i]
        for k, h in enumerate(hyps):
            assert [want['token'][i] for i in want['paths'][k][1:]] == h


def test_new_symbols_are_exported_and_declared():
    from wenet_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert f'int {name}(' in header
        assert getattr(L, name).argtypes is not None


def test_argument_validation_without_a_device():
    from wenet_amd import _lib
    L = _lib.lib()
    i32 = lambda *v: np.array(v, dtype=np.int32)      # noqa: E731
    one, toks, td = i32(1), i32(1, 2, 3, 4), np.zeros(4)
    assert L.wn_transducer_score(None, 4, _lib.i32p(one), _lib.i32p(i32(1, 0, 0, 0)),
                                 _lib.i32p(toks), 1, _lib.f64p(td), None) == -1
    assert b'null handle' in L.wn_last_error()
    assert L.wn_transducer_score_stats(None, None, None, None) == -1
    assert b'null handle' in L.wn_last_error()

    def trie(n, lens, toks, max_len, blank=0):
        out = [np.zeros(64, dtype=np.int32) for _ in range(6)]
        nn = ctypes.c_int32(0)
        return L.wn_op_rnnt_trie(n, _lib.i32p(i32(*lens)), _lib.i32p(i32(*toks)), max_len, blank,
                                 ctypes.byref(nn), *[_lib.i32p(o) for o in out])

    assert trie(1, [2], [3, 4], 2) == 0
    for n in (0, 17):
        assert trie(n, [2] * 17, [1] * 34, 2) == -1 and b'n_hyps' in L.wn_last_error()
    assert trie(1, [3], [3, 4], 2) == -1 and b'length' in L.wn_last_error()
    assert trie(1, [-1], [3, 4], 2) == -1 and b'length' in L.wn_last_error()
    assert trie(1, [2], [3, -4], 2) == -1 and b'token' in L.wn_last_error()
    assert trie(1, [2], [3, 4], 2, blank=-1) == -1 and b'blank' in L.wn_last_error()
    assert L.wn_op_rnnt_trie(1, None, None, 2, 0, None, None, None, None, None, None, None) == -1
    assert b'null' in L.wn_last_error()

    # the gather hook: its maps and lists are checked before the device is touched (the device
    # pointers are only compared with NULL)
    dev = ctypes.c_void_p(64)
    logp = np.zeros(64, dtype=np.float32)

    def gather(row_enc, row_pred, col_off, cols, M=2, J=32, V=10, enc_rows=3, pred_rows=2):
        return L.wn_op_joint_logp_gather(dev, enc_rows, dev, pred_rows, _lib.i32p(i32(*row_enc)),
                                         _lib.i32p(i32(*row_pred)), dev, dev, M, J, V,
                                         _lib.i32p(i32(*col_off)), _lib.i32p(i32(*cols)),
                                         _lib.f32p(logp), None)

    assert gather([0, 3], [0, 1], [0, 1, 2], [0, 1]) == -1 and b'row map' in L.wn_last_error()
    assert gather([0, 1], [0, 2], [0, 1, 2], [0, 1]) == -1 and b'row map' in L.wn_last_error()
    assert gather([0, 1], [0, 1], [1, 1, 2], [0, 1]) == -1 and b'start at 0' in L.wn_last_error()
    assert gather([0, 1], [0, 1], [0, 1, 2], [0, 10]) == -1 and b'column' in L.wn_last_error()
    assert gather([0, 1], [0, 1], [0, 18, 19], [0] * 19) == -1 and b'17' in L.wn_last_error()
    assert gather([0, 1], [0, 1], [0, 1, 2], [0, 1], M=0) == -1 and b'empty' in L.wn_last_error()
    assert L.wn_op_joint_logp_gather(None, 1, None, 1, None, None, None, None, 1, 32, 4, None,
                                     None, None, None) == -1 and b'null' in L.wn_last_error()

    # the lattice hook
    sc = np.zeros(4)
    f = np.zeros(16, dtype=np.float32)

    def lat(N, T, U):
        return L.wn_op_rnnt_lattice(N, _lib.i32p(i32(*T)), _lib.i32p(i32(*U)), _lib.f32p(f),
                                    _lib.f32p(f), _lib.f64p(sc), None)

    assert lat(0, [1], [1]) == -1 and b'N must' in L.wn_last_error()
    assert lat(1, [-1], [1]) == -1 and b'T must' in L.wn_last_error()
    assert lat(1, [1], [-1]) == -1 and lat(1, [1], [4096]) == -1
    assert L.wn_op_rnnt_lattice(1, None, None, None, None, None, None) == -1
    assert b'null' in L.wn_last_error()


def test_unknown_beam_search_type_is_rejected():
    from wenet_amd.transducer import RNNT_RESCORE_METHOD, Transducer
    speech, lens = torch.zeros(1, 20, 80), torch.tensor([20])
    with pytest.raises(ValueError, match='beam_search_type'):
        Transducer.transducer_attention_rescoring(None, speech, lens, 5, beam_search_type='attention')
    with pytest.raises(ValueError, match='beam_search_type'):
        Transducer.decode(None, [RNNT_RESCORE_METHOD], speech, lens, beam_size=5,
                          beam_search_type='rnnt')
    assert RNNT_RESCORE_METHOD == 'rnnt_beam_attn_rescoring'
    # reverse_weight > 0 without a right decoder is an assertion error, as in the reference
    import types
    no_right = types.SimpleNamespace(_cfg=types.SimpleNamespace(dec_r_layers=0))
    with pytest.raises(AssertionError):
        Transducer.transducer_attention_rescoring(no_right, speech, lens, 5, reverse_weight=0.3)
    with pytest.raises(AssertionError):
        Transducer.decode(no_right, [RNNT_RESCORE_METHOD], speech, lens, reverse_weight=0.3)


def test_combination_takes_the_first_maximum_and_never_a_nan():
    from wenet_amd.transducer import combine_scores
    nan = float('nan')
    best, scores = combine_scores([-1.0, -1.0, -3.0], [0, 0, 0], None, 1.0, 0.0, 0.0)
    assert best == 0 and scores == [-1.0, -1.0, -3.0]
    best, _ = combine_scores([nan, -2.0, -1.0], [0, 0, 0], None, 1.0, 0.0, 0.0)
    assert best == 2
    best, _ = combine_scores([nan, nan], [0, 0], None, 1.0, 0.0, 0.0)
    assert best == 0
    best, scores = combine_scores([-1.0, -2.0], [-5.0, -1.0], [-3.0, -1.0], 0.4, 0.3, 0.3)
    assert best == 1 and scores == [-1.0 * 0.4 + -5.0 * 0.3 + -3.0 * 0.3,
                                    -2.0 * 0.4 + -1.0 * 0.3 + -1.0 * 0.3]
    for a, s, t in (([-1.0, -2.0], [-5.0, -1.0], [-3.0, -1.0]), ([nan, -2.0], [0, 0], [0, 0])):
        assert combine_scores(a, s, t, 0.4, 0.3, 0.3)[0] == SF.combine(a, s, t, 0.4, 0.3, 0.3)[0]
