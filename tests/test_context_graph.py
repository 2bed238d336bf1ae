"""Host logic of context biasing (wenet_amd/context_graph.py): the product's
own ContextGraph against the oracle's restatement (itself pinned against the
reference in tests/test_oracle.py), the flat tables the C ABI takes, and the
flattening of a reference-style graph object."""
from types import SimpleNamespace

import numpy as np
import pytest

from golden_util import load_case
from oracle import wenet_oracle as O
from wenet_amd.context_graph import ContextGraph, FlatGraph, flatten, tokenize


def _random_phrases(rng, vocab, n):
    return [[int(t) for t in rng.randint(1, vocab, rng.randint(1, 6))]
            for _ in range(n)]


def _walk_flat(f: FlatGraph, state: int, token: int):
    """The device algorithm (ctc.hip ctx_step) over the flat tables."""
    edges = {(int(a), int(t)): int(b)
             for a, t, b in zip(f.edge_from, f.edge_token, f.edge_to)}
    n = edges.get((state, token))
    if n is not None:
        score = f.token_score[n]
    else:
        n = int(f.fail[state])
        c = edges.get((n, token))
        while c is None:
            n = int(f.fail[n])
            c = edges.get((n, token))
            if n == 0:
                break
        if c is not None:
            n = c
        score = f.node_score[n] - f.node_score[state]
    return score + f.output_score[n], n


def test_matches_oracle_graph_on_random_phrase_lists():
    rng = np.random.RandomState(1)
    for _ in range(40):
        vocab = int(rng.randint(3, 10))
        phrases = _random_phrases(rng, vocab, int(rng.randint(1, 15)))
        score = float(rng.choice([0.5, 2.0, 6.0]))
        g = ContextGraph(context_list=phrases, context_score=score)
        o = O.ContextGraph(phrases, score)
        f = g.flat()
        assert g.num_nodes == o.num_nodes and f.n_nodes == o.num_nodes + 1
        assert f.fail.tolist() == o.fail
        assert f.node_score.tolist() == o.node_score
        assert f.output_score.tolist() == o.output_score
        assert f.n_edges == o.num_nodes  # a trie: one arc into every non-root node
        for _ in range(10):
            s = so = sf = 0
            for tok in rng.randint(0, vocab + 1, 30):
                a, s = g.forward_one_step(s, int(tok))
                b, so = o.forward_one_step(so, int(tok))
                c, sf = _walk_flat(f, sf, int(tok))
                assert a == b == c and s == so == sf
                assert g.finalize(s) == o.finalize(so)


def test_tokenize_char_units(tmp_path):
    table = {'<blank>': 0, '<unk>': 1, 'a': 2, 'b': 3, '▁': 4, '你': 5}
    lines = ['ab a\n', ' b你z \n', '\n', 'zzz\n']
    path = tmp_path / 'ctx.txt'
    path.write_text(''.join(lines), encoding='utf8')
    assert tokenize(str(path), table) == O.tokenize_context(lines, table)
    assert tokenize(str(path), table) == [[2, 3, 4, 2], [3, 5, 1], [], [1, 1, 1]]
    table.pop('<unk>')
    assert tokenize(str(path), table) == [[2, 3, 4, 2], [3, 5], [], []]
    g = ContextGraph(str(path), table, None, 3.0)
    assert g.num_nodes == 6 and g.context_list[0] == [2, 3, 4, 2]


def test_constructor_needs_a_phrase_source():
    with pytest.raises(ValueError):
        ContextGraph()


def test_empty_graph_is_only_the_root():
    f = ContextGraph(context_list=[[]]).flat()
    assert f.n_nodes == 1 and f.n_edges == 0 and f.fail.tolist() == [0]


def _reference_style_graph(rec):
    """A graph object shaped like the reference's ContextGraph (``root``; ContextState
    nodes with ``id``, ``next``, ``fail`` and the three scores), rebuilt from a reference
    graph recorded state by state in tests/golden/live_context_graph.npz."""
    states = {r['id']: SimpleNamespace(id=r['id'], token_score=r['token_score'],
                                       node_score=r['node_score'],
                                       output_score=r['output_score'])
              for r in rec['states']}
    for r in rec['states']:
        states[r['id']].fail = states[r['fail']]
        states[r['id']].next = {tok: states[child] for tok, child in r['next']}
    return SimpleNamespace(root=states[0], num_nodes=rec['num_nodes'])


def test_flatten_accepts_the_reference_graph_object():
    recs = load_case('live_context_graph')[0]['flatten']
    rng = np.random.RandomState(5)
    for rec in recs:
        vocab = int(rng.randint(3, 9))
        phrases = _random_phrases(rng, vocab, int(rng.randint(1, 12)))
        assert phrases == rec['phrases']
        ref = _reference_style_graph(rec)
        f = flatten(ref)
        assert flatten(ref) is f  # cached on the object
        assert f.n_nodes == ref.num_nodes + 1
        steps = iter(rec['walk'])      # the reference's forward_one_step / finalize answers
        for _ in range(10):
            s = 0
            for tok in rng.randint(0, vocab + 1, 30):
                a, _, r_final = next(steps)
                b, s = _walk_flat(f, s, int(tok))
                assert a == b
                assert -f.node_score[s] == r_final


def test_tokenize_bpe_matches_reference(tmp_path):
    """The reference's tokenize on the same sentencepiece model (model and answer recorded
    in tests/golden/live_tokenizers.npz)."""
    spm = pytest.importorskip('sentencepiece')
    meta, arrays = load_case('live_tokenizers')
    model = tmp_path / 'bpe.model'
    model.write_bytes(arrays['context_bpe_model'].tobytes())
    sp = spm.SentencePieceProcessor()
    sp.load(str(model))
    table = {sp.id_to_piece(i): i for i in range(sp.get_piece_size())}
    table['你'] = len(table)
    ctx = tmp_path / 'ctx.txt'
    ctx.write_text('the cat\nhello 你 world\nzebra\n', encoding='utf8')
    assert tokenize(str(ctx), table, str(model)) == meta['context_bpe']
