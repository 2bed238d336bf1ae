#!/usr/bin/env python3
"""tests/golden/live_*: what the REAL reference returns for the inputs of the CPU tests
that used to call it in-process (tests/test_oracle.py, tests/test_context_graph.py,
tests/test_recognize_cli.py).  Those tests compare against these recorded answers, so
they run wherever the repository is checked out.  Runs only where the reference tree
exists and oracle/_ref has been built (`make -C oracle`):

    python oracle/gen_golden_live.py [step ...]

Every test input is regenerated here exactly as the test generates it (same seeds, same
order of random draws); only the reference's side of each comparison is stored.
"""
import copy
import hashlib
import json
import os
import sys
import tempfile
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import _ref_harness, gen_golden  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


def save(name, meta, **arrays):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        **arrays)
    print(name, os.path.getsize(path), 'bytes')


def fbank_cpp():
    """The reference's C++ fbank and its Whisper frontend (oracle/_ref)."""
    from oracle import ref_fbank
    from wenet_amd import synthetic as S
    arrays = {}
    for n, seed in [(8000, 21), (401, 22), (33333, 23)]:
        arrays[f'feats_{n}_{seed}'] = ref_fbank.ref_fbank(S.make_audio(n, seed=seed))
    wave_ = np.asarray(S.make_audio(16000 * 2 + 123, seed=9), dtype=np.float32)
    arrays['whisper_80'] = ref_fbank.ref_whisper_fbank(wave_, 80)
    save('live_fbank_cpp', {}, **arrays)


def whisper_encoder():
    from oracle import gen_golden_whisper
    from wenet_amd import synthetic as S
    configs = S.make_configs('whisper_tiny_like')
    sd = S.make_state_dict(configs, 5)
    enc, _ = gen_golden_whisper.build_reference_encoder(configs, sd)
    arrays = {}
    for i, (B, fr, seed) in enumerate([(3, (30, 71), 1), (2, (40, 41), 2), (4, (9, 33), 3)]):
        f, l = S.make_features(B, fr, seed=seed, feat_dim=configs['input_dim'])
        with torch.no_grad():
            ref, rmask = enc(f, l)
        arrays[f'out{i}'] = ref.numpy()
        arrays[f'n{i}'] = rmask.squeeze(1).sum(1).numpy()
    save('live_whisper_encoder', {}, **arrays)


def state_dict_names():
    """init_model's parameter names and shapes, and a digest of its positional table."""
    import argparse
    from wenet.utils.init_model import init_model
    from wenet_amd import synthetic as S
    meta = {}
    for config in ('tiny_causal', 'tiny_sym', 'aishell_u2pp'):
        rc = copy.deepcopy(S.make_configs(config))
        rc['cmvn'] = None
        model, _ = init_model(argparse.Namespace(), rc)
        ref = model.state_dict()
        pe = np.ascontiguousarray(ref['encoder.embed.pos_enc.pe'].numpy())
        meta[config] = dict(shapes={k: list(v.shape) for k, v in ref.items()},
                            pe_dtype=str(pe.dtype),
                            pe_sha256=hashlib.sha256(pe.tobytes()).hexdigest())
    save('live_state_dict_names', meta)


def decode():
    from wenet_amd import synthetic as S
    meta = []
    for config, chunk, left, beam in [('tiny_causal', -1, -1, 7), ('tiny_causal', 3, 1, 2),
                                      ('tiny_sym', -1, -1, 4), ('tiny_sym', 5, -1, 3)]:
        configs = S.make_configs(config)
        sd = S.make_state_dict(configs, 3)
        model = gen_golden.build_reference_model(configs, sd)
        feats, lens = S.make_features(4, (50, 220), seed=21)
        rw = 0.4 if configs['decoder'] == 'bitransformer' else 0.0
        with torch.no_grad():
            ref = model.decode(['ctc_greedy_search', 'ctc_prefix_beam_search',
                                'attention_rescoring'], feats, lens, beam_size=beam,
                               decoding_chunk_size=chunk, num_decoding_left_chunks=left,
                               ctc_weight=0.4, reverse_weight=rw)
        prefix, resc = ref['ctc_prefix_beam_search'], ref['attention_rescoring']
        meta.append(dict(
            config=config, chunk=chunk, left=left, beam=beam,
            greedy=[list(map(int, r.tokens)) for r in ref['ctc_greedy_search']],
            nbest=[[list(map(int, h)) for h in r.nbest] for r in prefix],
            nbest_scores=[[float(s) for s in r.nbest_scores] for r in prefix],
            nbest_times=[[list(map(int, t)) for t in r.nbest_times] for r in prefix],
            rescoring=[list(map(int, r.tokens)) for r in resc],
            rescoring_scores=[float(r.score) for r in resc],
            rescoring_confidence=[float(r.confidence) for r in resc]))
    save('live_decode', meta)


def attention_decoder():
    from oracle import wenet_oracle as O
    from wenet_amd import synthetic as S
    arrays = {}
    for config, rw in [('tiny_causal', 0.0), ('tiny_causal', 0.4), ('tiny_sym', 0.0)]:
        configs = S.make_configs(config)
        sd = S.make_state_dict(configs, 4)
        model = gen_golden.build_reference_model(configs, sd)
        sos, eos = O.special_symbols(configs)
        g = torch.Generator().manual_seed(9)
        V = configs['output_dim']
        lens = torch.tensor([7, 3, 1, 5])
        hyps = torch.full((4, 7), eos, dtype=torch.long)
        for i, n in enumerate(lens.tolist()):
            hyps[i, 0] = sos
            hyps[i, 1:n] = torch.randint(1, V - 1, (n - 1, ), generator=g)
        enc = torch.randn(1, 23, configs['encoder_conf']['output_size'], generator=g)
        with torch.no_grad():
            r_l, r_r = model.forward_attention_decoder(hyps, lens, enc, rw)
        arrays[f'{config}_{rw}_l'] = r_l.numpy()
        arrays[f'{config}_{rw}_r'] = r_r.numpy()
    save('live_attention_decoder', {}, **arrays)


def bf16_autocast():
    """The reference encoder in fp32 and under CPU bf16 autocast (recognize.py --dtype bf16)."""
    from wenet_amd import synthetic as S
    arrays = {}
    for config in ('tiny_causal', 'tiny_sym'):
        configs = S.make_configs(config)
        sd = S.make_state_dict(configs, 3)
        model = gen_golden.build_reference_model(configs, sd)
        feats, lens = S.make_features(4, (60, 200), seed=8)
        with torch.no_grad():
            ref32, mask = model._forward_encoder(feats, lens)
            with torch.autocast('cpu', dtype=torch.bfloat16):
                ref_ac, _ = model._forward_encoder(feats, lens)
        arrays[f'{config}_fp32'] = ref32.numpy()
        arrays[f'{config}_autocast'] = ref_ac.float().numpy()    # bf16 values: exact in fp32
        arrays[f'{config}_n'] = mask.squeeze(1).sum(1).numpy()
    save('live_bf16_autocast', {}, **arrays)


def _walk(ref, rng, vocab, walks, steps):
    """The reference automaton's [score, state id, finalize score] for every step of the
    token streams the tests draw from `rng`."""
    out = []
    for _ in range(walks):
        rs = ref.root
        for tok in rng.randint(0, vocab + 1, steps):
            score, rs = ref.forward_one_step(rs, int(tok))
            out.append([float(score), int(rs.id), float(ref.finalize(rs)[0])])
    return out


def _phrases(rng, vocab, n):
    return [[int(t) for t in rng.randint(1, vocab, rng.randint(1, 6))] for _ in range(n)]


def context_graph():
    """test_oracle.py test_context_graph_matches_live_reference and
    test_oracle_context_search_matches_live_reference; test_context_graph.py
    test_flatten_accepts_the_reference_graph_object (the reference's graph objects as plain
    records: every state's id, scores, fail id and arcs)."""
    from oracle import gen_golden_context
    from wenet.models.transformer.search import ctc_prefix_beam_search as ref_search
    from wenet.utils.context_graph import ContextGraph as RefGraph
    from wenet_amd import synthetic as S
    meta = dict(graph=[], search=[], flatten=[])
    rng = np.random.RandomState(0)
    for _ in range(20):
        vocab = int(rng.randint(3, 9))
        phrases = _phrases(rng, vocab, rng.randint(1, 12))
        ref = gen_golden_context.reference_graph(phrases, 1.5)
        meta['graph'].append(dict(phrases=phrases, num_nodes=int(ref.num_nodes),
                                  walk=_walk(ref, rng, vocab, 30, 25)))
    table = {'<blank>': 0, '<unk>': 1, 'a': 2, 'b': 3, '▁': 4, '你': 5}
    lines = ['ab a\n', ' b你z \n', '\n', 'zzz\n']
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'ctx.txt')
        with open(path, 'w', encoding='utf8') as f:
            f.write(''.join(lines))
        meta['tokenize_with_unk'] = RefGraph(path, table, None, 2.0).context_list
        table.pop('<unk>')
        meta['tokenize_without_unk'] = RefGraph(path, table, None, 2.0).context_list
    rng = np.random.RandomState(7)
    for trial in range(6):
        vocab = int(rng.randint(5, 30))
        beam = int(rng.randint(1, min(vocab, 12)))
        logp, lens = S.peaky_logprobs(3, (10, 60), vocab, float(rng.uniform(1, 5)),
                                      100 + trial)
        phrases = [[int(t) for t in rng.randint(1, vocab, rng.randint(1, 5))]
                   for _ in range(rng.randint(1, 15))]
        cs = float(rng.choice([0.5, 2.0, 6.0]))
        ref = ref_search(logp, lens, beam, gen_golden_context.reference_graph(phrases, cs), 0)
        meta['search'].append(gen_golden_context.pack(ref))
    rng = np.random.RandomState(5)
    for _ in range(10):
        vocab = int(rng.randint(3, 9))
        phrases = _phrases(rng, vocab, int(rng.randint(1, 12)))
        ref = gen_golden_context.reference_graph(phrases, 2.0)
        states, todo, seen = [], [ref.root], {id(ref.root)}
        while todo:
            st = todo.pop(0)
            states.append(dict(id=int(st.id), token_score=float(st.token_score),
                               node_score=float(st.node_score),
                               output_score=float(st.output_score), fail=int(st.fail.id),
                               next=[[int(t), int(c.id)] for t, c in st.next.items()]))
            for c in st.next.values():
                if id(c) not in seen:
                    seen.add(id(c))
                    todo.append(c)
        meta['flatten'].append(dict(phrases=phrases, num_nodes=int(ref.num_nodes),
                                    states=states, walk=_walk(ref, rng, vocab, 10, 30)))
    save('live_context_graph', meta)


def _train_bpe(tmp, name, lines, vocab_size, **kw):
    import sentencepiece as spm
    corpus = os.path.join(tmp, name + '.txt')
    with open(corpus, 'w') as f:
        f.write('\n'.join(lines))
    spm.SentencePieceTrainer.train(input=corpus, model_prefix=os.path.join(tmp, name),
                                   vocab_size=vocab_size, model_type='bpe', **kw)
    with open(os.path.join(tmp, name + '.model'), 'rb') as f:
        return f.read()


def tokenizers():
    """test_context_graph.py test_tokenize_bpe_matches_reference and test_recognize_cli.py
    test_tokenizers_match_the_reference.  The sentencepiece models those tests used to
    train are stored beside the reference's answers, so both sides read the same model."""
    import sentencepiece as spm
    from wenet.utils.context_graph import tokenize as ref_tokenize
    from wenet.utils.init_tokenizer import init_tokenizer as ref_init
    meta, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        arrays['context_bpe_model'] = np.frombuffer(_train_bpe(
            tmp, 'bpe', ['HELLO WORLD', 'THE CAT SAT ON THE MAT', 'SPEECH RECOGNITION',
                         'A QUICK BROWN FOX'] * 30, 40, character_coverage=1.0), dtype=np.uint8)
        sp = spm.SentencePieceProcessor()
        sp.load(os.path.join(tmp, 'bpe.model'))
        table = {sp.id_to_piece(i): i for i in range(sp.get_piece_size())}
        table['你'] = len(table)
        ctx = os.path.join(tmp, 'ctx.txt')
        with open(ctx, 'w', encoding='utf8') as f:
            f.write('the cat\nhello 你 world\nzebra\n')
        meta['context_bpe'] = ref_tokenize(ctx, table, os.path.join(tmp, 'bpe.model'))

        units = os.path.join(tmp, 'units.txt')
        syms = ['<blank>', '<unk>', '▁he', 'llo', '▁wor', 'ld', '你', '好',
                '<sos/eos>']
        with open(units, 'w') as f:
            f.write(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        meta['char'] = []
        for extra in ({}, {'connect_symbol': ' '}, {'split_with_space': True}):
            ref = ref_init({'tokenizer': 'char',
                            'tokenizer_conf': dict(symbol_table_path=units,
                                                   non_lang_syms_path=None, **extra)})
            meta['char'].append(dict(
                extra=extra, symbol_table=ref.symbol_table,
                detokenize=[ref.detokenize(ids) for ids in ([6, 7], [2, 3, 4, 5], [])]))
        arrays['cli_bpe_model'] = np.frombuffer(_train_bpe(
            tmp, 'b', ['HELLO WORLD', 'THE CAT SAT'] * 40, 30), dtype=np.uint8)
        sp = spm.SentencePieceProcessor()
        sp.load(os.path.join(tmp, 'b.model'))
        with open(units, 'w') as f:
            f.write(''.join(f'{sp.id_to_piece(i)} {i}\n' for i in range(sp.get_piece_size())))
        ref = ref_init({'tokenizer': 'bpe',
                        'tokenizer_conf': dict(symbol_table_path=units, non_lang_syms_path=None,
                                               bpe_path=os.path.join(tmp, 'b.model'))})
        ids = sp.encode('HELLO THE CAT')
        meta['bpe'] = dict(ids=ids, detokenize=ref.detokenize(ids))
    save('live_tokenizers', meta, **arrays)


def wav_reader():
    """test_recognize_cli.py test_read_wav_matches_the_reference_wav_reader: the reference
    reader's samples of the test's synthetic files and of the reference's own test file
    (whose RIFF image is stored too: it is the input of that check)."""
    from oracle import ref_fbank as RF
    from test_recognize_cli import _wav_bytes
    rng = np.random.Generator(np.random.PCG64(9))
    x = rng.random((3000, 2)) * 1.6 - 0.8
    meta, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for bits in (16, 32):
            for nch in (1, 2):
                for extra in (False, 26):
                    name = f'w{bits}_{nch}_{int(extra)}'
                    p = os.path.join(tmp, name + '.wav')
                    with open(p, 'wb') as f:
                        f.write(_wav_bytes(x[:, :nch], 22050, 1, bits, nch=nch,
                                           extra_chunk=extra))
                    ref, ch, sr, b = RF.ref_wav_read(p)
                    arrays[name] = ref
                    meta[name] = [ch, sr, b]
    ref_file = os.path.join(_ref_harness.REFERENCE_ROOT, 'test', 'resources',
                            'aishell-BAC009S0724W0121.wav')
    ref, ch, sr, b = RF.ref_wav_read(ref_file)
    with open(ref_file, 'rb') as f:
        arrays['aishell_riff'] = np.frombuffer(f.read(), dtype=np.uint8)
    with wave.open(ref_file) as w:
        assert w.getnframes() == len(ref)
    assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 32768
    arrays['aishell'] = ref.astype(np.int16)       # integer sample values: exact
    meta['aishell'] = [ch, sr, b]
    save('live_wav_reader', meta, **arrays)


def recipes():
    """test_recognize_cli.py test_every_reference_recipe_is_accepted_or_refused_cleanly:
    every examples/*/*/conf/*.yaml of the reference, parsed (settings only)."""
    import glob
    import yaml
    out = {}
    for p in sorted(glob.glob(os.path.join(_ref_harness.REFERENCE_ROOT,
                                           'examples', '*', '*', 'conf', '*.yaml'))):
        with open(p) as f:
            c = yaml.load(f, Loader=yaml.FullLoader)
        assert json.loads(json.dumps(c)) == c, p      # JSON holds it unchanged
        out[p.split('examples/')[1]] = c
    save('live_recipes', out)


STEPS = dict(fbank_cpp=fbank_cpp, whisper_encoder=whisper_encoder,
             state_dict_names=state_dict_names, decode=decode,
             attention_decoder=attention_decoder, bf16_autocast=bf16_autocast,
             context_graph=context_graph, tokenizers=tokenizers, wav_reader=wav_reader,
             recipes=recipes)


def main():
    steps = sys.argv[1:] or sorted(STEPS)
    unknown = [s for s in steps if s not in STEPS]
    if unknown:
        raise SystemExit(f'unknown step(s) {unknown}; steps: {sorted(STEPS)}')
    _ref_harness.install()
    torch.set_num_threads(8)
    for s in steps:
        STEPS[s]()


if __name__ == '__main__':
    main()
