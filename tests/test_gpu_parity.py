"""GPU parity tests: the HIP path (through the C ABI) against
  * the committed outputs of the real reference (tests/golden/), and
  * the CPU oracle on the same seeded inputs,
stage by stage (encoder, CTC log-probs, greedy, prefix beam, rescoring,
fbank) and end to end.

Tolerances (fp32 path, different summation order than torch-CPU):
  encoder output       |err| <= 2e-3 on unit-variance activations
  CTC log-probs        |err| <= 5e-3 (logits are sharpened x12)
  greedy tokens        per FRAME (tests/gpu_util.py): identical arg-max on every frame
                       whose reference top-1 margin > 1e-3, reference top-2 below it,
                       >= 95 % of frames strictly compared, flips counted
  prefix-beam scores   |err| <= 2e-3; rescoring scores |err| <= 1e-3 ABSOLUTE for
                       every hypothesis, the reference's winner required
Bit-exact (same log-prob tensor fed to both): greedy tokens, n-best token
lists, n-best time stamps; fp64 n-best scores to 1e-9.
"""
import os

import numpy as np
import pytest
import torch

from golden_util import (attention_case_names, build_inputs, case_names,
                         chunk_case_names, chunk_windows,
                         context_case_names, context_search_case_names, load_case,
                         stream_case_names,
                         whisper_case_names)
from gpu_util import (cached_model, compare_nbest, frame_margins, greedy_frame_check,
                      nbest_check, rescoring_check)

pytestmark = pytest.mark.gpu
_GALIGN_DEFAULT = 2      # wn_tune_set's process default of attn_x6_galign (csrc/tune.h)

METHODS = ['ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring']


def _oracle():
    from oracle import wenet_oracle as O
    return O


@pytest.mark.parametrize('name', case_names())
def test_golden_case(name):
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    _, _, feats, lens = build_inputs(meta)
    enc, mask = model._forward_encoder(feats.cuda(), lens, meta['chunk'],
                                       meta['left'])
    enc_lens = mask.squeeze(1).sum(1).cpu().numpy()
    np.testing.assert_array_equal(enc_lens, arrays['enc_lens'])
    enc = enc.cpu().numpy()
    for b, n in enumerate(arrays['enc_lens']):
        err = np.abs(enc[b, :n] - arrays['enc_out'][b, :n]).max()
        assert err < 2e-3, (name, b, err)
    logp = model.ctc_logprobs(torch.from_numpy(enc).cuda(),
                              encoder_lens=torch.from_numpy(enc_lens))
    k = arrays['ctc_topk_idx'].shape[-1]
    topv = logp.topk(k, dim=-1).values.cpu().numpy()
    for b, n in enumerate(arrays['enc_lens']):
        assert np.abs(topv[b, :n] - arrays['ctc_topk_val'][b, :n]).max() < 5e-3
    res = model.decode(METHODS, feats.cuda(), lens, beam_size=meta['beam'],
                       decoding_chunk_size=meta['chunk'],
                       num_decoding_left_chunks=meta['left'],
                       ctc_weight=meta['ctc_weight'],
                       reverse_weight=meta['reverse_weight'])
    top1 = logp.argmax(-1).cpu().numpy()
    n_frames = n_strict = n_flips = 0
    for b in range(meta['batch']):
        n = arrays['enc_lens'][b]
        f, st, fl = greedy_frame_check(
            top1[b, :n], arrays['ctc_topk_idx'][b, :n], arrays['ctc_topk_val'][b, :n],
            res['ctc_greedy_search'][b].tokens, meta['greedy'][b], what=f'{name}[{b}]')
        n_frames += f; n_strict += st; n_flips += fl
        g = meta['prefix'][b]
        nbest_check(res['ctc_prefix_beam_search'][b], g['nbest'],
                    g['nbest_scores'], g['nbest_times'], what=f'{name}[{b}]')
        # the reference fixture holds the winner only: its score is compared
        # whenever the GPU picked the same hypothesis, and it MUST pick it unless
        # the GPU's own top-2 rescoring gap is inside the tolerance
        r, gr = res['attention_rescoring'][b], meta['rescoring'][b]
        gs = sorted(r.all_scores, reverse=True)
        if len(gs) < 2 or gs[0] - gs[1] > 2e-3:
            assert list(r.tokens) == gr['tokens'], (name, b)
        if list(r.tokens) == gr['tokens']:
            assert abs(r.score - gr['score']) < 1e-3, (name, b, r.score, gr['score'])
            np.testing.assert_allclose(r.tokens_confidence,
                                       gr['tokens_confidence'], atol=2e-3)
    print(f'\n[{name}] frames {n_frames}, strictly compared {n_strict}, flips {n_flips}')
    assert n_strict >= 0.95 * n_frames


@pytest.mark.parametrize('name', whisper_case_names())
def test_whisper_encoder_golden_case(name):
    """Whisper-style TransformerEncoder (Conv1dSubsampling2, abs_pos_whisper,
    gelu, key_bias=False) + CTC head on the GPU against the real reference's
    committed outputs (BASELINE.json configs[4] family; fp32)."""
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    _, _, feats, lens = build_inputs(meta)
    enc, mask = model._forward_encoder(feats.cuda(), lens)
    enc_lens = mask.squeeze(1).sum(1).cpu().numpy()
    np.testing.assert_array_equal(enc_lens, arrays['enc_lens'])
    enc = enc.cpu().numpy()
    for b, n in enumerate(arrays['enc_lens']):
        ref = arrays['enc_out'][b, :n]
        err = np.abs(enc[b, :n] - ref).max()
        assert err < 2e-3 * max(1.0, np.abs(ref).max()), (name, b, err)
    res = model.decode(['ctc_greedy_search', 'ctc_prefix_beam_search'],
                       feats.cuda(), lens, beam_size=meta['beam'])
    logp = model.ctc_logprobs(torch.from_numpy(enc).cuda(),
                              encoder_lens=torch.from_numpy(enc_lens))
    top1 = logp.argmax(-1).cpu().numpy()
    n_frames = n_strict = 0
    for b in range(meta['batch']):
        n = arrays['enc_lens'][b]
        f, st, _ = greedy_frame_check(
            top1[b, :n], arrays['ctc_topk_idx'][b, :n], arrays['ctc_topk_val'][b, :n],
            res['ctc_greedy_search'][b].tokens, meta['greedy'][b], what=f'{name}[{b}]',
            eps=2e-3)   # unit-scale 1280-wide activations: logp error ~1e-3
        n_frames += f; n_strict += st
        g = meta['prefix'][b]
        nbest_check(res['ctc_prefix_beam_search'][b], g['nbest'],
                    g['nbest_scores'], g['nbest_times'], what=f'{name}[{b}]')
    assert n_strict >= 0.95 * n_frames
    with pytest.raises((RuntimeError, NotImplementedError, AssertionError)):
        model.decode(['attention_rescoring'], feats.cuda(), lens, beam_size=2)


@pytest.mark.parametrize('B,frames', [(5, (3, 140)), (1, (77, 77)), (3, (1, 2))])
def test_whisper_encoder_layers_vs_oracle(B, frames):
    """Every TransformerEncoderLayer output against the oracle, ragged batches
    with odd and even T, down to 1-frame utterances."""
    from wenet_amd import _lib, synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('whisper_tiny_like', 0)
    feats, lens = S.make_features(B, frames, seed=55, feat_dim=80)
    with torch.no_grad():
        ref, mask, layers = O.encoder_forward(configs, sd, feats, lens,
                                              return_layers=True)
    ref_lens = mask.squeeze(1).sum(1).numpy()
    L = _lib.lib()
    try:
        for n in range(len(layers)):
            _lib.check(L.wn_debug_set(model._h, b'n_layers', n), 'dbg')
            _lib.check(L.wn_debug_set(model._h, b'skip_after_norm', 1), 'dbg')
            enc, m = model._forward_encoder(feats.cuda(), lens)
            np.testing.assert_array_equal(m.squeeze(1).sum(1).cpu().numpy(), ref_lens)
            enc = enc.cpu()
            for b in range(B):
                nb = int(ref_lens[b])
                if nb:
                    err = (enc[b, :nb] - layers[n][b, :nb]).abs().max().item()
                    scale = max(layers[n][b, :nb].abs().max().item(), 1.0)
                    assert err < 1e-3 * scale, ('layer', n, 'utt', b, err)
    finally:
        L.wn_debug_set(model._h, b'n_layers', -1)
        L.wn_debug_set(model._h, b'skip_after_norm', 0)


@pytest.mark.parametrize('config,B,frames,chunk,left', [
    ('tiny_causal', 7, (30, 260), -1, -1),
    ('tiny_causal', 5, (30, 260), 8, 1),
    ('tiny_sym', 6, (7, 180), -1, -1),
    ('aishell_u2pp', 4, (400, 700), 16, -1),
])
def test_encoder_layers_vs_oracle(config, B, frames, chunk, left):
    """Every ConformerEncoderLayer output against the oracle (wn_debug_set)."""
    from wenet_amd import _lib, synthetic as S
    O = _oracle()
    configs, sd, model = cached_model(config, 0)
    feats, lens = S.make_features(B, frames, seed=77)
    with torch.no_grad():
        ref, mask, layers = O.encoder_forward(configs, sd, feats, lens, chunk,
                                              left, return_layers=True)
    ref_lens = mask.squeeze(1).sum(1).numpy()
    L = _lib.lib()
    try:
        for n in range(len(layers)):
            _lib.check(L.wn_debug_set(model._h, b'n_layers', n), 'dbg')
            _lib.check(L.wn_debug_set(model._h, b'skip_after_norm', 1), 'dbg')
            enc, m = model._forward_encoder(feats.cuda(), lens, chunk, left)
            enc = enc.cpu()
            for b in range(B):
                nb = int(ref_lens[b])
                err = (enc[b, :nb] - layers[n][b, :nb]).abs().max().item() \
                    if nb else 0.0
                scale = max(layers[n][b, :nb].abs().max().item(), 1.0) if nb else 1.0
                # n == 0 is the front end's output against the fp32 oracle: a coarse check of
                # the wiring only.  tests/test_gpu_frontend.py holds conv2, the projection and
                # the whole chain to fp32 rounding of an fp64 reference, on every route
                assert err < 1e-3 * scale, (config, 'layer', n, 'utt', b, err,
                                            'front end: see test_gpu_frontend.py' if n == 0 else '')
    finally:
        L.wn_debug_set(model._h, b'n_layers', -1)
        L.wn_debug_set(model._h, b'skip_after_norm', 0)
    enc, m = model._forward_encoder(feats.cuda(), lens, chunk, left)
    np.testing.assert_array_equal(m.squeeze(1).sum(1).cpu().numpy(), ref_lens)
    for b in range(B):
        nb = int(ref_lens[b])
        if nb:
            assert (enc[b, :nb].cpu() - ref[b, :nb]).abs().max() < 2e-3


@pytest.mark.parametrize('V,T,B,beam', [(67, 40, 5, 4), (4233, 120, 3, 10),
                                        (101, 33, 4, 1), (5002, 64, 2, 16),
                                        (300, 3, 3, 8)])
def test_search_free_functions_bit_exact(V, T, B, beam):
    """Same (B,T,V) log-prob tensor into the oracle's Python search and the
    GPU search: token lists, n-best order and time stamps must be identical."""
    from wenet_amd import search as S
    O = _oracle()
    g = torch.Generator().manual_seed(V + T)
    logits = torch.randn(B, T, V, generator=g) * 3.0
    logits[..., 0] += 6.0  # blank-heavy like a real CTC model
    # repeat frames so the "repeat" / "merge" branches are exercised
    for t in range(1, T, 3):
        logits[:, t] = logits[:, t - 1] + 0.05 * torch.randn(B, V, generator=g)
    logp = logits.log_softmax(-1)
    lens = torch.randint(max(1, T // 2), T + 1, (B, ), generator=g)
    lens[0] = T
    ref_g = O.ctc_greedy_search(logp, lens)
    got_g = S.ctc_greedy_search(logp.cuda(), lens)
    for b in range(B):
        assert got_g[b].tokens == ref_g[b].tokens
    ref_p = O.ctc_prefix_beam_search(logp, lens, beam)
    got_p = S.ctc_prefix_beam_search(logp.cuda(), lens, beam)
    for b in range(B):
        assert [list(x) for x in got_p[b].nbest] == \
            [list(x) for x in ref_p[b].nbest], b
        assert [list(x) for x in got_p[b].nbest_times] == \
            [list(x) for x in ref_p[b].nbest_times], b
        np.testing.assert_allclose(got_p[b].nbest_scores,
                                   ref_p[b].nbest_scores, rtol=0, atol=1e-9)
        assert list(got_p[b].tokens) == list(ref_p[b].tokens)
        assert got_p[b].times == ref_p[b].times


@pytest.mark.parametrize('V,T,beam', [(4, 50, 3), (5, 80, 4), (7, 60, 6),
                                      (3, 40, 2), (6, 120, 5), (8, 33, 8)])
def test_prefix_beam_small_vocab_stress(V, T, beam):
    """Tiny vocabularies make prefixes leave and re-enter the beam (the case
    where prefix identity must be the token sequence, not a node id)."""
    from wenet_amd import search as S
    O = _oracle()
    B = 48
    g = torch.Generator().manual_seed(V * 1000 + T + beam)
    logits = torch.randn(B, T, V, generator=g) * 2
    logits[..., 0] += torch.rand(B, 1, generator=g) * 3
    for t in range(1, T, 2):
        logits[:, t] = logits[:, t - 1] + 0.1 * torch.randn(B, V, generator=g)
    logp = logits.log_softmax(-1)
    lens = torch.randint(1, T + 1, (B, ), generator=g)
    ref = O.ctc_prefix_beam_search(logp, lens, beam)
    got = S.ctc_prefix_beam_search(logp.cuda(), lens, beam)
    for b in range(B):
        assert [list(x) for x in got[b].nbest] == \
            [list(x) for x in ref[b].nbest], b
        assert [list(x) for x in got[b].nbest_times] == \
            [list(x) for x in ref[b].nbest_times], b
        np.testing.assert_allclose(got[b].nbest_scores, ref[b].nbest_scores,
                                   rtol=0, atol=1e-9)


@pytest.mark.parametrize('V,T,beam,ctx', [(4, 50, 3, False), (7, 60, 6, True), (6, 120, 5, False),
                                          (8, 33, 8, True), (300, 40, 32, False),
                                          (20, 60, 20, True)])
@pytest.mark.parametrize('lds_pool', [1, 0])
def test_prefix_identity_is_exact_behind_a_2_bit_hash(V, T, beam, ctx, lds_pool):
    """Prefix identity = token sequence, exactly: with wn_tune_set("beam_weak_hash", 1) the
    64-bit prefix hash is replaced by a 2-bit one, so nearly every pair of prefixes passes the
    hash filter and the search is right only if the exact test behind it -- same node, else
    the token-by-token walk through the node pool -- is.  Both kernels (beam <= 16 and the
    general one), with and without a context graph: n-best lists, order, time stamps and
    fp64 scores identical to the oracle's.  lds_pool: the node pool in LDS (default where it
    fits) or in global scratch (what utterances past ~32 s get, wn_tune_set("beam_lds_pool", 0))."""
    from wenet_amd import _lib, search as S, synthetic
    from wenet_amd.context_graph import ContextGraph
    O = _oracle()
    logp, lens = synthetic.peaky_logprobs(32, (max(1, T // 2), T), V, 2.5, V * 11 + T + beam)
    og = gg = None
    if ctx:
        rng = np.random.RandomState(beam)
        phrases = [[int(t) for t in rng.randint(1, V, rng.randint(1, 4))] for _ in range(8)]
        og = O.ContextGraph(phrases, 2.0)
        gg = ContextGraph(context_list=phrases, context_score=2.0)
    ref = O.ctc_prefix_beam_search(logp, lens, beam, 0, og)
    L = _lib.lib()
    try:
        _lib.check(L.wn_tune_set(b'beam_weak_hash', 1), 'tune')
        _lib.check(L.wn_tune_set(b'beam_lds_pool', lds_pool), 'tune')
        got = S.ctc_prefix_beam_search(logp.cuda(), lens, beam, gg, 0)
    finally:
        L.wn_tune_set(b'beam_weak_hash', 0)
        L.wn_tune_set(b'beam_lds_pool', 1)
    for b in range(32):
        _same_nbest(got[b], ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times, f'utt {b}')


@pytest.mark.parametrize('T,beam', [(819, 10), (820, 10), (2047, 4), (2048, 4)])
def test_prefix_beam_at_the_lds_pool_boundary(T, beam):
    """The node pool (4 x (T * beam + 1) ints) moves from dynamic LDS to global scratch when it
    passes 128 KB (csrc/ctc.hip PB_LPOOL_BYTES): the last length that fits and the first that
    does not, for two beams, against the oracle (search.py:127-249) -- n-best, order, times, fp64
    scores."""
    from wenet_amd import search as S, synthetic
    O = _oracle()
    assert (4 * (T * beam + 1) * 4 <= 128 * 1024) == (T in (819, 2047))
    logp, lens = synthetic.peaky_logprobs(3, (T // 3, T), 12, 2.0, T + beam)
    ref = O.ctc_prefix_beam_search(logp, lens, beam)
    got = S.ctc_prefix_beam_search(logp.cuda(), lens, beam)
    for b in range(3):
        _same_nbest(got[b], ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times, f'utt {b}')


def test_prefix_beam_known_answer_gpu():
    """runtime/core/test/ctc_prefix_beam_search_test.cc:29-72 on the GPU."""
    from wenet_amd import search as S
    data = torch.tensor([[0.25, 0.40, 0.35], [0.40, 0.35, 0.25],
                         [0.10, 0.50, 0.40]]).log().unsqueeze(0)
    r = S.ctc_prefix_beam_search(data.cuda(), torch.tensor([3]), 3)[0]
    assert [list(x) for x in r.nbest] == [[2, 1], [1, 2], [1]]
    np.testing.assert_allclose(np.exp(r.nbest_scores),
                               [0.2185, 0.1550, 0.1525], rtol=1e-5)
    assert r.nbest_times == [[0, 2], [0, 2], [2]]


def test_maximum_length_utterance_and_one_frame_beyond():
    """The longest utterance the positional table allows (T' = 5000 encoder frames = 200 s of
    audio: RelPositionalEncoding max_len 5000, embedding.py:38-56,134-147) next to a short one,
    against the oracle: encoder output, greedy tokens, prefix-beam n-best (attention over 5000
    keys, 157 key tiles; the prefix beam search over 5000 dependent frames).  One encoder frame
    more must be refused like the reference's `assert offset + size <= self.max_len`
    (embedding.py:94), not read past the table."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 0)
    T = 4 * 5000 + 3                       # T' = ((T - 1) // 2 - 1) // 2 = 5000
    feats, _ = S.make_features(2, (T, T), seed=8)
    lens = torch.tensor([T, 431], dtype=torch.int32)
    feats[1, 431:] = 0.0
    with torch.no_grad():
        enc_ref, mask = O.encoder_forward(configs, sd, feats, lens)
    enc, gmask = model._forward_encoder(feats.cuda(), lens)
    ref_lens = mask.squeeze(1).sum(1).tolist()
    assert gmask.squeeze(1).sum(1).tolist() == ref_lens == [5000, 107]
    for b in range(2):
        n = ref_lens[b]
        err = (enc[b, :n].cpu() - enc_ref[b, :n]).abs().max().item()
        assert err < 2e-3, (b, err)
    ref = O.decode(configs, sd, METHODS[:2], feats, lens, beam_size=4)
    got = model.decode(METHODS[:2], feats.cuda(), lens, beam_size=4)
    logp = O.ctc_logprobs(sd, enc_ref)
    for b in range(2):
        n = ref_lens[b]
        top = logp[b, :n].topk(2, dim=-1)
        greedy_frame_check(model.ctc_logprobs(enc)[b, :n].argmax(-1).cpu().numpy(),
                           top.indices.numpy(), top.values.numpy(),
                           got['ctc_greedy_search'][b].tokens, ref['ctc_greedy_search'][b].tokens,
                           what=f'max length[{b}]')
    assert len(got['ctc_prefix_beam_search'][0].nbest) == len(ref['ctc_prefix_beam_search'][0].nbest)
    too_long = torch.zeros((1, T + 4, 80))
    with pytest.raises(RuntimeError, match='positional table'):
        model._forward_encoder(too_long.cuda(), torch.tensor([T + 4], dtype=torch.int32))


def test_zero_length_and_short_utterances():
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 0)
    feats, _ = S.make_features(4, 60, seed=3)
    lens = torch.tensor([60, 7, 6, 10], dtype=torch.int32)  # 6 -> no frames
    ref = O.decode(configs, sd, METHODS[:2], feats, lens, beam_size=3)
    got = model.decode(METHODS[:2], feats.cuda(), lens, beam_size=3)
    for b in range(4):
        assert got['ctc_greedy_search'][b].tokens == \
            ref['ctc_greedy_search'][b].tokens
        rp, gp = ref['ctc_prefix_beam_search'][b], got['ctc_prefix_beam_search'][b]
        assert len(gp.nbest) == len(rp.nbest)
        assert list(gp.tokens) == list(rp.tokens)


def test_rescoring_vs_oracle_on_same_hyps():
    """Feed the ORACLE's encoder output and n-best lists to the GPU rescoring:
    isolates the decoder path; scores within 1e-3."""
    from wenet_amd import search as S, synthetic as SY
    O = _oracle()
    for config, rw in [('tiny_causal', 0.3), ('tiny_sym', 0.0),
                       ('aishell_u2pp', 0.4), ('librispeech_bidecoder_large', 0.3)]:
        configs, sd, model = cached_model(config, 0)
        feats, lens = SY.make_features(3, (200, 330), seed=19)
        with torch.no_grad():
            enc, mask = O.encoder_forward(configs, sd, feats, lens)
            enc_lens = mask.squeeze(1).sum(1)
            logp = O.ctc_logprobs(sd, enc)
        pre = O.ctc_prefix_beam_search(logp, enc_lens, 6)
        sos, eos = O.special_symbols(configs)
        ref = O.attention_rescoring(configs, sd, pre, enc, enc_lens, 0.5, rw,
                                    sos, eos)
        got = S.attention_rescoring(model, pre, enc.cuda(), enc_lens, 0.5, rw)
        for b in range(3):
            np.testing.assert_allclose(got[b].all_scores, ref[b].all_scores,
                                       rtol=0, atol=1e-3)
            assert list(got[b].tokens) == list(ref[b].tokens)
            assert abs(got[b].confidence - ref[b].confidence) < 1e-4


def test_end_to_end_vs_oracle_ragged_batch():
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('aishell_u2pp', 0)
    feats, lens = S.make_features(6, (300, 520), seed=101)
    ref = O.decode(configs, sd, METHODS, feats, lens, beam_size=10,
                   ctc_weight=0.5, reverse_weight=0.3)
    got = model.decode(METHODS, feats.cuda(), lens, beam_size=10,
                       ctc_weight=0.5, reverse_weight=0.3)
    if True:
        # ctc_wave = 0: the block-per-row top-k kernel instead of the wave-per-row one (two-level
        # maxima): same top-k and bit-identical log-probs, so the same lists, bitwise
        from wenet_amd import _lib
        L = _lib.lib()
        try:
            _lib.check(L.wn_tune_set(b'ctc_wave', 0), 'tune')
            got2 = model.decode(METHODS, feats.cuda(), lens, beam_size=10,
                                ctc_weight=0.5, reverse_weight=0.3)
        finally:
            L.wn_tune_set(b'ctc_wave', 1)
        for b in range(6):
            for m in METHODS:
                assert got2[m][b].tokens == got[m][b].tokens, (m, b)
                assert got2[m][b].score == got[m][b].score, (m, b)
            p1, p2 = got['ctc_prefix_beam_search'][b], got2['ctc_prefix_beam_search'][b]
            assert p1.nbest == p2.nbest and p1.nbest_scores == p2.nbest_scores
            assert p1.nbest_times == p2.nbest_times
    with torch.no_grad():
        enc, mask = O.encoder_forward(configs, sd, feats, lens)
        ref_logp = O.ctc_logprobs(sd, enc)
    rv, ri = ref_logp.topk(2, dim=-1)
    enc_lens = mask.squeeze(1).sum(1)
    genc, _ = model._forward_encoder(feats.cuda(), lens)
    top1 = model.ctc_logprobs(genc, encoder_lens=enc_lens).argmax(-1).cpu().numpy()
    n_frames = n_strict = 0
    for b in range(6):
        n = int(enc_lens[b])
        f, st, _ = greedy_frame_check(top1[b, :n], ri[b, :n].numpy(), rv[b, :n].numpy(),
                                      got['ctc_greedy_search'][b].tokens,
                                      ref['ctc_greedy_search'][b].tokens, what=f'e2e[{b}]')
        n_frames += f; n_strict += st
        rp = ref['ctc_prefix_beam_search'][b]
        nbest_check(got['ctc_prefix_beam_search'][b], rp.nbest,
                    rp.nbest_scores, rp.nbest_times, what=f'e2e[{b}]')
        rr = ref['attention_rescoring'][b]
        rescoring_check(got['attention_rescoring'][b], got['ctc_prefix_beam_search'][b],
                        dict(all_scores=rr.all_scores, tokens=list(rr.tokens),
                             score=rr.score), rp.nbest, what=f'e2e[{b}]')
    assert n_strict >= 0.95 * n_frames


def test_padding_invariance_property():
    """Size-independent property: an utterance decodes identically whether it
    is alone or padded inside a ragged batch (the packed layout never lets pad
    frames leak)."""
    from wenet_amd import synthetic as S
    # (causal conv module + full attention: the reference itself is padding
    # invariant only then -- a symmetric conv module sees GLU(bias) instead of 0
    # right of the utterance end inside a padded batch, convolution.py:119-120)
    configs, sd, model = cached_model('tiny_causal', 0)
    feats, lens = S.make_features(5, (60, 300), seed=8)
    full = model.decode(METHODS[:2], feats.cuda(), lens, beam_size=4)
    for b in range(5):
        n = int(lens[b])
        one = model.decode(METHODS[:2], feats[b:b + 1, :n].cuda(), lens[b:b + 1],
                           beam_size=4)
        assert one['ctc_greedy_search'][0].tokens == \
            full['ctc_greedy_search'][b].tokens
        assert list(one['ctc_prefix_beam_search'][0].tokens) == \
            list(full['ctc_prefix_beam_search'][b].tokens)


def test_fbank_vs_oracle():
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_sym', 0)
    waves = [S.make_audio(n, seed=i) for i, n in enumerate([16000, 5000, 399, 24321])]
    feats, nfr = model.compute_fbank(waves)
    feats = feats.cpu().numpy()
    for i, w in enumerate(waves):
        ref = O.fbank(w)
        assert int(nfr[i]) == ref.shape[0]
        if ref.shape[0]:
            err = np.abs(feats[i, :ref.shape[0]] - ref)
            # log-mel of fp32 FFTs: a few low-energy bins carry the error
            assert np.percentile(err, 99) < 2e-3 and err.max() < 5e-2, \
                (i, np.percentile(err, 99), err.max())
        assert np.all(feats[i, ref.shape[0]:] == 0)


def test_fbank_vs_reference_cpp_golden():
    """wn_fbank against the committed outputs of the reference's own C++ fbank
    (tests/golden/fbank_*.npz, oracle/gen_golden_fbank.py)."""
    import glob
    import json
    import os
    from wenet_amd import synthetic as S
    configs, sd, model = cached_model('tiny_sym', 0)
    metas, refs, waves = [], [], []
    for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden',
                                           'fbank_*.npz'))):
        z = np.load(p)
        meta = json.loads(bytes(z['meta']).decode())
        metas.append(meta)
        refs.append(z['feats'])
        waves.append(S.make_audio(meta['samples'], seed=meta['seed']))
    assert len(waves) >= 4
    feats, nfr = model.compute_fbank(waves)
    feats = feats.cpu().numpy()
    for i, ref in enumerate(refs):
        assert int(nfr[i]) == ref.shape[0] == metas[i]['frames']
        if ref.shape[0]:
            err = np.abs(feats[i, :ref.shape[0]] - ref)
            assert np.percentile(err, 99) < 2e-3 and err.max() < 5e-2, \
                (metas[i]['case'], np.percentile(err, 99), err.max())


@pytest.mark.parametrize('name', stream_case_names())
def test_simulate_streaming_vs_reference_cache_path(name):
    """decode(simulate_streaming=True) against the committed outputs of the
    reference's cache-based forward_chunk_by_chunk (encoder.py:287-362)."""
    from wenet_amd import synthetic as S
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    feats, lens = S.make_features(1, (meta['frames'], meta['frames']),
                                  seed=meta['fseed'])
    enc, mask = model._forward_encoder(feats.cuda(), lens, meta['chunk'],
                                       meta['left'], simulate_streaming=True)
    assert enc.shape[1] == arrays['enc_out'].shape[0]
    assert np.abs(enc[0].cpu().numpy() - arrays['enc_out']).max() < 2e-3
    res = model.decode(METHODS, feats.cuda(), lens, beam_size=meta['beam'],
                       decoding_chunk_size=meta['chunk'],
                       num_decoding_left_chunks=meta['left'],
                       ctc_weight=meta['ctc_weight'],
                       reverse_weight=meta['reverse_weight'],
                       simulate_streaming=True)
    assert res['ctc_greedy_search'][0].tokens == meta['greedy']
    g = meta['prefix']
    nbest_check(res['ctc_prefix_beam_search'][0], g['nbest'], g['nbest_scores'],
                g['nbest_times'], what=name)
    r = res['attention_rescoring'][0]
    gs = sorted(r.all_scores, reverse=True)
    if len(gs) < 2 or gs[0] - gs[1] > 2e-3:
        assert list(r.tokens) == meta['rescoring']['tokens'], name
    if list(r.tokens) == meta['rescoring']['tokens']:
        assert abs(r.score - meta['rescoring']['score']) < 1e-3
    # the reference's preconditions
    two = torch.cat([feats, feats]).cuda()
    with pytest.raises(AssertionError):
        model.decode(METHODS[:1], two, torch.cat([lens, lens]),
                     decoding_chunk_size=meta['chunk'], simulate_streaming=True)


@pytest.mark.parametrize('name', attention_case_names())
def test_attention_mode_vs_reference(name):
    """decode(['attention']) (autoregressive beam search through
    wn_decoder_next_topk) against the committed outputs of the real reference."""
    meta, _ = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    _, _, feats, lens = build_inputs(meta)
    got = model.decode(['attention'], feats.cuda(), lens, beam_size=meta['beam'],
                       length_penalty=meta['length_penalty'])['attention']
    assert [list(r.tokens) for r in got] == meta['tokens']
    # together with the other modes, and after them (batch state is shared)
    allm = model.decode(['ctc_greedy_search', 'attention', 'attention_rescoring'],
                        feats.cuda(), lens, beam_size=meta['beam'],
                        length_penalty=meta['length_penalty'], ctc_weight=0.5)
    assert [list(r.tokens) for r in allm['attention']] == meta['tokens']


@pytest.mark.parametrize('beam,frames', [(20, (60, 120)), (33, (40, 90)), (3, (200, 260))])
def test_attention_mode_wide_beams_and_long_outputs_vs_oracle(beam, frames):
    """`--modes attention --beam_size 20` and beyond (the N x N re-ranking strided over the
    block: beams up to 64), and outputs longer than the 32 steps the self-attention cache
    starts with (T' ~ 50-65 steps with a random-init decoder that rarely emits <eos>: the cache
    doubles once or twice) -- token lists identical to the oracle's attention_beam_search
    (search.py:252-371 restated) on the GPU's own encoder output."""
    from gpu_util import make_model
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 0)
    if beam == 3:
        # a decoder that (almost) never ends a hypothesis: <eos> pushed far down in every
        # output layer, so the search runs all T' steps
        sd = dict(sd)
        for k in list(sd):
            if k.endswith('output_layer.bias'):
                b = sd[k].clone()
                b[model.eos] = -60.0
                sd[k] = b
        model = make_model(configs, sd)
    feats, lens = S.make_features(3, frames, seed=900 + beam)
    got = model.decode(['attention'], feats.cuda(), lens, beam_size=beam,
                       length_penalty=0.3)['attention']
    enc, mask = model._forward_encoder(feats.cuda(), lens)
    with torch.no_grad():
        ref = O.attention_beam_search(configs, sd, enc.cpu(), mask.cpu(), beam, 0.3,
                                      sos=model.sos, eos=model.eos)
    assert [list(r.tokens) for r in got] == [list(r.tokens) for r in ref]
    assert max(len(r.tokens) for r in got) > (32 if beam == 3 else 0)


@pytest.mark.parametrize('name', ['tiny_lite_one', 'tiny_lite_equal', 'aishell_lite_one'])
def test_filter_blank_embedding_vs_reference_output(name):
    """ASRModel.filter_blank_embedding (wn_filter_blank_embedding; asr_model.py:153-180) on the
    reference's own encoder output and CTC posteriors: the selected rows, their zero padding and
    the mask equal what the REAL reference's method returned (tests/golden/*lite*)."""
    O = _oracle()
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    enc = torch.from_numpy(arrays['enc_out'])
    logp = O.ctc_logprobs(sd, enc)
    sel, mask = model.filter_blank_embedding(logp.cuda(), enc.cuda())
    assert mask.squeeze(1).sum(1).tolist() == meta['nonblank_kept']
    np.testing.assert_array_equal(sel.cpu().numpy(), arrays['nonblank_out'])


def test_non_blank_embedding_rescoring_on_a_ragged_batch():
    """decode(attention_rescoring) of a model with model_conf.apply_non_blank_embedding on a
    RAGGED batch against the oracle with the path's one documented deviation (frames beyond an
    utterance's length never count: the accelerated path has no padded frames, the reference
    lets their arg-max decide too): every hypothesis' score within 1e-3, same winner; and the
    scores differ from rescoring on the unfiltered encoder output (the filter ran)."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_lite', 0)
    feats, lens = S.make_features(5, (60, 190), seed=4242)
    kw = dict(beam_size=5, ctc_weight=0.5, reverse_weight=0.3)
    got = model.decode(['ctc_prefix_beam_search', 'attention_rescoring'], feats.cuda(), lens, **kw)
    ref = O.decode(configs, sd, ['ctc_prefix_beam_search', 'attention_rescoring'], feats, lens,
                   nonblank_valid_only=True, **kw)
    plain = dict(configs)
    plain['model_conf'] = dict(configs['model_conf'], apply_non_blank_embedding=False)
    ref_plain = O.decode(plain, sd, ['attention_rescoring'], feats, lens, **kw)
    moved = 0.0
    for b in range(5):
        g, r = got['attention_rescoring'][b], ref['attention_rescoring'][b]
        assert [list(x) for x in got['ctc_prefix_beam_search'][b].nbest] == \
            [list(x) for x in ref['ctc_prefix_beam_search'][b].nbest]
        assert list(g.tokens) == list(r.tokens), b
        assert abs(g.score - r.score) < 1e-3, (b, g.score, r.score)
        moved = max(moved, abs(r.score - ref_plain['attention_rescoring'][b].score))
    assert moved > 1e-2, moved


@pytest.mark.parametrize('name', ['raggedlite_tiny', 'raggedlite_tiny_padded'])
def test_non_blank_embedding_rescoring_vs_the_reference_on_ragged_batches(name):
    """The same decode against the REAL reference (tests/golden/raggedlite_*.npz).  Where no
    padded frame has a non-blank arg-max (`raggedlite_tiny`) the accelerated path IS the
    reference: scores within 1e-3.  In `raggedlite_tiny_padded` the reference keeps 4 .. 23
    padded frames per shorter utterance and pads every utterance to the longest such selection;
    the accelerated path has no padded frames -- the one documented deviation of the path
    (include/wenet_amd.h wn_filter_blank_embedding): MEASURED tolerance 0.15 on the score of
    this random-weight model (oracle-to-reference 0.10 on CPU, tests/test_oracle.py), identical
    winners, and exact (1e-3) against the oracle restricted to valid frames."""
    from wenet_amd import synthetic as S
    O = _oracle()
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    _, _, feats, lens = build_inputs(meta)
    kw = dict(beam_size=meta['beam'], ctc_weight=meta['ctc_weight'],
              reverse_weight=meta['reverse_weight'])
    got = model.decode(['attention_rescoring'], feats.cuda(), lens, **kw)['attention_rescoring']
    val = O.decode(configs, sd, ['attention_rescoring'], feats, lens, nonblank_valid_only=True,
                   **kw)['attention_rescoring']
    tol = 1e-3 if name == 'raggedlite_tiny' else 0.15
    dev = 0.0
    for b in range(meta['batch']):
        gr = meta['rescoring'][b]
        assert list(got[b].tokens) == gr['tokens'], b
        assert abs(got[b].score - val[b].score) < 1e-3, (b, got[b].score, val[b].score)
        dev = max(dev, abs(got[b].score - gr['score']))
    print(f'\n[{name}] max |score - reference| {dev:.3e} (tolerance {tol})')
    assert dev < tol


@pytest.mark.parametrize('n_mels', [80, 128])
def test_log_mel_vs_oracle(n_mels):
    """wn_log_mel (Whisper frontend, processor.py:320-369) against the oracle
    (torch.stft + restated librosa mel) on ragged waveforms."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_sym', 0)
    waves = [S.make_audio(n, seed=40 + i) for i, n in enumerate([16000, 7001, 201, 48000])]
    feats, nfr = model.compute_log_mel_spectrogram(waves, n_mels)
    feats = feats.cpu().numpy()
    for i, w in enumerate(waves):
        ref = O.log_mel_spectrogram(w, n_mels)
        assert int(nfr[i]) == ref.shape[0] == len(w) // 160
        got = feats[i, :ref.shape[0]]
        err = np.abs(got - ref)
        # fp32 DFT noise only matters in the decade just above the 8-decade floor
        assert np.percentile(err, 99) < 2e-3 and err.max() < 5e-2, \
            (i, np.percentile(err, 99), err.max())
        high = ref > ref.max() - 1.0   # top 4 decades
        assert err[high].max() < 2e-4, err[high].max()
        assert np.all(feats[i, ref.shape[0]:] == 0)
    padded, n2 = model.compute_log_mel_spectrogram(waves[:2], n_mels, pad_or_trim=True)
    assert padded.shape == (2, 3000, n_mels) and n2.tolist() == [3000, 3000]
    ref = O.log_mel_spectrogram(waves[1], n_mels, pad_or_trim=True)
    assert np.percentile(np.abs(padded[1].cpu().numpy() - ref), 99) < 2e-3


def test_rejects_cpu_tensors_and_chunk_zero():
    configs, sd, model = cached_model('tiny_sym', 0)
    from wenet_amd import search as S
    with pytest.raises(RuntimeError):
        S.ctc_greedy_search(torch.zeros(1, 4, 8), torch.tensor([4]))
    feats = torch.zeros(1, 40, 80)
    with pytest.raises(AssertionError):
        model.decode(['ctc_greedy_search'], feats.cuda(), torch.tensor([40]),
                     decoding_chunk_size=0)


def test_pipeline_two_streams_matches_sequential_decode():
    """wenet_amd.pipeline.DecodePipeline (2 decodes in flight on cloned
    workspace handles) returns exactly what back-to-back decode() calls do."""
    from wenet_amd import synthetic as S
    from wenet_amd.pipeline import DecodePipeline
    configs, sd, model = cached_model('tiny_causal', 0)
    batches = []
    for i in range(5):
        feats, lens = S.make_features(3 + i % 2, (40, 160), seed=100 + i)
        batches.append((feats.cuda(), lens))
    kw = dict(beam_size=4, ctc_weight=0.5, reverse_weight=0.3)
    seq = [model.decode(METHODS, f, l, **kw) for f, l in batches]
    with DecodePipeline(model, n_streams=2) as pipe:
        par = pipe.decode_many(METHODS, batches, **kw)
        par2 = pipe.decode_many(METHODS, batches[::-1], **kw)[::-1]
    for got_all in (par, par2):
        for want, got in zip(seq, got_all):
            for m in METHODS:
                assert len(want[m]) == len(got[m])
                for a, b in zip(want[m], got[m]):
                    assert list(a.tokens) == list(b.tokens)
                    assert a.score == b.score
                    if a.nbest is not None:
                        assert [list(x) for x in a.nbest] == [list(x) for x in b.nbest]
                        assert list(a.nbest_scores) == list(b.nbest_scores)


def test_pipeline_six_free_running_streams_match_sequential_decode():
    """Round 6: above two streams DecodePipeline lets the encoders run free (no event chain;
    the bench's headline keeps six decodes in flight): on the full-size model, batches of
    different shapes decoded six at a time return exactly what back-to-back decode() calls do
    -- every decode has its own workspace handle, nothing depends on the order the GPU
    interleaves them in."""
    from wenet_amd import synthetic as S
    from wenet_amd.pipeline import DecodePipeline
    configs, sd, model = cached_model('aishell_u2pp', 0)
    batches = []
    for i in range(9):
        feats, lens = S.make_features(6 + 3 * (i % 3), (200 + 100 * (i % 4), 900), seed=300 + i)
        batches.append((feats.cuda(), lens))
    kw = dict(beam_size=10)
    methods = ['ctc_greedy_search', 'ctc_prefix_beam_search']
    seq = [model.decode(methods, f, l, **kw) for f, l in batches]
    with DecodePipeline(model, n_streams=6) as pipe:
        assert pipe.chain is False or os.environ.get('WN_PIPE_CHAIN') == '1'
        par = pipe.decode_many(methods, batches, **kw)
        par2 = pipe.decode_many(methods, batches[::-1], **kw)[::-1]
    for got_all in (par, par2):
        for want, got in zip(seq, got_all):
            for m in methods:
                assert len(want[m]) == len(got[m])
                for a, b in zip(want[m], got[m]):
                    assert list(a.tokens) == list(b.tokens)
                    assert a.score == b.score
                    if a.nbest is not None:
                        assert [list(x) for x in a.nbest] == [list(x) for x in b.nbest]
                        assert list(a.nbest_scores) == list(b.nbest_scores)


@pytest.mark.parametrize('gate', [True, False])
def test_pipeline_encode_gate_keeps_results_and_survives_a_failed_decode(gate):
    """wn_model_set_encode_gate (round 5): with two decodes in flight the wait for the previous
    decode's encoder is placed by the library -- behind wn_encode's descriptor uploads and in
    front of conv1 by default (tune enc_gate_pos = 0; 1 = behind CMVN + conv1, which then runs
    beside that encoder).  It only orders work for performance: each decode has its own
    workspace, so every result must equal the sequential decode()'s, on
    batches of different shapes back to back (a front end that ran too early or an encoder that
    did not wait shows up as another batch's numbers).  A decode that fails in front of
    wn_encode must not leave its gate on the handle."""
    from wenet_amd import synthetic as S
    from wenet_amd.pipeline import DecodePipeline
    configs, sd, model = cached_model('aishell_u2pp', 0)
    batches = []
    for i in range(6):
        feats, lens = S.make_features(6 + 5 * (i % 3), (300, 900), seed=300 + i)
        batches.append((feats.cuda(), lens))
    M = ['ctc_prefix_beam_search']
    seq = [model.decode(M, f, l, beam_size=6) for f, l in batches]
    with DecodePipeline(model, n_streams=2) as pipe:
        pipe.gate_front_end = gate
        par = pipe.decode_many(M, batches, beam_size=6)
        # a decode that raises before its encoder is queued (decoding_chunk_size = 0,
        # asr_model.py:310), then the same batches again in the other order
        with pytest.raises(AssertionError):
            pipe.submit(M, batches[0][0], batches[0][1], beam_size=6,
                        decoding_chunk_size=0).result()
        par2 = pipe.decode_many(M, batches[::-1], beam_size=6)[::-1]
    for got_all in (par, par2):
        for want, got in zip(seq, got_all):
            for a, b in zip(want[M[0]], got[M[0]]):
                assert list(a.tokens) == list(b.tokens) and a.score == b.score
                assert [list(x) for x in a.nbest] == [list(x) for x in b.nbest]
                assert list(a.nbest_scores) == list(b.nbest_scores)


# --------------------------------------------------------------------------
# context biasing (ContextGraph, search.py:127-249 with context_graph)


def _same_nbest(got, want_nbest, want_scores, want_times, what=''):
    assert [list(x) for x in got.nbest] == [list(x) for x in want_nbest], what
    assert [list(x) for x in got.nbest_times] == [list(x) for x in want_times], what
    np.testing.assert_allclose(got.nbest_scores, want_scores, rtol=0, atol=1e-9)


@pytest.mark.parametrize('name', context_search_case_names())
def test_context_search_vs_reference_golden(name):
    """The reference's biased ctc_prefix_beam_search on seeded log-probs (the
    same fp32 tensor goes to the GPU): n-best lists, order, time stamps
    identical, fp64 scores to 1e-9."""
    from wenet_amd import search as S
    from wenet_amd import synthetic
    from wenet_amd.context_graph import ContextGraph
    meta, _ = load_case(name)
    logp, lens = synthetic.peaky_logprobs(meta['batch'], meta['frames'], meta['vocab'],
                                          meta['peak'], meta['seed'])
    g = ContextGraph(context_list=meta['phrases'], context_score=meta['context_score'])
    got = S.ctc_prefix_beam_search(logp.cuda(), lens, meta['beam'], g, 0)
    w = meta['prefix']
    for b in range(meta['batch']):
        _same_nbest(got[b], w['nbest'][b], w['nbest_scores'][b], w['nbest_times'][b],
                    f'{name}[{b}]')
    # the handle's graph is cleared afterwards: an unbiased search is unbiased
    O = _oracle()
    plain = S.ctc_prefix_beam_search(logp.cuda(), lens, meta['beam'], None, 0)
    ref = O.ctc_prefix_beam_search(logp, lens, meta['beam'])
    for b in range(meta['batch']):
        _same_nbest(plain[b], ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times)


@pytest.mark.parametrize('V,T,beam,n_phr,score', [
    (4, 60, 3, 5, 1.0), (6, 90, 5, 12, 2.5), (9, 50, 8, 30, 0.7), (30, 70, 10, 40, 6.0),
    (5, 40, 16, 10, 3.0), (12, 100, 1, 8, 2.0)])
def test_context_search_stress_vs_oracle(V, T, beam, n_phr, score):
    """Random graphs over tiny vocabularies: phrases match, overlap, fail and
    re-merge in almost every frame; 32 utterances per case."""
    from wenet_amd import search as S
    from wenet_amd import synthetic
    from wenet_amd.context_graph import ContextGraph
    O = _oracle()
    beam = min(beam, V)
    rng = np.random.RandomState(V * 100 + T)
    phrases = [[int(t) for t in rng.randint(1, V, rng.randint(1, 6))]
               for _ in range(n_phr)]
    logp, lens = synthetic.peaky_logprobs(32, (1, T), V, 2.5, V * 7 + beam)
    ref = O.ctc_prefix_beam_search(logp, lens, beam, 0, O.ContextGraph(phrases, score))
    got = S.ctc_prefix_beam_search(logp.cuda(), lens, beam,
                                   ContextGraph(context_list=phrases,
                                                context_score=score), 0)
    for b in range(32):
        _same_nbest(got[b], ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times,
                    f'utt {b}')


@pytest.mark.parametrize('name', context_case_names())
def test_context_decode_vs_reference_golden(name):
    """decode(..., context_graph=g) through the model: (1) the biased search on
    the GPU's own CTC log-probs equals the oracle's on the same tensor, bit for
    bit; (2) the reference's committed result: best hypothesis, scores of the
    shared hypotheses, rescoring result."""
    from wenet_amd.context_graph import ContextGraph
    O = _oracle()
    meta, _ = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    _, _, feats, lens = build_inputs(meta)
    g = ContextGraph(context_list=meta['phrases'], context_score=meta['context_score'])
    kw = dict(beam_size=meta['beam'], ctc_weight=meta['ctc_weight'],
              reverse_weight=meta['reverse_weight'],
              blank_penalty=meta['blank_penalty'])
    res = model.decode(['ctc_prefix_beam_search', 'attention_rescoring'], feats.cuda(),
                       lens, context_graph=g, **kw)
    enc, mask = model._forward_encoder(feats.cuda(), lens)
    enc_lens = mask.squeeze(1).sum(1).cpu()
    logp = model.ctc_logprobs(enc, meta['blank_penalty'], 0, encoder_lens=enc_lens).cpu()
    ref = O.ctc_prefix_beam_search(logp, enc_lens, meta['beam'], 0,
                                   O.ContextGraph(meta['phrases'], meta['context_score']))
    w = meta['prefix']
    for b in range(meta['batch']):
        got = res['ctc_prefix_beam_search'][b]
        _same_nbest(got, ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times,
                    f'{name}[{b}]')
        assert list(got.tokens) == w['nbest'][b][0], (name, b)
        shared = 0
        for i, h in enumerate(w['nbest'][b]):
            if h in [list(x) for x in got.nbest]:
                j = [list(x) for x in got.nbest].index(h)
                assert abs(got.nbest_scores[j] - w['nbest_scores'][b][i]) < 2e-3
                shared += 1
        assert shared >= len(w['nbest'][b]) - 1, (name, b, shared)
        r = res['attention_rescoring'][b]
        assert list(r.tokens) == meta['rescoring_tokens'][b], (name, b)
        assert abs(r.score - meta['rescoring_scores'][b]) < 1e-3 * (len(r.tokens) + 1)
    # the same model without a graph is unbiased again (the handle is cleared)
    plain = model.decode(['ctc_prefix_beam_search'], feats.cuda(), lens, **kw)
    ref0 = O.ctc_prefix_beam_search(logp, enc_lens, meta['beam'], 0)
    for b in range(meta['batch']):
        _same_nbest(plain['ctc_prefix_beam_search'][b], ref0[b].nbest,
                    ref0[b].nbest_scores, ref0[b].nbest_times)


def test_context_graph_object_of_the_reference_is_accepted():
    """A duck-typed reference ContextGraph (root ContextState with next / fail /
    node_score / output_score / token_score) is flattened and gives the same
    result as the native class."""
    from wenet_amd import search as S
    from wenet_amd import synthetic
    from wenet_amd.context_graph import ContextGraph

    class St:
        def __init__(self, token, token_score, node_score, output_score):
            self.token, self.token_score = token, token_score
            self.node_score, self.output_score = node_score, output_score
            self.next, self.fail = {}, None

    phrases = [[1, 2, 3], [2, 3], [3, 1]]
    g = ContextGraph(context_list=phrases, context_score=2.0)
    f = g.flat()
    nodes = [St(-1 if i == 0 else 0, f.token_score[i], f.node_score[i],
                f.output_score[i]) for i in range(f.n_nodes)]
    for a, t, b in zip(f.edge_from, f.edge_token, f.edge_to):
        nodes[a].next[int(t)] = nodes[b]
        nodes[b].token = int(t)
    for i, n in enumerate(nodes):
        n.fail = nodes[f.fail[i]]

    class RefLike:
        root = nodes[0]

    logp, lens = synthetic.peaky_logprobs(6, (20, 50), 5, 2.0, 3)
    a = S.ctc_prefix_beam_search(logp.cuda(), lens, 4, g, 0)
    b = S.ctc_prefix_beam_search(logp.cuda(), lens, 4, RefLike(), 0)
    for x, y in zip(a, b):
        _same_nbest(x, y.nbest, y.nbest_scores, y.nbest_times)


# --------------------------------------------------------------------------
# streaming API: forward_encoder_chunk with caches (encoder.py:204-362)


@pytest.mark.parametrize('name', chunk_case_names())
def test_forward_encoder_chunk_vs_reference_golden(name):
    """Chunk outputs and the attention / convolution caches (the reference's
    tensor layouts) against the real reference's forward_encoder_chunk."""
    from wenet_amd import synthetic as S
    meta, arrays = load_case(name)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    feats, _ = S.make_features(1, (meta['frames'], meta['frames']), seed=meta['fseed'])
    feats = feats.cuda()
    att = cnn = None
    outs, offset = [], 0
    required = meta['chunk'] * meta['left']

    def close(t, want, what):
        assert tuple(t.shape) == want.shape, (what, tuple(t.shape), want.shape)
        if want.size:
            err = np.abs(t.cpu().numpy() - want).max()
            assert err < 2e-3, (name, what, err)

    for i, (a, b) in enumerate(chunk_windows(meta['frames'], meta['chunk'])):
        y, att, cnn = model.forward_encoder_chunk(feats[:, a:b], offset, required, att, cnn)
        outs.append(y)
        offset += y.size(1)
        if i == meta['probe']:
            close(att, arrays['att_probe'], 'att_probe')
            close(cnn, arrays['cnn_probe'], 'cnn_probe')
    assert [int(y.size(1)) for y in outs] == meta['chunk_sizes']
    close(torch.cat(outs, 1)[0], arrays['enc_out'], 'enc_out')
    close(att, arrays['att_last'], 'att_last')
    close(cnn, arrays['cnn_last'], 'cnn_last')
    if meta['config'] != 'tiny_sym':
        ys, mask = model.forward_encoder_chunk_by_chunk(feats, meta['chunk'], meta['left'])
        assert torch.equal(ys, torch.cat(outs, 1)) and mask.shape == (1, 1, ys.size(1))
        # causal chunk-trained model: the cache path equals the chunk-mask path
        full, _ = model._forward_encoder(feats, torch.tensor([meta['frames']]),
                                         meta['chunk'], meta['left'])
        assert (full[0] - ys[0]).abs().max() < 2e-3
        logp = model.ctc_activation(ys)
        assert logp.shape == (1, ys.size(1), model.vocab_size)
        assert torch.allclose(logp.exp().sum(-1), torch.ones_like(logp[..., 0]), atol=1e-4)


def test_forward_encoder_chunk_vs_oracle_random_sessions():
    """Sessions with varying window lengths and cache policies against the
    oracle's forward_chunk on the same inputs and caches."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 1)
    rng = np.random.RandomState(3)
    for session in range(4):
        feats, _ = S.make_features(1, (260, 260), seed=200 + session)
        required = int(rng.choice([-1, 0, 5, 9]))
        att = cnn = o_att = o_cnn = None
        offset, cur = 0, 0
        while cur + 7 <= 260:
            time = int(rng.choice([7, 11, 19, 23, 35]))
            win = feats[:, cur:min(cur + time, 260)]
            y, att, cnn = model.forward_encoder_chunk(win.cuda(), offset, required, att, cnn)
            oy, o_att, o_cnn = O.forward_chunk(configs, sd, win, offset, required,
                                               o_att, o_cnn)
            assert tuple(y.shape) == tuple(oy.shape)
            assert (y.cpu() - oy).abs().max() < 2e-3
            assert tuple(att.shape) == tuple(o_att.shape)
            if o_att.numel():
                assert (att.cpu() - o_att).abs().max() < 2e-3
            assert (cnn.cpu() - o_cnn).abs().max() < 2e-3
            # continue from the ORACLE's caches: errors must not compound in the test
            att, cnn = o_att.cuda(), o_cnn.cuda()
            offset += y.size(1)
            cur += 4 * y.size(1)


# --------------------------------------------------------------------------
# the recognize CLI end to end (wav list -> result files)


def test_recognize_cli_end_to_end(tmp_path):
    """wenet_amd.bin.recognize on a list of wav files: lines in the reference's
    order (batches in list order, longest first inside a batch); tokens equal to
    a direct decode() of the same features and, for greedy search, to the oracle
    on oracle-computed fbank features."""
    import json
    import wave
    import yaml
    from wenet_amd import synthetic as S
    from wenet_amd.bin import recognize as R
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 0)
    V = configs['output_dim']
    units = tmp_path / 'units.txt'
    syms = ['<blank>', '<unk>'] + [f't{i}' for i in range(2, V - 1)] + ['<sos/eos>']
    units.write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    cfg = dict(configs)
    cfg['tokenizer'] = 'char'
    cfg['tokenizer_conf'] = dict(symbol_table_path=str(units), non_lang_syms_path=None,
                                 connect_symbol=' ')
    cfg['dataset_conf'] = dict(fbank_conf=dict(num_mel_bins=80, frame_length=25,
                                               frame_shift=10, dither=0.1))
    (tmp_path / 'train.yaml').write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / 'final.pt')
    rng = np.random.RandomState(11)
    entries, pcm = [], {}
    for i in range(7):
        n = int(rng.randint(16000, 40000))
        t = np.arange(n) / 16000.0
        x = 0.3 * np.sin(2 * np.pi * (200 + 90 * i) * t) + 0.05 * rng.randn(n)
        x16 = np.clip(x * 32768, -32768, 32767).astype(np.int16)
        path = tmp_path / f'u{i}.wav'
        with wave.open(str(path), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(x16.tobytes())
        entries.append((f'utt{i}', str(path)))
        pcm[f'utt{i}'] = x16.astype(np.float32) / 32768.0
    lst = tmp_path / 'data.list'
    lst.write_text(''.join(json.dumps(dict(key=k, wav=w, txt='')) + '\n'
                           for k, w in entries))
    modes = ['ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring']
    out = tmp_path / 'out'
    rc = R.main(['--config', str(tmp_path / 'train.yaml'), '--checkpoint',
                 str(tmp_path / 'final.pt'), '--test_data', str(lst), '--result_dir',
                 str(out), '--batch_size', '3', '--beam_size', '4', '--ctc_weight', '0.5',
                 '--reverse_weight', '0.3', '--blank_penalty', '3.0', '--modes'] + modes)
    assert rc == 0
    got = {m: (out / m / 'text').read_text().splitlines() for m in modes}
    # expected: batch by batch, direct decode of device fbank features
    want = {m: [] for m in modes}
    greedy_ref = {}
    for batch in R.static_batches(entries, 3):
        waves = [pcm[k] for k, _ in batch]
        feats, nfr = model.compute_fbank(waves)
        perm = R.padding_order(nfr.tolist())
        idx = torch.as_tensor(perm)
        f = feats.index_select(0, idx.cuda())[:, :int(nfr.max())].contiguous()
        res = model.decode(modes, f, nfr.index_select(0, idx), beam_size=4, ctc_weight=0.5,
                           reverse_weight=0.3, blank_penalty=3.0)
        for j, i in enumerate(perm):
            for m in modes:
                toks = res[m][j].tokens
                want[m].append(batch[i][0] + ' ' + ' '.join(syms[t] for t in toks))
        # oracle: fbank + encoder + greedy on the CPU for the same waveforms
        ofe = [torch.as_tensor(O.fbank(pcm[batch[i][0]])) for i in perm]
        of = torch.nn.utils.rnn.pad_sequence(ofe, batch_first=True)
        ol = torch.tensor([x.shape[0] for x in ofe], dtype=torch.int32)
        ores = O.decode(configs, sd, ['ctc_greedy_search'], of, ol, blank_penalty=3.0)
        enc, mask = O.encoder_forward(configs, sd, of, ol)
        margins = frame_margins(O.ctc_logprobs(sd, enc, 3.0))
        for j, i in enumerate(perm):
            n = int(mask[j].sum())
            if margins[j, :n].min() > 2e-2:
                greedy_ref[batch[i][0]] = ' '.join(syms[t] for t in
                                                   ores['ctc_greedy_search'][j].tokens)
    for m in modes:
        assert got[m] == want[m], m
    checked = 0
    for ln in got['ctc_greedy_search']:
        key, _, text = ln.partition(' ')
        if key in greedy_ref:
            assert text == greedy_ref[key], key
            checked += 1
    assert checked >= 3


def test_transcribe_cli_with_resampling_and_context(tmp_path, capsys):
    """`python -m wenet_amd.bin.transcribe` on an 8 kHz wav in a model directory
    (train.yaml / final.pt / units.txt): the printed text equals a direct decode
    of the device-resampled, device-fbank features; a context list is accepted."""
    import wave
    import yaml
    from wenet_amd.bin import transcribe as T
    configs, sd, model = cached_model('tiny_causal', 0)
    V = configs['output_dim']
    syms = ['<blank>', '<unk>'] + [f't{i}' for i in range(2, V - 1)] + ['<sos/eos>']
    (tmp_path / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    cfg = dict(configs)
    cfg['tokenizer'] = 'char'
    cfg['tokenizer_conf'] = dict(symbol_table_path='units.txt', non_lang_syms_path=None,
                                 connect_symbol=' ')
    (tmp_path / 'train.yaml').write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / 'final.pt')
    rng = np.random.RandomState(5)
    n = 14000
    x = 0.4 * np.sin(2 * np.pi * 330 * np.arange(n) / 8000.0) + 0.05 * rng.randn(n)
    x16 = np.clip(x * 32768, -32768, 32767).astype(np.int16)
    wav = tmp_path / 'a8k.wav'
    with wave.open(str(wav), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(x16.tobytes())
    assert T.main([str(wav), '-m', str(tmp_path)]) == 0
    text = capsys.readouterr().out.strip().splitlines()[-1]
    pcm16k = model.resample(x16.astype(np.float32) / 32768.0, 8000, 16000)
    assert pcm16k.shape[0] == 2 * n
    feats, nfr = model.compute_fbank([pcm16k])
    want = model.decode(['attention_rescoring'], feats, nfr)['attention_rescoring'][0]
    assert text == ' '.join(syms[t] for t in want.tokens)
    ctx = tmp_path / 'ctx.txt'
    ctx.write_text('t5t6\nt7\n')  # chars 't','5',... are unknown symbols -> <unk> ids
    assert T.main([str(wav), '-m', str(tmp_path), '--beam', '4', '--context_path',
                   str(ctx), '--context_score', '2.0', '-t']) == 0
    out = capsys.readouterr().out
    assert 'tokens' in out and 'times' in out


# --------------------------------------------------------------------------
# beams above 16 (the general prefix-beam kernel, up to 64)


@pytest.mark.parametrize('V,T,B,beam,ctx', [(40, 30, 4, 17, False), (67, 50, 3, 20, True),
                                            (300, 40, 2, 32, False), (80, 25, 3, 64, True),
                                            (5002, 20, 2, 50, False), (20, 60, 6, 20, True)])
def test_prefix_beam_large_beams_bit_exact(V, T, B, beam, ctx):
    """beam_size 17..64 runs the general kernel: n-best lists, order and time
    stamps identical to the oracle, fp64 scores to 1e-9, with and without a
    context graph."""
    from wenet_amd import search as S
    from wenet_amd import synthetic
    from wenet_amd.context_graph import ContextGraph
    O = _oracle()
    logp, lens = synthetic.peaky_logprobs(B, (max(1, T // 2), T), V, 3.0, V + T + beam)
    og = gg = None
    if ctx:
        rng = np.random.RandomState(beam)
        phrases = [[int(t) for t in rng.randint(1, V, rng.randint(1, 5))] for _ in range(12)]
        og = O.ContextGraph(phrases, 2.0)
        gg = ContextGraph(context_list=phrases, context_score=2.0)
    ref = O.ctc_prefix_beam_search(logp, lens, beam, 0, og)
    got = S.ctc_prefix_beam_search(logp.cuda(), lens, beam, gg, 0)
    for b in range(B):
        _same_nbest(got[b], ref[b].nbest, ref[b].nbest_scores, ref[b].nbest_times,
                    f'utt {b}')


def test_large_beam_through_decode_and_rescoring():
    """beam 24 end to end (prefix beam + attention rescoring of 24 hypotheses)
    against the oracle on a small model."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 0)
    feats, lens = S.make_features(3, (60, 150), seed=77)
    kw = dict(beam_size=24, ctc_weight=0.5, reverse_weight=0.3, blank_penalty=3.0)
    got = model.decode(['ctc_prefix_beam_search', 'attention_rescoring'], feats.cuda(),
                       lens, **kw)
    enc, mask = model._forward_encoder(feats.cuda(), lens)
    enc_lens = mask.squeeze(1).sum(1).cpu()
    logp = model.ctc_logprobs(enc, 3.0, 0, encoder_lens=enc_lens).cpu()
    ref = O.ctc_prefix_beam_search(logp, enc_lens, 24, 0)
    for b in range(3):
        _same_nbest(got['ctc_prefix_beam_search'][b], ref[b].nbest, ref[b].nbest_scores,
                    ref[b].nbest_times)
    oref = O.attention_rescoring(configs, sd, ref, enc.cpu(), enc_lens, 0.5, 0.3,
                                 *O.special_symbols(configs))
    for b in range(3):
        r = got['attention_rescoring'][b]
        if list(r.tokens) == list(oref[b].tokens):
            assert abs(r.score - oref[b].score) < 1e-3 * (len(r.tokens) + 1)
    assert sum(list(got['attention_rescoring'][b].tokens) == list(oref[b].tokens)
               for b in range(3)) >= 2


@pytest.mark.parametrize('config,rw', [('tiny_causal', 0.0), ('tiny_causal', 0.4),
                                       ('tiny_sym', 0.3), ('tiny_bn', 0.0)])
def test_forward_attention_decoder_vs_oracle(config, rw):
    """ASRModel.forward_attention_decoder (asr_model.py:453-547): padded (N, L, V)
    log-softmax outputs of the left and right decoders, every position."""
    O = _oracle()
    configs, sd, model = cached_model(config, 0)
    sos, eos = O.special_symbols(configs)
    g = torch.Generator().manual_seed(21)
    V = configs['output_dim']
    lens = torch.tensor([9, 4, 1, 6, 9])
    hyps = torch.full((5, 9), eos, dtype=torch.long)
    for i, n in enumerate(lens.tolist()):
        hyps[i, 0] = sos
        hyps[i, 1:n] = torch.randint(1, V - 1, (n - 1, ), generator=g)
    enc = torch.randn(1, 31, configs['encoder_conf']['output_size'], generator=g)
    got_l, got_r = model.forward_attention_decoder(hyps, lens, enc.cuda(), rw)
    ref_l, ref_r = O.forward_attention_decoder(configs, sd, hyps, lens, enc, rw, sos, eos)
    assert tuple(got_l.shape) == tuple(ref_l.shape)
    assert (got_l.cpu() - ref_l).abs().max() < 2e-3
    assert tuple(got_r.shape) == tuple(ref_r.shape)
    assert (got_r.cpu() - ref_r).abs().max() < 2e-3
    if rw > 0 and configs['decoder'] == 'bitransformer':
        assert got_r.dim() == 3
    else:
        assert got_r.dim() == 0 and float(got_r) == 0.0


# --------------------------------------------------------------------------
# attention with the key range split over two wave groups (attn_split)


@pytest.mark.parametrize('config,B,frames,chunk,left', [
    ('tiny_causal', 7, (30, 700), -1, -1),
    ('tiny_causal', 5, (30, 600), 8, 1),
    ('tiny_causal', 4, (27, 400), 3, 0),
    ('tiny_sym', 6, (7, 500), -1, -1),
    ('tiny_bn', 3, (64, 333), -1, -1),
    ('aishell_u2pp', 3, (500, 1100), 16, -1),
])
def test_attention_key_split_vs_oracle(config, B, frames, chunk, left):
    """The key-split attention kernel forced on (attn_split = 2) for short and
    long, ragged sequences, full / chunk / limited-left-context masks, and off
    (attn_split = 1): both against the oracle's encoder output."""
    from wenet_amd import _lib, synthetic as S
    O = _oracle()
    configs, sd, model = cached_model(config, 0)
    feats, lens = S.make_features(B, frames, seed=123)
    with torch.no_grad():
        ref, mask = O.encoder_forward(configs, sd, feats, lens, chunk, left)
    ref_lens = mask.squeeze(1).sum(1).numpy()
    L = _lib.lib()
    outs = {}
    try:
        for mode in (2, 1):
            _lib.check(L.wn_tune_set(b'attn_split', mode), 'tune')
            enc, m = model._forward_encoder(feats.cuda(), lens, chunk, left)
            outs[mode] = enc.cpu()
            np.testing.assert_array_equal(m.squeeze(1).sum(1).cpu().numpy(), ref_lens)
            for b in range(B):
                nb = int(ref_lens[b])
                if nb:
                    err = (outs[mode][b, :nb] - ref[b, :nb]).abs().max().item()
                    assert err < 2e-3, (config, 'attn_split', mode, 'utt', b, err)
    finally:
        L.wn_tune_set(b'attn_split', 0)
    # the two kernels agree with each other far inside the oracle tolerance
    assert (outs[1] - outs[2]).abs().max() < 5e-4


@pytest.mark.parametrize('config,B,frames,chunk,left', [
    ('aishell_u2pp', 9, (300, 1200), -1, -1),     # the six-product kernel (full context)
    ('aishell_u2pp', 5, (500, 1100), 16, -1),     # the v_mfma_f32 kernel under chunk masks
    ('tiny_causal', 7, (30, 700), -1, -1),
    ('tiny_causal', 1, (260, 260), 8, 1),
])
def test_attention_xcd_block_order_is_bit_identical(config, B, frames, chunk, left):
    """Round 6: the fp32 attention kernels decode their (sequence, head, query block) from an
    XCD-aware 1-D block order (all query blocks of a (sequence, head) share one XCD's L2) --
    the same blocks doing the same arithmetic in another launch order: the encoder output is
    bit-identical to the plain 3-D grid's (tune attn_xcd = 0)."""
    from wenet_amd import _lib, synthetic as S
    configs, sd, model = cached_model(config, 0)
    feats, lens = S.make_features(B, frames, seed=77)
    L = _lib.lib()
    outs = {}
    try:
        for mode in (1, 0):
            _lib.check(L.wn_tune_set(b'attn_xcd', mode), 'tune')
            enc, _ = model._forward_encoder(feats.cuda(), lens, chunk, left)
            outs[mode] = enc.cpu()
    finally:
        L.wn_tune_set(b'attn_xcd', 1)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('config,B,frames', [
    ('aishell_u2pp', 9, (300, 1200)),
    ('aishell_u2pp', 32, (800, 1200)),
    ('aishell_u2pp', 24, (8, 900)),      # 1 .. 224 encoder frames: tiles that span 3+ sequences
    ('aishell_u2pp', 40, (8, 640)),
    ('tiny_causal', 7, (130, 700)),
])
def test_attention_x6_global_tile_alignment_vs_oracle(config, B, frames):
    """Round 6: the key-tile images of the six-product attention aligned to the GLOBAL 32-row
    blocks of the packed K / V matrix (tune attn_x6_galign = 1: the slots of a boundary tile
    that belong to the neighbouring sequence are masked) and, = 2, written by the QKV
    projection's epilogue instead of the pack pass.  Against the oracle within the encoder
    tolerance; 2 vs 1 BIT-identical (same planes, same scalars, same kernel); 1 vs 0 differs
    only by the grouping of the online softmax (far inside the tolerance)."""
    from wenet_amd import _lib, synthetic as S
    O = _oracle()
    configs, sd, model = cached_model(config, 0)
    feats, lens = S.make_features(B, frames, seed=31)
    with torch.no_grad():
        ref, mask = O.encoder_forward(configs, sd, feats, lens, -1, -1)
    ref_lens = mask.squeeze(1).sum(1).numpy()
    L = _lib.lib()
    outs = {}
    try:
        for mode in (0, 1, 2):
            _lib.check(L.wn_tune_set(b'attn_x6_galign', mode), 'tune')
            enc, _ = model._forward_encoder(feats.cuda(), lens, -1, -1)
            outs[mode] = enc.cpu()
            for b in range(B):
                nb = int(ref_lens[b])
                err = (outs[mode][b, :nb] - ref[b, :nb]).abs().max().item()
                assert err < 2e-3, (config, 'galign', mode, 'utt', b, err)
    finally:
        L.wn_tune_set(b'attn_x6_galign', _GALIGN_DEFAULT)
    assert (outs[1] - outs[0]).abs().max() < 5e-4
    assert torch.equal(outs[2], outs[1])
    # the block list (full blocks first, light ones last; dead query groups skip their work):
    # the same blocks in another dispatch order -- bit-identical to the plain grid
    try:
        _lib.check(L.wn_tune_set(b'attn_x6_order', 0), 'tune')
        enc, _ = model._forward_encoder(feats.cuda(), lens, -1, -1)
    finally:
        L.wn_tune_set(b'attn_x6_order', 1)
    assert torch.equal(enc.cpu(), outs[2])


def test_recognize_cli_shard_list_equals_raw_list(tmp_path):
    """--data_type shard (tar shards of <key>.wav / <key>.txt, one plain and one
    gzip-compressed) writes the same result files as --data_type raw on the same
    audio; a raw list with start / end decodes the segment; --dtype bf16 runs the
    same command on the bf16 matrix cores."""
    import io
    import json
    import tarfile
    import wave
    import yaml
    from wenet_amd.bin import recognize as R
    configs, sd, model = cached_model('tiny_causal', 0)
    V = configs['output_dim']
    units = tmp_path / 'units.txt'
    syms = ['<blank>', '<unk>'] + [f't{i}' for i in range(2, V - 1)] + ['<sos/eos>']
    units.write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    cfg = dict(configs)
    cfg['tokenizer'] = 'char'
    cfg['tokenizer_conf'] = dict(symbol_table_path=str(units), non_lang_syms_path=None,
                                 connect_symbol=' ')
    cfg['dataset_conf'] = dict(fbank_conf=dict(num_mel_bins=80, frame_length=25,
                                               frame_shift=10, dither=0.0))
    (tmp_path / 'train.yaml').write_text(yaml.safe_dump(cfg))
    torch.save(sd, tmp_path / 'final.pt')
    rng = np.random.RandomState(5)
    keys, blobs = [], {}
    for i in range(5):
        n = int(rng.randint(16000, 36000))
        t = np.arange(n) / 16000.0
        x = 0.3 * np.sin(2 * np.pi * (180 + 70 * i) * t) + 0.05 * rng.randn(n)
        path = tmp_path / f'u{i}.wav'
        with wave.open(str(path), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.clip(x * 32768, -32768, 32767).astype(np.int16).tobytes())
        keys.append(f'utt{i}')
        blobs[f'utt{i}'] = path.read_bytes()
    raw = tmp_path / 'raw.list'
    raw.write_text(''.join(json.dumps(dict(key=k, wav=str(tmp_path / f'u{i}.wav'), txt='')) +
                           '\n' for i, k in enumerate(keys)))
    for name, mode, ks in (('s0.tar', 'w', keys[:3]), ('s1.tar.gz', 'w:gz', keys[3:])):
        with tarfile.open(tmp_path / name, mode) as t:
            for k in ks:
                for ext, payload in (('wav', blobs[k]), ('txt', b'x')):
                    ti = tarfile.TarInfo(f'{k}.{ext}')
                    ti.size = len(payload)
                    t.addfile(ti, io.BytesIO(payload))
    shard = tmp_path / 'shard.list'
    shard.write_text(f"{tmp_path / 's0.tar'}\n{tmp_path / 's1.tar.gz'}\n")
    modes = ['ctc_greedy_search', 'attention_rescoring']

    def run(lst, out, *extra):
        rc = R.main(['--config', str(tmp_path / 'train.yaml'), '--checkpoint',
                     str(tmp_path / 'final.pt'), '--test_data', str(lst), '--result_dir',
                     str(out), '--batch_size', '2', '--beam_size', '3', '--ctc_weight',
                     '0.5', '--modes'] + modes + list(extra))
        assert rc == 0
        return {m: (out / m / 'text').read_text().splitlines() for m in modes}
    a = run(raw, tmp_path / 'o_raw')
    b = run(shard, tmp_path / 'o_shard', '--data_type', 'shard')
    assert a == b and len(a['ctc_greedy_search']) == 5
    # segment: the first second of utt0 == decoding a file that holds only that
    with wave.open(str(tmp_path / 'u0.wav'), 'rb') as w:
        head = w.readframes(16000)
    with wave.open(str(tmp_path / 'head.wav'), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(head)
    seg = tmp_path / 'seg.list'
    seg.write_text(json.dumps(dict(key='s', wav=str(tmp_path / 'u0.wav'), start=0.0, end=1.0))
                   + '\n')
    whole = tmp_path / 'head.list'
    whole.write_text(json.dumps(dict(key='s', wav=str(tmp_path / 'head.wav'))) + '\n')
    assert run(seg, tmp_path / 'o_seg') == run(whole, tmp_path / 'o_head')
    c = run(raw, tmp_path / 'o_bf16', '--dtype', 'bf16')
    assert [ln.split(' ')[0] for ln in c['ctc_greedy_search']] == \
        [ln.split(' ')[0] for ln in a['ctc_greedy_search']]


def test_busy_handle_is_refused_not_corrupted():
    """One host thread per wn_model handle: a second thread that enters a handle
    while a call is running gets a RuntimeError (status -4), and the first
    thread's results are unaffected.  (A feature-frontend call racing a decode on
    the same handle used to corrupt the descriptor staging buffer.)"""
    import threading
    import time
    from wenet_amd import synthetic as S
    configs, sd, model = cached_model('aishell_u2pp', 0)
    feats, lens = S.make_features(8, (300, 500), seed=77)
    fd = feats.cuda()
    want = model.decode(['ctc_prefix_beam_search'], fd, lens, beam_size=5)
    wave = (np.random.RandomState(1).rand(16000) * 0.2 - 0.1).astype(np.float32)
    stop, errors, n_ok = threading.Event(), [], [0]

    def intruder():
        torch.cuda.set_device(model.device)
        with torch.cuda.stream(torch.cuda.Stream()):
            while not stop.is_set():
                try:
                    model.compute_fbank([wave])
                    n_ok[0] += 1
                except RuntimeError as e:
                    errors.append(str(e))
                time.sleep(0.001)  # leave the handle free most of the time: every
                # decode() needs it free at each of its 3 entries to succeed
    t = threading.Thread(target=intruder)
    t.start()
    try:
        got, mine = [], []
        for _ in range(12):
            try:
                got.append(model.decode(['ctc_prefix_beam_search'], fd, lens, beam_size=5))
            except RuntimeError as e:   # the intruder held the handle at entry
                mine.append(str(e))
    finally:
        stop.set()
        t.join()
    for e in errors + mine:
        assert 'in use by another host thread' in e, e
    assert got, 'every decode lost the race'
    for g in got:
        for b in range(8):
            assert g['ctc_prefix_beam_search'][b].tokens == \
                want['ctc_prefix_beam_search'][b].tokens
            assert g['ctc_prefix_beam_search'][b].nbest_scores == \
                want['ctc_prefix_beam_search'][b].nbest_scores


def test_forward_encoder_chunk_batch_equals_single_sessions():
    """B streaming sessions per forward_chunk call.  Sessions at
    DIFFERENT positions with caches of DIFFERENT lengths (one of them on its first
    chunk) go through wn_encode_chunk_batch together; every session's output and new
    caches equal the single-session call (same kernels per row, so to fp32 GEMM-tile
    reordering) and the oracle's forward_chunk."""
    from wenet_amd import synthetic as S
    O = _oracle()
    configs, sd, model = cached_model('tiny_causal', 1)
    B, step_frames, required = 4, 19, 6
    feats = [S.make_features(1, (400, 400), seed=300 + b)[0] for b in range(B)]
    # bring the sessions to different states: session b has already consumed b chunks
    att = [None] * B
    cnn = [None] * B
    o_att = [None] * B
    o_cnn = [None] * B
    offset = [0] * B
    cur = [0] * B
    for b in range(B):
        for _ in range(b):
            win = feats[b][:, cur[b]:cur[b] + step_frames]
            y, att[b], cnn[b] = model.forward_encoder_chunk(win.cuda(), offset[b], required,
                                                            att[b], cnn[b])
            _, o_att[b], o_cnn[b] = O.forward_chunk(configs, sd, win, offset[b], required,
                                                    o_att[b], o_cnn[b])
            offset[b] += y.size(1)
            cur[b] += 4 * y.size(1)
    assert len({(a.size(2) if a is not None else 0) for a in att}) > 2   # ragged caches
    for _ in range(3):                               # three batched steps
        wins = torch.cat([feats[b][:, cur[b]:cur[b] + step_frames] for b in range(B)])
        ys, natt, ncnn = model.forward_encoder_chunk_batch(wins.cuda(), offset, required, att,
                                                           cnn)
        for b in range(B):
            y1, a1, c1 = model.forward_encoder_chunk(wins[b:b + 1].cuda(), offset[b], required,
                                                     att[b], cnn[b])
            assert (ys[b] - y1[0]).abs().max().item() < 1e-4
            assert tuple(natt[b].shape) == tuple(a1.shape)
            assert (natt[b] - a1).abs().max().item() < 1e-4
            assert (ncnn[b] - c1).abs().max().item() < 1e-4
            oy, o_att[b], o_cnn[b] = O.forward_chunk(configs, sd, wins[b:b + 1], offset[b],
                                                     required, o_att[b], o_cnn[b])
            assert (ys[b].cpu() - oy[0]).abs().max().item() < 2e-3
            assert (natt[b].cpu() - o_att[b]).abs().max().item() < 2e-3
            assert (ncnn[b].cpu() - o_cnn[b]).abs().max().item() < 2e-3
        att, cnn = natt, ncnn
        for b in range(B):
            offset[b] += ys.size(1)
            cur[b] += 4 * ys.size(1)


def test_forward_encoder_chunk_batch_aishell_16_sessions():
    """The AIShell 12-layer model, 16 sessions, chunk 16 (67-frame windows), caches
    limited to 32 frames: batched == single session per row."""
    from wenet_amd import synthetic as S
    configs, sd, model = cached_model('aishell_u2pp', 0)
    B, win_frames, required = 16, 67, 32
    feats, _ = S.make_features(B, (300, 300), seed=77)
    att = [None] * B
    cnn = [None] * B
    offset = [0] * B
    cur = 0
    for step in range(3):
        wins = feats[:, cur:cur + win_frames].cuda()
        ys, natt, ncnn = model.forward_encoder_chunk_batch(wins, offset, required, att, cnn)
        for b in (0, 7, 15):
            y1, a1, c1 = model.forward_encoder_chunk(wins[b:b + 1], offset[b], required, att[b],
                                                     cnn[b])
            assert (ys[b] - y1[0]).abs().max().item() < 2e-4, (step, b)
            assert (natt[b] - a1).abs().max().item() < 2e-4
            assert (ncnn[b] - c1).abs().max().item() < 2e-4
        att, cnn = natt, ncnn
        offset = [o + ys.size(1) for o in offset]
        cur += 4 * ys.size(1)


def test_filter_blank_embedding_of_an_all_blank_batch():
    """No frame of the batch has a non-blank arg-max: filter_blank_embedding returns an EMPTY
    selection (B, 0, d) with an all-False (B, 1, 0) mask instead of an opaque view error
    (round-4 advice; the reference itself fails in index_select here), and decode() with
    apply_non_blank_embedding says -- attribute + RuntimeWarning -- that it rescored against the
    unfiltered encoder output."""
    import warnings
    configs, sd, model = cached_model('tiny_lite', 0)
    B, T, V, d = 3, 17, model.vocab_size, configs['encoder_conf']['output_size']
    logp = torch.full((B, T, V), -20.0)
    logp[:, :, 0] = -1e-6
    enc = torch.randn(B, T, d, generator=torch.Generator().manual_seed(3))
    sel, mask = model.filter_blank_embedding(logp.cuda(), enc.cuda())
    assert tuple(sel.shape) == (B, 0, d) and tuple(mask.shape) == (B, 1, 0)
    assert mask.dtype == torch.bool
    # decode(): a CTC head that always answers blank
    sd2 = dict(sd)
    sd2['ctc.ctc_lo.weight'] = torch.zeros_like(sd['ctc.ctc_lo.weight'])
    b = torch.full_like(sd['ctc.ctc_lo.bias'], -30.0)
    b[0] = 0.0
    sd2['ctc.ctc_lo.bias'] = b
    from gpu_util import make_model
    from wenet_amd import synthetic as S
    m2 = make_model(configs, sd2)
    feats, lens = S.make_features(2, (60, 90), seed=7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        got = m2.decode(['attention_rescoring'], feats.cuda(), lens, beam_size=3)
    assert m2.last_non_blank_filter_empty is True
    assert any(issubclass(x.category, RuntimeWarning) and 'non-blank' in str(x.message) for x in w)
    assert all(len(r.tokens) == 0 for r in got['attention_rescoring'])
