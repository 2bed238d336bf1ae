"""The Whisper decoder on the accelerated path against the REAL reference's Whisper model
(tests/golden/whisperdec_tiny.npz, tools/gen_golden_whisper_decode.py: `whisper_tiny_dec`, a
weight seed whose reference decode is free of near-ties -- fp64 and fp32 give the same tokens):

  * forward_attention_decoder on a padded prompt + token batch, 2e-3 (the tolerance of
    test_gpu_parity.test_forward_attention_decoder_vs_oracle);
  * decode(['attention'], infos=...) token lists, beam 1 and 10, step GEMMs on linear()
    (dec_skinny 0) and on the skinny kernel (1), and again behind a ctc_greedy_search on the same
    handle (the batch state is shared);
  * the prompt prefill is shared through the ancestor paths: a batch decodes like its
    utterances one by one;
  * the positional cap: with a 24-row `pe` the search stops at position 24, says so
    (last_attention_truncated) and -- beam 1, where the winning path is well defined -- returns
    the first tokens of the uncapped run.
"""
import numpy as np
import pytest
import torch

from golden_util import load_case
from gpu_util import cached_model, make_model

pytestmark = pytest.mark.gpu

CASE = 'whisperdec_tiny'


@pytest.fixture(scope='module')
def setup():
    from wenet_amd import synthetic as S
    meta, arr = load_case(CASE)
    configs, sd, model = cached_model(meta['config'], meta['wseed'])
    feats, lens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'],
                                  feat_dim=configs['input_dim'])
    return meta, arr, configs, sd, model, feats, lens


def _decode(model, feats, lens, beam, infos, skinny):
    model.tune('dec_skinny', skinny)
    try:
        res = model.decode(['attention'], feats, lens, beam_size=beam, infos=infos)
    finally:
        model.tune('dec_skinny', 'inherit')
    return [list(r.tokens) for r in res['attention']]


def test_golden_is_a_real_decode(setup):
    """What the generator's seed filter promised: long, varied, prompt-dependent hypotheses, one
    that ends on <eot> early and one past 32 steps (the cache grows)."""
    meta = setup[0]
    toks = meta['tokens']
    assert all(len(set(u)) >= 8 for k, v in toks.items() if k.endswith('/10') for u in v)
    assert toks['default/10'] != toks['mixed/10']
    lens = [len(u) + 4 for k, v in toks.items() if k.endswith('/10') for u in v]
    assert min(lens) < meta['cap'] and max(lens) > 36
    assert meta['cap'] < 448


def test_forward_attention_decoder_vs_reference(setup):
    meta, arr, configs, sd, model = setup[:5]
    hyps = torch.from_numpy(arr['fwd_hyps'].astype(np.int64))
    lens = torch.tensor(meta['fwd_lens'])
    enc = torch.from_numpy(arr['fwd_enc']).cuda()
    got, got_r = model.forward_attention_decoder(hyps, lens, enc, 0.0)
    ref = torch.from_numpy(arr['fwd_logp'])
    assert tuple(got.shape) == tuple(ref.shape) == (4, 9, configs['output_dim'])
    err = (got.cpu() - ref).abs().max().item()
    print(f'whisper forward_attention_decoder: max |logp - reference| = {err:.3e}')
    assert err < 2e-3
    assert got_r.dim() == 0 and float(got_r) == 0.0


@pytest.mark.parametrize('skinny', [0, 1])
@pytest.mark.parametrize('beam', [1, 10])
def test_attention_decode_tokens_equal_reference(setup, beam, skinny):
    meta, arr, configs, sd, model, feats, lens = setup
    assert model.default_decode_method == 'attention'
    for name, infos in meta['infos'].items():
        want = meta['tokens'][f'{name}/{beam}']
        got = _decode(model, feats, lens, beam, infos, skinny)
        assert got == want, (name, beam, skinny)
        assert model.last_attention_truncated is False
    # the batch state of the handle is shared with the CTC searches: decode through one, then
    # the same attention decode again
    model.decode(['ctc_greedy_search'], feats, lens)
    name = 'mixed'
    assert _decode(model, feats, lens, beam, meta['infos'][name], skinny) == \
        meta['tokens'][f'{name}/{beam}']


def test_two_runs_give_the_same_tokens_and_skinny_equals_linear(setup):
    meta, arr, configs, sd, model, feats, lens = setup
    a = _decode(model, feats, lens, 10, meta['infos']['vad'], 1)
    b = _decode(model, feats, lens, 10, meta['infos']['vad'], 1)
    c = _decode(model, feats, lens, 10, meta['infos']['vad'], 0)
    assert a == b == c == meta['tokens']['vad/10']


@pytest.mark.parametrize('skinny', [0, 1])
def test_batch_decodes_like_single_utterances(setup, skinny):
    """All beams of an utterance share ONE set of prompt cache rows (the utterance's first
    slot); with equally long utterances (the same cap T' in the batch and alone) the batch must
    decode exactly like its utterances one by one."""
    meta, arr, configs, sd, model, feats, lens = setup
    n = int(lens.min())
    f = feats[:, :n].contiguous()
    ln = torch.full_like(lens, n)
    infos = meta['infos']['mixed']
    whole = _decode(model, f, ln, 10, infos, skinny)
    assert all(len(u) > 0 for u in whole)
    for b in range(f.shape[0]):
        one = _decode(model, f[b:b + 1], ln[b:b + 1], 10,
                      dict(tasks=[infos['tasks'][b]], langs=[infos['langs'][b]]), skinny)
        assert one == [whole[b]], (b, skinny)


@pytest.mark.parametrize('beam', [1, 10])
def test_positional_cap_stops_and_reports(setup, beam):
    """T' = 61 > dec_max_pos = 24: hypotheses of 24 tokens get their 25th, then the search
    stops (the reference asserts in its positional table there): at most 25 - 4 = 21 result
    tokens, the flag set.  Beam 1 has one path: its tokens are the uncapped run's first 21
    (positions < 24 read the same 24 table rows)."""
    meta, arr, configs, sd, model, feats, lens = setup
    cap = 24
    assert meta['cap'] > cap
    sd2 = dict(sd)
    sd2['decoder.embed.1.pe'] = sd['decoder.embed.1.pe'][:, :cap].contiguous()
    small = make_model(configs, sd2)
    assert small._cfg.dec_max_pos == cap
    for skinny in (0, 1):
        got = _decode(small, feats, lens, beam, None, skinny)
        full = meta['tokens'][f'default/{beam}']
        n_max = cap + 1 - 4
        assert all(len(u) <= n_max for u in got)
        # an utterance whose uncapped hypothesis is longer was still open at the cap
        assert any(len(u) > n_max for u in full)
        assert small.last_attention_truncated is True
        if beam == 1:
            assert got == [u[:n_max] for u in full]
        else:
            assert any(len(u) == n_max for u in got)
    # the flag belongs to the model that decoded
    assert model.last_attention_truncated is False
