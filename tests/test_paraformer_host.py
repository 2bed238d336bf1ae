"""CPU checks of the Paraformer port: the plain restatements of tests/paraformer_refs.py against
what the real reference's modules computed (tests/golden/paraformer/, recorded by
tools/gen_golden_paraformer.py), the fp32 fire chain bit for bit, the config parser on the shipped
recipes, the tokenizer rule, the margins of the tiny-model fixture, the C ABI declarations.
"""
import copy
import os

import numpy as np
import pytest
import torch

import paraformer_refs as PR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'paraformer')
TAIL = 0.45


@pytest.fixture(scope='module')
def modules():
    return PR.load_golden(GOLDEN, 'modules')


@pytest.fixture(scope='module')
def tiny():
    return PR.load_golden(GOLDEN, 'tiny')


def test_lfr_formula_is_the_reference_padding():
    """Row t = frames 6 t - 3 .. 6 t + 3 clamped to [0, n - 1] is what the reference's head / tail
    copies + unfold give on a batch of one, for every n in 1..59."""
    for n in range(1, 60):
        assert np.array_equal(PR.lfr_indices(n), PR.lfr_indices_by_padding(n)), n
        assert PR.lfr_indices(n).shape == (PR.lfr_rows(n), 7)


def test_lfr_equals_recorded(modules):
    _, arr = modules
    for n in PR.GOLDEN_LFR_N:
        x = PR.features(n, PR.MODULE_SEED)
        got = x[torch.from_numpy(PR.lfr_indices(n))].reshape(PR.lfr_rows(n), 560)
        assert np.array_equal(got.numpy(), arr[f'lfr_{n}']), n       # a gather: equal bits


def test_cif_equals_recorded(modules):
    _, arr = modules
    ci = PR.cif_module_inputs()
    h, d = ci['h'], ci['h'].shape[1]
    alphas = PR.ref_cif_alpha(h, ci['conv_w'], ci['conv_b'], ci['out_w'], ci['out_b'], 1.0, 0.0)
    rec = arr['cif_alphas']                          # T + 1 entries: the tail frame behind
    # (the tail is an fp32 0.45 even in a .double() module: tail_process_fn builds it in fp32)
    assert rec.shape[0] == h.shape[0] + 1 and rec[-1] == float(np.float32(TAIL))
    assert np.abs(alphas.numpy() - rec[:-1]).max() < 1e-12
    emb, fires, n_tok = PR.ref_cif_embeds(h, rec[:-1], float(np.float32(TAIL)))
    assert fires == [int(t) for t in np.nonzero(arr['cif_fires'] >= 1.0)[0]]
    assert n_tok == int(arr['cif_token_num'][0]) == len(fires)
    # cif() keeps `integrate` and `frame` in fp32 tensors whatever the module's dtype (cif.py:
    # 254-255, updated in place): the recorded embeddings carry fp32 roundings of up to 41 terms
    assert np.abs(emb.numpy() - arr['cif_emb'][:n_tok]).max() < 64 * 2.0 ** -24 * \
        np.abs(arr['cif_emb']).max()
    # the tap-major weight of the conv GEMM is the same conv
    w3 = PR.conv_w_tap_major(ci['conv_w'])
    z = torch.zeros(1, d, dtype=torch.float64)
    img = torch.cat([torch.cat([z, h[:-1]]), h, torch.cat([h[1:], z])], dim=1)
    mem = torch.relu(img @ w3.t() + ci['conv_b'])
    o = mem @ ci['out_w'].reshape(-1) + float(ci['out_b'][0])
    assert (torch.sigmoid(o) - alphas).abs().max() < 1e-12


def test_sanm_attention_equals_recorded(modules):
    """linear_out(softmax(q k^T / sqrt(128)) v) + fsmn(v) == MultiHeadedAttentionSANM.double() at
    2 heads x 128, 40 frames: every frame away from the ends sees all 11 taps."""
    _, arr = modules
    x, sd = PR.sanm_attention_inputs()
    # (the reference's softmax runs in fp32 whatever the module's dtype: restated for the pin)
    got = PR.ref_sanm_attention(x, {'A.' + k: v for k, v in sd.items()}, 'A', PR.SANM_H,
                                softmax32=True)
    plain = PR.ref_sanm_attention(x, {'A.' + k: v for k, v in sd.items()}, 'A', PR.SANM_H)
    rec = torch.from_numpy(arr['sanm_attention'])
    assert rec.shape == (PR.SANM_T, PR.SANM_D)
    assert (got - rec).abs().max() < 1e-9 * max(1.0, rec.abs().max().item())
    # and the all-fp64 formula the GPU tests use as their oracle is the fp32 softmax away: 2^-24
    # per weight
    assert (plain - rec).abs().max() < 1e-6 * max(1.0, rec.abs().max().item())


def test_sanm_decoder_layer_equals_recorded(modules):
    _, arr = modules
    tgt, mem, sd = PR.sanm_decoder_layer_inputs()
    got = PR.ref_sanm_decoder_layer(tgt, mem, {'L.' + k: v for k, v in sd.items()}, 'L',
                                    PR.SANM_H, softmax32=True)
    rec = torch.from_numpy(arr['sanm_decoder_layer'])
    assert rec.shape == (PR.DECL_TOKENS, PR.SANM_D)
    assert (got - rec).abs().max() < 1e-9 * max(1.0, rec.abs().max().item())


@pytest.mark.parametrize('name', list(PR.CIF_ALPHA_ROWS))
def test_fp32_fire_chain_bit_for_bit(modules, name):
    """The fp32 chain restated == the reference's cif() in fp32: the integrate values before the
    subtraction (its `fires` tensor) and the fired embeddings, equal bits."""
    _, arr = modules
    row = PR.CIF_ALPHA_ROWS[name]
    a = np.asarray(row, dtype=np.float32)
    fires, cur, rem, _ = PR.cif_chain(a, np.float32(TAIL), np.float32)
    rec = arr[f'chain_{name}_fires']
    assert rec.dtype == np.float32
    assert fires == [int(t) for t in np.nonzero(rec >= 1.0)[0]]
    # the recorded integrate values, step by step
    integ, vals = np.float32(0.0), []
    for x in np.concatenate([a, np.asarray([TAIL], dtype=np.float32)]):
        integ = np.float32(integ + x)
        vals.append(integ)
        if integ >= np.float32(1.0):
            integ = np.float32(integ - np.float32(1.0))
    assert np.array_equal(np.asarray(vals, dtype=np.float32), rec)
    h = torch.from_numpy(arr[f'chain_{name}_h'])
    emb, f2, _ = PR.ref_cif_embeds(h[:-1], a, np.float32(TAIL), fp32=True)
    assert f2 == fires
    assert np.array_equal(emb.float().numpy(), arr[f'chain_{name}_emb'][:len(fires)])


def test_tokenizer_rule_equals_recorded(modules):
    from wenet_amd.tokenizer import Tokenizer, paraformer_tokens2text
    meta, _ = modules
    assert len(meta['beautify']) == len(PR.BEAUTIFY_CASES) >= 12
    for toks, want in zip(PR.BEAUTIFY_CASES, meta['beautify']):
        assert paraformer_tokens2text(list(toks)) == want, toks
    tok = Tokenizer({'<blank>': 0, '你': 1, 'hel@@': 2, 'lo': 3}, 'paraformer')
    assert tok.detokenize([1, 2, 3]) == ('你hello', ['你', 'hel@@', 'lo'])


def _shipped_yamls():
    """The three recipes the reference ships (examples/aishell/paraformer/conf/, examples/
    wenetspeech/paraformer/conf/), kept as settings files under tests/golden/paraformer/recipes/."""
    import yaml
    out = []
    for name in ('aishell_train_paraformer.yaml', 'aishell_train_paraformer_dynamic.yaml',
                 'wenetspeech_fintune_paraformer_dynamic.yaml'):
        with open(os.path.join(GOLDEN, 'recipes', name)) as f:
            c = yaml.safe_load(f)
        c.setdefault('output_dim', 8404)
        out.append((name, c))
    assert len(out) == 3
    return out


def test_config_parser_accepts_the_recipes():
    from wenet_amd import synthetic as S
    from wenet_amd.paraformer import paraformer_config_from_yaml
    cases = [('paraformer_large', S.make_configs('paraformer_large')),
             ('tiny_paraformer', S.make_configs('tiny_paraformer'))] + _shipped_yamls()
    for name, c in cases:
        cfg, p = paraformer_config_from_yaml(c)
        assert cfg.feat_dim == 80 and cfg.d_model // cfg.n_heads == 128, name
        assert (p.lfr_m, p.lfr_n, p.kernel_size) == (7, 6, 11), name
        assert p.threshold == 1.0 and abs(p.tail_threshold - 0.45) < 1e-7, name
    cfg, p = paraformer_config_from_yaml(S.make_configs('paraformer_large'))
    assert (cfg.d_model, cfg.n_heads, cfg.n_layers, p.dec_blocks, cfg.vocab) == \
        (512, 4, 50, 16, 8404)
    c = S.make_configs('tiny_paraformer')
    c['encoder_conf']['attention_heads'] = 4        # d_k = 64: the existing attention kernel
    c['decoder_conf']['attention_heads'] = 4
    assert paraformer_config_from_yaml(c)[0].n_heads == 4


@pytest.mark.parametrize('section,key,value', [
    ('encoder_conf', 'sanm_shfit', 1), ('decoder_conf', 'sanm_shfit', 1),
    ('predictor_conf', 'cnn_groups', 0), ('predictor_conf', 'residual', True),
    ('predictor_conf', 'threshold', 0.9), ('predictor_conf', 'l_order', 2),
    ('predictor_conf', 'smooth_factor', 0.5), ('predictor_conf', 'noise_threshold', 0.1),
    ('encoder_conf', 'attention_heads', 8), ('encoder_conf', 'kernel_size', 12),
    ('encoder_conf', 'input_layer', 'conv2d'), ('encoder_conf', 'normalize_before', False),
    ('decoder_conf', 'att_layer_num', 1), ('decoder_conf', 'kernel_size', 15)])
def test_config_parser_refuses_by_key_name(section, key, value):
    from wenet_amd import synthetic as S
    from wenet_amd.paraformer import paraformer_config_from_yaml
    c = copy.deepcopy(S.make_configs('tiny_paraformer'))
    c[section][key] = value
    with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
        paraformer_config_from_yaml(c)
    assert key in str(e.value) or (key == 'attention_heads' and 'attention_heads' in str(e.value))


def test_asr_model_parser_still_refuses_paraformer():
    from wenet_amd import synthetic as S
    from wenet_amd.model import config_from_yaml
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        config_from_yaml(S.make_configs('tiny_paraformer'))


def test_fixture_margins_hold(tiny):
    """The conditions a weight seed was accepted under, recomputed from what is recorded."""
    meta, arr = tiny
    assert meta['lens'] == PR.TINY_LENS and meta['enc_lens'] == [70, 33, 32, 4, 2, 1]
    assert meta['raised'] == [False] * 5 + [True] and meta['token_num'][-1] == 0
    m = meta['margins']
    assert m['fire'] >= 1e-3 and m['sum'] >= 1e-2 and m['gap'] >= 1e-3
    for i, n in enumerate(PR.TINY_LENS):
        assert len(meta['fire_frames'][i]) == meta['token_num'][i]
        g = meta['tokens']['paraformer_greedy_search'][i]
        assert g == meta['tokens']['paraformer_beam_search'][i]
        assert len(g) == meta['token_num'][i]
        if meta['enc_lens'][i] >= 32:
            assert len(set(g)) >= 3
        assert all(0 <= t <= meta['enc_lens'][i] for t in meta['fire_frames'][i])
        if not meta['raised'][i]:
            assert arr[f'logp64_{n}'].shape == (meta['token_num'][i], )
    for n in PR.TINY_ENC_SAVED:
        assert arr[f'enc64_{n}'].shape == (PR.lfr_rows(n), 256)
    assert max(meta['e_enc']) < 1e-4 and max(meta['e_logp']) < 1e-4


def test_model_restatement_equals_recorded(tiny):
    """tests/paraformer_refs.ref_paraformer in fp64 == the .double() reference model: encoder
    output, token numbers, fire frames, tokens and their log-probs, on the 196-, the 24- and the
    1-frame utterance (T' = 33, 4, 1)."""
    from wenet_amd import synthetic as S
    meta, arr = tiny
    configs = S.make_configs('tiny_paraformer')
    sd = S.make_state_dict(configs, meta['wseed'])
    feats = PR.tiny_features()
    for i in (1, 3, 5):
        r = PR.ref_paraformer(sd, configs, feats[i])
        n = PR.TINY_LENS[i]
        assert r['token_num'] == meta['token_num'][i] and r['fires'] == meta['fire_frames'][i]
        # (the reference's position table is an fp32 buffer, 6e-8 per entry; the restatement's
        # and the library's are fp64 sinusoids -- and cif() accumulates in fp32, see above)
        if f'enc64_{n}' in arr:
            assert (r['enc'] - torch.from_numpy(arr[f'enc64_{n}'])).abs().max() < 1e-6
        if meta['raised'][i]:
            assert r['logp'] is None
            continue
        top = r['logp'].max(dim=-1)
        assert top.indices.tolist() == meta['tokens']['paraformer_greedy_search'][i]
        assert (top.values - torch.from_numpy(arr[f'logp64_{n}'])).abs().max() < 1e-5


def test_synthetic_state_dict_shapes():
    from wenet_amd import synthetic as S
    c = S.make_configs('tiny_paraformer')
    sd = S.make_state_dict(c, 0)
    assert sd['encoder.encoders0.0.self_attn.linear_q_k_v.weight'].shape == (768, 560)
    assert sd['encoder.encoders.1.self_attn.fsmn_block.weight'].shape == (256, 1, 11)
    assert sd['predictor.predictor.cif_conv1d.weight'].shape == (256, 256, 3)
    assert 'decoder.decoders.1.feed_forward.w_2.bias' not in sd
    assert sd['decoder.decoders3.0.feed_forward.norm.weight'].shape == (256, )
    assert 'encoder.encoders.2.norm1.weight' not in sd        # 1 + 2 blocks


def test_cabi_declares_the_paraformer_entry_points():
    from wenet_amd import _lib
    for name in ('wn_model_create_paraformer', 'wn_paraformer_decode', 'wn_op_attention_d128',
                 'wn_op_lfr_front', 'wn_op_layernorm_wide', 'wn_op_cif_alpha', 'wn_op_cif_fire'):
        assert name in _lib.EXPORTS, name
    with open(os.path.join(HERE, '..', 'include', 'wenet_amd.h')) as f:
        text = f.read()
    assert 'wn_paraformer_config' in text
    fields = [n for n, _ in _lib.WnParaformerConfig._fields_]
    assert fields == ['lfr_m', 'lfr_n', 'kernel_size', 'dec_blocks', 'max_frames', 'threshold',
                      'tail_threshold', 'smooth_factor', 'noise_threshold']
