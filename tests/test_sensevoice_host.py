"""SenseVoice Small without a GPU: the configuration parser, the lid / itn mapping, the C ABI's
declarations, and the fp64 formulation of tests/sensevoice_refs.py against what the REAL reference
recorded (tools/gen_golden_sensevoice.py, tests/golden/sensevoice/)."""
import copy
import os

import numpy as np
import pytest
import torch

import sensevoice_refs as SR

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module', params=SR.TINY_CONFIGS)
def tiny(request):
    meta, arr = SR.load_tiny(request.param)
    assert meta is not None, 'tests/golden/sensevoice is missing'
    return request.param, meta, arr


def test_config_parser_accepts_the_converter_recipe_and_the_synthetic_configs():
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import sensevoice_config_from_yaml
    cfg, p = sensevoice_config_from_yaml(S.make_configs('sensevoice_small'))
    assert (cfg.feat_dim, cfg.d_model, cfg.n_heads, cfg.ffn_dim, cfg.n_layers, cfg.vocab) == \
        (80, 512, 4, 2048, 50, 25055)
    assert (p.lfr_m, p.lfr_n, p.kernel_size, p.tp_blocks, p.n_query, p.n_embed) == \
        (7, 6, 11, 20, 4, 16)
    assert (cfg.sos, cfg.eos, cfg.has_cmvn, cfg.dec_layers) == (1, 2, 1, 0)
    for name, want in (('tiny_sensevoice', (256, 2, 256, 2, 2, 11, 50)),
                       ('tiny_sensevoice_h64', (128, 2, 64, 2, 1, 3, 50)),
                       ('sensevoice_small_1blk', (512, 4, 2048, 2, 1, 11, 50))):
        cfg, p = sensevoice_config_from_yaml(S.make_configs(name))
        assert (cfg.d_model, cfg.n_heads, cfg.ffn_dim, cfg.n_layers, p.tp_blocks, p.kernel_size,
                cfg.vocab) == want, name
    # what the converter writes and make_configs does not add: nothing else is needed
    c = copy.deepcopy(S.CONFIGS['sensevoice_small'])
    c['cmvn'] = 'global_cmvn'
    c['cmvn_conf'] = {'is_json_cmvn': True, 'cmvn_file': 'global_cmvn'}
    assert c['decoder'] is None and 'decoder_conf' not in c
    assert sensevoice_config_from_yaml(c)[1].tp_blocks == 20


@pytest.mark.parametrize('path,value,key', [
    (('encoder', ), 'sanm_encoder', 'encoder'),
    (('decoder', ), 'transformer', 'decoder'),
    (('cmvn', ), None, 'cmvn'),
    (('input_dim', ), 80, 'input_dim'),
    (('encoder_conf', 'input_layer'), 'conv2d', 'input_layer'),
    (('encoder_conf', 'pos_enc_layer_type'), 'abs_pos', 'pos_enc_layer_type'),
    (('encoder_conf', 'sanm_shfit'), 1, 'sanm_shfit'),
    (('encoder_conf', 'normalize_before'), False, 'normalize_before'),
    (('encoder_conf', 'static_chunk_size'), 16, 'static_chunk_size'),
    (('encoder_conf', 'use_dynamic_chunk'), True, 'use_dynamic_chunk'),
    (('encoder_conf', 'attention_heads'), 8, 'attention_heads'),
    (('encoder_conf', 'kernel_size'), 12, 'kernel_size'),
    (('encoder_conf', 'linear_units'), 100, 'linear_units'),
    (('lfr_conf', 'lfr_n'), 4, 'lfr_conf'),
    (('model_conf', 'ctc_weight'), 0.0, 'ctc_weight'),
    (('tokenizer_conf', 'special_tokens'), {'<sos>': 1, '<eos>': 2}, 'special_tokens'),
    (('ctc_conf', 'ctc_blank_id'), 3, 'ctc_blank_id')])
def test_config_parser_refuses_by_key_name(path, value, key):
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import sensevoice_config_from_yaml
    c = S.make_configs('tiny_sensevoice')
    node = c
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
        sensevoice_config_from_yaml(c)
    assert key in str(e.value)


def test_config_parser_needs_tp_blocks_and_the_model_name():
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import sensevoice_config_from_yaml
    c = S.make_configs('tiny_sensevoice')
    del c['encoder_conf']['tp_blocks']
    with pytest.raises(NotImplementedError, match='tp_blocks'):
        sensevoice_config_from_yaml(c)
    with pytest.raises(NotImplementedError, match='model'):
        sensevoice_config_from_yaml(S.make_configs('tiny_paraformer'))


def test_asr_model_parser_still_refuses_sensevoice():
    from wenet_amd import synthetic as S
    from wenet_amd.model import config_from_yaml
    with pytest.raises((NotImplementedError, KeyError, TypeError)):
        config_from_yaml(S.make_configs('tiny_sensevoice'))


def test_lid_itn_mapping():
    from wenet_amd import sensevoice as SV
    want = dict(auto=0, zh=3, en=4, yue=7, ja=11, ko=12, nospeech=13)
    for k, v in want.items():
        assert SV.lid_row(k) == v and SR.LID[k] == v
    assert SV.lid_row('tlh') == 0 and SV.lid_row(None) == 0
    assert SV.itn_row('withitn') == 14 and SV.itn_row('woitn') == 15 and SV.itn_row('x') == 15
    for infos in (None, {}):
        assert SV.query_ids(infos, 2).tolist() == [[0, 1, 2, 15]] * 2
    assert SV.query_ids({'lid': 'en', 'itn': 'withitn'}, 2).tolist() == [[4, 1, 2, 14]] * 2
    assert SV.query_ids({'lid': ['ko', 'tlh', 'yue']}, 3).tolist() == \
        [[12, 1, 2, 15], [0, 1, 2, 15], [7, 1, 2, 15]]
    with pytest.raises(ValueError, match='lid'):
        SV.query_ids({'lid': ['ko']}, 2)
    for name in SR.SETTINGS:
        assert SV.query_ids(SR.SETTINGS[name], 1)[0].tolist() == SR.setting_qid(name)
    assert [SV.out_len(n) for n in SR.TINY_LENS] == [5, 5, 6, 32, 33, 64, 76]
    assert SV.out_len(0) == 0


def test_synthetic_state_dict_shapes():
    from wenet_amd import synthetic as S
    sd = S.make_state_dict(S.make_configs('tiny_sensevoice'), 0)
    assert sd['embed.weight'].shape == (16, 560)
    assert sd['global_cmvn.mean'].shape == (560, ) and 'encoder.global_cmvn.mean' not in sd
    assert sd['encoder.encoders0.0.self_attn.linear_q_k_v.weight'].shape == (768, 560)
    assert sd['encoder.encoders.0.norm1.weight'].shape == (256, )
    assert 'encoder.encoders.1.norm1.weight' not in sd          # 1 + 1 blocks
    assert sd['encoder.tp_encoders.1.self_attn.fsmn_block.weight'].shape == (256, 1, 11)
    assert 'encoder.tp_encoders.2.norm1.weight' not in sd
    assert sd['encoder.tp_norm.bias'].shape == (256, ) and sd['ctc.ctc_lo.weight'].shape == (50, 256)
    assert not any(k.startswith('decoder.') for k in sd)


def test_cabi_declares_the_sensevoice_entry_points():
    from wenet_amd import _lib
    names = ('wn_model_create_sensevoice', 'wn_sensevoice_set_queries', 'wn_op_sv_front')
    for name in names:
        assert name in _lib.EXPORTS, name
    with open(os.path.join(HERE, '..', 'include', 'wenet_amd.h')) as f:
        text = f.read()
    assert 'wn_sensevoice_config' in text and all(n + '(' in text for n in names)
    fields = [n for n, _ in _lib.WnSenseVoiceConfig._fields_]
    assert fields == ['lfr_m', 'lfr_n', 'kernel_size', 'tp_blocks', 'max_frames', 'n_query',
                      'n_embed']


def test_built_library_exports_the_sensevoice_symbols():
    """The symbols resolve in the built library (loading it needs no GPU)."""
    import ctypes
    from wenet_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('wn_model_create_sensevoice', 'wn_sensevoice_set_queries', 'wn_op_sv_front'):
        assert getattr(L, name) is not None, name


def test_fixture_conditions_hold(tiny):
    """The conditions a weight seed was accepted under, recomputed from what is recorded."""
    config, meta, arr = tiny
    assert meta['config'] == config and meta['lens'] == SR.TINY_LENS
    assert meta['enc_lens'] == [5, 5, 6, 32, 33, 64, 76] and meta['ctc_beam'] == SR.CTC_BEAM
    assert meta['zero_raised'] is True      # the reference raises inside LFR without frames
    assert set(meta['settings']) == set(SR.SETTINGS)
    for name, s in meta['settings'].items():
        assert s['infos'] == SR.SETTINGS[name]
        for i in range(len(SR.TINY_LENS)):
            nb = s['nbest_scores'][i]
            assert s['scores'][i] == nb[0]
            if len(nb) > 1:
                assert nb[0] - nb[1] > 64 * s['e_score'][i]
            for m in SR.METHODS:
                assert len(s['tokens'][m][i]) <= meta['enc_lens'][i]
        assert max(s['e_enc']) < 1e-4 and max(s['e_logp']) < 1e-3 and max(s['e_score']) < 1e-3
    d = meta['settings']['default']['tokens']['ctc_greedy_search']
    e = meta['settings']['en_withitn']['tokens']['ctc_greedy_search']
    assert d != e, 'the query rows change nothing: the second setting shows nothing'
    width = 256 if config == 'tiny_sensevoice' else 128
    for n in SR.TINY_ENC_SAVED:
        assert arr[f'enc64_default_{n}'].shape == (SR.enc_rows(n), width)


def test_unknown_setting_equals_default(tiny):
    """An unknown lid / itn falls back to auto / woitn inside the reference: the third setting's
    recordings are the default's, bit for bit."""
    _, meta, arr = tiny
    a, b = meta['settings']['unknown'], meta['settings']['default']
    for k in ('tokens', 'scores', 'nbest_scores', 'e_enc', 'e_logp', 'e_score'):
        assert a[k] == b[k], k
    n = SR.TINY_ENC_SAVED[0]
    assert np.array_equal(arr[f'enc64_unknown_{n}'], arr[f'enc64_default_{n}'])


def test_formulation_equals_recorded(tiny):
    """sensevoice_refs.ref_sensevoice in fp64 == the .double() reference model at fp64 round-off
    scale, for every recorded encoder output: with the reference's own position rows (an fp32
    buffer in its state dict) and its attention softmax in fp32 (paraformer_refs._mha).  This
    also pins where the positions start: row t of the concatenated sequence takes pe[t + 1]."""
    from wenet_amd import synthetic as S
    config, meta, arr = tiny
    configs = S.make_configs(config)
    sd = S.make_state_dict(configs, meta['wseed'])
    feats = SR.tiny_features()
    seen = 0
    for name in SR.SETTINGS:
        for i, n in enumerate(SR.TINY_LENS):
            key = f'enc64_{name}_{n}'
            if key not in arr:
                continue
            seen += 1
            rec = torch.from_numpy(arr[key])
            r = SR.ref_sensevoice(sd, configs, feats[i], SR.setting_qid(name), softmax32=True,
                                  pe=sd['encoder.embed.pos_enc.pe'])
            assert r['enc'].shape == rec.shape
            assert (r['enc'] - rec).abs().max() < 1e-12, key
            # the plain fp64 formulation (fp64 sinusoids, fp64 softmax) stays within the fp32
            # reference's own error of it
            p = SR.ref_sensevoice(sd, configs, feats[i], SR.setting_qid(name))
            assert (p['enc'] - rec).abs().max() < 1e-6, key
            # greedy tokens of the formulation: collapse repeats, drop blanks
            am = r['logp'].argmax(-1).tolist()
            toks = [t for j, t in enumerate(am) if t != 0 and (j == 0 or t != am[j - 1])]
            assert toks == meta['settings'][name]['tokens']['ctc_greedy_search'][i], key
    assert seen == 5


def test_front_formulation_is_the_models_first_rows():
    """ref_sv_front (the operator's yardstick) is the front end ref_sensevoice runs: the same
    rows go into layer 0."""
    from wenet_amd import synthetic as S
    import paraformer_refs as PR
    configs = S.make_configs('tiny_sensevoice')
    sd = S.make_state_dict(configs, 0)
    f = PR.features(13, 3)
    pe = PR.whisper_sinusoids(16, SR.D0)
    a = SR.ref_sv_front(f, [4, 1, 2, 14], sd['embed.weight'], sd['global_cmvn.mean'],
                        sd['global_cmvn.istd'], pe, sd['encoder.encoders0.0.norm1.weight'],
                        sd['encoder.encoders0.0.norm1.bias'], 16.0, 1e-5)
    assert a.shape == (SR.enc_rows(13), SR.D0) == (7, 560)
    # rows 0..3 do not depend on the frames, rows 4.. do not depend on the ids
    g = SR.ref_sv_front(f + 1.0, [4, 1, 2, 14], sd['embed.weight'], sd['global_cmvn.mean'],
                        sd['global_cmvn.istd'], pe, sd['encoder.encoders0.0.norm1.weight'],
                        sd['encoder.encoders0.0.norm1.bias'], 16.0, 1e-5)
    h = SR.ref_sv_front(f, [0, 1, 2, 15], sd['embed.weight'], sd['global_cmvn.mean'],
                        sd['global_cmvn.istd'], pe, sd['encoder.encoders0.0.norm1.weight'],
                        sd['encoder.encoders0.0.norm1.bias'], 16.0, 1e-5)
    assert torch.equal(a[:4], g[:4]) and not torch.equal(a[4:], g[4:])
    assert torch.equal(a[4:], h[4:]) and torch.equal(a[1:3], h[1:3])
    assert not torch.equal(a[0], h[0]) and not torch.equal(a[3], h[3])
