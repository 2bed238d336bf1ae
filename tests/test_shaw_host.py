"""W2v-BERT 2.0 / conformer_shaw models without a GPU: what `shaw_config_from_yaml` accepts and
refuses, and that the coded table of the operator test exposes a wrong row."""
import copy
import os

import pytest
import yaml

import kernel_refs as KR
import shaw_refs as SR
from wenet_amd.model import config_from_yaml
from wenet_amd.shaw import shaw_config_from_yaml

RECIPE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shaw', 'recipes',
                      'w2vbert_conformer_600m.yaml')


def _recipe():
    with open(RECIPE) as f:
        return yaml.safe_load(f)


def test_converter_yaml_is_accepted():
    c, h = shaw_config_from_yaml(_recipe())
    assert (c.feat_dim, c.d_model, c.n_heads, c.ffn_dim, c.n_layers) == (80, 1024, 16, 4096, 24)
    assert (c.cnn_kernel, c.causal, c.cnn_norm, c.has_cmvn, c.vocab) == (31, 1, 0, 0, 1024)
    assert (c.use_dynamic_chunk, c.static_chunk_size, c.encoder_type, c.input_layer) == (0, 0, 0, 0)
    # `attention_head` is not the decoder's key: 4 heads of 256, no decoder on this path
    assert (c.dec_heads, c.dec_layers, c.dec_r_layers, c.bidirectional) == (4, 0, 0, 0)
    assert (h.max_left, h.max_right, h.stack) == (64, 8, 2)
    assert config_from_yaml(_recipe()).d_model == 1024        # the public entry dispatches


def test_decoder_heads_of_64_keep_the_decoder():
    r = _recipe()
    r['decoder_conf']['attention_heads'] = 16
    assert shaw_config_from_yaml(r)[0].dec_layers == 6


DEVIATIONS = [('encoder_conf.input_layer', 'conv2d'), ('encoder_conf.pos_enc_layer_type', 'rel_pos'),
              ('encoder_conf.selfattention_layer_type', 'rel_selfattn'),
              ('encoder_conf.cnn_module_norm', 'batch_norm'), ('encoder_conf.conv_bias', True),
              ('encoder_conf.activation_type', 'relu'), ('encoder_conf.macaron_style', False),
              ('encoder_conf.use_cnn_module', False), ('encoder_conf.normalize_before', False),
              ('encoder_conf.use_dynamic_chunk', True), ('encoder_conf.static_chunk_size', 16),
              ('encoder_conf.final_norm', False), ('encoder_conf.key_bias', False),
              ('encoder_conf.conv_inner_factor', 4), ('encoder_conf.layer_norm_type', 'rms_norm'),
              ('encoder_conf.mlp_type', 'gated'), ('encoder_conf.n_kv_head', 2),
              ('encoder_conf.attention_heads', 8), ('encoder_conf.cnn_module_kernel', 65),
              ('decoder_conf.activation_type', 'gelu'), ('decoder_conf.tie_word_embedding', True),
              ('encoder', 'transformer'), ('model', 'transducer'), ('input_dim', 160)]


@pytest.mark.parametrize('key,value', DEVIATIONS, ids=[k for k, _ in DEVIATIONS])
def test_deviation_is_refused_by_key(key, value):
    r = copy.deepcopy(_recipe())
    conf, _, leaf = key.rpartition('.')
    (r[conf] if conf else r)[leaf] = value
    with pytest.raises(NotImplementedError, match=leaf):
        shaw_config_from_yaml(r)


@pytest.mark.parametrize('key,value', [('causal', False), ('cnn_module_kernel', 15),
                                       ('gradient_checkpointing', False), ('use_sdpa', True)])
def test_free_keys(key, value):
    r = _recipe()
    r['encoder_conf'][key] = value
    shaw_config_from_yaml(r)


@pytest.mark.parametrize('wrong', sorted(SR.WRONG_INDEX))
def test_coded_regime_exposes_wrong_rows(wrong):
    """fp64: each wrong reading of the table is far outside the operator test's bound on the
    coded regime (tests/test_gpu_shaw_ops.py)."""
    c = SR.make_case(2, 'coded', None)
    ref, e_plain, scale = SR.case_refs(c)
    bad, _, _ = SR.case_refs(c, index=SR.WRONG_INDEX[wrong])
    err = (bad - ref).abs().max().item()
    print(f'{wrong}: err={err:.3e} bound={KR.bound(e_plain, scale):.3e}')
    assert KR.cap_ok(e_plain, scale)
    assert err > 100 * KR.bound(e_plain, scale)


def test_formulation_equals_the_reference_encoder():
    """shaw_refs.ref_encoder, the fp64 yardstick of the test at the converter's widths, on the
    recorded `tiny_shaw` utterances against the real reference's .double() encoder output -- whose
    softmax runs in fp32 (softmax_fp32); the plain fp64 formulation is within that rounding."""
    import json
    import numpy as np
    from wenet_amd import synthetic as S
    with np.load(os.path.join(os.path.dirname(RECIPE), '..', 'tiny_shaw.npz')) as z:
        meta = json.loads(bytes(z['meta']).decode())
        enc = {k: z[k] for k in z.files if k != 'meta'}
    configs = S.make_configs('tiny_shaw')
    sd = S.make_state_dict(configs, meta['wseed'])
    import torch
    for i, f in enumerate(SR.tiny_features()):
        if f.shape[0] >= 2:
            ref = torch.from_numpy(enc[f'enc64_{i}'])
            same = SR.ref_encoder(f, sd, configs, softmax_fp32=True)
            assert (same - ref).abs().max().item() < 1e-11
            assert (SR.ref_encoder(f, sd, configs) - ref).abs().max().item() < 1e-6
