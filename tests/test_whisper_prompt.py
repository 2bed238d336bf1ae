"""CPU checks of the Whisper decoder path: the recipe's decoder configuration maps to a
wn_config WITH its decoder, the prompt builder equals what the reference's add_whisper_tokens
returned (tests/golden/whisperdec_tiny.npz, tools/gen_golden_whisper_decode.py), and the C ABI
declares and exports the two new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from golden_util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = 'aishell/whisper/conf/finetune_whisper_largev3.yaml'


def test_largev3_recipe_keeps_its_decoder():
    """examples/aishell/whisper/conf/finetune_whisper_largev3.yaml:20-37 (recorded, parsed, in
    tests/golden/live_recipes.npz): 32 decoder blocks and the Whisper variants, not the
    encoder-only configuration."""
    from wenet_amd.model import config_from_yaml
    conf = load_case('live_recipes')[0][RECIPE]
    conf.setdefault('input_dim', 128)
    conf.setdefault('output_dim', 51866)
    dc = conf['decoder_conf']
    assert (dc['activation_type'], dc['input_layer'], dc['key_bias'], dc['src_key_bias'],
            dc['tie_word_embedding']) == ('gelu', 'embed_learnable_pe', False, False, True)
    c = config_from_yaml(conf)
    assert c.dec_layers == 32 and c.dec_r_layers == 0 and c.bidirectional == 0
    assert (c.dec_heads, c.dec_ffn_dim) == (20, 5120)
    assert (c.dec_activation, c.dec_key_bias, c.dec_src_key_bias, c.dec_learned_pos,
            c.dec_max_pos) == (1, 1, 1, 1, 448)
    st = conf['tokenizer_conf']['special_tokens']
    assert (c.sos, c.eos) == (st['sot'], st['eot'])


def test_classic_decoders_keep_zero_variant_fields():
    from wenet_amd import synthetic as S
    from wenet_amd.model import config_from_yaml
    for name in ('tiny_sym', 'tiny_bn', 'aishell_u2pp', 'whisper_tiny_like'):
        c = config_from_yaml(S.make_configs(name))
        assert (c.dec_activation, c.dec_key_bias, c.dec_src_key_bias, c.dec_learned_pos,
                c.dec_max_pos) == (0, 0, 0, 0, 0), name
    assert config_from_yaml(S.make_configs('whisper_tiny_like')).dec_layers == 0
    c = config_from_yaml(S.make_configs('whisper_tiny_dec'))
    assert c.dec_layers == 2 and c.dec_learned_pos == 1 and c.dec_activation == 1


def test_other_decoder_variants_stay_off_the_path():
    """Only the recipe's five values are accepted; any other non-default decoder key leaves a
    Transformer-encoder model encoder-only and refuses a Conformer one, as before."""
    from wenet_amd import synthetic as S
    from wenet_amd.model import config_from_yaml
    conf = S.make_configs('whisper_tiny_dec')
    conf['decoder_conf']['value_bias'] = False
    assert config_from_yaml(conf).dec_layers == 0
    conf = S.make_configs('whisper_tiny_dec')
    conf['decoder_conf']['activation_type'] = 'swish'
    assert config_from_yaml(conf).dec_layers == 0
    conf = S.make_configs('tiny_sym')
    conf['decoder_conf']['query_bias'] = False
    with pytest.raises(NotImplementedError):
        config_from_yaml(conf)
    conf = S.make_configs('aishell_u2pp')       # bitransformer: no Whisper variants
    conf['decoder_conf']['key_bias'] = False
    with pytest.raises(NotImplementedError):
        config_from_yaml(conf)


def test_prompts_equal_add_whisper_tokens():
    from wenet_amd import whisper
    meta, arr = load_case('whisperdec_tiny')
    st = meta['special_tokens']
    B = meta['batch']
    assert whisper.is_whisper(st) and not whisper.is_whisper({'<sos>': 2}) \
        and not whisper.is_whisper(None)
    for name, infos in meta['infos'].items():
        got = whisper.build_prompts(st, B, infos)
        assert got.dtype == np.int32 and got.shape == (B, 4)
        assert got.tolist() == arr['prompt_' + name].tolist(), name
    # defaults: transcribe / en
    assert whisper.build_prompts(st, 2, None).tolist() == [
        [st['sot'], st['sot'] + 1, st['transcribe'], st['no_timestamps']]] * 2
    assert whisper.prompt_row(st, 'vad', 'zh') == [st['sot'], st['sot'] + 2, st['no_speech'],
                                                   st['no_speech']]


def test_language_index_and_errors():
    from wenet_amd import whisper
    st = load_case('whisperdec_tiny')[0]['special_tokens']
    assert len(whisper.WHISPER_LANGS) == 100 == len(set(whisper.WHISPER_LANGS))
    assert whisper.WHISPER_LANGS[:2] == ('en', 'zh')      # the two the reference harness pins
    for code, idx in (('en', 0), ('zh', 1)):
        assert whisper.prompt_row(st, 'translate', idx) == whisper.prompt_row(st, 'translate',
                                                                              code)
    infos = dict(tasks=['transcribe', 'translate'], langs=[1, np.int64(0)])
    assert whisper.build_prompts(st, 2, infos).tolist() == whisper.build_prompts(
        st, 2, dict(tasks=['transcribe', 'translate'], langs=['zh', 'en'])).tolist()
    with pytest.raises(ValueError):
        whisper.build_prompts(st, 1, dict(tasks=['transcribe'], langs=['xx']))
    with pytest.raises(ValueError):
        whisper.build_prompts(st, 1, dict(tasks=['transcribe'], langs=[100]))
    with pytest.raises(ValueError):
        whisper.build_prompts(st, 2, dict(tasks=['transcribe'], langs=['en']))
    with pytest.raises(NotImplementedError):
        whisper.build_prompts(st, 1, dict(tasks=['summarize'], langs=['en']))


def test_header_and_library_have_the_new_entry_points():
    from wenet_amd import _lib, build
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('wn_attention_beam_search_prompt', 'wn_op_gemm_skinny'):
        assert re.search(r'\b%s\s*\(' % name, src), name
    fields = re.search(r'typedef struct \{(.*?)\} wn_config;', src, re.S).group(1)
    names = re.findall(r'\b(\w+)\s*[;,]', fields)
    assert names[-5:] == ['dec_activation', 'dec_key_bias', 'dec_src_key_bias',
                          'dec_learned_pos', 'dec_max_pos']
    assert [n for n, _ in _lib.WnConfig._fields_][-5:] == names[-5:]
    assert ctypes.sizeof(_lib.WnConfig) == 4 * len(names)
    build.build(force=False, verbose=False)
    L = _lib.lib()
    for name in ('wn_attention_beam_search_prompt', 'wn_op_gemm_skinny',
                 'wn_attention_truncated'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    # argument checks that need no device
    assert L.wn_attention_truncated(None) == -1
    assert L.wn_op_gemm_skinny(None, None, None, None, None, 1, 1, 32, 0, 0, 0, None) == -1
