"""CPU checks of the hybrid transducer's host side: which `model: transducer` recipes
transducer_config_from_yaml accepts and refuses (config_from_yaml keeps refusing all of them),
wn_transducer_config beside an unchanged wn_config, the new C-ABI symbols, the synthetic
configurations."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from golden_util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNNT = ('aishell/rnnt/conf/conformer_rnnt.yaml', 'aishell/rnnt/conf/conformer_u2pp_rnnt.yaml')
EMBEDDING = 'aishell/rnnt/conf/example_embedding_predictor.yaml'
NEW_FIELDS = ['pred_embed', 'pred_hidden', 'pred_layers', 'pred_out', 'join_dim', 'blank']


@pytest.fixture(scope='module')
def recipes():
    r = load_case('live_recipes')[0]
    out = {}
    for name in RNNT + (EMBEDDING, ):
        c = copy.deepcopy(r[name])
        c.setdefault('input_dim', 80)
        c.setdefault('output_dim', 4233)
        out[name] = c
    return out


@pytest.mark.parametrize('name', RNNT)
def test_rnnt_recipes_are_accepted(recipes, name):
    from wenet_amd.transducer import transducer_config_from_yaml
    c, tc = transducer_config_from_yaml(recipes[name])
    assert tc.blank == 0
    assert (tc.pred_embed, tc.pred_hidden, tc.pred_layers, tc.pred_out, tc.join_dim) == \
        (256, 256, 2, 256, 512)
    assert (c.d_model, c.n_layers, c.vocab, c.dec_layers) == (256, 12, 4233, 3)
    if 'u2pp' in name:
        assert c.causal == 1 and c.cnn_kernel == 8 and c.bidirectional == 1


def test_other_predictors_and_joints_are_refused(recipes):
    from wenet_amd.transducer import transducer_config_from_yaml
    with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
        transducer_config_from_yaml(recipes[EMBEDDING])
    assert 'predictor' in str(e.value)
    base = recipes[RNNT[1]]
    for section, key, value in (('predictor_conf', 'rnn_type', 'gru'),
                                ('predictor_conf', 'bias', False),
                                ('joint_conf', 'hat_joint', True),
                                ('joint_conf', 'postjoin_linear', True),
                                ('joint_conf', 'prejoin_linear', False),
                                ('joint_conf', 'activation', 'relu'),
                                ('joint_conf', 'join_dim', 500)):
        c = copy.deepcopy(base)
        c[section][key] = value
        with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
            transducer_config_from_yaml(c)
        assert f'{section}.{key}' in str(e.value)
    c = copy.deepcopy(base)
    c['predictor'] = 'conv'
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        transducer_config_from_yaml(c)
    # an encoder config_from_yaml refuses stays refused, naming its key
    c = copy.deepcopy(base)
    c['encoder_conf']['pos_enc_layer_type'] = 'abs_pos'
    with pytest.raises(NotImplementedError, match='pos_enc_layer_type'):
        transducer_config_from_yaml(c)
    # and an asr_model is not a transducer
    c = copy.deepcopy(base)
    c['model'] = 'asr_model'
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        transducer_config_from_yaml(c)


def test_config_from_yaml_still_refuses_transducers(recipes):
    from wenet_amd.model import config_from_yaml
    for name, c in recipes.items():
        with pytest.raises(NotImplementedError, match='outside the accelerated path'):
            config_from_yaml(c)


def _struct_fields(src, name):
    body = re.search(r'typedef struct \{([^{}]*?)\} %s;' % name, src, re.S).group(1)
    out = []
    for typ, decl in re.findall(r'\b(int32_t|float)\s+([^;]+);', body):
        out += [(typ, n.strip()) for n in decl.split(',')]
    return out


def test_transducer_config_matches_the_header_and_wn_config_is_unchanged():
    """The predictor / joint widths travel in a struct of their own (wn_transducer_config, taken
    by wn_model_create_transducer): wn_config still ends with dec_max_pos, so every existing
    caller of wn_model_create passes what it passed before."""
    from wenet_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for struct, name in ((_lib.WnConfig, 'wn_config'),
                         (_lib.WnTransducerConfig, 'wn_transducer_config')):
        declared = _struct_fields(src, name)
        assert [n for _, n in declared] == [n for n, _ in struct._fields_], name
        assert ctypes.sizeof(struct) == 4 * len(declared)
        for (typ, n), (_, ctype) in zip(declared, struct._fields_):
            assert ctype is (ctypes.c_float if typ == 'float' else ctypes.c_int32), n
    assert _lib.WnConfig._fields_[-1][0] == 'dec_max_pos'
    assert [n for n, _ in _lib.WnTransducerConfig._fields_] == NEW_FIELDS


def test_library_exports_the_transducer_symbols():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    for name in ('wn_model_create_transducer', 'wn_transducer_greedy_search', 'wn_op_lstm_step',
                 'wn_op_joint_argmax'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    # argument validation that needs no device
    assert L.wn_transducer_greedy_search(None, 64, None, None, 0, None, None) == -1
    assert b'null' in L.wn_last_error()
    assert L.wn_model_create_transducer(None, None, None, 0, 0, None) == -1
    assert b'null' in L.wn_last_error()
    assert L.wn_tune_set(b'rnnt_lookahead', 0) == -1
    assert b'rnnt_lookahead' in L.wn_last_error()
    assert L.wn_tune_set(b'rnnt_lookahead', 17) == -1
    v = ctypes.c_int32(0)
    assert L.wn_tune_set(b'rnnt_lookahead', 16) == 0
    assert L.wn_tune_get(None, b'rnnt_lookahead', ctypes.byref(v)) == 0 and v.value == 16
    assert L.wn_tune_set(b'rnnt_lookahead', 4) == 0


def test_transducer_refuses_cpu_device():
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    with pytest.raises(RuntimeError, match='needs a GPU device'):
        Transducer(S.make_configs('tiny_rnnt'), {}, device='cpu')


def test_synthetic_configs():
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import transducer_config_from_yaml
    tiny = S.make_configs('tiny_rnnt')
    c, tc = transducer_config_from_yaml(tiny)
    assert (tc.pred_embed, tc.pred_hidden, tc.pred_out, tc.pred_layers, tc.join_dim) == \
        (64, 80, 96, 2, 160)
    assert (c.d_model, c.vocab) == (128, 67)
    full, ftc = transducer_config_from_yaml(S.make_configs('aishell_u2pp_rnnt'))
    assert (full.d_model, ftc.join_dim, full.vocab) == (256, 512, 4233)
    # the new tensors leave every tensor of the base configuration as it was
    sd = S.make_state_dict(tiny, 3)
    base = S.make_state_dict(S.make_configs('tiny_causal'), 3)
    assert list(sd)[:len(base)] == list(base)
    assert all(np.array_equal(sd[k].numpy(), base[k].numpy()) for k in base)
    extra = [k for k in sd if k not in base]
    assert extra and all(k.startswith(('predictor.', 'joint.')) for k in extra)
    assert sd['predictor.rnn.weight_ih_l1'].shape == (320, 80)
    # the blank bias knob moves the blank logit's bias only
    heavy = S.make_state_dict(tiny, 3, rnnt_blank_bias=9.0)
    diff = (heavy['joint.ffn_out.bias'] - sd['joint.ffn_out.bias']).numpy()
    assert diff[0] == pytest.approx(3.0) and not diff[1:].any()
    assert all(np.array_equal(heavy[k].numpy(), sd[k].numpy()) for k in sd
               if k != 'joint.ffn_out.bias')


def test_load_model_routes_transducer_directories(tmp_path):
    """load_model builds a Transducer for `model: transducer` (it reaches the device check,
    not config_from_yaml's refusal)."""
    from wenet_amd import synthetic as S
    from wenet_amd.model import load_model
    d = S.write_model_dir(str(tmp_path / 'rnnt'), 'tiny_rnnt')
    with pytest.raises(RuntimeError, match='needs a GPU device'):
        load_model(d, device='cpu')
