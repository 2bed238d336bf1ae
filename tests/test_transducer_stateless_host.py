"""CPU checks of the stateless predictors' host side: which `predictor: embedding` / `predictor:
conv` recipes stateless_transducer_config_from_yaml accepts and refuses (transducer_config_from_yaml
keeps refusing both kinds), wn_stateless_predictor_config against the header, the new C-ABI
symbols, the synthetic configurations."""
import copy
import ctypes
import os
import re

import pytest

from golden_util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMBEDDING = 'aishell/rnnt/conf/example_embedding_predictor.yaml'
FIELDS = ['kind', 'context', 'heads', 'activation', 'conv_bias', 'norm_eps']


@pytest.fixture(scope='module')
def recipe():
    c = copy.deepcopy(load_case('live_recipes')[0][EMBEDDING])
    c.setdefault('input_dim', 80)
    c.setdefault('output_dim', 4233)
    return c


def _conv(recipe):
    c = copy.deepcopy(recipe)
    c['predictor'] = 'conv'
    c['predictor_conf'] = dict(embed_size=320, output_size=320, embed_dropout=0.1, history_size=2,
                               activation='relu', bias=True)
    return c


def test_the_embedding_recipe_is_accepted(recipe):
    from wenet_amd.transducer import stateless_transducer_config_from_yaml
    c, tc, sc = stateless_transducer_config_from_yaml(recipe)
    assert (sc.kind, sc.heads, sc.context, sc.activation, sc.conv_bias) == (1, 4, 6, 0, 0)
    assert sc.norm_eps == pytest.approx(1e-5)
    assert (tc.pred_embed, tc.pred_out, tc.pred_hidden, tc.pred_layers) == (320, 320, 0, 0)
    assert tc.join_dim == 320 and tc.blank == 0
    assert (c.d_model, c.n_layers, c.vocab) == (256, 12, 4233)


def test_a_conv_recipe_is_accepted(recipe):
    from wenet_amd.transducer import stateless_transducer_config_from_yaml
    c, tc, sc = stateless_transducer_config_from_yaml(_conv(recipe))
    assert (sc.kind, sc.heads, sc.context, sc.activation, sc.conv_bias) == (2, 1, 3, 1, 1)
    assert (tc.pred_embed, tc.pred_out, tc.pred_hidden, tc.pred_layers) == (320, 320, 0, 0)
    # the predictors' own defaults (predictor.py:224-227, :386-389)
    conv = _conv(recipe)
    for k in ('history_size', 'activation', 'bias'):
        del conv['predictor_conf'][k]
    _, _, sc = stateless_transducer_config_from_yaml(conv)
    assert (sc.context, sc.activation, sc.conv_bias) == (3, 1, 0)
    emb = copy.deepcopy(recipe)
    del emb['predictor_conf']['history_size']
    emb['predictor_conf']['activation'] = 'relu'
    emb['predictor_conf']['layer_norm_epsilon'] = 1e-3
    _, _, sc = stateless_transducer_config_from_yaml(emb)
    assert (sc.context, sc.activation) == (3, 1) and sc.norm_eps == pytest.approx(1e-3)


def test_refusals_name_their_key(recipe):
    from wenet_amd.transducer import stateless_transducer_config_from_yaml
    cases = [('predictor_conf', 'output_size', 256, 'predictor_conf.output_size'),
             ('joint_conf', 'pred_output_size', 256, 'joint_conf.pred_output_size'),
             ('predictor_conf', 'activation', 'gelu', 'predictor_conf.activation'),
             ('predictor_conf', 'history_size', 16, 'predictor_conf.history_size'),
             ('predictor_conf', 'n_head', 17, 'predictor_conf.n_head'),
             ('joint_conf', 'hat_joint', True, 'joint_conf.hat_joint'),
             ('joint_conf', 'postjoin_linear', True, 'joint_conf.postjoin_linear'),
             ('joint_conf', 'prejoin_linear', False, 'joint_conf.prejoin_linear'),
             ('joint_conf', 'activation', 'relu', 'joint_conf.activation'),
             ('joint_conf', 'joint_mode', 'concat', 'joint_conf.joint_mode'),
             ('joint_conf', 'join_dim', 500, 'joint_conf.join_dim')]
    for base in (recipe, _conv(recipe)):
        for section, key, value, named in cases:
            if key == 'n_head' and base['predictor'] == 'conv':
                continue
            c = copy.deepcopy(base)
            c[section][key] = value
            with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
                stateless_transducer_config_from_yaml(c)
            assert named in str(e.value), (named, str(e.value))
        # widths above 1024 (embed_size == output_size == pred_output_size, so only the width)
        c = copy.deepcopy(base)
        c['predictor_conf']['embed_size'] = c['predictor_conf']['output_size'] = 1088
        c['joint_conf']['pred_output_size'] = 1088
        with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
            stateless_transducer_config_from_yaml(c)
        assert 'predictor_conf.embed_size' in str(e.value)
    # the largest window and head count that have kernels
    c = copy.deepcopy(recipe)
    c['predictor_conf'].update(history_size=15, n_head=16)
    assert stateless_transducer_config_from_yaml(c)[2].context == 16
    # an LSTM recipe, another joint class, an encoder config_from_yaml refuses, an asr_model
    for key, value, named in (('predictor', 'rnn', 'predictor'), ('joint', 'other_joint', 'joint'),
                              ('model', 'asr_model', 'model')):
        c = copy.deepcopy(recipe)
        c[key] = value
        with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
            stateless_transducer_config_from_yaml(c)
        assert named in str(e.value)
    c = copy.deepcopy(recipe)
    c['encoder_conf']['pos_enc_layer_type'] = 'abs_pos'
    with pytest.raises(NotImplementedError, match='pos_enc_layer_type'):
        stateless_transducer_config_from_yaml(c)


def test_transducer_config_from_yaml_still_refuses_both_kinds(recipe):
    from wenet_amd.model import config_from_yaml
    from wenet_amd.transducer import transducer_config_from_yaml
    for c in (recipe, _conv(recipe)):
        with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
            transducer_config_from_yaml(c)
        assert 'predictor' in str(e.value)
        with pytest.raises(NotImplementedError, match='outside the accelerated path'):
            config_from_yaml(c)


def _struct_fields(src, name):
    body = re.search(r'typedef struct \{([^{}]*?)\} %s;' % name, src, re.S).group(1)
    out = []
    for typ, decl in re.findall(r'\b(int32_t|float)\s+([^;]+);', body):
        out += [(typ, n.strip()) for n in decl.split(',')]
    return out


def test_the_struct_matches_the_header():
    from wenet_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = _struct_fields(src, 'wn_stateless_predictor_config')
    struct = _lib.WnStatelessPredictorConfig
    assert [n for _, n in declared] == [n for n, _ in struct._fields_] == FIELDS
    assert ctypes.sizeof(struct) == 4 * len(declared)
    for (typ, n), (_, ctype) in zip(declared, struct._fields_):
        assert ctype is (ctypes.c_float if typ == 'float' else ctypes.c_int32), n
    # the older structs did not grow
    assert [n for _, n in _struct_fields(src, 'wn_transducer_config')] == \
        [n for n, _ in _lib.WnTransducerConfig._fields_]
    assert len(_lib.WnTransducerConfig._fields_) == 6


def test_library_exports_the_stateless_symbols():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    for name in ('wn_model_create_transducer_stateless', 'wn_op_stateless_step'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    # argument validation that needs no device
    assert L.wn_model_create_transducer_stateless(None, None, None, None, 0, 0, None) == -1
    assert b'null' in L.wn_last_error()
    tc = _lib.WnTransducerConfig()
    assert L.wn_model_create_transducer_stateless(None, ctypes.byref(tc), None, None, 0, 0,
                                                  None) == -1
    assert b'null' in L.wn_last_error()
    assert L.wn_op_stateless_step(None, None, None, None, None, 1, 1, 1, 1, None) == -1
    assert b'null' in L.wn_last_error()


def test_the_operator_hook_validates_on_the_host():
    """Ids outside [-1, V) and widths outside their ranges are refused before anything is
    launched (no device is touched: the checks come first)."""
    import numpy as np
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    sc = _lib.WnStatelessPredictorConfig()
    sc.kind, sc.context, sc.heads, sc.activation, sc.norm_eps = 1, 3, 2, 0, 1e-5
    one = ctypes.c_float(0.0)
    ptrs = (ctypes.c_void_p * 8)(*[ctypes.addressof(one)] * 8)
    out = ctypes.c_void_p(ctypes.addressof(one))

    def run(ctx, V=10, E=8, J=8, cfg=sc):
        ctx = np.ascontiguousarray(ctx, dtype=np.int32)
        return L.wn_op_stateless_step(ctypes.byref(cfg), _lib.i32p(ctx), ptrs, None, out,
                                      ctx.shape[0], V, E, J, None)

    for bad in ([[0, 1, 10]], [[0, -2, 1]]):
        assert run(bad) == -1
        assert b'context id outside' in L.wn_last_error()
    assert run([[0, 1, 2]], E=1025) == -1 and b'widths' in L.wn_last_error()
    assert run([[0, 1, 2]], J=0) == -1 and b'widths' in L.wn_last_error()
    for field, value, text in (('context', 17, b'context and heads'), ('heads', 17, b'context and heads'),
                               ('kind', 3, b'kind'), ('activation', 2, b'activation')):
        bad = _lib.WnStatelessPredictorConfig.from_buffer_copy(sc)
        setattr(bad, field, value)
        assert run(np.zeros((1, bad.context if field != 'context' else 3)), cfg=bad) == -1
        assert text in L.wn_last_error(), field


def test_synthetic_configurations():
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import stateless_transducer_config_from_yaml
    want = {'tiny_rnnt_embed': (1, 80, 4, 4, 0, 160), 'tiny_rnnt_conv': (2, 96, 3, 1, 1, 160),
            'aishell_u2pp_rnnt_embed': (1, 320, 6, 4, 0, 320)}
    for name, (kind, E, C, heads, act, J) in want.items():
        configs = S.make_configs(name)
        _, tc, sc = stateless_transducer_config_from_yaml(configs)
        assert (sc.kind, tc.pred_embed, sc.context, sc.heads, sc.activation, tc.join_dim) == \
            (kind, E, C, heads, act, J), name
    for name in ('tiny_rnnt_embed', 'tiny_rnnt_conv'):
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, 3)
        E, C = configs['predictor_conf']['embed_size'], configs['predictor_conf']['history_size'] + 1
        assert tuple(sd['predictor.embed.weight'].shape) == (configs['output_dim'], E)
        assert tuple(sd['predictor.norm.weight'].shape) == (E, )
        assert tuple(sd['joint.pred_ffn.weight'].shape) == (160, E)
        assert not any(k.startswith('predictor.rnn') or k.startswith('predictor.projection')
                       for k in sd)
        if name == 'tiny_rnnt_embed':
            assert tuple(sd['predictor.pos_embed.weight'].shape) == (4, E * C)
            assert tuple(sd['predictor.ffn.weight'].shape) == (E, E)
            assert 'predictor.pos_embed.bias' not in sd
        else:
            assert tuple(sd['predictor.conv.weight'].shape) == (E, 1, C)
            assert tuple(sd['predictor.conv.bias'].shape) == (E, )
    # the LSTM configuration's state dict is what it was: the same names in the same order
    configs = S.make_configs('tiny_rnnt')
    sd = S.make_state_dict(configs, 3)
    names = [k for k in sd if k.startswith(('predictor.', 'joint.'))]
    assert names[0] == 'predictor.embed.weight' and names[-1] == 'joint.ffn_out.bias'
    assert names[-8:] == [f'{p}.{w}' for p in ('predictor.projection', 'joint.enc_ffn',
                                                'joint.pred_ffn', 'joint.ffn_out')
                          for w in ('weight', 'bias')]
