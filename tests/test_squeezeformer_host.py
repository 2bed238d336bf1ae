"""Squeezeformer, host side (no GPU): the fp64 formulations of tests/squeezeformer_refs.py against
what the REAL reference's modules computed (tests/golden/squeezeformer/,
tools/gen_golden_squeezeformer.py), what the operator cases would catch, the yardsticks of the GPU
operator tests, the fold arithmetic, the recipe mapping and its refusals, the argument checks of
the operator hooks.
"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kernel_refs as KR
import squeezeformer_refs as SQ
from golden_util import load_case

PIN = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def modules():
    return SQ.load_fixture('modules')[1]


# ---------------------------------------------------------------------------------------------
# the formulations are the reference's modules


def test_attention_with_the_wrapped_shift_is_the_reference_module(modules):
    """Pins the closed form of the shift (both branches, the zero, the next query row), the
    adaptive scale on query, key AND value, the scale 1 / sqrt(d_k)."""
    x, sd, pos = SQ.attn_module_inputs()
    w = {'m.' + k: v for k, v in sd.items()}
    for T in SQ.ATTN_MODULE['frames']:
        got = SQ.attention_module(x[:T], w, 'm', SQ.ATTN_MODULE['H'], pos, True)
        err = (got - torch.from_numpy(modules[f'attn_{T}'])).abs().max().item()
        print(f'attention T={T}: {err:.3e}')
        assert err <= PIN


@pytest.mark.parametrize('K,key', [(5, 'reduce1d'), (1, 'reducestream')])
def test_time_reduction_is_the_reference_module(modules, K, key):
    """Pins the padding 3 of the 5-tap conv, the stride, ceil(T / 2) frames (the reference's
    extra frame is cut), the pointwise conv behind it."""
    x, sd = SQ.reduce_module_inputs(K)
    w = {'m.' + k: v for k, v in sd.items()}
    for T in SQ.REDUCE_MODULE['frames']:
        got = SQ.time_reduction_module(x[:T], w, 'm', K)
        ref = torch.from_numpy(modules[f'{key}_{T}'])
        assert got.shape == ref.shape == ((T + 1) // 2, SQ.REDUCE_MODULE['d'])
        err = (got - ref).abs().max().item()
        print(f'{key} T={T}: {err:.3e}')
        assert err <= PIN


@pytest.mark.parametrize('name', sorted(SQ.TINY))
def test_layer_formulation_and_the_folds_are_the_reference_layer(modules, name):
    """The block written from the module text, and the block as the library evaluates it -- the
    adaptive scale folded into Q / K / V / w_1 / pointwise_conv1, the causal pad frame from the
    UNFOLDED bias, BatchNorm as an affine -- both against the recorded reference layer."""
    x, configs, sd = SQ.layer_module_inputs(name)
    ec = configs['encoder_conf']
    w = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    pos = sd['encoder.embed.pos_enc.pe'].reshape(-1, ec['encoder_dim']).double()
    ref = torch.from_numpy(modules[f'layer_{name}'])
    plain = SQ.layer_formulation(x, w, 'encoder.encoders.0', ec, pos)
    folded = SQ.folded_layer(x, w, 'encoder.encoders.0', ec, pos)
    e1, e2 = (plain - ref).abs().max().item(), (folded - ref).abs().max().item()
    print(f'{name}: formulation {e1:.3e}, folded {e2:.3e}')
    assert e1 <= PIN and e2 <= PIN
    if ec['causal']:
        # the trap: a pad frame computed from the FOLDED bias is another function
        p = 'encoder.encoders.0.conv_module'
        b1 = w[p + '.pointwise_conv1.bias']
        _, bf = SQ.fold_ada(w[p + '.pointwise_conv1.weight'][:, :, 0], b1, w[p + '.ada_scale'],
                            w[p + '.ada_bias'])
        d = ec['encoder_dim']
        assert (bf[:d] * torch.sigmoid(bf[d:]) - b1[:d] * torch.sigmoid(b1[d:])).abs().max() > 1e-2


def test_input_scale_fold():
    """input_proj(x sqrt d) = sqrt(d) (W x + b / sqrt d): the form the Conformer front end has."""
    g = torch.Generator().manual_seed(3)
    d = 128
    W, b = torch.randn(d, 19 * d, generator=g).double(), torch.randn(d, generator=g).double()
    x = torch.randn(5, 19 * d, generator=g).double()
    want = (x * d ** 0.5) @ W.t() + b
    got = (x @ W.t() + b / d ** 0.5) * d ** 0.5
    assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()


@pytest.mark.parametrize('name', sorted(SQ.TINY))
def test_model_fixture(name):
    meta, arrays = SQ.load_fixture(name)
    assert meta['enc_lens'] == SQ.ENC_LENS and meta['frames'] == SQ.FRAMES
    for n, t in zip(SQ.FRAMES, SQ.ENC_LENS):
        assert arrays[f'enc64_{n}'].shape[0] == t
    assert sum(len(u) > 0 for u in meta['tokens']['ctc_greedy_search']) >= 3
    if name == 'tiny_squeezeformer_u2pp':   # the two left-chunk settings are different functions
        assert np.abs(arrays['enc64_135_c4_l-1'] - arrays['enc64_135_c4_l2']).max() > 1e-3
        assert np.abs(arrays['enc64_135_c4_l-1'] - arrays['enc64_135']).max() > 1e-3


# ---------------------------------------------------------------------------------------------
# the operator cases: their yardsticks, and what they would catch


@pytest.fixture(scope='module')
def sq_cases():
    out = {}
    for name, kw in SQ.SQSHIFT_CASES.items():
        c = SQ.make_sqshift_case(**kw)
        out[name] = (c, ) + SQ.sqshift_refs(c)
    return out


def test_yardsticks_hold_their_cap(sq_cases):
    for name, (c, ref, e_plain, scale) in sq_cases.items():
        print(f'attention_sqshift {name}: e_plain={e_plain:.3e} scale={scale:.3e}')
        assert KR.cap_ok(e_plain, scale), name
        assert torch.isfinite(ref).all()
    for K in (5, 1):
        for C in (128, 512):
            c = SQ.make_time_case(C, K, seed=K + C)
            ref, e_plain, scale = SQ.time_reduce_refs(c)
            print(f'time_reduce K={K} C={C}: e_plain={e_plain:.3e} scale={scale:.3e}')
            assert KR.cap_ok(e_plain, scale)
            assert torch.isfinite(ref).all()


@pytest.mark.parametrize('mutate', SQ.MUTANTS)
def test_sign_cases_catch_a_wrong_shift(sq_cases, mutate):
    """Each wrong variant of the shift moves the reference by more than 100 x the tolerance of
    the GPU test on at least one sign case."""
    caught = []
    for name in SQ.SIGN_CASES:
        c, ref, e_plain, scale = sq_cases[name]
        tol = KR.bound(e_plain, scale)
        bad = SQ.ref_attention_sqshift(c['q'], c['k'], c['v'], c['P'], c['bias_u'], c['bias_v'],
                                       c['seqs'], c['scale'], mutate=mutate)
        moved = (bad - ref).abs().max().item()
        print(f'{mutate} on {name}: moved {moved:.3e}, tolerance {tol:.3e}')
        caught.append(moved > 100 * tol)
    assert any(caught)


def test_closed_form_wraps():
    """The three branches on a 3 x 3 example, entry by entry."""
    bd = torch.arange(9, dtype=torch.float64).view(1, 3, 3)
    got = SQ.wrapped_shift(bd, 3)[0]
    want = torch.tensor([[bd[0, 0, 2], 0.0, bd[0, 1, 0]],
                         [bd[0, 1, 1], bd[0, 1, 2], 0.0],
                         [bd[0, 2, 0], bd[0, 2, 1], bd[0, 2, 2]]], dtype=torch.float64)
    assert torch.equal(got, want)
    assert torch.equal(SQ.wrapped_shift(bd[:, :1, :1], 1), bd[:, :1, :1])


# ---------------------------------------------------------------------------------------------
# the recipe mapping


def test_config_accepts_the_shipped_recipes():
    from wenet_amd.model import config_from_yaml
    from wenet_amd.squeezeformer import squeezeformer_config_from_yaml
    recipes = load_case('live_recipes')[0]
    # d, heads, ffn, K, cnn_norm, causal, dynamic chunk, reduce kernel, shift, decoders
    want = {'librispeech/s0/conf/train_squeezeformer.yaml': (256, 4, 1024, 31, 0, 0, 0, 5, 1, 0),
            'librispeech/s0/conf/train_u2++_squeezeformer.yaml':
                (256, 4, 2048, 31, 0, 1, 1, 1, 0, 1),
            'librispeech/s0/conf/train_squeezeformer_bidecoder_large.yaml':
                (512, 8, 2048, 31, 1, 0, 0, 5, 1, 1)}
    for name, w in want.items():
        c = copy.deepcopy(recipes[name])
        c.setdefault('input_dim', 80)
        c.setdefault('output_dim', 5002)
        cfg, q = squeezeformer_config_from_yaml(c)
        assert (cfg.d_model, cfg.n_heads, cfg.ffn_dim, cfg.cnn_kernel, cfg.cnn_norm, cfg.causal,
                cfg.use_dynamic_chunk, q.reduce_kernel, q.do_rel_shift, cfg.bidirectional) == w, name
        assert (q.reduce_idx, q.recover_idx, cfg.n_layers, cfg.encoder_type) == (5, 11, 12, 0)
        assert config_from_yaml(c).d_model == w[0]


def _refused(configs, key):
    from wenet_amd.model import config_from_yaml
    with pytest.raises(NotImplementedError) as e:
        config_from_yaml(configs)
    assert key in str(e.value) and 'outside the accelerated path' in str(e.value), str(e.value)


@pytest.mark.parametrize('key,value', [
    ('time_reduction_layer_type', 'conv2d'),
    ('dw_stride', True),
    ('output_size', 256),                 # != encoder_dim: the final_proj
    ('normalize_before', True),
    ('concat_after', True),
    ('pos_enc_layer_type', 'abs_pos'),
    ('reduce_idx', [1, 2]),
    ('recover_idx', [2, 3]),
    ('recover_idx', None),                # a reduction without a recovery
    ('recover_idx', 1),                   # not behind the reduction
    ('recover_idx', 4),                   # not a block
    ('attention_heads', 4),               # 128 / 4 = 32
    ('activation_type', 'relu'),
    ('feed_forward_expansion_factor', 0),
    ('cnn_norm_type', 'group_norm'),
    ('cnn_module_kernel', 30),            # even, non-causal
])
def test_config_refusals_name_the_key(key, value):
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_squeezeformer')
    configs['encoder_conf'][key] = value
    _refused(configs, key)


@pytest.mark.parametrize('ec', [
    dict(reduce_idx=None, recover_idx=None), dict(reduce_idx=[1], recover_idx=[3]),
    dict(reduce_idx=0, recover_idx=1), dict(time_reduction_layer_type='stream'),
    dict(do_rel_shift=False), dict(cnn_norm_type='layer_norm'), dict(causal=True),
    dict(adaptive_scale=False), dict(use_dynamic_chunk=True, use_dynamic_left_chunk=True),
    dict(static_chunk_size=4, do_rel_shift=False), dict(feed_forward_expansion_factor=8),
])
def test_config_accepts(ec):
    from wenet_amd import synthetic as S
    from wenet_amd.squeezeformer import squeezeformer_config_from_yaml
    configs = S.make_configs('tiny_squeezeformer')
    configs['encoder_conf'].update(ec)
    cfg, q = squeezeformer_config_from_yaml(configs)
    if 'reduce_idx' in ec and ec['reduce_idx'] is None:
        assert (q.reduce_idx, q.recover_idx) == (-1, -1)
    assert cfg.ffn_dim == 128 * configs['encoder_conf']['feed_forward_expansion_factor']


def test_transducer_on_this_encoder_is_refused():
    from wenet_amd import synthetic as S
    from wenet_amd.squeezeformer import Squeezeformer
    from wenet_amd.transducer import transducer_config_from_yaml
    t = S.make_configs('tiny_rnnt')
    t['encoder'] = 'squeezeformer'
    t['encoder_conf'] = S.make_configs('tiny_squeezeformer')['encoder_conf']
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        transducer_config_from_yaml(t)
    configs = S.make_configs('tiny_squeezeformer')
    configs['model'] = 'transducer'
    with pytest.raises(NotImplementedError, match='transducer'):
        Squeezeformer._config(object.__new__(Squeezeformer), configs)


def test_load_model_dispatches_on_the_encoder(tmp_path, monkeypatch):
    """load_model on a Squeezeformer directory builds a wenet_amd.Squeezeformer from the
    directory's recipe and weights.  (No GPU here: the constructor is recorded, not run.)"""
    import yaml

    import wenet_amd
    from wenet_amd import squeezeformer as SQM
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_squeezeformer')
    sd = S.make_state_dict(configs, 0)
    V = configs['output_dim']
    syms = ['<blank>', '<unk>', '<sos/eos>'] + [f'w{i}' for i in range(3, V)]
    (tmp_path / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    (tmp_path / 'train.yaml').write_text(yaml.safe_dump(configs))
    torch.save(sd, tmp_path / 'final.pt')
    seen = {}

    def fake_init(self, cfgs, state, device='cuda'):
        seen.update(encoder=cfgs.get('encoder'), keys=len(state))
        self.configs = cfgs
        self._h = None

    monkeypatch.setattr(SQM.Squeezeformer, '__init__', fake_init)
    m = wenet_amd.load_model(str(tmp_path))
    assert type(m) is wenet_amd.Squeezeformer
    assert seen['encoder'] == 'squeezeformer' and seen['keys'] >= len(sd) - 2


@pytest.mark.parametrize('name', sorted(SQ.TINY))
def test_synthetic_state_dict_loads_strictly_into_the_reference(name):
    from oracle import _ref_harness
    if not _ref_harness.available():
        pytest.skip('the reference tree is not on this machine')
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, 1)
    model = build_reference_model(configs, sd)        # load_state_dict(strict=True) inside
    assert type(model.encoder).__name__ == 'SqueezeformerEncoder'


# ---------------------------------------------------------------------------------------------
# the operator hooks


def _declared(src, name):
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', src, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_operator_hooks_are_declared_exported_and_check_their_arguments():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('wn_op_attention_sqshift', 'wn_op_time_reduce', 'wn_op_time_recover',
                 'wn_model_create_squeezeformer'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert len(_declared(src, name)) == len(getattr(L, name).argtypes), name
    assert ctypes.sizeof(_lib.WnSqueezeformerConfig) == 4 * 4
    assert ctypes.sizeof(_lib.WnConfig) == 4 * 30      # wn_config is what it was

    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    one = ctypes.c_void_p(1 << 20)     # a non-null pointer no accepted call would reach
    far = ctypes.c_void_p(1 << 30)
    err = lambda: L.wn_last_error().decode()

    def shift(off, ln, rows=8, p_rows=8, ld=128, heads=2, Q=one):
        return L.wn_op_attention_sqshift(Q, one, one, ld, ld, ld, rows, one, ld, p_rows, one, one,
                                         one, ld, _lib.i32p(off), _lib.i32p(ln), len(off), heads,
                                         0.125, None)

    assert shift(i32(0), i32(8), Q=None) == -1 and 'null' in err()
    assert shift(i32(0), i32(9)) == -1 and 'outside the buffer' in err()
    assert shift(i32(0, 2), i32(4, 4)) == -1 and 'overlapping' in err()
    assert shift(i32(0), i32(8), ld=126) == -1 and 'multiples of 4' in err()
    assert shift(i32(0), i32(8), ld=64) == -1 and 'smaller than n_heads' in err()
    assert shift(i32(0), i32(0)) == -1 and 'empty' in err()
    assert shift(i32(0), i32(8), p_rows=7) == -1 and 'position table' in err()

    def reduce(off, ln, off2, rows=8, rows2=4, C=64, ld=64, K=5, pad=3, x=one, y=far):
        return L.wn_op_time_reduce(x, ld, rows, C, one, one, K, pad, y, ld, rows2, _lib.i32p(off),
                                   _lib.i32p(ln), _lib.i32p(off2), len(off), None)

    assert reduce(i32(0), i32(8), i32(0), x=None) == -1 and 'null' in err()
    assert reduce(i32(0), i32(9), i32(0)) == -1 and 'outside the buffer' in err()
    assert reduce(i32(0, 2), i32(4, 4), i32(0, 2)) == -1 and 'overlapping' in err()
    assert reduce(i32(0), i32(8), i32(1)) == -1 and 'half-rate rows outside' in err()
    assert reduce(i32(0, 4), i32(4, 4), i32(0, 1)) == -1 and 'half-rate' in err()
    assert reduce(i32(0), i32(0), i32(0)) == -1 and 'empty' in err()
    assert reduce(i32(0), i32(8), i32(0), ld=66) == -1 and 'multiples of 4' in err()
    assert reduce(i32(0), i32(8), i32(0), C=96, ld=96) == -1 and 'multiple of 64' in err()
    assert reduce(i32(0), i32(8), i32(0), y=one) == -1 and 'overlaps' in err()
    assert reduce(i32(0), i32(8), i32(0), K=3, pad=1) == -1 and '5 taps' in err()

    def recover(off, ln, off2, rows=8, rows2=4, C=64, ld=64, skip=one, z=far, y=one):
        return L.wn_op_time_recover(skip, ld, z, ld, rows2, y, ld, rows, C, _lib.i32p(off),
                                    _lib.i32p(ln), _lib.i32p(off2), len(off), None)

    assert recover(i32(0), i32(8), i32(0), z=None) == -1 and 'null' in err()
    assert recover(i32(0), i32(9), i32(0)) == -1 and 'outside the buffer' in err()
    assert recover(i32(0), i32(8), i32(1)) == -1 and 'half-rate' in err()
    assert recover(i32(0), i32(0), i32(0)) == -1 and 'empty' in err()
    assert recover(i32(0), i32(8), i32(0), ld=66) == -1 and 'multiples of 4' in err()
    assert recover(i32(0), i32(8), i32(0), z=one) == -1 and 'overlaps' in err()
