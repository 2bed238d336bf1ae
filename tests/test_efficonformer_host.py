"""CPU checks of the Efficient Conformer path: the recipe mapping and its refusals
(wenet_amd/efficonformer.py), the fp64 formulations of tests/efficonformer_refs.py against what
the REAL reference's modules computed (tests/golden/efficonformer/, recorded by
tools/gen_golden_efficonformer.py) -- which is what makes them the yardstick of the GPU tests --
the mask rule against the reference's chunk masks, and the hook checks that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import efficonformer_refs as EF
from conftest import has_reference

pytestmark = pytest.mark.filterwarnings('ignore')

NOISE = 1e-11        # fp64 evaluations of one formula in two orders, values of order 1 - 10


def _recipe(name):
    cfg = EF.load_recipe(name)
    cfg.update(input_dim=80, output_dim=4233)
    return cfg


# name -> (front rate, blocks, stride layers, grouped layers, kernel of the first / last layer)
RECIPE_PLANS = {
    'aishell_v1': (4, 12, [3], [0, 1, 2, 3], 15, 7),
    'aishell_v1_stream': (4, 12, [3], [0, 1, 2, 3], 15, 7),
    'aishell_v2': (2, 12, [3, 7], [3, 7], 15, 15),
    'librispeech_v1': (4, 12, [3], [0, 1, 2, 3], 15, 7),
    'librispeech_v2': (2, 12, [3, 7], [3, 7], 15, 15),
}


@pytest.mark.parametrize('name', EF.RECIPES)
def test_the_five_recipes_parse(name):
    from wenet_amd.efficonformer import efficonformer_config_from_yaml, efficonformer_plan
    cfg = _recipe(name)
    front, blocks, strides, groups, k0, k1 = RECIPE_PLANS[name]
    plan = efficonformer_plan(cfg)
    assert plan['front_rate'] == front and plan['blocks'] == blocks
    assert plan['stride_layers'] == strides and plan['group_layers'] == groups
    assert plan['group_size'] == 3 and plan['d'] == 256 and plan['head_dim'] == 32
    rates, kernels, r, k = [], [], 1, k0
    for i in range(blocks):
        rates.append(r)
        kernels.append(k)
        if i in strides:
            r *= 2
            k = k1 if k1 != k0 else k
    assert plan['rates'] == rates and plan['kernels'] == kernels
    assert plan['total_rate'] == 2 ** len(strides)
    c, e = efficonformer_config_from_yaml(cfg)
    assert (c.d_model, c.n_heads, c.n_layers, c.cnn_kernel) == (256, 8, 12, 15)
    assert e.group_mask == sum(1 << i for i in groups) and e.n_stride == len(strides)
    assert list(e.stride_layers)[:len(strides)] == strides
    assert (e.front_rate, e.head_dim, e.group_size) == (front, 32, 3)
    assert e.stride_kernel == int(k1 != k0)
    assert c.causal == int(name == 'aishell_v1_stream')


def test_flattened_keys_ints_and_lists_mean_the_same():
    from wenet_amd.efficonformer import efficonformer_plan
    cfg = _recipe('aishell_v1')
    want = efficonformer_plan(cfg)
    flat = _recipe('aishell_v1')
    flat['encoder_conf'].update(flat['encoder_conf'].pop('efficient_conf'))
    assert {k: v for k, v in efficonformer_plan(flat).items() if k != 'ec'} == \
        {k: v for k, v in want.items() if k != 'ec'}
    ints = _recipe('aishell_v1')
    ints['encoder_conf']['efficient_conf'].update(stride_layer_idx=3, stride=2)
    assert efficonformer_plan(ints)['stride_layers'] == [3]
    for sk in (True, False):
        cfg['encoder_conf']['efficient_conf']['stride_kernel'] = sk
        assert efficonformer_plan(cfg)['kernels'][-1] == (7 if sk else 15)


def _with(path, value, base='aishell_v1'):
    cfg = _recipe(base)
    node = cfg['encoder_conf']
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value
    return cfg


REFUSALS = [
    (('efficient_conf', 'stride'), [3], 'stride'),
    (('efficient_conf', 'stride'), 4, 'stride'),
    (('efficient_conf', 'group_size'), 2, 'group_size'),
    (('efficient_conf', 'group_size'), 4, 'group_size'),
    (('attention_heads', ), 2, 'attention_heads'),              # heads of 128
    (('cnn_module_kernel', ), 17, 'cnn_module_kernel'),         # 17 // 2 = 8 on a non-causal model
    (('pos_enc_layer_type', ), 'abs_pos', 'pos_enc_layer_type'),
    (('normalize_before', ), False, 'normalize_before'),
    (('macaron_style', ), False, 'macaron_style'),
    (('use_cnn_module', ), False, 'use_cnn_module'),
    (('input_layer', ), 'conv2d6', 'input_layer'),
    (('input_layer', ), 'linear', 'input_layer'),
    (('efficient_conf', 'stride_layer_idx'), [3], 'stride_layer_idx'),          # descending
    (('efficient_conf', 'stride_layer_idx'), [12], 'stride_layer_idx'),         # behind the last
    (('efficient_conf', 'no_such_key'), 1, 'no_such_key'),
    (('activation_type', ), 'relu', 'activation_type'),
]


@pytest.mark.parametrize('path,value,key', REFUSALS)
def test_refusals_name_their_key(path, value, key):
    from wenet_amd.efficonformer import efficonformer_config_from_yaml
    cfg = _with(path, value)
    if value == [3] and key == 'stride_layer_idx':
        cfg['encoder_conf']['efficient_conf'].update(stride_layer_idx=[3, 2], stride=[2, 2])
    with pytest.raises(NotImplementedError) as e:
        efficonformer_config_from_yaml(cfg)
    assert f'{key}=' in str(e.value) and 'outside the accelerated path' in str(e.value)


def test_asr_model_and_other_encoders_point_at_the_class():
    from wenet_amd.efficonformer import efficonformer_config_from_yaml
    from wenet_amd.model import ASRModel
    cfg = _recipe('aishell_v2')
    with pytest.raises(NotImplementedError, match='EfficientConformer'):
        ASRModel._config(object.__new__(ASRModel), cfg)
    with pytest.raises(NotImplementedError, match='conformer'):
        efficonformer_config_from_yaml(dict(cfg, encoder='conformer'))
    from wenet_amd.efficonformer import EfficientConformer
    with pytest.raises(NotImplementedError, match="model 'transducer'"):
        EfficientConformer._config(object.__new__(EfficientConformer),
                                   dict(cfg, model='transducer'))


# ---------------------------------------------------------------------------------------------
# the formulations against the reference's modules


@pytest.fixture(scope='module')
def modules():
    return EF.load_fixture('modules')[1]


def _close(got, want, what):
    want = torch.from_numpy(np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    assert err <= NOISE * max(1.0, want.abs().max().item()), (what, err)


@pytest.mark.parametrize('name', sorted(EF.ATTN_MODULE))
def test_grouped_attention_formulation_is_the_reference_module(modules, name):
    m = EF.ATTN_MODULE[name]
    x, sd, pos = EF.attn_module_inputs(name)
    w = {'a.' + k: v for k, v in sd.items()}
    for T in m['frames']:
        y = EF.grouped_attention_module(x[:T], w, 'a', m['H'], m['g'], pos)
        _close(y, modules[f'attn_{name}_{T}'], f'{name} T={T}')
    T = EF.ATTN_MASK_T
    ng = (T + m['g'] - 1) // m['g']
    for (mm, c, left) in EF.ATTN_MASK_CASES:
        vis = EF.group_visible(ng, mm, c, left)
        y = EF.grouped_attention_module(x[:T], w, 'a', m['H'], m['g'], pos, vis)
        _close(y, modules[f'attn_{name}_{T}_c{c}_l{left}_m{mm}'], f'{name} c={c} l={left} m={mm}')


@pytest.mark.parametrize('name', sorted(EF.ATTN_MODULE))
def test_operator_formulation_is_the_module_without_its_projections(name):
    """ref_attention_grouped (what the kernel is held to) on the projected q / k / v / p of the
    module's inputs, followed by linear_out, is grouped_attention_module."""
    m = EF.ATTN_MODULE[name]
    x, sd, pos = EF.attn_module_inputs(name)
    w = {'a.' + k: v for k, v in sd.items()}
    T, g, H, d = 33, m['g'], m['H'], m['d']
    lin = lambda n: x[:T] @ sd[n + '.weight'].t() + sd[n + '.bias']
    P = pos[:T] @ sd['linear_pos.weight'].t()
    for (mm, c, left) in [(3, 0, -1)] + EF.ATTN_MASK_CASES:
        ctx = EF.ref_attention_grouped(lin('linear_q'), lin('linear_k'), lin('linear_v'), P,
                                       sd['pos_bias_u'], sd['pos_bias_v'], [(0, T)], [0], g, H,
                                       1.0 / np.sqrt(g * d // H), mm, c, left)
        y = ctx @ sd['linear_out.weight'].t() + sd['linear_out.bias']
        vis = EF.group_visible((T + g - 1) // g, mm, c, left) if c > 0 else None
        want = EF.grouped_attention_module(x[:T], w, 'a', H, g, pos, vis)
        assert (y - want).abs().max().item() <= NOISE * 10


@pytest.mark.parametrize('name', sorted(EF.CONV_MODULE))
def test_strided_conv_formulations_are_the_reference_module(modules, name):
    m = EF.CONV_MODULE[name]
    x, sd = EF.conv_module_inputs(name)
    w = {'c.' + k: v for k, v in sd.items()}
    d, K = m['d'], m['K']
    bn = m['norm'] == 'batch_norm'
    for T in EF.CONV_FRAMES:
        y = EF.conv_module(x[:T], w, 'c', K, m['causal'], bn, 2)
        _close(y, modules[f'conv_{name}_{T}'], f'{name} T={T}')
        # the operator's statement: GLU of the utterance's own frames, the causal pad frame = the
        # GLU of pointwise_conv1's bias (the module pads in FRONT of pointwise_conv1)
        b1 = sd['pointwise_conv1.bias']
        h = x[:T] @ sd['pointwise_conv1.weight'][:, :, 0].t() + b1
        glu = h[:, :d] * torch.sigmoid(h[:, d:])
        cpad = b1[:d] * torch.sigmoid(b1[d:])
        if bn:
            sc = sd['norm.weight'] / torch.sqrt(sd['norm.running_var'] + 1e-5)
            nw, nb = sc, sd['norm.bias'] - sd['norm.running_mean'] * sc
        else:
            nw, nb = sd['norm.weight'], sd['norm.bias']
        z = EF.ref_stride_dwconv(glu, sd['depthwise_conv.weight'], sd['depthwise_conv.bias'], nw,
                                 nb, int(bn), K, m['causal'], [(0, T)], [0], (T + 1) // 2,
                                 cpad if m['causal'] else None)
        z = z @ sd['pointwise_conv2.weight'][:, :, 0].t() + sd['pointwise_conv2.bias']
        _close(z, modules[f'conv_{name}_{T}'], f'{name} operator T={T}')


def test_average_pool_formulation(modules):
    for T in (1, 2, 3, 4):
        x = torch.arange(1.0, T + 1.0).double().view(T, 1)
        _close(EF.avgpool_time(x)[:, 0], modules[f'pool_{T}'], f'pool T={T}')
        z = torch.zeros((T + 1) // 2, 1, dtype=torch.float64)
        _close(EF.ref_avgpool_residual(x, z, [(0, T)], [0])[:, 0], modules[f'pool_{T}'], 'operator')
    assert EF.avgpool_time(torch.tensor([[1.0], [3.0], [10.0]]))[:, 0].tolist() == [2.0, 10.0]


@pytest.mark.parametrize('name', sorted(EF.TINY))
def test_stride_layer_formulation_is_the_reference_layer(modules, name):
    from wenet_amd.efficonformer import efficonformer_plan
    x, configs, sd = EF.layer_module_inputs(name)
    plan = efficonformer_plan(configs)
    i = plan['stride_layers'][0]
    d = plan['d']
    w = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    pe = sd['encoder.embed.pos_enc.pe'].reshape(-1, d).double()
    y = EF.layer_formulation(x, w, f'encoder.encoders.{i}', plan['heads'], pe, plan['kernels'][i],
                             plan['causal'],
                             plan['ec']['cnn_module_norm'] == 'batch_norm', True, True,
                             plan['group_size'])
    _close(y, modules[f'layer_{name}'], name)


def test_mask_rule_is_the_decimated_chunk_mask(modules):
    """group_visible (the rule attention_grouped evaluates on frame indices) equals the
    reference's chunk_masks[:, ::m, ::m], recorded and -- where the reference is present -- live."""
    live = None
    if has_reference():
        from oracle import _ref_harness
        _ref_harness.install()
        from wenet.utils.mask import subsequent_chunk_mask as live
    for (m, c, left) in EF.MASK_CASES:
        ng = (EF.MASK_T + m - 1) // m
        got = EF.group_visible(ng, m, c, left)
        assert torch.equal(got, torch.from_numpy(modules[f'mask_m{m}_c{c}_l{left}']).bool()), \
            (m, c, left)
        if live is not None:
            assert torch.equal(got, live(EF.MASK_T, c, left)[::m, ::m]), (m, c, left)
    # c = 16 at the group rate is no chunk window: rows of one "chunk" see different key sets
    vis = EF.group_visible(17, 3, 16, -1)
    assert vis[5].sum() != vis[6].sum() and 16 % 3 != 0


@pytest.mark.parametrize('name', sorted(EF.TINY))
def test_encoder_formulation_is_the_reference_encoder(name):
    """Front end + every layer + after_norm, each utterance alone, against the recorded fp64
    encoder outputs: full context and the chunk-mask cases."""
    from wenet_amd import synthetic as S
    from wenet_amd.efficonformer import efficonformer_plan
    meta, arrays = EF.load_fixture(name)
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, meta['wseed'])
    plan = efficonformer_plan(configs)
    tiny = EF.TINY[name]
    for f, n_out in zip(EF.tiny_features(name), meta['enc_lens']):
        n = f.shape[0]
        x0 = EF.frontend_formulation(f, sd, plan['d'], plan['front_rate'])
        y = EF.encoder_formulation(x0, sd, plan)
        assert y.shape[0] == n_out
        _close(y, arrays[f'enc64_{n}'], f'{name} {n}')
        if n in tiny['chunk_frames']:
            for (cs, lc) in tiny['chunk_cases']:
                y = EF.encoder_formulation(x0, sd, plan, cs, lc)
                _close(y, arrays[f'enc64_{n}_c{cs}_l{lc}'], f'{name} {n} c{cs} l{lc}')


def test_fixture_lengths_cover_the_edge_cases():
    """At every grouped layer's input rate T mod 3 = 0, 1, 2 and T = 1, 2; at every stride layer
    odd and even T and T = 1."""
    from wenet_amd import synthetic as S
    from wenet_amd.efficonformer import efficonformer_plan
    for name, tiny in EF.TINY.items():
        plan = efficonformer_plan(S.make_configs(name))
        t0 = [((n - 1) // 2 - 1) // 2 if plan['front_rate'] == 4 else (n - 1) // 2
              for n in tiny['frames']]
        for i in range(plan['blocks']):
            lens = list(t0)
            for _ in range(plan['rates'][i].bit_length() - 1):
                lens = [(t + 1) // 2 for t in lens]
            if i in plan['group_layers']:
                assert {t % 3 for t in lens} == {0, 1, 2} and {1, 2} <= set(lens), (name, i, lens)
            if i in plan['stride_layers']:
                assert 1 in lens and any(t % 2 == 0 for t in lens) and \
                    any(t % 2 == 1 and t > 1 for t in lens), (name, i, lens)


# ---------------------------------------------------------------------------------------------
# hook checks that need no device


def test_hooks_refuse_by_argument_name_before_any_device_call():
    from wenet_amd import _lib
    L = _lib.lib()
    host = ctypes.create_string_buffer(16384)
    p = ctypes.addressof(host)
    one = np.asarray([0], dtype=np.int32)
    ln = np.asarray([4], dtype=np.int32)
    i32 = _lib.i32p

    def grouped(width=96, group=3, ld=128, mask_step=3, chunk=0, heads=4):
        return L.wn_op_attention_grouped(p, p, p, ld, ld, ld, 8, p, ld, 8, None, p, p, p, ld,
                                         i32(one), i32(ln), 1, heads, group, width, mask_step,
                                         chunk, -1, 0.1, None)

    for call, words in ((lambda: grouped(width=64), 'width = 64'),
                        (lambda: grouped(width=128), 'width = 128'),
                        (lambda: grouped(group=5), 'group'),
                        (lambda: grouped(ld=64), 'stride'),
                        (lambda: grouped(mask_step=0), 'mask_step'),
                        (lambda: grouped(chunk=-1), 'chunk_size')):
        assert call() == -1
        msg = L.wn_last_error().decode()
        assert 'cabi_ops.hip' in msg and words in msg, msg

    def strided(stride=2, K=15, causal=0, D=128, norm_mode=0):
        return L.wn_op_stride_dwconv_ln_silu(p, D, 8, D, p, p, None, p, p, norm_mode, 1e-5, K,
                                             causal, stride, p + 8192, D, 4, i32(one), i32(ln),
                                             i32(one), 1, None)

    for call, words in ((lambda: strided(stride=3), 'stride = 3'),
                        (lambda: strided(stride=1), 'stride = 1'),
                        (lambda: strided(K=14), 'K must be'),
                        (lambda: strided(K=65, causal=1), 'K must be'),
                        (lambda: strided(D=96), 'D must be'),
                        (lambda: strided(norm_mode=2), 'norm_mode')):
        assert call() == -1
        msg = L.wn_last_error().decode()
        assert 'cabi_ops.hip' in msg and words in msg, msg
    assert L.wn_op_avgpool_residual_add(p, 128, 8, p + 8192, 128, p + 8192, 128, 4, 128, 4,
                                        i32(one), i32(ln), i32(one), 1, None) == -1
    assert 'stride = 4' in L.wn_last_error().decode()
    assert host.raw == bytes(16384)
