"""Branchformer / E-Branchformer, host side (no GPU): the fp64 formulations of
tests/branchformer_refs.py against what the REAL reference's modules computed
(tests/golden/branchformer/, tools/gen_golden_branchformer.py), what the fixtures would catch,
the recipe mapping and its refusals, the zero-padded head layout.
"""
import copy

import numpy as np
import pytest
import torch

import branchformer_refs as BR
import kernel_refs as KR
from golden_util import load_case

PIN = 1e-9


@pytest.fixture(scope='module')
def modules():
    return BR.load_fixture('modules')[1]


@pytest.mark.parametrize('causal,linear', [(False, False), (False, True), (True, False),
                                           (True, True)])
def test_cgmlp_formulation_is_the_reference_module(modules, causal, linear):
    """Pins the pad value per mode, the chunk order r, g, the exact-erf GELU."""
    x, sd = BR.cgmlp_module_inputs(causal, linear)
    w = {'m.' + k: v for k, v in sd.items()}
    for T in BR.MODULE_T if causal else BR.MODULE_T[:1]:
        got = BR.cgmlp_formulation(x[:T], w, 'm', BR.CGMLP_MODULE['K'], causal)
        ref = torch.from_numpy(modules[f'cgmlp_{int(causal)}{int(linear)}_{T}'])
        err = (got - ref).abs().max().item()
        print(f'cgmlp causal={causal} linear={linear} T={T}: {err:.3e}')
        assert err <= PIN


@pytest.mark.parametrize('name,key', [('tiny_ebranchformer', 'elayer'),
                                      ('tiny_branchformer', 'blayer')])
def test_layer_formulation_is_the_reference_layer(modules, name, key):
    """Pins the two branches, the merge (its conv and zero padding), the 0.5 FFN scales."""
    x, configs, sd = BR.layer_module_inputs(name)
    ec = configs['encoder_conf']
    w = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    pos = sd['encoder.embed.pos_enc.pe'].reshape(-1, ec['output_size'])
    for T in BR.MODULE_T if ec.get('causal', False) else BR.MODULE_T[:1]:
        got = BR.layer_formulation(x[:T], w, 'encoder.encoders.0', ec, key == 'elayer', pos,
                                   torch.ones(T, T, dtype=torch.bool))
        err = (got - torch.from_numpy(modules[f'{key}_{T}'])).abs().max().item()
        print(f'{key} T={T}: {err:.3e}')
        assert err <= PIN


@pytest.mark.parametrize('name', sorted(BR.TINY))
def test_encoder_formulation_is_the_reference_encoder(name):
    """The whole encoder (front end, layers, after_norm; the chunk masks) on every utterance of
    the model fixture, decoded alone."""
    from wenet_amd import synthetic as S
    meta, arrays = BR.load_fixture(name)
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, meta['wseed'])
    for f in BR.tiny_features(name):
        n = f.shape[0]
        cases = [(-1, -1, f'enc64_{n}')]
        cases += [(cs, lc, f'enc64_{n}_c{cs}_l{lc}') for (cs, lc) in BR.CHUNK_CASES
                  if f'enc64_{n}_c{cs}_l{lc}' in arrays]
        for cs, lc, key in cases:
            got = BR.encoder_formulation(f, sd, configs, cs, lc)
            err = (got - torch.from_numpy(arrays[key])).abs().max().item()
            print(f'{name} {key}: {err:.3e}')
            assert err <= PIN
    if name == 'tiny_branchformer':     # the two left-chunk settings are different functions
        assert np.abs(arrays['enc64_135_c4_l-1'] - arrays['enc64_135_c4_l2']).max() > 1e-3


@pytest.mark.parametrize('causal,mutate', [(True, 'pad_zero'), (False, 'pad_bias'),
                                           (True, 'drop_tap'), (False, 'drop_tap'),
                                           (True, 'neighbours'), (False, 'neighbours'),
                                           (True, 'swap'), (False, 'swap')])
def test_fixture_sensitivity(causal, mutate):
    """Each mistake moves the formulation by more than 100 x the tolerance the GPU operator test
    has on the same case."""
    c = BR.make_csgu_case(128, 31, causal, BR.op_lens(32), seed=3, gap=0, lead=0)
    ref, e_plain, scale = BR.csgu_refs(c)
    tol = KR.bound(e_plain, scale)
    bad = BR.ref_csgu(c['h'], c['ln_w'], c['ln_b'], c['wt'], c['bias'], c['K'], causal,
                      c['seqs'], mutate=mutate)
    moved = (bad - ref).abs().max().item()
    print(f'causal={causal} {mutate}: moved {moved:.3e}, tolerance {tol:.3e}')
    assert moved > 100 * tol


def test_config_accepts_the_shipped_recipes():
    from wenet_amd.branchformer import branchformer_config_from_yaml
    from wenet_amd.model import config_from_yaml
    recipes = load_case('live_recipes')[0]
    want = {'aishell/s0/conf/train_ebranchformer.yaml': (2, 32, 8, 1024, 31, 31, 0),
            'aishell/s0/conf/train_u2++_branchformer.yaml': (1, 64, 4, 2048, 63, 0, 1),
            'librispeech/s0/conf/train_u2++_branchformer.yaml': (1, 64, 4, 2048, 31, 0, 1)}
    for name, (kind, hd, heads, units, k, km, causal) in want.items():
        c = copy.deepcopy(recipes[name])
        c.setdefault('input_dim', 80)
        c.setdefault('output_dim', 5000)
        cfg, b = branchformer_config_from_yaml(c)
        assert (b.kind, b.head_dim, cfg.n_heads, b.cgmlp_units, b.cgmlp_kernel, b.merge_kernel,
                cfg.causal) == (kind, hd, heads, units, k, km, causal), name
        assert cfg.d_model == 256 and b.linear_after_conv == 0 and cfg.encoder_type == 0
        assert config_from_yaml(c).d_model == 256


def _refused(configs, key):
    from wenet_amd.model import config_from_yaml
    with pytest.raises(NotImplementedError) as e:
        config_from_yaml(configs)
    assert key in str(e.value) and 'outside the accelerated path' in str(e.value), str(e.value)


@pytest.mark.parametrize('name,key,value', [
    ('tiny_branchformer', 'merge_method', 'learned_ave'),
    ('tiny_branchformer', 'merge_method', 'fixed_ave'),
    ('tiny_branchformer', 'use_attn', False),
    ('tiny_branchformer', 'use_cgmlp', False),
    ('tiny_branchformer', 'gate_activation', 'swish'),
    ('tiny_ebranchformer', 'gate_activation', 'relu'),
    ('tiny_ebranchformer', 'use_ffn', False),
    ('tiny_ebranchformer', 'macaron_style', False),
    ('tiny_ebranchformer', 'input_layer', 'conv2d6'),
    ('tiny_branchformer', 'pos_enc_layer_type', 'abs_pos'),
    ('tiny_ebranchformer', 'selfattention_layer_type', 'selfattn'),
    ('tiny_ebranchformer', 'activation_type', 'relu'),
    ('tiny_ebranchformer', 'attention_heads', 4),        # 64 / 4 = 16
    ('tiny_branchformer', 'attention_heads', 1),         # 128 / 1 = 128
    ('tiny_ebranchformer', 'cgmlp_linear_units', 192),   # 96 gate channels
    ('tiny_ebranchformer', 'cgmlp_linear_units', 4096),  # 2048 gate channels
    ('tiny_ebranchformer', 'cgmlp_conv_kernel', 30),     # even, non-causal
    ('tiny_branchformer', 'cgmlp_conv_kernel', 65),
    ('tiny_ebranchformer', 'merge_conv_kernel', 65),
])
def test_config_refusals_name_the_key(name, key, value):
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    configs['encoder_conf'][key] = value
    _refused(configs, key)


def test_transducer_on_these_encoders_is_refused():
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import transducer_config_from_yaml
    configs = S.make_configs('tiny_ebranchformer')
    configs['model'] = 'transducer'
    _refused(configs, 'transducer')
    t = S.make_configs('tiny_rnnt')
    t['encoder'] = 'e_branchformer'
    t['encoder_conf'] = S.make_configs('tiny_ebranchformer')['encoder_conf']
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        transducer_config_from_yaml(t)


def test_zero_padded_heads_are_exact():
    """H heads of 32 laid out as H x 64 columns with zero upper halves: the attention output and
    the output projection are EQUAL to the 32-wide ones in fp64 (every added term is 0 * 0)."""
    rng = np.random.default_rng(5)
    T, H, hd = 9, 2, 32
    d = H * hd
    x = rng.standard_normal((T, d))
    pos = rng.standard_normal((T, d))
    W = {n: rng.standard_normal((d, d)) / 8 for n in ('q', 'k', 'v', 'pos', 'out')}
    b = {n: rng.standard_normal(d) / 4 for n in ('q', 'k', 'v', 'out')}
    u, v = rng.standard_normal((H, hd)), rng.standard_normal((H, hd))

    def mm(a, bm):
        """a @ bm with the inner index added in ascending order (a BLAS may pick another order
        for another width; the claim is about the terms, not about a library's blocking)."""
        acc = np.zeros((a.shape[0], bm.shape[1]))
        for k in range(a.shape[1]):
            acc = acc + a[:, k:k + 1] * bm[k:k + 1, :]
        return acc

    def attend(Wq, bq, Wk, bk, Wv, bv, Wp, uu, vv, width):
        q, k, val, p = mm(x, Wq.T) + bq, mm(x, Wk.T) + bk, mm(x, Wv.T) + bv, mm(pos, Wp.T)
        out = np.zeros((T, H * width))
        for h in range(H):
            s = slice(h * width, (h + 1) * width)
            sc = (mm(q[:, s] + uu[h], k[:, s].T) + mm(q[:, s] + vv[h], p[:, s].T)) / np.sqrt(hd)
            e = np.exp(sc - sc.max(axis=1, keepdims=True))
            out[:, s] = mm(e / e.sum(axis=1, keepdims=True), val[:, s])
        return out

    ctx = attend(W['q'], b['q'], W['k'], b['k'], W['v'], b['v'], W['pos'], u, v, hd)
    pr = lambda a: BR.pad_heads_rows(a, H, hd)
    ctx_p = attend(pr(W['q']), pr(b['q']), pr(W['k']), pr(b['k']), pr(W['v']), pr(b['v']),
                   pr(W['pos']), pr(u.reshape(-1)).reshape(H, 64), pr(v.reshape(-1)).reshape(H, 64),
                   64)
    for h in range(H):
        assert np.array_equal(ctx_p[:, h * 64:h * 64 + hd], ctx[:, h * hd:(h + 1) * hd])
        assert not ctx_p[:, h * 64 + hd:(h + 1) * 64].any()
    w_out_p = pr(W['out'].T).T                       # (d, H * 64): zero columns
    assert not w_out_p[:, hd:64].any() and not w_out_p[:, 64 + hd:].any()
    assert np.array_equal(mm(ctx_p, w_out_p.T) + b['out'], mm(ctx, W['out'].T) + b['out'])


@pytest.mark.parametrize('name', ['tiny_ebranchformer', 'tiny_branchformer'])
def test_synthetic_state_dict_loads_strictly_into_the_reference(name):
    from oracle import _ref_harness
    if not _ref_harness.available():
        pytest.skip('the reference tree is not on this machine')
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, 1)
    model = build_reference_model(configs, sd)        # load_state_dict(strict=True) inside
    assert type(model.encoder).__name__ == ('EBranchformerEncoder' if 'eb' in name
                                            else 'BranchformerEncoder')
    if name == 'tiny_branchformer':
        assert 'encoder.encoders.0.pooling_proj1.weight' in sd
