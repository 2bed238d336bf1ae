"""CPU checks behind the decoders with heads of 32: the width-parameterised reference of
tests/attention_d32_refs.py against kernel_refs.ref_attention at 64, the cap of every case the GPU
file runs, the recorded fixtures, the recipes' decoder heads and the hook's declaration.

The cap (kernel_refs.cap_ok: e_plain <= 1e-3 of the output scale, the plain fp32 evaluation
alone): every regime keeps the parameter it has at heads of 64 -- `peaked` 10 and 30, ramps of 1.0
per key, shifts of +-80, needles of 60 -- none had to be lowered at 32.
"""
import os
import re

import pytest
import torch

import attention_d32_refs as D
import efficonformer_refs as EF
import kernel_refs as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('self_attn', [True, False])
def test_restatement_equals_kernel_refs_at_64(self_attn):
    c = KR.make_attention_case('unit', 2, [1, 31, 33, 65], None if self_attn else [3, 32, 70, 9],
                               mask_mode=1 if self_attn else 0, seed=3)
    seqs = [s[:4] for s in c['seqs']]
    for fp32 in (False, True):
        want = KR.ref_attention(c['q'], c['k'], c['v'], None, None, None, c['seqs'],
                                c['mask_mode'], 0, -1, c['scale'], fp32=fp32)
        got = D.ref_attention_w(c['q'], c['k'], c['v'], seqs, 2, 64, c['scale'], c['mask_mode'],
                                fp32=fp32)
        assert torch.equal(got, want)


@pytest.mark.parametrize('name', sorted(D.ATTENTION_CASES))
def test_attention_cases_keep_the_cap(name):
    c = D.make_case(**D.ATTENTION_CASES[name])
    ref, e_plain, scale, w = D.case_refs(c)
    print(f'{name}: e_plain={e_plain:.3e} scale={scale:.3e}')
    assert torch.isfinite(ref).all()
    assert KR.cap_ok(e_plain, scale), (name, e_plain, scale)
    kw = D.ATTENTION_CASES[name]
    key = (kw['regime'], {'0': 'first'}.get(kw['param'], kw['param']))
    if key in KR.NON_FLAT and not (kw['mask_mode'] == 1 and kw['param'] in ('31', '32')):
        # (under the causal mask the needle is hidden from the rows in front of it)
        assert (w > 0.5).double().mean().item() >= KR.NON_FLAT[key], name
    # the packed buffers hold the poison wherever no sequence owns
    own = torch.zeros(c['q_rows'], dtype=torch.bool)
    for (qo, ql, _, _) in c['seqs']:
        own[qo:qo + ql] = True
    assert (c['buf_q'][~own].abs() == KR.POISON).all()
    # a reversed packing order moves the rows, not the data
    r = D.make_case(order=list(range(len(c['q_lens'])))[::-1], **kw)
    for u, t in enumerate(c['q_lens']):
        assert torch.equal(c['q'][c['q_offs'][u]:c['q_offs'][u] + t],
                           r['q'][r['q_offs'][u]:r['q_offs'][u] + t])


@pytest.mark.parametrize('name', sorted(D.STEP_CASES))
def test_step_cases_keep_the_cap(name):
    c = D.make_step_case(**D.STEP_CASES[name])
    ref, e_plain, scale, w = D.step_refs(c)
    print(f'{name}: e_plain={e_plain:.3e} scale={scale:.3e}')
    assert KR.cap_ok(e_plain, scale), (name, e_plain, scale)
    assert c['qkv'].shape == (c['n'], 3 * c['H'] * 32)
    assert int(c['path'][:, :c['length']].max()) < c['n']
    if name.startswith('needle'):
        assert (w > 0.5).double().mean().item() >= 0.9, name


def test_step_case_at_64_is_kernel_refs():
    """The same generator at a head width of 64 gives a case kernel_refs' own reference accepts:
    the layout (qkv, cache, path, gathered rows) is make_self_step_case's."""
    c = D.make_step_case('unit', None, H=2, n=5, length=66, seed=7, dk=64)
    k = dict(c, seqs=[s + (0, ) for s in c['seqs']])
    ref, _, _, _ = KR.self_step_refs(k)
    assert torch.equal(ref, D.step_refs(c)[0])
    # the cache holds what the paths name and the poison elsewhere
    for r in range(c['n']):
        for j in range(c['step']):
            row = c['cache'][j, c['path'][r, j]]
            assert torch.equal(row[:c['d']], c['kg'][r * c['length'] + j])
    assert (c['cache'][c['step']:].abs() == KR.POISON).all()


@pytest.mark.parametrize('name', sorted(D.MODELS))
def test_model_fixtures_load(name):
    meta, arrays = D.load_fixture(name)
    spec = D.MODELS[name]
    assert meta['frames'] == spec['frames'] and meta['config'] == name
    n = len(spec['frames'])
    for mode in D.BEAM_METHODS + tuple(f'attention_b{b}' for b in D.ATTENTION_BEAMS):
        assert len(meta['tokens'][mode]) == n
    for mode in D.BEAM_METHODS:
        assert len(meta['scores'][mode]) == n and len(meta['e_score'][mode]) == n
        assert max(meta['e_score'][mode]) < 1e-4
    for i, f in enumerate(spec['frames']):
        assert arrays[f'enc64_{f}'].shape == (meta['enc_lens'][i], 128)
    ctc, res = meta['tokens']['ctc_prefix_beam_search'], meta['tokens']['attention_rescoring']
    assert sum(len(u) > 0 for u in ctc) >= 3
    assert sum(a != b for a, b in zip(ctc, res)) >= 3      # the decoder decides something
    if spec['long_attention']:                             # the step kernel's second key block
        assert max(len(u) for u in meta['tokens']['attention_b5']) > 64


def test_width_fixture_loads():
    from wenet_amd import synthetic as S
    meta, arrays = D.load_fixture(D.WIDTH_MODEL)
    configs = S.make_configs(D.WIDTH_MODEL)
    hyps, lens, enc = D.width_inputs(configs)
    assert meta['hyps'] == hyps.tolist() and meta['lens'] == lens.tolist()
    assert enc.shape == (1, 31, 256)
    V = configs['output_dim']
    assert arrays['logp_l'].shape == (5 * 9, V) and arrays['logp_r'].shape == (5 * 9, V)
    dc = configs['decoder_conf']
    assert configs['encoder_conf']['output_size'] // dc['attention_heads'] == 32


@pytest.mark.parametrize('name', D.RECIPES)
def test_the_shipped_recipes_have_eight_decoder_heads(name):
    from wenet_amd.efficonformer import efficonformer_config_from_yaml
    from wenet_amd.model import config_from_yaml
    cfg = EF.load_recipe(name)
    cfg.update(input_dim=80, output_dim=4233)
    c, _ = efficonformer_config_from_yaml(cfg)
    assert (c.d_model, c.dec_heads) == (256, 8)
    # config_from_yaml itself, on the recipe's decoder / model sections behind a Conformer encoder
    # section of the same widths
    from wenet_amd import synthetic as S
    base = dict(cfg, encoder='conformer')
    base['encoder_conf'] = dict(S.CONFIGS['aishell_conformer']['encoder_conf'], attention_heads=4)
    b = config_from_yaml(base)
    assert (b.d_model, b.dec_heads, b.dec_layers) == (256, 8, c.dec_layers)


def test_synthetic_configs():
    from wenet_amd import synthetic as S
    for name, heads, d in (('tiny_dec32', 4, 128), ('tiny_efficonformer_v1_dec32', 4, 128),
                           ('aishell_efficonformer_v1_dec8', 8, 256), (D.WIDTH_MODEL, 8, 256)):
        c = S.make_configs(name)
        assert c['decoder'] == 'bitransformer'
        assert c['decoder_conf']['attention_heads'] == heads
        assert c['encoder_conf']['output_size'] == d
    c = S.make_configs('tiny_dec32')
    assert (c['output_dim'], c['decoder_conf']['linear_units'], c['decoder_conf']['num_blocks'],
            c['decoder_conf']['r_num_blocks'], c['model_conf']['reverse_weight']) == \
        (41, 96, 2, 2, 0.3)
    assert c['encoder_conf']['cnn_module_norm'] == 'layer_norm'
    # the 4-head entry the recorded profile was measured on is as it was
    assert S.make_configs('aishell_efficonformer_v1')['decoder_conf']['attention_heads'] == 4


def test_the_header_declares_the_hook_and_the_library_lists_it():
    from wenet_amd import _lib
    with open(os.path.join(ROOT, 'include', 'wenet_amd.h')) as f:
        text = f.read()
    m = re.search(r'int wn_op_attention_d32\(([^;]*)\);', text)
    assert m and 'int32_t mask_mode' in m.group(1)
    d128 = re.search(r'int wn_op_attention_d128\(([^;]*)\);', text).group(1)
    norm = lambda s: re.sub(r'\s+', ' ', s).strip()
    assert norm(m.group(1)) == norm(d128).replace('float scale,', 'float scale, int32_t mask_mode,')
    assert 'wn_op_attention_d32' in _lib.EXPORTS
