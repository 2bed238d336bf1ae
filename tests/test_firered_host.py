"""CPU checks of the FireRedASR-AED encoder kernels' references and host-side contracts
(tests/firered_refs.py; kernels in csrc/firered.hip, GPU tests in tests/test_gpu_firered_ops.py):
the references against what the reference's own modules computed
(tests/golden/firered/firered_modules.npz, tools/gen_golden_firered.py), the LayerNorm fold, the
T' rule, the yardstick caps of every GPU case, and the operator hooks' argument checks (which
need no device)."""
import copy
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import firered_refs as FR
import kernel_refs as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'firered', 'firered_modules.npz'))
    meta = json.loads(bytes(z['meta']).decode('utf8'))
    return meta, {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def test_position_rows_match_the_module(golden):
    meta, arr = golden
    assert meta['attn'] == FR.ATTN_MODULE
    pe = FR.rel_positions(FR.ATTN_MODULE['T'], FR.ATTN_MODULE['d'])
    assert pe.shape == (2 * FR.ATTN_MODULE['T'] - 1, FR.ATTN_MODULE['d'])
    assert torch.equal(pe[FR.POS_ROWS], arr['pos_emb_rows'])
    # row c is the sinusoid of the relative position T - 1 - c: the centre row is position 0
    c = FR.ATTN_MODULE['T'] - 1
    assert torch.equal(pe[c, 0::2], torch.zeros(64, dtype=torch.float64))
    assert torch.equal(pe[c, 1::2], torch.ones(64, dtype=torch.float64))
    assert pe[c - 1, 0] > 0 > pe[c + 1, 0]       # sin(+1), sin(-1)


def test_ref_attention_relshift_matches_the_module(golden):
    """The recorded fp64 output of FiredRelPositionMultiHeadedAttention.forward: pins the
    distance and its sign, the three LayerNorms at eps 1e-5, the missing biases.  The module's
    softmax runs in fp32 even in a .double() model (forward_attention: scores.float()): with the
    softmax restated that way the formulation meets the record within 1e-9 relative; the all-fp64
    reference of the GPU tests is that far from it as fp32 weights are (a convex combination of
    weights that are each within a few 2^-24 relative: 1e-6 relative is 16 such steps)."""
    _, arr = golden
    x, sd = FR.attn_module_inputs()
    out, (q, k, v) = FR.attention_module_formulation(x, sd, FR.ATTN_MODULE['H'], softmax32=True)
    r = _rel(out, arr['attn_out'])
    out64, _ = FR.attention_module_formulation(x, sd, FR.ATTN_MODULE['H'])
    r64 = _rel(out64, arr['attn_out'])
    print(f'attention module: rel err {r:.3e} (fp32 softmax as the module), {r64:.3e} (fp64)')
    assert r <= 1e-9
    assert r64 <= 1e-6
    # the sign matters to this check: the mirrored table misses it by orders of magnitude
    T, d = x.shape
    P = FR.rel_positions(T, d) @ sd['linear_pos.weight'].t()
    wrong = FR.ref_attention_relshift(q, k, v, P.flip(0), T - 1, sd['pos_bias_u'],
                                      sd['pos_bias_v'], [(0, T)]) @ sd['linear_out.weight'].t()
    assert _rel(wrong, arr['attn_out']) > 1e-3


def test_layernorm_fold_is_exact():
    """One plain normalisation + QKV weights W diag(g), biases W b == three LayerNorms + three
    Linears, within 1e-12 relative in fp64."""
    x, sd = FR.attn_module_inputs()
    _, qkv = FR.attention_module_formulation(x, sd, FR.ATTN_MODULE['H'])
    _, qkv_f = FR.attention_module_formulation(x, sd, FR.ATTN_MODULE['H'], fold=True)
    for a, b in zip(qkv_f, qkv):
        assert _rel(a, b) <= 1e-12


def test_rel_shift_index_is_the_modules_view_trick():
    """rel_shift(raw)[i, j] == raw[i, T - 1 - i + j], exhaustively for T = 1 .. 9."""
    for T in range(1, 10):
        raw = torch.arange(2 * T * (2 * T - 1), dtype=torch.float64).view(2, T, 2 * T - 1)
        got = FR.module_rel_shift(raw)
        i = torch.arange(T).unsqueeze(1)
        j = torch.arange(T).unsqueeze(0)
        want = torch.gather(raw, 2, (T - 1 - i + j).unsqueeze(0).expand(2, T, T))
        assert torch.equal(got, want), T


def test_ref_attention_relshift_equals_the_query_loops():
    case = FR.make_relshift_case(H=2, lens=[1, 5, 33], seed=11, t_table=40)
    a = FR.ref_attention_relshift(case['q'], case['k'], case['v'], case['P'], case['p_center'],
                                  case['bias_u'], case['bias_v'], case['seqs'])
    b = FR.ref_attention_relshift_loops(case)
    assert (a - b).abs().max().item() <= 1e-12
    assert (a[~case['own']] == 0).all()


@pytest.mark.parametrize('name', sorted(FR.RELSHIFT_CASES))
def test_relshift_case_yardsticks(name):
    """The plain fp32 evaluation stays inside the cap of the GPU rule (kernel_refs.cap_ok) on
    every case of tests/test_gpu_firered_ops.py, and the steered cases are not flat."""
    kw = FR.RELSHIFT_CASES[name]
    case = FR.make_relshift_case(**kw)
    ref, e_plain, scale, w = FR.relshift_refs(case)
    print(f'{name}: e_plain={e_plain:.3e} scale={scale:.3e} bound={KR.bound(e_plain, scale):.3e}')
    assert torch.isfinite(ref).all()
    assert KR.cap_ok(e_plain, scale)
    if kw.get('regime') == 'peaked':
        assert (w > 0.5).double().mean().item() >= 0.5
    if kw.get('neg_only'):
        # the mirrored distance must miss the bound by far: the case can tell the sign
        P = case['P']
        wrong = FR.ref_attention_relshift(case['q'], case['k'], case['v'], P.flip(0),
                                          case['p_center'], case['bias_u'], case['bias_v'],
                                          case['seqs'])
        own = case['own']
        assert (wrong[own] - ref[own]).abs().max().item() > 1000 * KR.bound(e_plain, scale)
        # and so must a band shifted by one row
        off1 = FR.ref_attention_relshift(case['q'], case['k'], case['v'], P.roll(1, 0),
                                         case['p_center'], case['bias_u'], case['bias_v'],
                                         case['seqs'])
        assert (off1[own] - ref[own]).abs().max().item() > 1000 * KR.bound(e_plain, scale)


def test_frontend_reference_and_length_rule(golden):
    """ref_firered_frontend + the output projection == FireRedConv2dSubsampling4.forward of each
    utterance ALONE; the reference's batched mask gives the shorter one a frame more (recorded
    as data: 17 against 16 for 61 frames next to 97)."""
    meta, arr = golden
    assert meta['front'] == FR.FRONT_MODULE
    c, w, b = FR.frontend_module_inputs()
    outs = FR.ref_firered_frontend(c['feats'], c['lens'], None, None, c['w1'], c['b1'], c['w2'],
                                   c['b2'])
    for n, o in zip(c['lens'], outs):
        want = arr[f'front_alone_{n}']
        assert o.shape[0] == FR.firered_out_len(n) == want.shape[0]
        assert _rel(o @ w.double().t() + b.double(), want) <= 1e-9
    assert meta['alone_lens'] == [25, 16] == [FR.firered_out_len(n) for n in c['lens']]
    assert meta['batched_lens'] == [25, 17]
    # one input frame already yields an output frame (1 + 6 zero frames); 7 is the shortest for
    # the Conformer's Conv2dSubsampling4, not here
    assert [FR.firered_out_len(n) for n in (0, 1, 2, 3, 7, 290)] == [0, 1, 1, 1, 2, 73]


def test_frontend_case_yardstick():
    c = FR.make_frontend_case(FR.FRONTEND_LENS, seed=5)
    ref, e_plain, scale = FR.frontend_refs(c)
    print(f'frontend: e_plain={e_plain:.3e} scale={scale:.3e}')
    assert KR.cap_ok(e_plain, scale)
    assert [r.shape[0] for r in ref] == [FR.firered_out_len(n) for n in FR.FRONTEND_LENS]
    # alone == batched by construction of the reference; padding frames are never read
    one = FR.ref_firered_frontend(c['feats'][1:2, :61], [61], c['mean'], c['istd'], c['w1'],
                                  c['b1'], c['w2'], c['b2'])
    assert torch.equal(one[0], ref[1])


def test_config_from_yaml_still_refuses_firered():
    from wenet_amd import synthetic as S
    from wenet_amd.model import config_from_yaml
    configs = S.make_configs('tiny_sym')
    configs['model'] = 'firered'
    with pytest.raises(NotImplementedError):
        config_from_yaml(configs)


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
    for name in ('wn_op_attention_relshift', 'wn_op_firered_frontend'):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert len(_declared(src, name)) == len(getattr(L, name).argtypes), name
    # wn_config is what it was: the new operators take no handle and add no field
    assert _lib.WnConfig._fields_[-1][0] == 'dec_max_pos'
    assert ctypes.sizeof(_lib.WnConfig) == 4 * 30

    i32 = lambda *v: np.asarray(v, dtype=np.int32)
    one = ctypes.c_void_p(64)          # a non-null pointer no accepted call would reach

    def relshift(off, ln, rows=8, p_rows=15, p_center=7, ld=128, heads=2, Q=one):
        return L.wn_op_attention_relshift(Q, one, one, ld, ld, ld, rows, one, ld, p_rows,
                                          p_center, one, one, one, ld, _lib.i32p(off),
                                          _lib.i32p(ln), len(off), heads, 0.125, None)

    err = lambda: L.wn_last_error().decode()
    assert relshift(i32(0), i32(8), Q=None) == -1 and 'null' in err()
    assert relshift(i32(0), i32(9)) == -1 and 'outside the buffer' in err()
    assert relshift(i32(0, 2), i32(4, 4)) == -1 and 'overlapping' in err()
    assert relshift(i32(0), i32(8), ld=126) == -1 and 'multiples of 4' in err()
    assert relshift(i32(0), i32(8), ld=64) == -1 and 'smaller than n_heads' in err()
    assert relshift(i32(0), i32(0)) == -1 and 'empty' in err()
    # a table that does not hold every distance of the longest sequence, on either side
    assert relshift(i32(0), i32(8), p_center=6) == -1 and 'position table' in err()
    assert relshift(i32(0), i32(8), p_rows=14) == -1 and 'position table' in err()

    def front(lens, off, rows=4, T=16, F=80, C=32, ldo=32 * 19, feats=one):
        out_len = np.zeros(len(lens), dtype=np.int32)
        r = L.wn_op_firered_frontend(feats, None, None, one, one, one, one, one, ldo, rows,
                                     _lib.i32p(lens), _lib.i32p(off), _lib.i32p(out_len),
                                     len(lens), T, F, C, None)
        return r, out_len

    assert front(i32(16), i32(0), feats=None)[0] == -1 and 'null' in err()
    assert front(i32(17), i32(0))[0] == -1 and 'outside [0, T]' in err()
    assert front(i32(16), i32(0), ldo=32 * 19 - 1)[0] == -1 and 'stride' in err()
    assert front(i32(16), i32(0), F=6)[0] == -1
    assert FR.firered_out_len(20) == 5 and FR.firered_out_len(11) == 3
    r, out_len = front(i32(20), i32(0), T=20)    # 20 frames -> 5 rows, 4 given
    assert r == -1 and 'outside the buffer' in err() and out_len[0] == 5
    r, out_len = front(i32(11, 11), i32(0, 2), rows=8)   # 3 rows each from offsets 0 and 2
    assert r == -1 and 'overlapping' in err() and list(out_len) == [3, 3]
    assert front(i32(0), i32(0))[0] == -1 and 'empty' in err()


# ---------------------------------------------------------------------------------------------
# the model: recipe, refusals, the whole-encoder formulation against the recorded reference


@pytest.fixture(scope='module')
def tiny():
    from wenet_amd import synthetic as S
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'firered', 'firered_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode('utf8'))
    configs = S.make_configs(meta['config'])
    return meta, configs, {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}


def test_encoder_formulation_matches_the_recorded_reference(tiny):
    """firered_encoder_formulation (folded QKV; the softmax in fp32 as the reference's
    forward_attention has it) == the reference's .double() encoder output of the utterances the
    fixture carries, within 1e-9 relative; T' as recorded."""
    from wenet_amd import synthetic as S
    meta, configs, arr = tiny
    assert dict(FR.TINY) == {k: meta[k] for k in FR.TINY}
    sd = S.make_state_dict(configs, meta['wseed'])
    feats = FR.tiny_features()
    assert meta['enc_lens'] == [FR.firered_out_len(f.shape[0]) for f in feats] == [73, 33, 32, 31]
    z3 = np.load(os.path.join(ROOT, 'tests', 'golden', 'firered', 'firered_tiny_enc3.npz'))
    assert json.loads(bytes(z3['meta']).decode('utf8'))['wseed'] == meta['wseed']
    arr = dict(arr, **{k: torch.from_numpy(z3[k]) for k in z3.files if k != 'meta'})
    for n in FR.RECORDED_ENC + (FR.RECORDED_ENC_3TILE, ):
        f = feats[meta['frames'].index(n)]
        got = FR.firered_encoder_formulation(f, sd, configs)
        r = _rel(got, arr[f'enc64_{n}'])
        print(f'encoder formulation[{n}]: rel err {r:.3e}')
        assert r <= 1e-9
    # the fixture's decode lists are not degenerate and carry the recipe's special tokens
    assert meta['special_tokens'] == {'sos': 3, 'eos': 4}
    for i in range(len(feats)):
        assert len(set(t for b in meta['beams'] for t in meta['tokens'][f'attention/{b}'][i])) >= 3


def test_recipe_is_accepted_and_every_other_value_refused():
    from wenet_amd import synthetic as S
    from wenet_amd.firered import firered_config_from_yaml, out_len
    from wenet_amd.model import config_from_yaml
    for name, (d, H, ffn, nl, V) in (('tiny_firered', (128, 2, 256, 2, 41)),
                                      ('firered_aed_l', (1280, 20, 5120, 16, 7832)),
                                      ('firered_aed_l_1blk', (1280, 20, 5120, 1, 41))):
        configs = S.make_configs(name)
        c, f = firered_config_from_yaml(configs)
        assert (c.d_model, c.n_heads, c.ffn_dim, c.n_layers, c.dec_layers, c.vocab) == \
            (d, H, ffn, nl, nl, V)
        assert (c.cnn_kernel, c.cnn_norm, c.sos, c.eos, c.bidirectional) == (33, 0, 3, 4, 0)
        assert (c.dec_activation, c.dec_key_bias, c.dec_src_key_bias, c.dec_learned_pos) == \
            (1, 1, 1, 0)
        assert (f.sub_channels, f.conv_inner_factor) == (32, 4) and f.max_frames >= 1
        assert abs(f.attn_norm_eps - 1e-5) < 1e-12
        with pytest.raises(NotImplementedError, match='outside the accelerated path'):
            config_from_yaml(configs)
    assert [out_len(n) for n in (0, 1, 61, 97, 290)] == [0, 1, 16, 25, 73]
    base = S.make_configs('tiny_firered')
    ignored = copy.deepcopy(base)
    ignored['encoder_conf'].update(use_sdpa=True, gradient_checkpointing=False)
    firered_config_from_yaml(ignored)
    bad = [('encoder_conf', 'input_layer', 'conv2d'), ('encoder_conf', 'pos_enc_layer_type', 'rel_pos'),
           ('encoder_conf', 'selfattention_layer_type', 'rel_selfattn'),
           ('encoder_conf', 'final_norm', True), ('encoder_conf', 'query_bias', True),
           ('encoder_conf', 'key_bias', True), ('encoder_conf', 'value_bias', True),
           ('encoder_conf', 'conv_bias', True), ('encoder_conf', 'conv_inner_factor', 2),
           ('encoder_conf', 'cnn_module_norm', 'batch_norm'),
           ('encoder_conf', 'activation_type', 'relu'), ('encoder_conf', 'macaron_style', False),
           ('encoder_conf', 'causal', True), ('encoder_conf', 'use_dynamic_chunk', True),
           ('encoder_conf', 'static_chunk_size', 16), ('encoder_conf', 'cnn_module_kernel', 32),
           ('encoder_conf', 'attention_heads', 4),
           ('decoder_conf', 'activation_type', 'relu'),
           ('decoder_conf', 'tie_word_embedding', False), ('decoder_conf', 'key_bias', True),
           ('decoder_conf', 'src_key_bias', True),
           ('decoder_conf', 'input_layer', 'embed_learnable_pe')]
    for sec, k, v in bad:
        c2 = copy.deepcopy(base)
        c2[sec][k] = v
        with pytest.raises(NotImplementedError, match='outside the accelerated path') as e:
            firered_config_from_yaml(c2)
        assert k.split('_')[0] in str(e.value), (k, str(e.value))
    for k, v in (('model', 'asr_model'), ('encoder', 'conformer'), ('decoder', 'bitransformer')):
        c2 = copy.deepcopy(base)
        c2[k] = v
        with pytest.raises(NotImplementedError, match=k):
            firered_config_from_yaml(c2)
    c2 = copy.deepcopy(base)
    c2['tokenizer_conf']['special_tokens'] = {'<sos>': 3}
    with pytest.raises(NotImplementedError, match='special_tokens'):
        firered_config_from_yaml(c2)


def test_firered_config_layout_and_entry_point():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'typedef struct\s*\{([^}]*)\}\s*wn_firered_config\s*;', src)
    assert m
    declared = []
    for decl in filter(None, (x.strip() for x in m.group(1).split(';'))):
        typ, names = decl.split(None, 1)
        declared += [(typ, n.strip()) for n in names.split(',')]
    assert [n for _, n in declared] == [n for n, _ in _lib.WnFireRedConfig._fields_] == \
        ['sub_channels', 'conv_inner_factor', 'max_frames', 'attn_norm_eps']
    for (typ, n), (_, ct) in zip(declared, _lib.WnFireRedConfig._fields_):
        assert ct is (ctypes.c_float if typ == 'float' else ctypes.c_int32), n
    assert ctypes.sizeof(_lib.WnFireRedConfig) == 16
    assert hasattr(L, 'wn_model_create_firered') and 'wn_model_create_firered' in _lib.EXPORTS
    assert len(_declared(src, 'wn_model_create_firered')) == \
        len(L.wn_model_create_firered.argtypes)
    assert L.wn_model_create_firered(None, None, None, 0, 0, None) == -1
    assert b'null' in L.wn_last_error()


def test_firered_refuses_cpu_device_and_load_model_routes(tmp_path, monkeypatch):
    import yaml
    from wenet_amd import FireRed
    from wenet_amd import model as M
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_firered')
    with pytest.raises(RuntimeError, match='needs a GPU device'):
        FireRed(configs, {}, device='cpu')
    (tmp_path / 'units.txt').write_text('<blank> 0\n')
    (tmp_path / 'train.yaml').write_text(yaml.safe_dump(configs))
    torch.save({'encoder.global_cmvn.mean': torch.zeros(80),
                'encoder.global_cmvn.istd': torch.ones(80)}, tmp_path / 'final.pt')
    seen = {}

    def fake_init(self, configs, sd, device='cuda'):
        seen['cls'] = type(self).__name__

    monkeypatch.setattr(FireRed, '__init__', fake_init)
    M.load_model(str(tmp_path))
    assert seen['cls'] == 'FireRed'
