"""Branchformer / E-Branchformer through the public interface -- `load_model` on a model directory
written from the fixture's recipe and weights -- against what the reference's own model computed
(tests/golden/branchformer/, tools/gen_golden_branchformer.py): `tiny_ebranchformer` (d_k = 32
through zero-padded heads, non-causal convs of 31 taps) and `tiny_branchformer` (causal cgMLP,
chunk masks, two decoders), five utterances of 291, 135, 131, 127 and 15 frames (T' = 72, 33, 32,
31, 3), every one decoded ALONE by the reference.

Encoder tolerance: 8 * e_enc + 16 fp32 ulps of the output scale per utterance, e_enc = the fp32
reference's own max abs error against its fp64 run (recorded).  Scores: 8 * e_score + 16 ulps of
|score| likewise.  Token lists are the reference's, every utterance, every mode.
"""
import copy

import numpy as np
import pytest
import torch

import branchformer_refs as BR
import kernel_refs as KR

pytestmark = pytest.mark.gpu

NAMES = sorted(BR.TINY)
_CASES = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    def get(name):
        if name in _CASES:
            return _CASES[name]
        import yaml
        from wenet_amd import load_model
        from wenet_amd import synthetic as S
        meta, arrays = BR.load_fixture(name)
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, meta['wseed'])
        d = tmp_path_factory.mktemp(name)
        V = configs['output_dim']
        syms = ['<blank>', '<unk>', '<sos/eos>'] + [f'▁w{i}' for i in range(3, V)]
        (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        (d / 'train.yaml').write_text(yaml.safe_dump(configs))
        torch.save(sd, d / 'final.pt')
        _CASES[name] = dict(meta=meta, arrays=arrays, configs=configs, sd=sd,
                            model=load_model(str(d)), feats=BR.tiny_features(name))
        return _CASES[name]
    yield get
    _CASES.clear()


def _batch(feats):
    T = max(f.shape[0] for f in feats)
    x = torch.full((len(feats), T, feats[0].shape[1]), KR.POISON)
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    return x, torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)


def _enc_ok(name, got, ref, e_ref):
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    bound = 8 * e_ref + 16 * KR.ULP32 * scale
    print(f'{name}: err={err:.3e} e_ref={e_ref:.3e} scale={scale:.3e} bound={bound:.3e}')
    assert torch.isfinite(got).all(), name
    assert err <= bound, name


@pytest.mark.parametrize('name', NAMES)
def test_load_model_gives_a_branchformer(cases, name):
    from wenet_amd import Branchformer
    c = cases(name)
    assert type(c['model']) is Branchformer
    assert c['model']._bcfg.head_dim == (32 if name == 'tiny_ebranchformer' else 64)


@pytest.mark.parametrize('name', NAMES)
def test_encoder_against_the_fp64_reference(cases, name):
    c = cases(name)
    m, meta = c['model'], c['meta']
    x, lens = _batch(c['feats'])
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == meta['enc_lens']
    for i, n in enumerate(meta['frames']):
        ref = torch.from_numpy(c['arrays'][f'enc64_{n}'])
        _enc_ok(f'{name} encoder[{n}]', out[i, :ref.shape[0]].double().cpu(), ref,
                meta['e_enc'][i])
        assert (out[i, ref.shape[0]:] == 0).all()


@pytest.mark.parametrize('chunk,left', BR.CHUNK_CASES)
def test_chunk_masks(cases, chunk, left):
    c = cases('tiny_branchformer')
    m, meta = c['model'], c['meta']
    idx = [i for i, n in enumerate(meta['frames']) if f'enc64_{n}_c{chunk}_l{left}' in c['arrays']]
    assert len(idx) == 2
    x, lens = _batch([c['feats'][i] for i in idx])
    out, _ = m._forward_encoder(x, lens, chunk, left)
    for j, i in enumerate(idx):
        key = f'{meta["frames"][i]}_c{chunk}_l{left}'
        ref = torch.from_numpy(c['arrays']['enc64_' + key])
        _enc_ok(f'tiny_branchformer chunk[{key}]', out[j, :ref.shape[0]].double().cpu(), ref,
                meta['e_enc_chunk'][key])


@pytest.mark.parametrize('name', NAMES)
def test_batched_equals_alone_and_clone_bit_for_bit(cases, name):
    c = cases(name)
    m = c['model']
    feats = c['feats']
    x, lens = _batch(feats)
    out = m._forward_encoder(x, lens)[0].clone()
    xr, lr = _batch(feats[::-1])
    out_r = m._forward_encoder(xr, lr)[0].clone()
    twin = m.clone()
    out_c = twin._forward_encoder(x, lens)[0].clone()
    assert torch.equal(out_c.view(torch.int32), out.view(torch.int32))
    for i, f in enumerate(feats):
        o1 = m._forward_encoder(f.unsqueeze(0), torch.tensor([f.shape[0]]))[0]
        n = o1.shape[1]
        assert torch.equal(o1[0].view(torch.int32), out[i, :n].view(torch.int32)), i
        assert torch.equal(o1[0].view(torch.int32),
                           out_r[len(feats) - 1 - i, :n].view(torch.int32)), i


def _score_ok(name, got, want, e):
    bound = 8 * e + 16 * KR.ULP32 * abs(want)
    print(f'{name}: got={got:.6f} ref={want:.6f} e_score={e:.3e} bound={bound:.3e}')
    assert abs(got - want) <= bound, name


@pytest.mark.parametrize('name', NAMES)
def test_tokens_and_scores_are_the_references(cases, name):
    c = cases(name)
    m, meta = c['model'], c['meta']
    x, lens = _batch(c['feats'])
    kw = dict(beam_size=meta['ctc_beam'], ctc_weight=meta['rescore_ctc_weight'],
              reverse_weight=meta['reverse_weight'])
    got = m.decode(list(BR.METHODS), x, lens, **kw)
    for mode in BR.METHODS:
        assert [list(r.tokens) for r in got[mode]] == meta['tokens'][mode], mode
    for mode in ('ctc_prefix_beam_search', 'attention_rescoring'):
        for i, r in enumerate(got[mode]):
            _score_ok(f'{name} {mode}[{i}]', float(r.score), meta['scores'][mode][i],
                      meta['e_score'][mode][i])
    # align() and the two-stream pipeline return what plain decode() returns on the same batch
    from wenet_amd.pipeline import DecodePipeline
    with DecodePipeline(m, 2) as pipe:
        par = pipe.decode_many(list(BR.METHODS), [(x, lens), (x, lens)], **kw)
    for res in par:
        for mode in BR.METHODS:
            assert [list(r.tokens) for r in res[mode]] == [list(r.tokens) for r in got[mode]]
            assert np.allclose([r.score for r in res[mode]], [r.score for r in got[mode]],
                               rtol=0, atol=1e-5)
    labels = [list(r.tokens) for r in got['ctc_greedy_search']]
    keep = [i for i, u in enumerate(labels) if u]
    xa, la = _batch([c['feats'][i] for i in keep])
    for i, a in zip(keep, m.align(xa, la, [labels[i] for i in keep])):
        assert a.ok and list(a.tokens) == labels[i]
        path = [t for j, t in enumerate(a.alignment) if t != 0 and (j == 0 or a.alignment[j - 1] != t)]
        assert path == labels[i], i


def _one_block(base, frames, **encoder_conf):
    """One block of the configuration `base` against the fp64 formulation, e_plain bound."""
    from wenet_amd import Branchformer
    from wenet_amd import synthetic as S
    configs = S.make_configs(base)
    configs['encoder_conf'].update(encoder_conf, num_blocks=1)
    configs['decoder_conf'].update(num_blocks=1)
    if 'r_num_blocks' in configs['decoder_conf']:
        configs['decoder_conf']['r_num_blocks'] = 1
    configs['output_dim'] = 41
    sd = S.make_state_dict(configs, 2)
    m = Branchformer(configs, sd, device='cuda:0')
    feats = [S.make_features(1, n, seed=60 + i)[0][0] for i, n in enumerate(frames)]
    x, lens = _batch(feats)
    out, mask = m._forward_encoder(x, lens)
    for i, f in enumerate(feats):
        ref = BR.encoder_formulation(f, sd, configs, softmax32=False)
        plain = BR.encoder_formulation(f, sd, configs, softmax32=False,
                                       dtype=torch.float32).double()
        e_plain = (plain - ref).abs().max().item()
        assert KR.cap_ok(e_plain, ref.abs().max().item())
        _enc_ok(f'{base} one block[{f.shape[0]}]', out[i, :ref.shape[0]].double().cpu(), ref,
                e_plain)
    assert mask.squeeze(1).sum(1).tolist() == [72, 33]


def test_ebranchformer_recipe_width_one_block():
    """d 256, 8 heads (d_k 32), cgMLP 1024, K 31, merge 31; T' 72 and 33."""
    _one_block('aishell_ebranchformer', (291, 135))


def test_branchformer_recipe_width_one_block():
    """d 256, 4 heads, cgMLP 2048 (1024 gate channels), K 63, causal."""
    _one_block('aishell_u2pp_branchformer', (291, 135))


@pytest.mark.parametrize('name', NAMES)
def test_linear_after_conv(name):
    """use_linear_after_conv: csgu_gate stops behind the conv, the Linear runs, csgu_mul gates."""
    _one_block(name, (291, 135), use_linear_after_conv=True)


def test_refusals_on_a_live_model(cases):
    import ctypes
    from wenet_amd import _lib
    from wenet_amd.model import ASRModel
    from wenet_amd.streaming import StreamingRecognizer
    c = cases('tiny_branchformer')
    m = c['model']
    x, lens = _batch(c['feats'][1:2])
    for dt in ('bf16', 'fp8'):
        with pytest.raises(NotImplementedError, match='outside the accelerated path'):
            m.set_compute_dtype(dt)
    with pytest.raises(NotImplementedError, match='Conformer encoders only'):
        m.forward_encoder_chunk(x.cuda(), 0, -1)
    with pytest.raises(NotImplementedError, match='Conformer encoders only'):
        m.forward_encoder_chunk_batch(x.cuda(), [0], -1)
    with pytest.raises(NotImplementedError, match='Conformer encoders only'):
        StreamingRecognizer(m, n_sessions=1, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        m.decode(['ctc_greedy_search'], x, lens, simulate_streaming=True, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        ASRModel(c['configs'], c['sd'], device='cuda:0')
    # the C ABI refuses too, with an error string
    L = m._L
    assert L.wn_model_set_precision(m._h, 1) == -1
    assert b'Branchformer handle stays fp32' in L.wn_last_error()
    h = ctypes.c_void_p()
    assert L.wn_stream_create(m._h, 1, 64, 4, 0, ctypes.byref(h), None) == -1
    assert b'does not stream' in L.wn_last_error() and not h.value
    xs = x.cuda().contiguous()
    out = torch.zeros(4, m._cfg.d_model, device='cuda')
    zero = np.zeros(1, dtype=np.int32)
    ci, co = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.wn_encode_chunk_batch(m._h, 1, xs.data_ptr(), 23, _lib.i32p(zero), -1, None,
                                   _lib.i32p(zero), None, out.data_ptr(), None, None,
                                   ctypes.byref(ci), ctypes.byref(co), None) == -1
    assert b'Branchformer' in L.wn_last_error()
    # a head width without a kernel and a gate width past the kernel's, at model creation
    bad = type(m._bcfg).from_buffer_copy(m._bcfg)
    cfg = type(m._cfg).from_buffer_copy(m._cfg)
    h2 = ctypes.c_void_p()
    tensors = (_lib.WnTensor * 1)()
    bad.head_dim = 16
    assert L.wn_model_create_branchformer(ctypes.byref(cfg), ctypes.byref(bad), tensors, 0, 0,
                                          ctypes.byref(h2)) == -1
    assert b'32 or 64' in L.wn_last_error()
    bad.head_dim, bad.cgmlp_units = 64, 4096
    assert L.wn_model_create_branchformer(ctypes.byref(cfg), ctypes.byref(bad), tensors, 0, 0,
                                          ctypes.byref(h2)) == -1
    assert b'multiple of 64 up to 1024' in L.wn_last_error()
    # and the handle still encodes
    m._forward_encoder(x, lens)
