"""Efficient Conformer through the public interface -- `load_model` on a model directory written
from the fixture's recipe and weights -- against what the reference's own model computed
(tests/golden/efficonformer/, tools/gen_golden_efficonformer.py): `tiny_efficonformer_v1` (conv2d,
heads of 32: W = 96, grouped layers 0 and 1, stride layer 1, the kernel halved behind it, two
decoders) and `tiny_efficonformer_v2` (conv2d2, heads of 64: W = 192, two grouped stride layers,
causal conv, an eval-mode BatchNorm), every utterance decoded ALONE by the reference.

Encoder tolerance: 8 * e_enc + 16 fp32 ulps of the output scale per utterance, e_enc = the fp32
reference's own max abs error against its fp64 run (recorded).  Scores: 8 * e_score + 16 ulps of
|score| likewise.  Token lists are the reference's, every utterance, every mode.
"""
import ctypes

import pytest
import torch

import efficonformer_refs as EF
import kernel_refs as KR

pytestmark = pytest.mark.gpu

NAMES = sorted(EF.TINY)
_CASES = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    def get(name):
        if name in _CASES:
            return _CASES[name]
        import yaml
        from wenet_amd import load_model
        from wenet_amd import synthetic as S
        meta, arrays = EF.load_fixture(name)
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, meta['wseed'])
        d = tmp_path_factory.mktemp(name)
        V = configs['output_dim']
        syms = ['<blank>', '<unk>', '<sos/eos>'] + [f'▁w{i}' for i in range(3, V)]
        (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        (d / 'train.yaml').write_text(yaml.safe_dump(configs))
        torch.save(sd, d / 'final.pt')
        _CASES[name] = dict(meta=meta, arrays=arrays, configs=configs, sd=sd,
                            model=load_model(str(d)), feats=EF.tiny_features(name))
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
def test_load_model_gives_an_efficient_conformer(cases, name):
    from wenet_amd import EfficientConformer
    c = cases(name)
    m = c['model']
    assert type(m) is EfficientConformer
    v1 = name == 'tiny_efficonformer_v1'
    assert m.plan['stride_layers'] == ([1] if v1 else [1, 3])
    assert m.plan['group_layers'] == ([0, 1] if v1 else [1, 3])
    assert m.plan['kernels'] == ([15, 15, 7, 7] if v1 else [15] * 5)
    assert m.plan['rates'] == ([1, 1, 2, 2] if v1 else [1, 1, 2, 2, 4])
    assert m.subsampling_rate() == 8
    e = m._ecfg
    assert (e.front_rate, e.head_dim, e.group_size) == ((4, 32, 3) if v1 else (2, 64, 3))


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


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('case', [0, 1])
def test_chunk_masks(cases, name, case):
    c = cases(name)
    m, meta = c['model'], c['meta']
    chunk, left = EF.TINY[name]['chunk_cases'][case]
    idx = [i for i, n in enumerate(meta['frames']) if f'enc64_{n}_c{chunk}_l{left}' in c['arrays']]
    assert len(idx) == 2
    x, lens = _batch([c['feats'][i] for i in idx])
    out, _ = m._forward_encoder(x, lens, chunk, left)
    for j, i in enumerate(idx):
        key = f'{meta["frames"][i]}_c{chunk}_l{left}'
        ref = torch.from_numpy(c['arrays']['enc64_' + key])
        _enc_ok(f'{name} chunk[{key}]', out[j, :ref.shape[0]].double().cpu(), ref,
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
    got = m.decode(list(EF.METHODS), x, lens, **kw)
    for mode in EF.METHODS:
        assert [list(r.tokens) for r in got[mode]] == meta['tokens'][mode], mode
    for mode in ('ctc_prefix_beam_search', 'attention_rescoring'):
        for i, r in enumerate(got[mode]):
            _score_ok(f'{name} {mode}[{i}]', float(r.score), meta['scores'][mode][i],
                      meta['e_score'][mode][i])
    # align() and the two-stream pipeline return what plain decode() returns on the same batch
    from wenet_amd.pipeline import DecodePipeline
    with DecodePipeline(m, 2) as pipe:
        par = pipe.decode_many(list(EF.METHODS), [(x, lens), (x, lens)], **kw)
    for res in par:
        for mode in EF.METHODS:
            assert [list(r.tokens) for r in res[mode]] == [list(r.tokens) for r in got[mode]]
    labels = [list(r.tokens) for r in got['ctc_greedy_search']]
    keep = [i for i, u in enumerate(labels) if u]
    xa, la = _batch([c['feats'][i] for i in keep])
    for i, a in zip(keep, m.align(xa, la, [labels[i] for i in keep])):
        assert a.ok and list(a.tokens) == labels[i]


def test_recipe_width_one_block():
    """One grouped stride block at the shipped widths (256, 8 heads: W = 96, K 15) against the
    fp64 formulation at T' = 32 and 3, within 8 * e_plain + 16 ulp (e_plain: the same formulation
    in fp32)."""
    from wenet_amd import EfficientConformer
    from wenet_amd import synthetic as S
    from wenet_amd.efficonformer import efficonformer_plan
    configs = EF.width_case_configs()
    sd = S.make_state_dict(configs, 2)
    plan = efficonformer_plan(configs)
    m = EfficientConformer(configs, sd, device='cuda:0')
    feats = [S.make_features(1, n, seed=61 + n)[0][0] for n in (131, 15)]
    x, lens = _batch(feats)
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == [16, 2]
    for i, f in enumerate(feats):
        refs = []
        for dt in (torch.float64, torch.float32):
            x0 = EF.frontend_formulation(f, sd, 256, 4, dt)
            refs.append(EF.encoder_formulation(x0, sd, plan, dtype=dt).double())
        ref, plain = refs
        e_plain = (plain - ref).abs().max().item()
        assert KR.cap_ok(e_plain, ref.abs().max().item())
        _enc_ok(f'one block [{f.shape[0]}]', out[i, :ref.shape[0]].double().cpu(), ref, e_plain)


def test_refusals_on_a_live_model(cases):
    from wenet_amd import _lib
    from wenet_amd.model import ASRModel
    from wenet_amd.streaming import StreamingRecognizer
    c = cases('tiny_efficonformer_v2')
    m = c['model']
    x, lens = _batch(c['feats'][1:2])
    for dt in ('bf16', 'fp8'):
        with pytest.raises(NotImplementedError, match='outside the accelerated path'):
            m.set_compute_dtype(dt)
    with pytest.raises(NotImplementedError, match='Conformer encoders only'):
        m.forward_encoder_chunk(x.cuda(), 0, -1)
    with pytest.raises(NotImplementedError, match='Conformer encoders only'):
        m.forward_encoder_chunk_batch(x.cuda(), [0], -1)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        StreamingRecognizer(m, n_sessions=1, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='simulate_streaming'):
        m.decode(['ctc_greedy_search'], x, lens, simulate_streaming=True, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='global_chunk_size'):
        m.set_global_chunk_size(16)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        ASRModel(c['configs'], c['sd'], device='cuda:0')
    # a chunk mask the product of the strides (4) does not divide, naming the argument
    with pytest.raises(NotImplementedError, match='decoding_chunk_size=6'):
        m._forward_encoder(x, lens, 6, -1)
    # the C ABI refuses too, with an error string, and the handle stays usable
    L = m._L
    enc_lens = _lib.i32p(torch.zeros(1, dtype=torch.int32).numpy())
    xs = x.cuda().contiguous()
    assert L.wn_encode(m._h, xs.data_ptr(), _lib.i32p(lens.numpy()), 1, xs.shape[1], 6, -1, None,
                       enc_lens, None) == -1
    assert b'decoding_chunk_size' in L.wn_last_error()
    assert b'product of the strides' in L.wn_last_error()
    assert L.wn_model_set_precision(m._h, 1) == -1
    assert b'Efficient Conformer handle stays fp32' in L.wn_last_error()
    h = ctypes.c_void_p()
    assert L.wn_stream_create(m._h, 1, 64, 4, 0, ctypes.byref(h), None) == -1
    assert b'does not stream' in L.wn_last_error() and not h.value
    a = m._forward_encoder(x, lens, 8, -1)[0]
    assert torch.isfinite(a).all()
    # model creation: a stride list out of order, a head width without a grouped kernel
    cfg = type(m._cfg).from_buffer_copy(m._cfg)
    tensors = (_lib.WnTensor * 1)()
    for field, value, words in (('stride_layers', (3, 1, 0, 0), b'stride_layers'),
                                ('group_size', 2, b'group_size'),
                                ('front_rate', 6, b'front_rate')):
        bad = type(m._ecfg).from_buffer_copy(m._ecfg)
        if field == 'stride_layers':
            for j, v in enumerate(value):
                bad.stride_layers[j] = v
        else:
            setattr(bad, field, value)
        h2 = ctypes.c_void_p()
        assert L.wn_model_create_efficonformer(ctypes.byref(cfg), ctypes.byref(bad), tensors, 0,
                                               0, ctypes.byref(h2)) == -1
        assert words in L.wn_last_error(), L.wn_last_error()
