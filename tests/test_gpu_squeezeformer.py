"""Squeezeformer through the public interface -- `load_model` on a model directory written from
the fixture's recipe and weights -- against what the reference's own model computed
(tests/golden/squeezeformer/, tools/gen_golden_squeezeformer.py): `tiny_squeezeformer` (conv1d
reduction, the wrapped shift, an eval-mode BatchNorm) and `tiny_squeezeformer_u2pp` (stream
reduction, no shift, causal conv, chunk masks, two decoders), seven utterances of 291, 135, 131,
127, 15, 11 and 7 frames (T' = 72, 33, 32, 31, 3, 2, 1), every one decoded ALONE by the reference.

Encoder tolerance: 8 * e_enc + 16 fp32 ulps of the output scale per utterance, e_enc = the fp32
reference's own max abs error against its fp64 run (recorded).  Scores: 8 * e_score + 16 ulps of
|score| likewise.  Token lists are the reference's, every utterance, every mode.
"""
import copy

import pytest
import torch

import kernel_refs as KR
import squeezeformer_refs as SQ

pytestmark = pytest.mark.gpu

NAMES = sorted(SQ.TINY)
_CASES = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    def get(name):
        if name in _CASES:
            return _CASES[name]
        import yaml
        from wenet_amd import load_model
        from wenet_amd import synthetic as S
        meta, arrays = SQ.load_fixture(name)
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, meta['wseed'])
        d = tmp_path_factory.mktemp(name)
        V = configs['output_dim']
        syms = ['<blank>', '<unk>', '<sos/eos>'] + [f'▁w{i}' for i in range(3, V)]
        (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        (d / 'train.yaml').write_text(yaml.safe_dump(configs))
        torch.save(sd, d / 'final.pt')
        _CASES[name] = dict(meta=meta, arrays=arrays, configs=configs, sd=sd,
                            model=load_model(str(d)), feats=SQ.tiny_features(name))
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
def test_load_model_gives_a_squeezeformer(cases, name):
    from wenet_amd import Squeezeformer
    c = cases(name)
    assert type(c['model']) is Squeezeformer
    q = c['model']._qcfg
    assert (q.reduce_idx, q.recover_idx) == (1, 3)
    assert (q.reduce_kernel, q.do_rel_shift) == ((5, 1) if name == 'tiny_squeezeformer' else (1, 0))


@pytest.mark.parametrize('name', NAMES)
def test_encoder_against_the_fp64_reference(cases, name):
    c = cases(name)
    m, meta = c['model'], c['meta']
    x, lens = _batch(c['feats'])
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == meta['enc_lens'] == SQ.ENC_LENS
    for i, n in enumerate(meta['frames']):
        ref = torch.from_numpy(c['arrays'][f'enc64_{n}'])
        _enc_ok(f'{name} encoder[{n}]', out[i, :ref.shape[0]].double().cpu(), ref,
                meta['e_enc'][i])
        assert (out[i, ref.shape[0]:] == 0).all()


@pytest.mark.parametrize('chunk,left', SQ.CHUNK_CASES)
def test_chunk_masks(cases, chunk, left):
    c = cases('tiny_squeezeformer_u2pp')
    m, meta = c['model'], c['meta']
    idx = [i for i, n in enumerate(meta['frames']) if f'enc64_{n}_c{chunk}_l{left}' in c['arrays']]
    assert len(idx) == 2
    x, lens = _batch([c['feats'][i] for i in idx])
    out, _ = m._forward_encoder(x, lens, chunk, left)
    for j, i in enumerate(idx):
        key = f'{meta["frames"][i]}_c{chunk}_l{left}'
        ref = torch.from_numpy(c['arrays']['enc64_' + key])
        _enc_ok(f'tiny_squeezeformer_u2pp chunk[{key}]', out[j, :ref.shape[0]].double().cpu(), ref,
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
    got = m.decode(list(SQ.METHODS), x, lens, **kw)
    for mode in SQ.METHODS:
        assert [list(r.tokens) for r in got[mode]] == meta['tokens'][mode], mode
    for mode in ('ctc_prefix_beam_search', 'attention_rescoring'):
        for i, r in enumerate(got[mode]):
            _score_ok(f'{name} {mode}[{i}]', float(r.score), meta['scores'][mode][i],
                      meta['e_score'][mode][i])
    # align() and the two-stream pipeline return what plain decode() returns on the same batch
    from wenet_amd.pipeline import DecodePipeline
    with DecodePipeline(m, 2) as pipe:
        par = pipe.decode_many(list(SQ.METHODS), [(x, lens), (x, lens)], **kw)
    for res in par:
        for mode in SQ.METHODS:
            assert [list(r.tokens) for r in res[mode]] == [list(r.tokens) for r in got[mode]]
    labels = [list(r.tokens) for r in got['ctc_greedy_search']]
    keep = [i for i, u in enumerate(labels) if u]
    xa, la = _batch([c['feats'][i] for i in keep])
    for i, a in zip(keep, m.align(xa, la, [labels[i] for i in keep])):
        assert a.ok and list(a.tokens) == labels[i]


@pytest.mark.parametrize('name', sorted(SQ.WIDTH_CASES))
def test_recipe_width_one_block(name):
    """One block at a shipped recipe's widths against the fp64 formulation, at T' = 33, within
    8 * e_plain + 16 ulp (e_plain: the same formulation in fp32)."""
    from wenet_amd import Squeezeformer
    from wenet_amd import synthetic as S
    configs = SQ.width_case_configs(name)
    sd = S.make_state_dict(configs, 2)
    m = Squeezeformer(configs, sd, device='cuda:0')
    f = S.make_features(1, 135, seed=61)[0][0]
    x, lens = _batch([f])
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == [33]
    ref = SQ.block_model_formulation(f, sd, configs)
    plain = SQ.block_model_formulation(f, sd, configs, dtype=torch.float32).double()
    e_plain = (plain - ref).abs().max().item()
    assert KR.cap_ok(e_plain, ref.abs().max().item())
    _enc_ok(f'{name} one block', out[0, :33].double().cpu(), ref, e_plain)


def test_refusals_on_a_live_model(cases):
    import ctypes
    from wenet_amd import Squeezeformer
    from wenet_amd.model import ASRModel
    from wenet_amd.streaming import StreamingRecognizer
    c = cases('tiny_squeezeformer_u2pp')
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
    # an ODD chunk size on a model with a time reduction, naming the argument
    with pytest.raises(NotImplementedError, match='decoding_chunk_size=3'):
        m._forward_encoder(x, lens, 3, -1)
    # the C ABI refuses too, with an error string, and the handle stays usable
    L = m._L
    from wenet_amd import _lib
    enc_lens = _lib.i32p(torch.zeros(1, dtype=torch.int32).numpy())
    xs = x.cuda().contiguous()
    assert L.wn_encode(m._h, xs.data_ptr(), _lib.i32p(lens.numpy()), 1, xs.shape[1], 3, -1, None,
                       enc_lens, None) == -1
    assert b'odd decoding_chunk_size' in L.wn_last_error()
    assert L.wn_model_set_precision(m._h, 1) == -1
    assert b'Squeezeformer handle stays fp32' in L.wn_last_error()
    h = ctypes.c_void_p()
    assert L.wn_stream_create(m._h, 1, 64, 4, 0, ctypes.byref(h), None) == -1
    assert b'does not stream' in L.wn_last_error() and not h.value
    a = m._forward_encoder(x, lens, 4, -1)[0]
    assert torch.isfinite(a).all()
    # the wrapped shift with a chunk mask: the shifting model with use_dynamic_chunk switched on
    s = cases('tiny_squeezeformer')
    configs = copy.deepcopy(s['configs'])
    configs['encoder_conf']['use_dynamic_chunk'] = True
    ms = Squeezeformer(configs, s['sd'], device='cuda:0')
    with pytest.raises(NotImplementedError, match='decoding_chunk_size=4'):
        ms._forward_encoder(x, lens, 4, -1)
    assert L.wn_encode(ms._h, xs.data_ptr(), _lib.i32p(lens.numpy()), 1, xs.shape[1], 4, -1, None,
                       enc_lens, None) == -1
    assert b'do_rel_shift' in L.wn_last_error()
    full = ms._forward_encoder(x, lens)[0]           # full context: what the plain model gives
    assert torch.equal(full.view(torch.int32),
                       s['model']._forward_encoder(x, lens)[0].view(torch.int32))
    # a reduction without a recovery at model creation
    bad = type(m._qcfg).from_buffer_copy(m._qcfg)
    cfg = type(m._cfg).from_buffer_copy(m._cfg)
    h2 = ctypes.c_void_p()
    tensors = (_lib.WnTensor * 1)()
    bad.recover_idx = -1
    assert L.wn_model_create_squeezeformer(ctypes.byref(cfg), ctypes.byref(bad), tensors, 0, 0,
                                           ctypes.byref(h2)) == -1
    assert b'reduce_idx' in L.wn_last_error()
