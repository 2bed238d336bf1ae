"""Models whose decoders have heads of 32 (4 heads at 128, 8 at 256: csrc/attention_d32.hip and the
d_k = 32 step kernel behind the decoder driver) through the public interface, against what the
reference's own model computed (tests/golden/dec32/, tools/gen_golden_dec32.py): `tiny_dec32` (a
Conformer under two decoders of 4 heads) and `tiny_efficonformer_v1_dec32`, every utterance decoded
ALONE by the reference, and the one-block model at the shipped widths.

Encoder tolerance: 8 * e_enc + 16 fp32 ulps of the output scale per utterance (this guards the
fixture, not new code).  Scores: 8 * e_score + 16 ulps of |score|; log-probs: 8 * e_logp + 16 ulps
of the largest |log-prob|.  Token lists are the reference's, every utterance, every mode.

The fixtures hold every utterance decoded ALONE, and the comparisons with them decode every
utterance alone too: a non-causal Conformer in a padded batch computes what the reference computes
on that BATCH (its conv module lets the biased padding frames into an utterance's last frames,
DESIGN 1), which is not what it computes on the utterance alone.  The Efficient Conformer encodes
every utterance of a batch as the reference encodes it alone, so there the whole batch is held to
the bits of the single decodes; on `tiny_dec32` the utterance without padding is.
"""
import ctypes

import pytest
import torch

import attention_d32_refs as D
import kernel_refs as KR

pytestmark = pytest.mark.gpu

NAMES = sorted(D.MODELS)
MODES = D.BEAM_METHODS
_CASES = {}


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    def get(name):
        if name in _CASES:
            return _CASES[name]
        import yaml
        from wenet_amd import load_model
        from wenet_amd import synthetic as S
        meta, arrays = D.load_fixture(name)
        configs = S.make_configs(name)
        sd = S.make_state_dict(configs, meta['wseed'])
        d = tmp_path_factory.mktemp(name)
        V = configs['output_dim']
        syms = ['<blank>', '<unk>', '<sos/eos>'] + [f'▁w{i}' for i in range(3, V)]
        (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        (d / 'train.yaml').write_text(yaml.safe_dump(configs))
        torch.save(sd, d / 'final.pt')
        model = load_model(str(d))
        feats = D.model_features(name)
        x, lens = _batch(feats)
        kw = dict(beam_size=meta['ctc_beam'], ctc_weight=meta['rescore_ctc_weight'],
                  reverse_weight=meta['reverse_weight'])
        _CASES[name] = dict(meta=meta, arrays=arrays, configs=configs, sd=sd, model=model,
                            feats=feats, x=x, lens=lens, kw=kw,
                            got=model.decode(list(MODES), x, lens, **kw),
                            alone=_decode_each(model, list(MODES), feats, **kw))
        return _CASES[name]
    yield get
    _CASES.clear()


def _batch(feats):
    T = max(f.shape[0] for f in feats)
    x = torch.full((len(feats), T, feats[0].shape[1]), KR.POISON)
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    return x, torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)


def _decode_each(model, modes, feats, **kw):
    """{mode: [the result of utterance i decoded alone]}"""
    out = {m: [] for m in modes}
    for f in feats:
        n = torch.tensor([f.shape[0]], dtype=torch.int32)
        r = model.decode(modes, f.unsqueeze(0), n, **kw)
        for m in modes:
            out[m].append(r[m][0])
    return out


def _tokens(results):
    return [list(r.tokens) for r in results]


@pytest.mark.parametrize('name', NAMES)
def test_models_load(cases, name):
    from wenet_amd import EfficientConformer
    from wenet_amd.model import ASRModel
    m = cases(name)['model']
    assert type(m) is (ASRModel if name == 'tiny_dec32' else EfficientConformer)
    assert (m._cfg.d_model, m._cfg.dec_heads, m._cfg.bidirectional) == (128, 4, 1)


@pytest.mark.parametrize('name', NAMES)
def test_encoder_against_the_fp64_reference(cases, name):
    c = cases(name)
    m, meta = c['model'], c['meta']
    for i, n in enumerate(meta['frames']):
        out, mask = m._forward_encoder(c['feats'][i].unsqueeze(0),
                                       torch.tensor([n], dtype=torch.int32))
        assert int(mask.sum()) == meta['enc_lens'][i]
        ref = torch.from_numpy(c['arrays'][f'enc64_{n}'])
        got = out[0, :ref.shape[0]].double().cpu()
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        bound = 8 * meta['e_enc'][i] + 16 * KR.ULP32 * scale
        print(f'{name} encoder[{n}]: err={err:.3e} e_enc={meta["e_enc"][i]:.3e} bound={bound:.3e}')
        assert torch.isfinite(got).all() and err <= bound


def _score_ok(name, got, want, e):
    bound = 8 * e + 16 * KR.ULP32 * abs(want)
    print(f'{name}: got={got:.6f} ref={want:.6f} e_score={e:.3e} bound={bound:.3e}')
    assert abs(got - want) <= bound, name


@pytest.mark.parametrize('name', NAMES)
def test_beam_modes_are_the_references(cases, name):
    c = cases(name)
    meta, got = c['meta'], c['alone']
    for mode in MODES:
        assert _tokens(got[mode]) == meta['tokens'][mode], mode
        for i, r in enumerate(got[mode]):
            _score_ok(f'{name} {mode}[{i}]', float(r.score), meta['scores'][mode][i],
                      meta['e_score'][mode][i])


@pytest.mark.parametrize('beam', D.ATTENTION_BEAMS)
@pytest.mark.parametrize('name', NAMES)
def test_attention_mode_is_the_references(cases, name, beam):
    """The `attention` beam search: the step kernel at d_k = 32 (two key blocks on the 72 encoder
    frames of tiny_dec32's longest utterance), cross attention on attention_d32."""
    c = cases(name)
    got = _decode_each(c['model'], ['attention'], c['feats'], beam_size=beam)['attention']
    assert _tokens(got) == c['meta']['tokens'][f'attention_b{beam}']
    batched = c['model'].decode(['attention'], c['x'], c['lens'], beam_size=beam)['attention']
    # (a batch decodes every utterance up to the LONGEST one's frames, as the reference's search
    # does; only the longest utterance has the length limit it has alone)
    assert list(batched[0].tokens) == list(got[0].tokens)
    if D.MODELS[name]['long_attention']:
        assert max(len(r.tokens) for r in got) > 64


@pytest.mark.parametrize('name', NAMES)
def test_batched_equals_alone_bit_for_bit(cases, name):
    """Every utterance of the Efficient Conformer batch, and the utterance without padding of the
    Conformer batch (see the head of this file): tokens and the bits of the scores."""
    c = cases(name)
    got, alone = c['got'], c['alone']
    for i in (range(len(c['feats'])) if name != 'tiny_dec32' else [0]):
        for mode in MODES:
            assert list(alone[mode][i].tokens) == list(got[mode][i].tokens), (mode, i)
            a = torch.tensor([float(alone[mode][i].score)], dtype=torch.float64)
            b = torch.tensor([float(got[mode][i].score)], dtype=torch.float64)
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (mode, i)


@pytest.mark.parametrize('name', NAMES)
def test_clone_and_pipeline_return_what_decode_returns(cases, name):
    from wenet_amd.pipeline import DecodePipeline
    c = cases(name)
    m, got = c['model'], c['got']
    twin = m.clone().decode(list(MODES), c['x'], c['lens'], **c['kw'])
    with DecodePipeline(m, 2) as pipe:
        par = pipe.decode_many(list(MODES), [(c['x'], c['lens']), (c['x'], c['lens'])], **c['kw'])
    for res in [twin] + list(par):
        for mode in MODES:
            assert _tokens(res[mode]) == _tokens(got[mode]), mode
            assert [float(r.score) for r in res[mode]] == [float(r.score) for r in got[mode]], mode


def test_streaming_finish_is_the_rescoring_of_the_same_frames():
    """StreamingRecognizer accepts causal, chunk-trained Conformers only, so this is tiny_dec32
    with `causal` and `use_dynamic_chunk` set in its encoder section (same decoders): finish()
    returns the attention_rescoring result of the same frames under the same chunk mask, asserted
    as tests/test_gpu_streaming.py asserts it."""
    from wenet_amd import synthetic as S
    from wenet_amd.model import ASRModel
    from wenet_amd.streaming import StreamingRecognizer
    configs = S.make_configs('tiny_dec32')
    configs['encoder_conf'].update(causal=True, use_dynamic_chunk=True)
    sd = S.make_state_dict(configs, 1)
    m = ASRModel(configs, sd, device='cuda:0')
    chunk, beam, cw, rw = 4, 5, 0.5, 0.3
    f = S.make_features(1, 131, seed=702)[0][0]
    want = m.decode(['attention_rescoring'], f.unsqueeze(0),
                    torch.tensor([f.shape[0]], dtype=torch.int32), beam_size=beam,
                    decoding_chunk_size=chunk, num_decoding_left_chunks=-1, ctc_weight=cw,
                    reverse_weight=rw)['attention_rescoring'][0]
    rec = StreamingRecognizer(m, 1, chunk, -1, beam_size=beam, max_seconds=2.0)
    sid = rec.open()
    fc = f.cuda()
    for a in range(0, fc.shape[0], 50):
        rec.accept(sid, fc[a:a + 50])
        while rec.step():
            pass
    r = rec.finish(sid, rescoring=True, ctc_weight=cw, reverse_weight=rw)
    rec.close(sid)
    assert len(want.tokens) > 0
    gs = sorted(r.all_scores, reverse=True)
    if len(gs) < 2 or gs[0] - gs[1] > 2e-3:
        assert list(r.tokens) == list(want.tokens)
    if list(r.tokens) == list(want.tokens):
        assert abs(r.score - want.score) < 1e-3


def test_width_model_forward_attention_decoder():
    """8 decoder heads at 256, the recipes' width: the padded log-softmax outputs of both
    decoders on hypotheses of 9, 4, 1, 6 and 9 tokens over 31 encoder frames, every position of
    every hypothesis's own length."""
    from wenet_amd import EfficientConformer
    from wenet_amd import synthetic as S
    meta, arrays = D.load_fixture(D.WIDTH_MODEL)
    configs = S.make_configs(D.WIDTH_MODEL)
    sd = S.make_state_dict(configs, meta['wseed'])
    m = EfficientConformer(configs, sd, device='cuda:0')
    assert (m._cfg.d_model, m._cfg.dec_heads) == (256, 8)
    hyps, lens, enc = D.width_inputs(configs)
    got_l, got_r = m.forward_attention_decoder(hyps, lens, enc.cuda(), meta['reverse_weight'])
    V = configs['output_dim']
    for side, got in (('l', got_l), ('r', got_r)):
        ref = torch.from_numpy(arrays['logp_' + side]).view(5, 9, V)
        assert tuple(got.shape) == (5, 9, V)
        for i, n in enumerate(lens.tolist()):
            g, w = got[i, :n].double().cpu(), ref[i, :n]
            err = (g - w).abs().max().item()
            bound = 8 * meta['e_logp'][side] + 16 * KR.ULP32 * w.abs().max().item()
            print(f'logp_{side}[{i}]: err={err:.3e} e_logp={meta["e_logp"][side]:.3e} '
                  f'bound={bound:.3e}')
            assert torch.isfinite(g).all() and err <= bound


def test_bf16_handle_runs(cases):
    """A smoke test: the decoder's attention stays fp32 on a bf16 handle (attention_d32 is called
    directly, not through the precision-dependent choice of attention())."""
    c = cases('tiny_dec32')
    m = c['model'].clone()
    m.set_compute_dtype('bf16')
    got = m.decode(['attention_rescoring'], c['x'], c['lens'], **c['kw'])['attention_rescoring']
    assert len(got) == len(c['feats'])
    assert all(torch.isfinite(torch.tensor(float(r.score))) for r in got)


def test_other_head_widths_are_still_refused(cases):
    """8 decoder heads at 128 (d_k = 16): refused at creation, naming both widths."""
    from wenet_amd import _lib
    m = cases('tiny_dec32')['model']
    cfg = type(m._cfg).from_buffer_copy(m._cfg)
    cfg.dec_heads = 8
    tensors = (_lib.WnTensor * 1)()
    h = ctypes.c_void_p()
    assert m._L.wn_model_create(ctypes.byref(cfg), tensors, 0, 0, ctypes.byref(h)) == -1
    msg = m._L.wn_last_error()
    assert b'decoder head dim must be 32 or 64' in msg and not h.value
