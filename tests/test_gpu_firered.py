"""FireRedASR-AED through the public interface -- `load_model` on a model directory written from
the fixture's recipe and weights -- against what the reference's own FireRedModel computed
(tests/golden/firered/firered_tiny.npz, tools/gen_golden_firered.py): `tiny_firered`, four
utterances of 290, 131, 127 and 121 frames (T' = 73, 33, 32, 31), every one decoded ALONE by the
reference.

Encoder tolerance: 8 * e_enc + 16 fp32 ulps of the output scale per utterance, e_enc = the fp32
reference's own max abs error against its fp64 run (recorded): the project's margin over the
reference's own fp32 error.  The fp64 reference is firered_refs.firered_encoder_formulation,
pinned on the CPU (tests/test_firered_host.py) within 1e-9 relative to the recorded fp64 encoder
output of three of the four utterances (the fixtures have room for those); the token lists are
the reference's.  e_enc was measured between the fp32 reference and a `.double()` reference whose
attention softmax still runs in fp32 (forward_attention: scores.float()), while the target here
keeps the softmax in fp64: yardstick and target differ by that fp32 softmax rounding, which both
fp32 runs carry.

Scores: decode(['attention']) returns no score in the reference (search.py builds
DecodeResult(hyp)), so the fixture records, per attention list, the decoder's teacher-forced
log-probability of the list followed by <eos>, and the scores of attention_rescoring and
ctc_prefix_beam_search; each is held within 8 * e_score + 16 fp32 ulps of |score|, e_score = the
reference's own |fp32 - fp64| on that number (the rule of the encoder bound).
"""
import json
import os
import wave

import numpy as np
import pytest
import torch

import firered_refs as FR
import kernel_refs as KR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    import yaml
    from wenet_amd import load_model
    from wenet_amd import synthetic as S
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'firered', 'firered_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode('utf8'))
    configs = S.make_configs(meta['config'])
    sd = S.make_state_dict(configs, meta['wseed'])
    d = tmp_path_factory.mktemp('firered_tiny')
    V = configs['output_dim']
    syms = ['<blank>', '<unk>', '<pad>', '<sos>', '<eos>'] + [f'▁w{i}' for i in range(5, V)]
    (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    cfg = dict(configs)
    cfg['tokenizer_conf'] = dict(configs['tokenizer_conf'], bpe_path=None)
    (d / 'train.yaml').write_text(yaml.safe_dump(cfg))
    torch.save(sd, d / 'final.pt')
    model = load_model(str(d))
    feats = FR.tiny_features()
    ref = [FR.firered_encoder_formulation(f, sd, configs, softmax32=False) for f in feats]
    return dict(meta=meta, configs=configs, sd=sd, model=model, feats=feats, ref=ref, dir=d,
                syms=syms)


def _batch(feats):
    T = max(f.shape[0] for f in feats)
    x = torch.full((len(feats), T, feats[0].shape[1]), KR.POISON)
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    return x, torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)


def test_load_model_gives_a_firered(case):
    from wenet_amd import FireRed
    m = case['model']
    assert isinstance(m, FireRed) and m.default_decode_method == 'attention'
    assert (m.sos, m.eos) == (3, 4)


def test_encoder_against_the_fp64_reference(case):
    m, meta = case['model'], case['meta']
    x, lens = _batch(case['feats'])
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == meta['enc_lens']
    for i, ref in enumerate(case['ref']):
        n = ref.shape[0]
        got = out[i, :n].double().cpu()
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        bound = 8 * meta['e_enc'][i] + 16 * KR.ULP32 * scale
        print(f'firered encoder[{meta["frames"][i]}]: err={err:.3e} e_enc={meta["e_enc"][i]:.3e} '
              f'scale={scale:.3e} bound={bound:.3e}')
        assert torch.isfinite(got).all()
        assert err <= bound
        assert (out[i, n:] == 0).all()


def test_batched_equals_alone_bit_for_bit(case):
    m = case['model']
    x, lens = _batch(case['feats'])
    out, _ = m._forward_encoder(x, lens)
    out = out.clone()
    both = m.decode(['attention', 'ctc_prefix_beam_search'], x, lens, beam_size=3)
    for i, f in enumerate(case['feats']):
        o1, _ = m._forward_encoder(f.unsqueeze(0), torch.tensor([f.shape[0]]))
        n = o1.shape[1]
        assert torch.equal(o1[0].view(torch.int32), out[i, :n].view(torch.int32)), i
        one = m.decode(['attention', 'ctc_prefix_beam_search'], f.unsqueeze(0),
                       torch.tensor([f.shape[0]]), beam_size=3)
        for k in one:
            assert list(one[k][0].tokens) == list(both[k][i].tokens), (k, i)


@pytest.mark.parametrize('beam', [1, 3, 10])
def test_attention_tokens_are_the_references(case, beam):
    m, meta = case['model'], case['meta']
    x, lens = _batch(case['feats'])
    got = m.decode(['attention'], x, lens, beam_size=beam)['attention']
    assert [list(r.tokens) for r in got] == meta['tokens'][f'attention/{beam}']


def _score_ok(name, got, want, e):
    bound = 8 * e + 16 * KR.ULP32 * abs(want)
    print(f'{name}: got={got:.6f} ref={want:.6f} e_score={e:.3e} bound={bound:.3e}')
    assert abs(got - want) <= bound, name


@pytest.mark.parametrize('beam', [1, 3, 10])
def test_attention_scores_are_the_references(case, beam):
    """The decoder's log-probability of every recorded attention list followed by <eos>, teacher
    forced on this encoder's output: a shift of the log-probs that flips no arg-max shows here."""
    m, meta = case['model'], case['meta']
    key = f'attention/{beam}'
    for i, f in enumerate(case['feats']):
        enc, _ = m._forward_encoder(f.unsqueeze(0), torch.tensor([f.shape[0]]))
        u = meta['tokens'][key][i]
        hyp = torch.tensor([[m.sos] + u], dtype=torch.long)
        logp, _ = m.forward_attention_decoder(hyp, torch.tensor([len(u) + 1]), enc.clone())
        tgt = torch.tensor(u + [m.eos])
        got = float(logp[0].double().cpu()[torch.arange(len(tgt)), tgt].sum())
        _score_ok(f'{key}[{i}]', got, meta['scores'][key][i], meta['e_score'][key][i])


def test_ctc_tokens_are_the_references(case):
    m, meta = case['model'], case['meta']
    x, lens = _batch(case['feats'])
    got = m.decode(['ctc_greedy_search'], x, lens)['ctc_greedy_search']
    assert [list(r.tokens) for r in got] == meta['tokens']['ctc_greedy_search']
    got = m.decode(['ctc_prefix_beam_search'], x, lens,
                   beam_size=meta['ctc_beam'])['ctc_prefix_beam_search']
    assert [list(r.tokens) for r in got] == meta['tokens']['ctc_prefix_beam_search']
    for i, r in enumerate(got):
        _score_ok(f'ctc_prefix_beam_search[{i}]', float(r.score),
                  meta['scores']['ctc_prefix_beam_search'][i],
                  meta['e_score']['ctc_prefix_beam_search'][i])


def test_attention_rescoring_is_the_references(case):
    """attention_rescoring at ctc_weight 1, beam 5: the winner and its score are what the
    reference returns for every utterance (a wrong combination of the CTC and the decoder score
    moves the score, and the winner where the two disagree), alone and in the batch."""
    m, meta = case['model'], case['meta']
    x, lens = _batch(case['feats'])
    r = m.decode(['ctc_prefix_beam_search', 'attention_rescoring'], x, lens,
                 beam_size=meta['ctc_beam'], ctc_weight=meta['rescore_ctc_weight'])
    assert [list(a.tokens) for a in r['attention_rescoring']] == \
        meta['tokens']['attention_rescoring']
    for i, a in enumerate(r['attention_rescoring']):
        _score_ok(f'attention_rescoring[{i}]', float(a.score),
                  meta['scores']['attention_rescoring'][i],
                  meta['e_score']['attention_rescoring'][i])
    # the decoder moves the order: the rescored winner is not the CTC winner everywhere, or the
    # check above could not see the decoder's share
    print('rescored winner == ctc winner:',
          [list(a.tokens) == list(b.tokens)
           for a, b in zip(r['attention_rescoring'], r['ctc_prefix_beam_search'])])


def test_refusals_on_a_live_model(case):
    from wenet_amd.streaming import StreamingRecognizer
    from wenet_amd.pipeline import DecodePipeline
    m = case['model']
    x, lens = _batch(case['feats'][1:2])
    with pytest.raises(NotImplementedError, match='streaming'):
        m.forward_encoder_chunk(x, 0, -1)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        m.decode(['attention'], x, lens, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        m.decode(['rnnt_greedy_search'], x, lens)
    with pytest.raises(NotImplementedError, match='reverse_weight'):
        m.decode(['attention_rescoring'], x, lens, reverse_weight=0.3)
    for dt in ('bf16', 'fp8'):
        with pytest.raises(NotImplementedError, match="stays 'fp32'"):
            m.set_compute_dtype(dt)
    with pytest.raises(NotImplementedError):
        StreamingRecognizer(m, n_sessions=1, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='DecodePipeline'):
        DecodePipeline(m)
    # the C ABI refuses too, with an error string
    from wenet_amd import _lib
    assert m._L.wn_model_set_precision(m._h, 1) == -1
    assert b'fp32' in m._L.wn_last_error()
    enc_lens = np.zeros(1, dtype=np.int32)
    xs = x.cuda().contiguous()
    assert m._L.wn_encode(m._h, xs.data_ptr(), _lib.i32p(lens.numpy().astype(np.int32)), 1,
                          xs.shape[1], 4, -1, None, _lib.i32p(enc_lens), None) == -1
    assert b'chunk' in m._L.wn_last_error()
    # the chunk encoders, the streaming sessions and the Conformer front-end hook
    import ctypes
    L = m._L
    out = torch.zeros(4, m._cfg.d_model, device='cuda')
    zero = np.zeros(1, dtype=np.int32)
    ci, co = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.wn_encode_chunk_batch(m._h, 1, xs.data_ptr(), 23, _lib.i32p(zero), -1, None,
                                   _lib.i32p(zero), None, out.data_ptr(), None, None,
                                   ctypes.byref(ci), ctypes.byref(co), None) == -1
    assert b'FireRed encoder does not stream' in L.wn_last_error()
    assert L.wn_encode_chunk(m._h, xs.data_ptr(), 23, 0, -1, None, 0, None, out.data_ptr(),
                             None, None, ctypes.byref(ci), ctypes.byref(co), None) == -1
    assert b'FireRed encoder does not stream' in L.wn_last_error()
    h = ctypes.c_void_p()
    assert L.wn_stream_create(m._h, 1, 64, 4, 0, ctypes.byref(h), None) == -1
    assert b'FireRed encoder does not stream' in L.wn_last_error() and not h.value
    route = ctypes.c_int32(0)
    assert L.wn_op_conv2d4(m._h, xs.data_ptr(), _lib.i32p(lens.numpy().astype(np.int32)), 1,
                           xs.shape[1], None, None, None, None, ctypes.byref(route), None) == -1
    assert b'needs a Conformer encoder' in L.wn_last_error()
    # and the handle still encodes
    m._forward_encoder(x, lens)


def test_aed_l_width_one_block(case):
    """FireRedASR-AED-L's widths -- d_model 1280, 20 heads, ffn 5120, the conv module over 2560
    channels -- with ONE encoder and ONE decoder block (`firered_aed_l_1blk`: the 16 + 16 blocks of
    the full model are 4.5 GB of synthetic weights): the handle is created and the encoder output
    meets the fp64 formulation within 8 * e_plain + 16 ulp, e_plain = the same formulation
    evaluated in fp32."""
    from wenet_amd import FireRed
    from wenet_amd import synthetic as S
    configs = S.make_configs('firered_aed_l_1blk')
    sd = S.make_state_dict(configs, 1)
    m = FireRed(configs, sd, device='cuda:0')
    feats = [S.make_features(1, n, seed=40 + i)[0][0] for i, n in enumerate((139, 61))]
    x, lens = _batch(feats)
    out, mask = m._forward_encoder(x, lens)
    assert mask.squeeze(1).sum(1).tolist() == [35, 16]
    for i, f in enumerate(feats):
        ref = FR.firered_encoder_formulation(f, sd, configs, softmax32=False)
        plain = FR.firered_encoder_formulation(f, sd, configs, softmax32=False,
                                               dtype=torch.float32).double()
        e_plain = (plain - ref).abs().max().item()
        scale = ref.abs().max().item()
        err = (out[i, :ref.shape[0]].double().cpu() - ref).abs().max().item()
        bound = 8 * e_plain + 16 * KR.ULP32 * scale
        print(f'firered aed-l width[{f.shape[0]}]: err={err:.3e} e_plain={e_plain:.3e} '
              f'scale={scale:.3e} bound={bound:.3e}')
        assert KR.cap_ok(e_plain, scale)
        assert err <= bound
    got = m.decode(['attention', 'ctc_greedy_search'], x, lens, beam_size=2)
    assert len(got['attention']) == 2


def test_transcribe_a_wav(case):
    from wenet_amd import synthetic as S
    m = case['model']
    pcm = S.make_audio(16000 * 2, seed=9)
    wav = case['dir'] / 'a.wav'
    with wave.open(str(wav), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(pcm * 32768, -32768, 32767).astype(np.int16).tobytes())
    r = m.transcribe(str(wav))
    assert isinstance(r.text, str)
    feats = m.compute_feature(str(wav))
    want = m.decode(['attention'], feats.unsqueeze(0), torch.tensor([feats.shape[0]]))
    assert list(r.tokens) == list(want['attention'][0].tokens)
    assert r.text == ''.join(case['syms'][t] for t in r.tokens).replace('▁', ' ').strip()

