"""SenseVoice Small on the GPU (wenet_amd.SenseVoiceSmall: csrc/sensevoice.hip,
csrc/cabi_sensevoice.hip) against what the real reference computed for `tiny_sensevoice` and
`tiny_sensevoice_h64` (tests/golden/sensevoice/, recorded by tools/gen_golden_sensevoice.py with
every utterance ALONE under three query settings), and one block per stack at the released widths
against the fp64 formulation of tests/sensevoice_refs.py.

Bounds: the encoder output within 8 e_enc + 16 fp32 ulps of its scale of the fp64 reference, the
prefix-beam score within 8 e_score + 16 ulps, e_* = the fp32 reference's own error against fp64 on
the same utterance and setting.  Token lists of both methods equal the recorded ones; the seven
utterances batched (+ one without frames) give the bits each gives alone.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as KR
import paraformer_refs as PR
import sensevoice_refs as SR

pytestmark = pytest.mark.gpu

METHODS = list(SR.METHODS)


def _batch(feats):
    T = max(max(f.shape[0] for f in feats), 1)
    x = torch.zeros(len(feats), T, 80)
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    return x, torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)


def _run(model, feats, infos):
    """One batch under `infos`: per utterance (encoder rows, tokens of both methods, the
    prefix-beam score, times)."""
    x, lens = _batch(feats)
    enc, mask = model._forward_encoder(x, lens, infos=infos)
    res = model.decode(METHODS, x, lens, beam_size=SR.CTC_BEAM, infos=infos)
    torch.cuda.synchronize()
    out = []
    for b, f in enumerate(feats):
        tp = SR.enc_rows(f.shape[0])
        assert int(mask[b].sum()) == tp
        pb = res['ctc_prefix_beam_search'][b]
        out.append(dict(enc=enc[b, :tp].cpu(), score=float(pb.score),
                        tokens={m: [int(t) for t in res[m][b].tokens] for m in METHODS},
                        times={m: list(res[m][b].times or []) for m in METHODS}))
    return out


@pytest.fixture(scope='module', params=SR.TINY_CONFIGS)
def tiny(request):
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import SenseVoiceSmall
    meta, arr = SR.load_tiny(request.param)
    configs = S.make_configs(request.param)
    model = SenseVoiceSmall(configs, S.make_state_dict(configs, meta['wseed']))
    feats = SR.tiny_features()
    alone = {name: [_run(model, [f], dict(infos))[0] for f in feats]
             for name, infos in SR.SETTINGS.items()}
    return dict(config=request.param, meta=meta, arr=arr, model=model, feats=feats, alone=alone)


def test_encoder_output_against_fp64(tiny):
    meta, arr = tiny['meta'], tiny['arr']
    seen = 0
    for name in SR.SETTINGS:
        s = meta['settings'][name]
        for i, n in enumerate(SR.TINY_LENS):
            if f'enc64_{name}_{n}' not in arr:
                continue
            seen += 1
            ref = torch.from_numpy(arr[f'enc64_{name}_{n}'])
            got = tiny['alone'][name][i]['enc']
            assert got.shape == ref.shape
            err = (got.double() - ref).abs().max().item()
            bound = 8 * s['e_enc'][i] + 16 * KR.ULP32 * ref.abs().max().item()
            print(f'{tiny["config"]} enc[{name}, {n}] err={err:.3e} e_enc={s["e_enc"][i]:.3e} '
                  f'bound={bound:.3e}')
            assert err <= bound
    assert seen == 5


def test_token_lists_equal_recorded(tiny):
    meta = tiny['meta']
    for name in SR.SETTINGS:
        for i, r in enumerate(tiny['alone'][name]):
            for m in METHODS:
                assert r['tokens'][m] == meta['settings'][name]['tokens'][m][i], (name, m, i)
            # times count the four query frames: inside [0, 4 + T')
            assert all(0 <= t < meta['enc_lens'][i] for t in r['times']['ctc_prefix_beam_search'])


def test_prefix_beam_scores_against_fp64(tiny):
    meta = tiny['meta']
    for name in SR.SETTINGS:
        s = meta['settings'][name]
        for i, r in enumerate(tiny['alone'][name]):
            ref = s['scores'][i]
            err = abs(r['score'] - ref)
            bound = 8 * s['e_score'][i] + 16 * KR.ULP32 * abs(ref)
            print(f'{tiny["config"]} score[{name}, {SR.TINY_LENS[i]}] err={err:.3e} '
                  f'e_score={s["e_score"][i]:.3e} bound={bound:.3e}')
            assert err <= bound


def test_unknown_setting_gives_the_default_bits(tiny):
    for a, b in zip(tiny['alone']['unknown'], tiny['alone']['default']):
        _same(a, b, 'unknown lid / itn')
    # infos=None is the default too
    got = _run(tiny['model'], [tiny['feats'][2]], None)[0]
    _same(got, tiny['alone']['default'][2], 'infos=None')


def _same(a, b, what):
    assert torch.equal(a['enc'].view(torch.int32), b['enc'].view(torch.int32)), what
    assert a['tokens'] == b['tokens'] and a['times'] == b['times'], what
    assert np.float64(a['score']).view(np.int64) == np.float64(b['score']).view(np.int64), what


def test_batched_with_an_empty_utterance_is_bit_identical_to_alone(tiny):
    feats = list(tiny['feats'])
    feats.insert(3, torch.zeros(0, 80))          # no frames, between neighbours
    for name in ('default', 'en_withitn'):
        got = _run(tiny['model'], feats, dict(SR.SETTINGS[name]))
        assert got[3]['enc'].shape[0] == 0
        assert got[3]['tokens'] == {m: [] for m in METHODS}
        for i, (a, b) in enumerate(zip(got[:3] + got[4:], tiny['alone'][name])):
            _same(a, b, f'{name}: utterance {i} of the batch of eight')
    # 6 frames as the longest of its batch (n % 6 == 0: the reference's batched LFR would pad the
    # 1-frame utterance from the batch's zero padding)
    got = _run(tiny['model'], tiny['feats'][:2], {})
    for i, (a, b) in enumerate(zip(got, tiny['alone']['default'][:2])):
        _same(a, b, f'utterance {i} beside the 6-frame one')
    # nothing but empty utterances: empty results, no error
    res = tiny['model'].decode(METHODS, torch.zeros(2, 3, 80), torch.tensor([0, 0]), beam_size=5)
    assert [list(r.tokens) for m in METHODS for r in res[m]] == [[]] * 4


def test_per_utterance_lid_list(tiny):
    """As an extension `lid` / `itn` may be lists: every utterance gets the bits of its own
    single-setting run."""
    feats = [tiny['feats'][i] for i in (4, 2, 3, 6)]
    names = ['default', 'en_withitn', 'default', 'en_withitn']
    infos = dict(lid=[SR.SETTINGS[n].get('lid', 'auto') for n in names],
                 itn=[SR.SETTINGS[n].get('itn', 'woitn') for n in names])
    got = _run(tiny['model'], feats, infos)
    for r, n, i in zip(got, names, (4, 2, 3, 6)):
        _same(r, tiny['alone'][n][i], f'utterance {i} under {n}')
    # a list for lid alone, one string for itn
    got = _run(tiny['model'], feats[:2], dict(lid=['en', 'en'], itn='withitn'))
    _same(got[0], tiny['alone']['en_withitn'][4], 'lid list + itn string')
    with pytest.raises(ValueError, match='lid'):
        tiny['model'].decode(METHODS, *_batch(feats), infos=dict(lid=['en']))


def test_speech_lengths_is_left_alone(tiny):
    x, lens = _batch(tiny['feats'][:3])
    lens = lens.to(torch.int64)
    before = lens.clone()
    tiny['model'].decode(['ctc_greedy_search'], x, lens, infos={'lid': 'zh'})
    assert torch.equal(lens, before)
    r = tiny['model'].decode(['ctc_greedy_search'], x, lens)
    assert torch.equal(lens, before) and len(r['ctc_greedy_search']) == 3


def test_stale_or_missized_queries_are_refused_through_the_c_abi(tiny):
    from wenet_amd import _lib
    from wenet_amd.model import _stream_ptr
    model = tiny['model']
    L, h = model._L, model._h
    x, lens = _batch(tiny['feats'][1:4])
    xd = x.cuda().contiguous()
    ln = lens.numpy().astype(np.int32)
    enc_lens = np.zeros(3, dtype=np.int32)
    out = torch.empty(3, SR.enc_rows(x.shape[1]), model._cfg.d_model, device='cuda')

    def encode():
        return L.wn_encode(h, xd.data_ptr(), _lib.i32p(ln), 3, x.shape[1], -1, -1, out.data_ptr(),
                           _lib.i32p(enc_lens), _stream_ptr(model.device))

    def qid(rows):
        return np.ascontiguousarray(np.asarray(rows, dtype=np.int32))

    en = [4, 1, 2, 14]
    # ids for two utterances, an encode of three: refused, and the argument is named
    _lib.check(L.wn_sensevoice_set_queries(h, _lib.i32p(qid([en] * 2)), 2), 'set_queries')
    with pytest.raises(RuntimeError, match=r'B = 3 differs from the B = 2'):
        _lib.check(encode(), 'wn_encode')
    # the refused call used the ids up: the next encode runs on the defaults
    _lib.check(encode(), 'wn_encode')
    torch.cuda.synchronize()
    for b in range(3):
        ref = tiny['alone']['default'][1 + b]['enc']
        assert torch.equal(out[b, :ref.shape[0]].cpu().view(torch.int32), ref.view(torch.int32))
    # ids serve ONE encode: the second one is back on the defaults
    _lib.check(L.wn_sensevoice_set_queries(h, _lib.i32p(qid([en] * 3)), 3), 'set_queries')
    _lib.check(encode(), 'wn_encode')
    torch.cuda.synchronize()
    ref = tiny['alone']['en_withitn'][2]['enc']
    assert torch.equal(out[1, :ref.shape[0]].cpu().view(torch.int32), ref.view(torch.int32))
    _lib.check(encode(), 'wn_encode')
    torch.cuda.synchronize()
    ref = tiny['alone']['default'][2]['enc']
    assert torch.equal(out[1, :ref.shape[0]].cpu().view(torch.int32), ref.view(torch.int32))
    # ids outside the table, a batch size out of range, another kind of handle
    for bad in (16, -1):
        with pytest.raises(RuntimeError, match=r'outside \[0, 16\)'):
            _lib.check(L.wn_sensevoice_set_queries(h, _lib.i32p(qid([en, [0, 1, bad, 15]])), 2),
                       'set_queries')
    with pytest.raises(RuntimeError, match='B out of range'):
        _lib.check(L.wn_sensevoice_set_queries(h, _lib.i32p(qid([en])), 0), 'set_queries')
    ws = ctypes.c_void_p()
    _lib.check(L.wn_workspace_create(model.device.index, ctypes.byref(ws)), 'workspace')
    try:
        with pytest.raises(RuntimeError, match='not a SenseVoice handle'):
            _lib.check(L.wn_sensevoice_set_queries(ws, _lib.i32p(qid([en])), 1), 'set_queries')
    finally:
        L.wn_model_destroy(ws)


def test_create_refuses_other_query_shapes_and_missing_weights():
    from wenet_amd import _lib
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import SenseVoiceSmall

    class Odd(SenseVoiceSmall):
        def _config(self, configs):
            cfg = super()._config(configs)
            for k, v in self.odd.items():
                setattr(self._scfg, k, v)
            return cfg

    configs = S.make_configs('tiny_sensevoice_h64')
    sd = S.make_state_dict(configs, 0)
    for odd, msg in ((dict(n_query=3), 'n_query must be 4'), (dict(n_embed=8), 'n_embed must be 16'),
                     (dict(max_frames=0), 'max_frames')):
        Odd.odd = odd
        with pytest.raises(RuntimeError, match=msg):
            Odd(configs, sd)
    for drop in ('global_cmvn.mean', 'ctc.ctc_lo.weight', 'embed.weight',
                 'encoder.tp_encoders.0.norm1.weight', 'encoder.tp_norm.bias'):
        with pytest.raises(RuntimeError, match=drop.replace('.', r'\.')):
            SenseVoiceSmall(configs, {k: v for k, v in sd.items() if k != drop})
    # a package whose CMVN arrives under the encoder's names (from the json file) loads
    alias = {('encoder.' + k if k.startswith('global_cmvn.') else k): v for k, v in sd.items()}
    SenseVoiceSmall(configs, alias)


def test_refusals(tiny):
    model = tiny['model']
    x, lens = _batch(tiny['feats'][2:3])
    np_ = pytest.raises(NotImplementedError, match='outside the accelerated path')
    for m in ('attention', 'attention_rescoring'):
        with pytest.raises(NotImplementedError, match=m):
            model.decode([m], x, lens)
    with np_:
        model.decode(['ctc_greedy_search'], x, lens, decoding_chunk_size=4)
    with np_:
        model.decode(['ctc_greedy_search'], x, lens, simulate_streaming=True)
    for fn in (model.forward_encoder_chunk, model.forward_encoder_chunk_batch,
               model.forward_encoder_chunk_by_chunk):
        with np_:
            fn(x, 0, -1)
    with np_:
        model.clone()
    from wenet_amd.pipeline import DecodePipeline
    with pytest.raises(NotImplementedError):
        DecodePipeline(model)
    for dt in ('bf16', 'fp8'):
        with np_:
            model.set_compute_dtype(dt)
    assert model.set_compute_dtype('fp32') is model
    with np_:
        model.align(x, lens, [[3, 4]])
    assert model.default_decode_method == 'ctc_greedy_search'
    assert model.subsampling_rate() == 6


def test_penalties_are_taken_and_do_not_stick(tiny):
    """blank_penalty and length_penalty are taken as on ASRModel (zero values give the recorded
    lists, a blank penalty of 100 leaves no blank frame: at least one token) and leave the next
    plain decode unchanged."""
    model = tiny['model']
    x, lens = _batch(tiny['feats'][4:5])
    plain = tiny['alone']['default'][4]['tokens']
    zero = model.decode(METHODS, x, lens, beam_size=SR.CTC_BEAM, blank_penalty=0.0,
                        length_penalty=0.0, context_graph=None)
    assert {m: [int(t) for t in zero[m][0].tokens] for m in METHODS} == plain
    pen = model.decode(METHODS, x, lens, beam_size=SR.CTC_BEAM, blank_penalty=100.0,
                       length_penalty=0.5)
    assert len(pen['ctc_greedy_search'][0].tokens) >= 1
    again = model.decode(METHODS, x, lens, beam_size=SR.CTC_BEAM)
    assert {m: [int(t) for t in again[m][0].tokens] for m in METHODS} == plain


def test_one_block_at_the_released_widths():
    """encoders0 + one block, one tp block at d 512, 4 heads of 128, 2048 units on 240 frames
    (44 rows), against the fp64 formulation (pinned to the reference's model on the CPU in
    tests/test_sensevoice_host.py); e_plain = the same formulation evaluated in fp32."""
    from wenet_amd import synthetic as S
    from wenet_amd.sensevoice import SenseVoiceSmall
    configs = S.make_configs('sensevoice_small_1blk')
    sd = S.make_state_dict(configs, 0)
    f = PR.features(240, 31)
    qid = SR.query_rows('ko', 'withitn')
    r64 = SR.ref_sensevoice(sd, configs, f, qid)
    r32 = SR.ref_sensevoice(sd, configs, f, qid, fp32=True)
    model = SenseVoiceSmall(configs, sd)
    x, lens = _batch([f])
    enc, mask = model._forward_encoder(x, lens, infos=dict(lid='ko', itn='withitn'))
    torch.cuda.synchronize()
    assert int(mask.sum()) == 44 and enc.shape == (1, 44, 512)
    e_plain = (r32['enc'] - r64['enc']).abs().max().item()
    scale = r64['enc'].abs().max().item()
    err = (enc[0].cpu().double() - r64['enc']).abs().max().item()
    print(f'1blk enc err={err:.3e} e_plain={e_plain:.3e} bound={KR.bound(e_plain, scale):.3e}')
    assert KR.cap_ok(e_plain, scale) and err <= KR.bound(e_plain, scale)


def test_load_model_and_transcribe_cli(tmp_path, capsys):
    import json
    import wave
    import yaml
    import wenet_amd
    from wenet_amd import synthetic as S
    from wenet_amd.bin import transcribe
    d = tmp_path / 'sv'
    d.mkdir()
    configs = S.make_configs('tiny_sensevoice_h64')
    sd = S.make_state_dict(configs, 0)
    mean, istd = sd.pop('global_cmvn.mean').double().numpy(), \
        sd.pop('global_cmvn.istd').double().numpy()
    n, var = 1000, 1.0 / (istd * istd)
    (d / 'global_cmvn').write_text(json.dumps(
        {'mean_stat': (mean * n).tolist(), 'var_stat': ((var + mean * mean) * n).tolist(),
         'frame_num': n}))
    (d / 'units.txt').write_text('<blank> 0\n<s> 1\n</s> 2\n' + ''.join(
        f'▁u{i} {i}\n' for i in range(3, configs['output_dim'])), encoding='utf8')
    configs['cmvn_conf'] = {'cmvn_file': str(d / 'global_cmvn'), 'is_json_cmvn': True}
    (d / 'train.yaml').write_text(yaml.safe_dump(configs))
    torch.save(sd, str(d / 'final.pt'))
    model = wenet_amd.load_model(str(d))
    assert isinstance(model, wenet_amd.SenseVoiceSmall)
    pcm = (S.make_audio(24000) * 32767.0).astype('<i2')
    wav = str(tmp_path / 'a.wav')
    with wave.open(wav, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    r = model.transcribe(wav)
    speech = model.compute_feature(wav)
    ln = torch.tensor([speech.size(0)])
    want = model.decode(['ctc_greedy_search'], speech.unsqueeze(0), ln)['ctc_greedy_search'][0]
    assert list(r.tokens) == list(want.tokens) and isinstance(r.text, str)
    en = model.decode(['ctc_greedy_search'], speech.unsqueeze(0), ln,
                      infos=dict(lid='en', itn='withitn'))['ctc_greedy_search'][0]
    capsys.readouterr()
    assert transcribe.main([wav, '-m', str(d), '--lid', 'en', '--itn', 'withitn', '-t']) == 0
    printed = capsys.readouterr().out
    assert f'tokens {list(en.tokens)}' in printed
    assert printed.splitlines()[0] == model.tokenizer.detokenize(list(en.tokens))[0]
