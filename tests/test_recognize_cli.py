"""Host logic of wenet_amd/bin/recognize.py and wenet_amd/tokenizer.py (no GPU):
argument handling, list reading, batching / in-batch order, the rank-part merge,
detokenisation against the reference's tokenizers."""
import json
import os

import pytest

from golden_util import load_case
from wenet_amd.bin import recognize as R
from wenet_amd.tokenizer import Tokenizer, get_blank_id, init_tokenizer


def test_args_reject_modes_outside_the_path():
    base = ['--config', 'c', '--test_data', 'd', '--checkpoint', 'k', '--result_dir', 'o']
    a = R.get_args(base + ['--modes', 'ctc_greedy_search', 'attention_rescoring'])
    assert a.modes == ['ctc_greedy_search', 'attention_rescoring'] and a.batch_size == 16
    with pytest.raises(SystemExit):
        R.get_args(base + ['--modes', 'rnnt_greedy_search'])
    assert R.get_args(base + ['--modes', 'attention', '--data_type', 'shard']
                      ).data_type == 'shard'
    with pytest.raises(SystemExit):
        R.get_args(base + ['--modes', 'attention', '--dtype', 'fp16'])
    assert R.get_args(base + ['--modes', 'attention', '--dtype', 'bf16']).dtype == 'bf16'
    # the reference's transducer / HLG options are accepted (unused by these modes)
    a = R.get_args(base + ['--modes', 'attention_rescoring', '--attn_weight', '0.3',
                           '--transducer_weight', '0.2', '--lm_scale', '0.7', '--hlg', 'x',
                           '--search_ctc_weight', '0.5', '--use_lora', 'False'])
    assert a.attn_weight == 0.3 and a.search_ctc_weight == 0.5 and not a.use_lora
    assert R.get_args(base + ['--modes', 'attention']).search_ctc_weight == 1.0
    with pytest.raises(SystemExit):
        R.get_args(base + ['--modes', 'attention', '--use_lora', 'True'])


def test_data_list_batches_and_order(tmp_path):
    p = tmp_path / 'data.list'
    p.write_text('\n'.join(json.dumps(dict(key=f'u{i}', wav=f'/w/{i}.wav', txt='x'))
                           for i in range(7)) + '\n\n')
    entries = R.read_data_list(str(p))
    assert entries[3] == ('u3', '/w/3.wav') and len(entries) == 7
    b = R.static_batches(entries, 3)
    assert [len(x) for x in b] == [3, 3, 1]
    # processor.padding: longest first, ties keep list order
    assert R.padding_order([50, 80, 50, 90, 80]) == [3, 1, 4, 0, 2]
    p.write_text('{"wav": "x"}\n')
    with pytest.raises(ValueError):
        R.read_data_list(str(p))


def _wav_bytes(samples, rate, tag, bits, nch=1, extensible=False, extra_chunk=True):
    """A RIFF/WAVE image of `samples` ((n, nch) float in [-1, 1))."""
    import struct
    import numpy as np
    x = np.asarray(samples, dtype=np.float64).reshape(-1, nch)
    if tag == 1 and bits == 8:
        raw = np.clip(np.round(x * 128 + 128), 0, 255).astype(np.uint8).tobytes()
    elif tag == 1 and bits == 16:
        raw = np.round(x * 32768).clip(-32768, 32767).astype('<i2').tobytes()
    elif tag == 1 and bits == 24:
        v = np.round(x * (1 << 23)).clip(-(1 << 23), (1 << 23) - 1).astype(np.int64)
        v = np.where(v < 0, v + (1 << 24), v).reshape(-1)
        raw = b''.join(int(t).to_bytes(3, 'little') for t in v)
    elif tag == 1 and bits == 32:
        raw = np.round(x * 2147483648.0).clip(-2 ** 31, 2 ** 31 - 1).astype('<i4').tobytes()
    elif tag == 3 and bits == 32:
        raw = x.astype('<f4').tobytes()
    else:
        raw = x.astype('<f8').tobytes()
    block = nch * bits // 8
    if extensible:
        guid = struct.pack('<H', tag) + bytes.fromhex('000000001000800000aa00389b71')
        fmt = struct.pack('<HHIIHHHHI', 0xFFFE, nch, rate, rate * block, block, bits,
                          22, bits, 0) + guid
    else:
        fmt = struct.pack('<HHIIHH', tag, nch, rate, rate * block, block, bits)
    chunks = b'fmt ' + struct.pack('<I', len(fmt)) + fmt
    if extra_chunk is True:
        chunks += b'LIST' + struct.pack('<I', 5) + b'hello' + b'\0'  # odd size + pad
    elif extra_chunk:  # an even-sized chunk of that many bytes
        chunks += b'LIST' + struct.pack('<I', int(extra_chunk)) + bytes(int(extra_chunk))
    chunks += b'data' + struct.pack('<I', len(raw)) + raw
    return b'RIFF' + struct.pack('<I', 4 + len(chunks)) + b'WAVE' + chunks


def test_read_wav_formats_segments_and_bytes(tmp_path):
    """decode_wav (processor.py:125-153): every linear wav encoding with
    torchaudio.load's normalisation, first channel of multi-channel files, byte
    strings (shard members) and `start` / `end` segments."""
    import io
    import wave
    import numpy as np
    from wenet_amd.model import read_wav
    rng = np.random.Generator(np.random.PCG64(3))
    x = (rng.random((4000, 2)) * 1.8 - 0.9)
    x16 = np.round(x * 32768) / 32768          # exactly representable in s16
    for tag, bits, tol in [(1, 16, 0), (1, 24, 0), (1, 32, 0), (3, 32, 1e-7), (3, 64, 1e-7),
                           (1, 8, 1 / 128)]:
        for ext in (False, True):
            buf = _wav_bytes(x16, 16000, tag, bits, nch=2, extensible=ext)
            got = read_wav(buf)
            assert got.dtype == np.float32 and got.shape == (4000, )
            assert np.abs(got - x16[:, 0]).max() <= tol + 1e-9, (tag, bits, ext)
    # the stdlib writer's s16 file, from a path, a file object, with a rate
    p = tmp_path / 'a.wav'
    with wave.open(str(p), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(np.round(x16[:, 1] * 32768).astype('<i2').tobytes())
    got, sr = read_wav(str(p), return_rate=True)
    assert sr == 8000 and np.array_equal(got, x16[:, 1].astype(np.float32))
    got2, _ = read_wav(io.BytesIO(p.read_bytes()), return_rate=True)
    assert np.array_equal(got, got2)
    with pytest.raises(NotImplementedError):
        read_wav(str(p))                         # 8 kHz without return_rate
    seg, _ = read_wav(str(p), return_rate=True, start=0.1, end=0.25)
    assert np.array_equal(seg, got[800:2000])
    with pytest.raises(ValueError):
        read_wav(b'OggS' + bytes(64))
    with pytest.raises(NotImplementedError):
        read_wav(_wav_bytes(x16, 16000, 1, 16).replace(b'\x01\x00\x01\x00', b'\x11\x00\x01\x00', 1))


def test_shard_list_reads_tar_members_lazily(tmp_path):
    """tar_file_and_group (datapipes.py:365-427): <key>.wav + <key>.txt groups in
    member order; plain tars are read by offset, compressed ones through tarfile."""
    import io
    import tarfile
    import numpy as np
    from wenet_amd.model import read_wav
    waves = {f'utt{i}': _wav_bytes(np.full((100 + i, 1), i / 10.0), 16000, 1, 16)
             for i in range(5)}

    def build(path, mode, keys, with_orphan=False):
        with tarfile.open(path, mode) as t:
            for k in keys:
                for ext, payload in (('txt', ('text ' + k).encode()), ('wav', waves[k])):
                    ti = tarfile.TarInfo(f'{k}.{ext}')
                    ti.size = len(payload)
                    t.addfile(ti, io.BytesIO(payload))
            if with_orphan:  # a transcript without audio is dropped
                ti = tarfile.TarInfo('orphan.txt')
                ti.size = 1
                t.addfile(ti, io.BytesIO(b'x'))
    build(tmp_path / 's0.tar', 'w', ['utt0', 'utt1', 'utt2'], with_orphan=True)
    build(tmp_path / 's1.tar.gz', 'w:gz', ['utt3', 'utt4'])
    lst = tmp_path / 'shards.list'
    lst.write_text(f"{tmp_path / 's0.tar'}\nfile://{tmp_path / 's1.tar.gz'}\n\n")
    entries = R.read_data_list(str(lst), 'shard')
    assert [k for k, _ in entries] == ['utt0', 'utt1', 'utt2', 'utt3', 'utt4']
    assert entries[0][1].offset is not None and entries[3][1].offset is None
    for k, m in entries:
        assert m.read() == waves[k]
        assert len(read_wav(m.read())) == 100 + int(k[3:])
    lst.write_text('https://example.com/s.tar\n')
    with pytest.raises(ValueError):
        R.read_data_list(str(lst), 'shard')


def test_raw_list_segments(tmp_path):
    p = tmp_path / 'd.list'
    p.write_text(json.dumps(dict(key='a', wav='/w/a.wav', start=1.5, end=2.0)) + '\n' +
                 json.dumps(dict(key='b', wav='/w/b.wav')) + '\n')
    assert R.read_data_list(str(p)) == [('a', ('/w/a.wav', 1.5, 2.0)), ('b', '/w/b.wav')]
    p.write_text(json.dumps(dict(key='a', wav='/w/a.wav', start=1.5)) + '\n')
    with pytest.raises(ValueError):
        R.read_data_list(str(p))


def test_merge_parts_restores_batch_order(tmp_path):
    d = tmp_path / 'm'
    d.mkdir()
    (d / 'text.part0').write_text('0\tu0 a\n0\tu1 b\n2\tu4 e\n')
    (d / 'text.part1').write_text('1\tu2 c\n1\tu3 d\n')
    R.merge_parts(str(tmp_path), ['m'], 2, 3)
    assert (d / 'text').read_text() == 'u0 a\nu1 b\nu2 c\nu3 d\nu4 e\n'
    assert sorted(os.listdir(d)) == ['text']


def test_override_config_and_feature_checks():
    cfg = {'input_dim': 80, 'dataset_conf': {'fbank_conf': {'num_mel_bins': 80}},
           'encoder_conf': {'num_blocks': 12}}
    R.override_config(cfg, ['encoder_conf.num_blocks 6'])
    assert cfg['encoder_conf']['num_blocks'] == 6
    with pytest.raises(KeyError):
        R.override_config(cfg, ['encoder_conf.nope 1'])
    R.check_feature_conf(cfg)
    cfg['dataset_conf']['fbank_conf']['frame_shift'] = 20
    with pytest.raises(NotImplementedError):
        R.check_feature_conf(cfg)
    # the Whisper recipes' frontend (examples/aishell/whisper/conf/finetune_whisper_largev3.yaml)
    wcfg = {'input_dim': 128, 'dataset_conf': {
        'feats_type': 'log_mel_spectrogram',
        'log_mel_spectrogram_conf': {'hop_length': 160, 'n_fft': 400, 'num_mel_bins': 128,
                                     'padding': 0}}}
    R.check_feature_conf(wcfg)

    class M:
        configs = wcfg
        compute_fbank = staticmethod(lambda waves: ('fbank', waves))
        compute_log_mel_spectrogram = staticmethod(lambda waves, **kw: ('log_mel', kw))
    fn, frames_of = R.feature_function(M, wcfg)
    assert frames_of is None and fn(['w']) == (
        'log_mel', dict(num_mel_bins=128, padding=0, pad_or_trim=False, max_duration=30))
    fn, frames_of = R.feature_function(M, cfg)
    assert fn(['w']) == ('fbank', ['w'])
    # kaldi fbank, snip_edges: 25 ms window / 10 ms shift at 16 kHz
    assert [frames_of(n) for n in (0, 399, 400, 559, 560, 160000)] == [0, 0, 1, 1, 2, 998]
    wcfg['dataset_conf']['log_mel_spectrogram_conf']['num_mel_bins'] = 80
    with pytest.raises(NotImplementedError):
        R.check_feature_conf(wcfg)
    with pytest.raises(NotImplementedError):
        R.check_feature_conf({'dataset_conf': {'feats_type': 'mfcc'}})


def test_tokenizer_char_and_bpe_detokenize():
    table = {'<blank>': 0, '<unk>': 1, '▁he': 2, 'llo': 3, '▁wor': 4, 'ld': 5, '你': 6}
    bpe = Tokenizer(table, 'bpe')
    assert bpe.detokenize([2, 3, 4, 5]) == ('he llo wor ld'.replace('he llo', 'hello')
                                            .replace('wor ld', 'world'),
                                            ['▁he', 'llo', '▁wor', 'ld'])
    ch = Tokenizer(table, 'char')
    assert ch.detokenize([6, 6])[0] == '你你'
    assert ch.detokenize([2, 3])[0] == '▁hello'  # char units keep the mark
    assert Tokenizer(table, 'char', connect_symbol=' ').detokenize([6, 6])[0] == '你 你'
    with pytest.raises(KeyError):
        ch.detokenize([99])
    cfg = {}
    assert get_blank_id(cfg, table) == 0 and cfg['ctc_conf']['ctc_blank_id'] == 0
    with pytest.raises(AssertionError):
        get_blank_id({}, {'a': 1})


def test_tokenizers_match_the_reference(tmp_path):
    """Against the reference's init_tokenizer: its detokenize answers, symbol tables and
    the sentencepiece model they were taken with are recorded in
    tests/golden/live_tokenizers.npz (oracle/gen_golden_live.py)."""
    meta, arrays = load_case('live_tokenizers')
    units = tmp_path / 'units.txt'
    syms = ['<blank>', '<unk>', '▁he', 'llo', '▁wor', 'ld', '你', '好', '<sos/eos>']
    units.write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
    assert [r['extra'] for r in meta['char']] == [{}, {'connect_symbol': ' '},
                                                  {'split_with_space': True}]
    for ref in meta['char']:
        cfg = {'tokenizer': 'char',
               'tokenizer_conf': dict(symbol_table_path=str(units), non_lang_syms_path=None,
                                      **ref['extra'])}
        got = init_tokenizer(cfg)
        for ids, want in zip(([6, 7], [2, 3, 4, 5], []), ref['detokenize']):
            text, tokens = got.detokenize(ids)
            assert [text, list(tokens)] == want
        assert got.symbol_table == ref['symbol_table']
    spm = pytest.importorskip('sentencepiece')
    model = tmp_path / 'b.model'
    model.write_bytes(arrays['cli_bpe_model'].tobytes())
    sp = spm.SentencePieceProcessor()
    sp.load(str(model))
    units.write_text(''.join(f'{sp.id_to_piece(i)} {i}\n'
                             for i in range(sp.get_piece_size())))
    cfg = {'tokenizer': 'bpe',
           'tokenizer_conf': dict(symbol_table_path=str(units), non_lang_syms_path=None,
                                  bpe_path=str(model))}
    got = init_tokenizer(cfg)
    ids = sp.encode('HELLO THE CAT')
    assert ids == meta['bpe']['ids']
    text, tokens = got.detokenize(ids)
    assert [text, list(tokens)] == meta['bpe']['detokenize']


def test_transcribe_cli_args():
    from wenet_amd.bin import transcribe as T
    a = T.get_args(['a.wav', '-m', '/models/x'])
    assert a.audio_file == 'a.wav' and a.model == '/models/x' and a.beam is None
    assert a.context_score == 6.0 and a.device == 'cuda'
    with pytest.raises(SystemExit):
        T.get_args(['a.wav'])                      # no model download: -m is required
    with pytest.raises(SystemExit):
        T.get_args(['a.wav', '-m', 'x', '--device', 'cpu'])


def test_read_wav_matches_the_reference_wav_reader(tmp_path):
    """Audio in against the REFERENCE's own reader
    (runtime/core/frontend/wav.h:59-134, built from where it lies into
    oracle/_ref): identical samples for PCM16 / PCM32, mono and stereo, with and
    without extra chunks between `fmt ` and `data`, and the reference's own test
    file.  The reader's answers and that file are recorded in
    tests/golden/live_wav_reader.npz (oracle/gen_golden_live.py)."""
    import numpy as np
    from wenet_amd.model import read_wav
    meta, arrays = load_case('live_wav_reader')
    rng = np.random.Generator(np.random.PCG64(9))
    x = rng.random((3000, 2)) * 1.6 - 0.8
    for bits, scale in ((16, 32768.0), (32, 2147483648.0)):
        for nch in (1, 2):
            # (an odd-sized chunk with its pad byte, which read_wav handles per the
            # RIFF rules, sends the reference's chunk loop out of step: even only)
            for extra in (False, 26):
                p = tmp_path / f'w{bits}_{nch}_{int(extra)}.wav'
                p.write_bytes(_wav_bytes(x[:, :nch], 22050, 1, bits, nch=nch,
                                         extra_chunk=extra))
                name = f'w{bits}_{nch}_{int(extra)}'
                ref, (ch, sr, b) = arrays[name], meta[name]
                got, rate = read_wav(str(p), return_rate=True)
                assert (ch, sr, b) == (nch, 22050, bits) and rate == 22050
                ref0 = ref.reshape(-1, nch)[:, 0]      # first channel (singal_channel)
                assert len(got) == len(ref0) == 3000
                # both are float32 views of the same integers (PCM32 exceeds the
                # 24-bit mantissa: compare after the same float32 rounding)
                np.testing.assert_array_equal(
                    (got.astype(np.float64) * scale).astype(np.float32),
                    ref0.astype(np.float32))
    ref_file = tmp_path / 'aishell-BAC009S0724W0121.wav'
    ref_file.write_bytes(arrays['aishell_riff'].tobytes())
    ref, (ch, sr, b) = arrays['aishell'].astype(np.float32), meta['aishell']
    got, rate = read_wav(str(ref_file), return_rate=True)
    assert (ch, sr, b, rate) == (1, 16000, 16, 16000)
    np.testing.assert_array_equal(got * np.float32(32768.0), ref)


def test_compute_feature_follows_feats_type():
    """load_feature (cli/model.py:47-66): the feature function is chosen by
    dataset_conf.feats_type and gets its <type>_conf.  Dispatch only -- the
    kernels behind it are covered by the GPU tests."""
    import numpy as np
    import torch
    from wenet_amd.model import ASRModel
    calls = []

    class Fake(ASRModel):
        def __init__(self, configs):
            self.configs = configs

        def __del__(self):
            pass

        def load_wav(self, wav_file):
            return np.zeros(1600, np.float32)

        def compute_fbank(self, waves):
            calls.append(('fbank', len(waves)))
            return torch.zeros(1, 9, 80), torch.tensor([8])

        def compute_log_mel_spectrogram(self, waves, **kw):
            calls.append(('log_mel', kw))
            return torch.zeros(1, 10, kw['num_mel_bins']), torch.tensor([10])

    assert Fake({}).compute_feature('a.wav').shape == (8, 80)
    assert Fake({'dataset_conf': {'feats_type': 'fbank'}}).compute_feature('a').shape == (8, 80)
    m = Fake({'dataset_conf': {'feats_type': 'log_mel_spectrogram',
                               'log_mel_spectrogram_conf': {
                                   'num_mel_bins': 128, 'padding': 0, 'pad_or_trim': True,
                                   'max_duration': 30, 'n_fft': 400, 'hop_length': 160}}})
    assert m.compute_feature('a').shape == (10, 128)
    assert calls[-1] == ('log_mel', dict(num_mel_bins=128, padding=0, pad_or_trim=True,
                                         max_duration=30))
    with pytest.raises(NotImplementedError):
        Fake({'dataset_conf': {'feats_type': 'mfcc'}}).compute_feature('a')
    with pytest.raises(NotImplementedError):
        Fake({'dataset_conf': {'feats_type': 'log_mel_spectrogram',
                               'log_mel_spectrogram_conf': {'hop_length': 128}}}
             ).compute_feature('a')


def test_every_reference_recipe_is_accepted_or_refused_cleanly():
    """The reference's own construction test (test/wenet/utils/test_init_model.py:
    every examples/*/*/conf/*.yaml builds) mirrored for this path: each recipe either
    maps to a wn_config or is refused with NotImplementedError naming the key -- never
    a crash, never a silent mis-configuration.  The BASELINE recipes are accepted.  The
    recipes, parsed, are recorded in tests/golden/live_recipes.npz."""
    from wenet_amd.model import config_from_yaml
    accepted, refused = [], {}
    recipes = load_case('live_recipes')[0]
    assert len(recipes) > 50
    for name, c in sorted(recipes.items()):
        if not isinstance(c, dict) or 'encoder_conf' not in c:
            continue
        c.setdefault('input_dim', 80)
        c.setdefault('output_dim', 5000)
        try:
            cfg = config_from_yaml(c)
        except NotImplementedError as e:
            refused[name] = str(e)
            continue
        accepted.append(name)
        assert cfg.d_model % 64 == 0 and cfg.n_layers > 0 and cfg.vocab == c['output_dim']
    for must in ('aishell/s0/conf/train_u2++_conformer.yaml',
                 'aishell/s0/conf/train_conformer.yaml',
                 'librispeech/s0/conf/train_conformer_bidecoder_large.yaml',
                 'wenetspeech/s0/conf/train_u2++_conformer.yaml',
                 'aishell/whisper/conf/finetune_whisper_largev3.yaml'):
        assert must in accepted, (must, refused.get(must))
    for name, why in refused.items():
        assert 'outside the accelerated path' in why, (name, why)
    for family in ('rnnt', 'paraformer'):
        assert not [a for a in accepted if f'/{family}/' in a], family
    # the encoder output is filtered to non-blank frames before rescoring in this recipe
    # (model_conf.apply_non_blank_embedding, asr_model.py:337-342): built in round 3
    # (wn_filter_blank_embedding), so the recipe is on the path
    lite = 'aishell/s0/conf/train_u2++_lite_conformer.yaml'
    assert lite in accepted, refused.get(lite)
    assert len(accepted) >= 25 and len(refused) >= 20
