"""W2v-BERT 2.0 from audio through the public interface: `tiny_shaw` under the `w2vbert_fbank`
recipe (synthetic `tiny_shaw_w2vbert`), synthetic PCM of 98, 153 (odd), 248 and 323 frames.

Tolerances: the normalised features within kernel_refs.bound(e_plain, scale) of the fp64
normalisation of compute_fbank's own output; the encoder fed raw fbank (set_raw_fbank_input, the
division inside the front end) within 8 e_enc + 16 fp32 ulps of its scale of the encoder fed the
fp64-normalised features rounded to fp32, e_enc = the fp32 run of shaw_refs.ref_encoder with the
normalisation in front against its fp64 run."""
import wave

import numpy as np
import pytest
import torch

import kernel_refs as KR
import shaw_refs as SR
import utt_norm_refs as UR
from test_gpu_attention_d32 import record

pytestmark = pytest.mark.gpu

SAMPLES = [52000, 40000, 24720, 16000]       # 323, 248, 153 (odd), 98 frames (under 2 s)


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    import wenet_amd
    from wenet_amd import synthetic as S
    d = tmp_path_factory.mktemp('tiny_shaw_w2vbert')
    model = wenet_amd.load_model(S.write_model_dir(str(d), 'tiny_shaw_w2vbert', 3))
    waves = [S.make_audio(n, seed=20 + i) for i, n in enumerate(SAMPLES)]
    raw, lens = model.compute_fbank(waves)
    got, got_lens = model.compute_w2vbert_fbank(waves)
    assert got_lens.tolist() == lens.tolist() == [323, 248, 153, 98]
    raw = raw.cpu()
    r64 = [UR.normalize(raw[i, :n])[2] for i, n in enumerate(lens.tolist())]
    model.set_raw_fbank_input(True)
    enc_b, _ = model._forward_encoder(raw, lens)
    model.set_raw_fbank_input(False)
    return dict(model=model, dir=d, waves=waves, raw=raw, lens=lens, got=got.cpu(), r64=r64,
                enc_b=enc_b.cpu())


def test_compute_w2vbert_fbank(case):
    assert isinstance(case['model'], __import__('wenet_amd').ShawConformer)
    for i, n in enumerate(case['lens'].tolist()):
        ref = case['r64'][i]
        plain = UR.normalize(case['raw'][i, :n], fp32=True)[2]
        record(f'w2vbert_fbank[len={n}]', (case['got'][i, :n].double() - ref).abs().max().item(),
               (plain.double() - ref).abs().max().item(), ref.abs().max().item())
        assert bool((case['got'][i, n:] == 0).all())


def test_encoder_on_raw_fbank(case):
    m = case['model']
    configs, sd = m.configs, torch.load(str(case['dir'] / 'final.pt'))
    x = torch.zeros_like(case['raw'])
    for i, r in enumerate(case['r64']):
        x[i, :r.shape[0]] = r.float()
    enc_a = m._forward_encoder(x, case['lens'])[0].cpu()
    for i, n in enumerate(case['lens'].tolist()):
        ref = SR.ref_encoder(case['r64'][i], sd, configs)
        plain = SR.ref_encoder(UR.normalize(case['raw'][i, :n], fp32=True)[2], sd, configs,
                               fp32=True)
        e_enc = (plain - ref).abs().max().item()
        err = (case['enc_b'][i, :n // 2] - enc_a[i, :n // 2]).abs().max().item()
        b = 8 * e_enc + 16 * KR.ULP32 * ref.abs().max().item()
        print(f'raw fbank route, len={n}: err={err:.3e} e_enc={e_enc:.3e} bound={b:.3e}')
        assert err <= b


def test_batched_bits_equal_alone_bits(case):
    m = case['model']
    for i, n in enumerate(case['lens'].tolist()):
        alone, _ = m.compute_w2vbert_fbank(case['waves'][i:i + 1])
        assert torch.equal(alone[0].cpu().view(torch.int32), case['got'][i, :n].view(torch.int32))
        m.set_raw_fbank_input(True)
        enc, _ = m._forward_encoder(case['raw'][i:i + 1, :n], case['lens'][i:i + 1])
        m.set_raw_fbank_input(False)
        assert torch.equal(enc[0].cpu().view(torch.int32),
                           case['enc_b'][i, :n // 2].view(torch.int32))


def test_transcribe_a_wav(case):
    """transcribe() under ctc_greedy_search as the model's default method: the tokens of decode()
    on the features compute_w2vbert_fbank makes of the same samples."""
    m = case['model']
    m.default_decode_method = 'ctc_greedy_search'
    wav = str(case['dir'] / 'a.wav')
    pcm = np.clip(case['waves'][2] * 32768, -32768, 32767).astype(np.int16)
    with wave.open(wav, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    feats, lens = m.compute_w2vbert_fbank([pcm.astype(np.float32) / 32768])
    assert torch.equal(m.compute_feature(wav), feats[0])
    want = m.decode(['ctc_greedy_search'], feats, lens)['ctc_greedy_search'][0]
    assert list(m.transcribe(wav).tokens) == list(want.tokens)
