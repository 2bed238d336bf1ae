"""`tiny_conv2d6` (Conv2dSubsampling6, d 256, causal, dynamic chunk, two decoders) through the
public interface -- load_model on a model directory, decode, the chunk API, StreamingRecognizer,
align -- against what the reference's own model computed on five utterances down to 11 frames,
every utterance alone (tests/golden/conv2d6/tiny_conv2d6.npz, tools/gen_golden_conv2d6.py).

Encoder: 8 e_enc + 16 fp32 ulps of the output scale per utterance, e_enc = the fp32 reference's
own error against its fp64 run; scores: 8 e_score + 16 ulps of |score|; token lists are the
reference's, every utterance, every mode.
"""
import json
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv2d6',
                      'tiny_conv2d6.npz')
MODES = ['ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring']
_CASE = {}


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    if not _CASE:
        import yaml
        from wenet_amd import load_model
        from wenet_amd import synthetic as S
        with np.load(GOLDEN) as z:
            meta = json.loads(bytes(z['meta']).decode())
            arrays = {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}
        configs = S.make_configs(meta['config'])
        d = tmp_path_factory.mktemp('tiny_conv2d6')
        syms = ['<blank>', '<unk>', '<sos/eos>'] + \
            [f'▁w{i}' for i in range(3, configs['output_dim'])]
        (d / 'units.txt').write_text(''.join(f'{s} {i}\n' for i, s in enumerate(syms)))
        (d / 'train.yaml').write_text(yaml.safe_dump(configs))
        torch.save(S.make_state_dict(configs, meta['wseed']), d / 'final.pt')
        feats = [S.make_features(1, n, seed=meta['fseed'] + i)[0][0].cuda()
                 for i, n in enumerate(meta['frames'])]
        _CASE.update(meta=meta, arrays=arrays, model=load_model(str(d)), feats=feats)
    yield _CASE


def _close(what, got, ref, e):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = 8 * e + 16 * KR.ULP32 * ref.abs().max().item()
    print(f'{what}: err={err:.3e} e_ref={e:.3e} bound={bound:.3e}')
    assert torch.isfinite(got).all() and err <= bound, what


def test_model_is_rate_six(case):
    m = case['model']
    assert (m._cfg.input_layer, m._cfg.d_model, m.subsampling_rate(), m.right_context()) == \
        (2, 256, 6, 10)


@pytest.mark.parametrize('kind', ['full', 'c4', 'cbc'])
def test_encoder_against_the_fp64_reference(case, kind):
    """Full context, decoding_chunk_size 4, and chunk by chunk through wn_encode_chunk_batch."""
    m, meta = case['model'], case['meta']
    for i, n in enumerate(meta['frames']):
        x, ln = case['feats'][i].unsqueeze(0), torch.tensor([n], dtype=torch.int32)
        if kind == 'cbc':
            out = m.forward_encoder_chunk_by_chunk(x, 4, -1)[0]
        else:
            out, mask = m._forward_encoder(x, ln, *((4, -1) if kind == 'c4' else ()))
            assert int(mask.sum()) == meta['enc_lens'][i]
        _close(f'encoder {kind}[{n}]', out[0], case['arrays'][f'enc64_{kind}_{n}'],
               meta[f'e_enc_{kind}'][i])


def test_batch_gives_each_utterance_its_own_frames(case):
    """The five utterances as one padded batch (the padding holds large values)."""
    m, meta, feats = case['model'], case['meta'], case['feats']
    x = torch.full((len(feats), max(meta['frames']), 80), 1.0e30, device='cuda')
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    out, mask = m._forward_encoder(x, torch.tensor(meta['frames'], dtype=torch.int32))
    assert mask.squeeze(1).sum(1).tolist() == meta['enc_lens']
    for i, n in enumerate(meta['frames']):
        _close(f'batched encoder[{n}]', out[i, :meta['enc_lens'][i]],
               case['arrays'][f'enc64_full_{n}'], meta['e_enc_full'][i])


@pytest.mark.parametrize('mode', MODES)
def test_decode_modes_are_the_references(case, mode):
    m, meta = case['model'], case['meta']
    for i, n in enumerate(meta['frames']):
        r = m.decode([mode], case['feats'][i].unsqueeze(0), torch.tensor([n], dtype=torch.int32),
                     **meta['kw'])[mode][0]
        assert list(r.tokens) == meta['tokens'][mode][i], (mode, n)
        want, e = meta['scores'][mode][i], meta['e_score'][mode][i]
        bound = 8 * e + 16 * KR.ULP32 * abs(want)
        print(f'{mode}[{n}]: got={float(r.score):.6f} ref={want:.6f} bound={bound:.3e}')
        assert abs(float(r.score) - want) <= bound, (mode, n)


def test_streaming_recognizer_and_align(case):
    """A session fed in pieces emits the chunk-by-chunk encoder frames; align counts 60 ms."""
    from wenet_amd.streaming import StreamingRecognizer
    m, meta = case['model'], case['meta']
    n, f = meta['frames'][-1], case['feats'][-1]
    rec = StreamingRecognizer(m, 1, 4, -1, beam_size=5, max_seconds=n / 100.0)
    sid = rec.open()
    for a in range(0, n, 50):
        rec.accept(sid, f[a:a + 50])
        while rec.step():
            pass
    rec.finish(sid, rescoring=False)
    _close(f'streamed encoder[{n}]', rec.encoder_out(sid)[0], case['arrays'][f'enc64_cbc_{n}'],
           meta['e_enc_cbc'][-1])
    rec.close(sid)
    labels = meta['tokens']['ctc_prefix_beam_search'][-1]
    res = m.align(f.unsqueeze(0), torch.tensor([n], dtype=torch.int32), [labels])[0]
    assert res.ok and len(res.alignment) == meta['enc_lens'][-1]
    edges = [res.intervals[0][0]] + [iv[1] for iv in res.intervals]
    assert edges[0] == 0.0 and abs(edges[-1] - 0.06 * meta['enc_lens'][-1]) < 1e-9
    assert all(abs(e / 0.06 - round(e / 0.06)) < 1e-6 for e in edges), edges
