"""Rotary Conformer models end to end on the GPU (wenet_amd/rope.py, csrc/cabi_rope.hip):
`tiny_rope` (GQA, causal, dynamic chunk) and `tiny_rope_mqa` (MQA, batch_norm) from a model
directory against what the real reference computed for every utterance ALONE
(tools/gen_golden_rope.py -> tests/golden/rope/).

Tolerances: the encoder output within 8 e_enc + 16 fp32 ulps of its scale, a score within
8 e_score + 16 ulps of its size, e_enc / e_score = the fp32 reference's own error against its
fp64 run; token lists equal the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR
import rope_refs as RR

pytestmark = pytest.mark.gpu

METHODS = ['ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rope')


@pytest.fixture(scope='module', params=sorted(RR.MODELS))
def tiny(request, tmp_path_factory):
    import wenet_amd
    from wenet_amd import synthetic as S
    name = request.param
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        meta = json.loads(bytes(z['meta']).decode())
        enc = {k: z[k] for k in z.files if k != 'meta'}
    model = wenet_amd.load_model(S.write_model_dir(str(tmp_path_factory.mktemp(name)), name,
                                                   meta['wseed']))
    assert isinstance(model, wenet_amd.RopeConformer)
    feats = RR.model_features(name)
    lens = torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)
    x = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    return dict(model=model, meta=meta, enc=enc, x=x, lens=lens)


def test_encoder_against_reference(tiny):
    """Every recorded setting, all utterances in one batch."""
    for s, (chunk, left) in enumerate(tiny['meta']['settings']):
        out, mask = tiny['model']._forward_encoder(tiny['x'], tiny['lens'], chunk, left)
        for i, n in enumerate(mask.squeeze(1).sum(1).tolist()):
            ref = torch.from_numpy(tiny['enc'][f'enc64_{s}_{i}'])
            assert ref.shape[0] == n
            err = (out[i, :n].cpu().double() - ref).abs().max().item()
            b = 8 * tiny['meta']['e_enc'][s][i] + 16 * KR.ULP32 * ref.abs().max().item()
            print(f'chunk {chunk} left {left} utterance {i}: err={err:.3e} bound={b:.3e}')
            assert err <= b


def test_batched_bits_equal_alone_bits(tiny):
    m = tiny['model']
    chunk, left = tiny['meta']['settings'][-1]
    batched, _ = m._forward_encoder(tiny['x'], tiny['lens'], chunk, left)
    for i, L in enumerate(tiny['lens'].tolist()):
        out, _ = m._forward_encoder(tiny['x'][i:i + 1, :L], tiny['lens'][i:i + 1], chunk, left)
        n = out.shape[1]
        assert torch.equal(out[0].view(torch.int32), batched[i, :n].view(torch.int32))


def test_decode_against_reference(tiny):
    meta = tiny['meta']
    res = tiny['model'].decode(METHODS, tiny['x'], tiny['lens'], beam_size=meta['beam'],
                               ctc_weight=meta['ctc_weight'],
                               reverse_weight=meta['reverse_weight'])
    for i, want in enumerate(meta['tokens']):
        for k in METHODS:
            got = res[k][i]
            assert list(map(int, got.tokens)) == want[k], (i, k)
            s = meta['scores'][i][k]
            b = 8 * meta['e_score'][i][k] + 16 * KR.ULP32 * max(abs(s), 1.0)
            print(f'utterance {i} {k}: |ds|={abs(got.score - s):.3e} bound={b:.3e}')
            assert abs(got.score - s) <= b


def test_refusals_by_name(tiny):
    m = tiny['model']
    with pytest.raises(NotImplementedError, match='bf16'):
        m.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError, match='simulate_streaming'):
        m._forward_encoder(tiny['x'][:1], tiny['lens'][:1], 4, 2, simulate_streaming=True)
    with pytest.raises(ValueError, match='speech_lengths'):
        m._forward_encoder(torch.zeros(1, 12008, 80), torch.tensor([12008], dtype=torch.int32))
