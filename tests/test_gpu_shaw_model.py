"""A W2v-BERT 2.0 / conformer_shaw model end to end on the GPU (wenet_amd/shaw.py,
csrc/cabi_shaw.hip): `tiny_shaw` from a model directory against what the real reference computed
for every utterance ALONE (tools/gen_golden_shaw.py -> tests/golden/shaw/tiny_shaw.npz), and one
block at the converter's widths against the batch-of-one result.

Tolerances: the encoder output within 8 e_enc + 16 fp32 ulps of its scale, a score within
8 e_score + 16 ulps of its size, e_enc / e_score = the fp32 reference's own error against its
fp64 run; token lists equal the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR
import shaw_refs as SR

pytestmark = pytest.mark.gpu

METHODS = ['ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shaw', 'tiny_shaw.npz')


def _padded(feats):
    lens = torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)
    x = torch.zeros(len(feats), int(lens.max()), feats[0].shape[1])
    for b, f in enumerate(feats):
        x[b, :f.shape[0]] = f
    return x, lens


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    import wenet_amd
    from wenet_amd import synthetic as S
    with np.load(GOLDEN) as z:
        meta = json.loads(bytes(z['meta']).decode())
        enc = {k: z[k] for k in z.files if k != 'meta'}
    path = S.write_model_dir(str(tmp_path_factory.mktemp('tiny_shaw')), 'tiny_shaw', meta['wseed'])
    model = wenet_amd.load_model(path)
    x, lens = _padded(SR.tiny_features())
    out, mask = model._forward_encoder(x, lens)
    return dict(model=model, meta=meta, enc=enc, x=x, lens=lens, out=out.cpu(),
                enc_lens=mask.squeeze(1).sum(1).cpu().tolist())


def test_class_and_rates(tiny):
    import wenet_amd
    m = tiny['model']
    assert isinstance(m, wenet_amd.ShawConformer)
    assert (m.subsampling_rate(), m.right_context()) == (2, 0)
    assert tiny['enc_lens'] == [n // 2 for n in SR.TINY['frames']]


def test_encoder_against_reference(tiny):
    for i, n in enumerate(tiny['enc_lens']):
        if n == 0:
            continue
        ref = torch.from_numpy(tiny['enc'][f'enc64_{i}'])
        err = (tiny['out'][i, :n].double() - ref).abs().max().item()
        b = 8 * tiny['meta']['e_enc'][i] + 16 * KR.ULP32 * ref.abs().max().item()
        print(f'utterance {i}: err={err:.3e} bound={b:.3e}')
        assert err <= b


def test_batched_bits_equal_alone_bits(tiny):
    m = tiny['model']
    for i, n in enumerate(tiny['enc_lens']):
        L = int(tiny['lens'][i])
        out, _ = m._forward_encoder(tiny['x'][i:i + 1, :L], tiny['lens'][i:i + 1])
        assert out.shape[1] == n
        assert torch.equal(out[0].cpu().view(torch.int32), tiny['out'][i, :n].view(torch.int32))


def test_decode_against_reference(tiny):
    """The CTC modes on all six utterances; attention_rescoring on the five that have encoder
    frames (the rescoring entry point refuses an utterance without any, and the reference has no
    result for it either)."""
    meta, m = tiny['meta'], tiny['model']
    res = m.decode(METHODS[:2], tiny['x'], tiny['lens'], beam_size=meta['beam'])
    res['attention_rescoring'] = m.decode(METHODS[1:], tiny['x'][:5], tiny['lens'][:5],
                                          beam_size=meta['beam'],
                                          ctc_weight=meta['ctc_weight'])['attention_rescoring']
    for i, want in enumerate(meta['tokens']):
        if want is None:                    # no encoder frame: nothing to decode
            assert all(list(res[k][i].tokens) == [] for k in METHODS[:2])
            continue
        for k in METHODS:
            got = res[k][i]
            assert list(map(int, got.tokens)) == want[k], (i, k)
            s = meta['scores'][i][k]
            b = 8 * meta['e_score'][i][k] + 16 * KR.ULP32 * max(abs(s), 1.0)
            print(f'utterance {i} {k}: |ds|={abs(got.score - s):.3e} bound={b:.3e}')
            assert abs(got.score - s) <= b


def test_align_times_are_20_ms_frames(tiny):
    labels = [tiny['meta']['tokens'][0]['ctc_greedy_search']]
    r = tiny['model'].align(tiny['x'][:1], tiny['lens'][:1], labels)[0]
    assert r.ok and len(r.alignment) == 72
    lead = next(i for i, t in enumerate(r.frames[0]) if t != 0)
    dur = sum(1 for t in r.frames[0] if t != 0)
    begin, end, _ = r.intervals[0]
    assert begin == pytest.approx(lead * 0.02) and end == pytest.approx((lead + dur) * 0.02)


@pytest.fixture(scope='module')
def wide():
    from wenet_amd import synthetic as S
    from wenet_amd.shaw import ShawConformer
    configs = S.make_configs('w2vbert_600m_1blk')
    return ShawConformer(configs, S.make_state_dict(configs, 1))


def test_converter_decoder_spelling_runs_ctc_only(wide):
    """decoder_conf.attention_head (the converter's spelling) leaves 4 heads of 256: the model
    loads, the CTC modes run, the attention modes are refused by name."""
    from wenet_amd import synthetic as S
    x, lens = S.make_features(2, (150, 200), seed=3)
    res = wide.decode(['ctc_greedy_search', 'ctc_prefix_beam_search'], x, lens, beam_size=3)
    assert len(res['ctc_greedy_search']) == 2
    for m in ('attention_rescoring', 'attention'):
        with pytest.raises(NotImplementedError, match=m):
            wide.decode([m], x, lens, beam_size=3)
    with pytest.raises(NotImplementedError, match='bf16'):
        wide.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError, match='decoding_chunk_size'):
        wide.decode(['ctc_greedy_search'], x, lens, decoding_chunk_size=16)


def test_one_block_at_the_converters_widths(wide):
    """d 1024, 16 heads, 4096 units, K 31 causal, 200 frames (400 feature frames) against the fp64
    formulation of the layer in tests/shaw_refs.py."""
    from wenet_amd import synthetic as S
    configs = S.make_configs('w2vbert_600m_1blk')
    sd = S.make_state_dict(configs, 1)
    x, lens = S.make_features(1, 400, seed=4)
    out, _ = wide._forward_encoder(x, lens)
    ref = SR.ref_encoder(x[0], sd, configs)
    plain = SR.ref_encoder(x[0], sd, configs, fp32=True)
    e_enc = (plain - ref).abs().max().item()
    err = (out[0].cpu().double() - ref).abs().max().item()
    b = 8 * e_enc + 16 * KR.ULP32 * ref.abs().max().item()
    print(f'one block at d 1024: err={err:.3e} e_enc={e_enc:.3e} bound={b:.3e}')
    assert out.shape[1] == 200 and err <= b
