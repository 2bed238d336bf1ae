"""Encoders with heads of 32 run them 32 wide on attention_d32_relpos: `tiny_ebranchformer` and
the plain layers of `tiny_efficonformer_v1`; `tiny_branchformer` (heads of 64) stays on
attention_kernel.  The route is read from ASRModel.encoder_head_cols; the encoder outputs are held
to the recorded fp64 references of tests/golden/ with the bound of the model tests, 8 e_enc + 16
fp32 ulps of the output scale, at full context and under the recorded chunk mask, and a batch
gives the bits every utterance gives alone.
"""
import pytest
import torch

import branchformer_refs as BR
import efficonformer_refs as EF
from test_gpu_branchformer import _batch, _enc_ok

pytestmark = pytest.mark.gpu

COLS = {'tiny_ebranchformer': 32, 'tiny_efficonformer_v1': 32, 'tiny_branchformer': 64}
_MODELS = {}


def model(name):
    if name not in _MODELS:
        from wenet_amd import Branchformer, EfficientConformer
        from wenet_amd import synthetic as S
        R, cls = (EF, EfficientConformer) if 'effi' in name else (BR, Branchformer)
        meta, arrays = R.load_fixture(name)
        configs = S.make_configs(name)
        m = cls(configs, S.make_state_dict(configs, meta['wseed']), device='cuda:0')
        feats = EF.tiny_features(name) if R is EF else BR.tiny_features(name)
        _MODELS[name] = (m, meta, arrays, feats)
    return _MODELS[name]


@pytest.mark.parametrize('name', sorted(COLS))
def test_route(name):
    assert model(name)[0].encoder_head_cols == COLS[name]


@pytest.mark.parametrize('name', [n for n in sorted(COLS) if COLS[n] == 32])
def test_encoder_against_the_fp64_reference(name):
    m, meta, arrays, feats = model(name)
    x, lens = _batch(feats)
    out = m._forward_encoder(x, lens)[0].clone()
    for i, n in enumerate(meta['frames']):
        ref = torch.from_numpy(arrays[f'enc64_{n}'])
        _enc_ok(f'{name} encoder[{n}]', out[i, :ref.shape[0]].double().cpu(), ref,
                meta['e_enc'][i])
        o1 = m._forward_encoder(feats[i].unsqueeze(0), torch.tensor([feats[i].shape[0]]))[0]
        assert torch.equal(o1[0].view(torch.int32), out[i, :o1.shape[1]].view(torch.int32)), i


def test_chunk_mask():
    """The recorded chunk mask (4 frames, all left chunks) of tiny_efficonformer_v1: chunks of 2
    rows on its plain layers behind the stride layer.  (tiny_ebranchformer has none recorded.)"""
    name = 'tiny_efficonformer_v1'
    m, meta, arrays, feats = model(name)
    chunk, left = EF.TINY[name]['chunk_cases'][0]
    idx = [i for i, n in enumerate(meta['frames']) if f'enc64_{n}_c{chunk}_l{left}' in arrays]
    assert len(idx) == 2
    x, lens = _batch([feats[i] for i in idx])
    out = m._forward_encoder(x, lens, chunk, left)[0]
    for j, i in enumerate(idx):
        key = f'{meta["frames"][i]}_c{chunk}_l{left}'
        ref = torch.from_numpy(arrays['enc64_' + key])
        _enc_ok(f'{name} chunk[{key}]', out[j, :ref.shape[0]].double().cpu(), ref,
                meta['e_enc_chunk'][key])
