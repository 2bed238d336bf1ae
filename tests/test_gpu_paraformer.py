"""Paraformer on the GPU (wenet_amd.Paraformer: csrc/cabi_paraformer.hip) against what the real
reference computed for `tiny_paraformer` (tests/golden/paraformer/tiny*.npz, recorded by
tools/gen_golden_paraformer.py with every utterance ALONE), and one encoder block + one decoder
block at the recipe's widths against the fp64 formulation of tests/paraformer_refs.py.

Bounds: the encoder output within 8 e_enc + 16 fp32 ulps of its scale of the fp64 reference,
log(tokens_confidence) within 8 e_logp + 16 ulps, e_* = the fp32 reference's own error against
fp64 on the same utterance.  Token numbers, fire frames and the token lists of all four methods
equal the recorded ones; the six utterances batched give the bits each gives alone.
"""
import math
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR
import paraformer_refs as PR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'paraformer')
METHODS = ['paraformer_greedy_search', 'paraformer_beam_search', 'ctc_greedy_search',
           'ctc_prefix_beam_search']


def _batch(feats):
    T = max(f.shape[0] for f in feats)
    x = torch.zeros(len(feats), T, 80)
    for i, f in enumerate(feats):
        x[i, :f.shape[0]] = f
    return x, torch.tensor([f.shape[0] for f in feats], dtype=torch.int32)


def _run(model, feats):
    """decode + the raw arrays of one batch: per utterance (encoder rows, token number, fire
    frames, tokens of every method, log-probs, confidences)."""
    x, lens = _batch(feats)
    enc, mask = model._forward_encoder(x, lens)
    res = model.decode(METHODS, x, lens, beam_size=PR.CTC_BEAM)
    raw = model._forward_paraformer(x, lens)
    torch.cuda.synchronize()
    out = []
    for b, f in enumerate(feats):
        tp = PR.lfr_rows(f.shape[0])
        assert int(mask[b].sum()) == tp
        n = int(raw['decoder_out_lens'][b])
        out.append(dict(enc=enc[b, :tp].cpu(), token_num=n,
                        fires=raw['fire_frames'][b, :int(raw['n_fire'][b])].tolist(),
                        logp=raw['decoder_out'][b, :n].copy(),
                        tokens={m: list(res[m][b].tokens) for m in METHODS},
                        greedy=res['paraformer_greedy_search'][b]))
    return out


@pytest.fixture(scope='module')
def tiny():
    from wenet_amd import synthetic as S
    from wenet_amd.paraformer import Paraformer
    meta, arr = PR.load_golden(GOLDEN, 'tiny')
    configs = S.make_configs('tiny_paraformer')
    model = Paraformer(configs, S.make_state_dict(configs, meta['wseed']))
    feats = PR.tiny_features()
    alone = [_run(model, [f])[0] for f in feats]
    return dict(meta=meta, arr=arr, model=model, feats=feats, alone=alone)


def test_encoder_output_against_fp64(tiny):
    meta, arr = tiny['meta'], tiny['arr']
    for i, n in enumerate(PR.TINY_LENS):
        if n not in PR.TINY_ENC_SAVED:
            continue
        ref = torch.from_numpy(arr[f'enc64_{n}'])
        err = (tiny['alone'][i]['enc'].double() - ref).abs().max().item()
        bound = 8 * meta['e_enc'][i] + 16 * KR.ULP32 * ref.abs().max().item()
        print(f'enc[{n}] err={err:.3e} e_enc={meta["e_enc"][i]:.3e} bound={bound:.3e}')
        assert err <= bound


def test_token_numbers_fires_and_tokens(tiny):
    meta = tiny['meta']
    for i, r in enumerate(tiny['alone']):
        assert r['token_num'] == meta['token_num'][i], i
        assert r['fires'] == meta['fire_frames'][i], i
        for m in METHODS:
            assert r['tokens'][m] == meta['tokens'][m][i], (m, i)
        assert r['greedy'].times == []


def test_token_log_probs_against_fp64(tiny):
    meta, arr = tiny['meta'], tiny['arr']
    for i, n in enumerate(PR.TINY_LENS):
        r = tiny['alone'][i]
        if meta['raised'][i]:
            continue
        ref = arr[f'logp64_{n}']
        got = np.log(np.asarray(r['greedy'].tokens_confidence, dtype=np.float64))
        err = float(np.abs(got - ref).max())
        bound = 8 * meta['e_logp'][i] + 16 * KR.ULP32 * float(np.abs(ref).max())
        print(f'logp[{n}] err={err:.3e} e_logp={meta["e_logp"][i]:.3e} bound={bound:.3e}')
        assert err <= bound
        assert abs(math.log(r['greedy'].confidence) - float(ref.mean())) <= bound


def _same(a, b, what):
    assert torch.equal(a['enc'].view(torch.int32), b['enc'].view(torch.int32)), what
    assert a['token_num'] == b['token_num'] and a['fires'] == b['fires'], what
    assert a['tokens'] == b['tokens'], what
    assert np.array_equal(a['logp'].view(np.int32), b['logp'].view(np.int32)), what


def test_batched_is_bit_identical_to_alone(tiny):
    got = _run(tiny['model'], tiny['feats'])
    for i, (a, b) in enumerate(zip(got, tiny['alone'])):
        _same(a, b, f'utterance {i} of the batch of six')
    # 24 frames as the longest of its batch (n % 6 == 0: the reference's batched LFR would pad
    # the 7-frame utterance from the batch's zero padding)
    got = _run(tiny['model'], tiny['feats'][3:])
    for i, (a, b) in enumerate(zip(got, tiny['alone'][3:])):
        _same(a, b, f'utterance {i + 3} beside the 24-frame one')


def test_zero_token_utterance(tiny):
    """One frame: alpha + 0.45 < 1, no token.  The reference raises (recorded); here the empty
    result, alone and between neighbours."""
    assert tiny['meta']['raised'][5] and tiny['alone'][5]['token_num'] == 0
    g = tiny['alone'][5]['greedy']
    assert (g.tokens, g.confidence, g.tokens_confidence) == ([], 0.0, [])
    feats = [tiny['feats'][1], tiny['feats'][5], tiny['feats'][4]]
    got = _run(tiny['model'], feats)
    assert got[1]['token_num'] == 0 and got[1]['greedy'].tokens == []
    _same(got[0], tiny['alone'][1], 'the neighbour in front')
    _same(got[2], tiny['alone'][4], 'the neighbour behind')


def test_refusals(tiny):
    model = tiny['model']
    x, lens = _batch(tiny['feats'][3:4])
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        model.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        model.decode(['paraformer_greedy_search'], x, lens, decoding_chunk_size=4)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        model.decode(['paraformer_greedy_search'], x, lens, simulate_streaming=True)
    with pytest.raises(NotImplementedError, match='outside the accelerated path'):
        model.decode(['attention_rescoring'], x, lens)
    with pytest.raises(NotImplementedError):
        model.clone()
    from wenet_amd.pipeline import DecodePipeline
    with pytest.raises(NotImplementedError):
        DecodePipeline(model)


def test_load_model_and_transcribe(tmp_path):
    import wave
    import wenet_amd
    from wenet_amd import synthetic as S
    path = S.write_model_dir(str(tmp_path / 'pf'), 'tiny_paraformer', seed=0)
    model = wenet_amd.load_model(path)
    assert isinstance(model, wenet_amd.Paraformer)
    assert model.default_decode_method == 'paraformer_greedy_search'
    pcm = (S.make_audio(24000) * 32767.0).astype('<i2')
    wav = str(tmp_path / 'a.wav')
    with wave.open(wav, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    r = model.transcribe(wav)
    speech = model.compute_feature(wav)
    d = model.decode(['paraformer_greedy_search'], speech.unsqueeze(0),
                     torch.tensor([speech.size(0)]))['paraformer_greedy_search'][0]
    assert r.tokens == d.tokens and isinstance(r.text, str)


def _held_to_formulation(configs, n_frames, name):
    """One utterance of a model with synthetic weights against tests/paraformer_refs.ref_paraformer
    in fp64 (pinned to the reference's modules and model on the CPU, tests/test_paraformer_host.py);
    e_plain = the same formulation evaluated in fp32.  The weight seed is the first whose fp64
    result has the fixture's margins."""
    from wenet_amd import synthetic as S
    from wenet_amd.paraformer import Paraformer
    f = PR.features(n_frames, 31)
    for seed in range(20):
        sd = S.make_state_dict(configs, seed)
        r64 = PR.ref_paraformer(sd, configs, f)
        a = np.concatenate([r64['alphas'].numpy(), [float(np.float32(0.45))]])
        gap = (r64['logp'].topk(2, dim=-1).values if r64['logp'] is not None else None)
        if r64['token_num'] >= 5 and PR.fire_margin(a[:-1], a[-1]) >= 1e-3 and \
                abs(a.sum() - round(a.sum())) >= 1e-2 and \
                float((gap[:, 0] - gap[:, 1]).min()) >= 1e-3:
            break
    else:
        pytest.fail('no weight seed with margins')
    r32 = PR.ref_paraformer(sd, configs, f, fp32=True)
    assert r32['fires'] == r64['fires'] and r32['token_num'] == r64['token_num']
    model = Paraformer(configs, sd)
    got = _run(model, [f])[0]
    assert got['token_num'] == r64['token_num'] and got['fires'] == r64['fires']
    e_enc = (r32['enc'] - r64['enc']).abs().max().item()
    scale = r64['enc'].abs().max().item()
    err = (got['enc'].double() - r64['enc']).abs().max().item()
    print(f'{name} enc err={err:.3e} e_plain={e_enc:.3e} tokens={got["token_num"]}')
    assert KR.cap_ok(e_enc, scale) and err <= KR.bound(e_enc, scale)
    top64, top32 = r64['logp'].max(dim=-1), r32['logp'].max(dim=-1)
    assert got['tokens']['paraformer_greedy_search'] == top64.indices.tolist()
    e_lp = (top32.values - top64.values).abs().max().item()
    s_lp = top64.values.abs().max().item()
    err = float(np.abs(got['logp'].astype(np.float64) - top64.values.numpy()).max())
    print(f'{name} logp err={err:.3e} e_plain={e_lp:.3e}')
    assert KR.cap_ok(e_lp, s_lp) and err <= KR.bound(e_lp, s_lp)


def test_one_block_at_the_recipe_widths():
    """encoders0 + one encoder block and one decoder block at d 512, 4 heads of 128, 2048 units,
    T' = 40, against the fp64 formulation."""
    from wenet_amd import synthetic as S
    _held_to_formulation(S.make_configs('paraformer_large_1blk'), 240, '1blk')


def test_heads_of_64_run_on_the_existing_attention_kernel():
    """`tiny_paraformer` with 4 heads at d 256 (d_k = 64): self attention and the decoder's cross
    attention (separate Q and K / V layouts) go through attention(); T' = 33, two key tiles."""
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_paraformer')
    configs['encoder_conf']['attention_heads'] = 4
    configs['decoder_conf']['attention_heads'] = 4
    _held_to_formulation(configs, 196, 'dk64')


def test_padded_wider_than_the_longest_utterance(tiny):
    """speech.shape[1] past max(speech_lengths), across a 6-frame boundary (24 frames in a
    tensor of 25 and of 40; the 7-frame utterance beside it): the bits of the exact padding."""
    model = tiny['model']
    feats = [tiny['feats'][3], tiny['feats'][4]]
    lens = torch.tensor([24, 7], dtype=torch.int32)
    for width in (25, 40):
        x = torch.full((2, width, 80), 1e18)
        for i, f in enumerate(feats):
            x[i, :f.shape[0]] = f
        enc, mask = model._forward_encoder(x, lens)
        assert enc.shape[1] == -(-width // 6) and mask.sum(-1).flatten().tolist() == [4, 2]
        res = model.decode(METHODS, x, lens, beam_size=PR.CTC_BEAM)
        raw = model._forward_paraformer(x, lens)
        for b, ref in enumerate(tiny['alone'][3:5]):
            tp, n = ref['enc'].shape[0], ref['token_num']
            assert torch.equal(enc[b, :tp].cpu().view(torch.int32), ref['enc'].view(torch.int32))
            assert int(raw['decoder_out_lens'][b]) == n
            assert np.array_equal(raw['decoder_out'][b, :n].view(np.int32),
                                  ref['logp'].view(np.int32))
            assert {m: list(res[m][b].tokens) for m in METHODS} == ref['tokens']
    # no frame at all: nothing to decode, no error
    res = model.decode(['paraformer_greedy_search', 'paraformer_beam_search'], x,
                       torch.tensor([0, 0], dtype=torch.int32))
    assert [r.tokens for r in res['paraformer_greedy_search']] == [[], []]
