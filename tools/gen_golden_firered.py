#!/usr/bin/env python3
"""Record what the REAL reference's FireRedASR encoder modules (wenet/models/firered/) compute,
for tests/test_firered_host.py.

    python tools/gen_golden_firered.py        # CPU only; needs the reference tree

Recorded in tests/golden/firered/firered_modules.npz, every module in fp64 (.double()) on the
inputs tests/firered_refs.py rebuilds from their seeds:
  attn_out    FiredRelPositionMultiHeadedAttention(H = 2, d = 128, no q / k / v bias).forward on
              one 40-frame utterance with the position rows FireRedRelPositionalEncoding hands
              it -- the pin of ref_attention_relshift (the distance, its sign, the three
              LayerNorms, eps) and of the LayerNorm fold
  pos_emb_rows  rows firered_refs.POS_ROWS of those position rows (2 T - 1, d): the pin of
              firered_refs.rel_positions
  front_alone_<n>   FireRedConv2dSubsampling4(80, 64, odim 32).forward of an utterance of n
              frames decoded alone (97 and 61 frames): the pin of ref_firered_frontend + the
              output projection, and of the T' rule
  meta.batched_lens  the frames the reference's own mask gives the same two utterances decoded
              as ONE batch (the 61-frame one gets 17, alone it gets 16: DESIGN.md, deviations)

and in tests/golden/firered/firered_tiny.npz, for tests/test_gpu_firered.py: the reference
FireRedModel of wenet_amd.synthetic `tiny_firered` (init_model + the synthetic state dict, loaded
strictly) on four utterances of 290, 131, 127 and 121 frames (T' = 73, 33, 32, 31: three key
tiles, 33 / 32, one tile), every utterance decoded ALONE, in fp32 and as .double():
  enc64_<n>   the fp64 encoder output of the 131- and the 121-frame utterance, and in a file of
              its own (firered_tiny_enc3.npz, the size limit of one fixture) of the three-tile
              290-frame one: the pins of firered_refs.firered_encoder_formulation, the fp64
              reference of all four
  meta.scores / meta.e_score   from the fp64 reference, and |fp32 - fp64| of the reference
              itself: per attention list the decoder's teacher-forced log-probability of the
              list followed by <eos> (forward_attention_decoder; decode(['attention']) itself
              returns token lists only, search.py builds DecodeResult(hyp)), and the scores of
              attention_rescoring (ctc_weight 1, beam 5) and ctc_prefix_beam_search
  meta.e_enc  per utterance, the fp32 reference's own max abs error against fp64 on the
              encoder output
  meta.tokens decode(['attention']) at beams 1, 3, 10, ctc_greedy_search and
              ctc_prefix_beam_search (beam 5)
A weight seed is REJECTED unless every utterance's attention lists (the three beams together:
the greedy list of a random decoder with a tied output layer is one token repeated, whatever the
scales) hold >= 3 distinct tokens, a non-empty list ends on eos before its length cap, and the fp64 reference decodes the same lists as the fp32 one
in every mode and beam, attention_rescoring included (no near-ties: the rule
tools/gen_golden_whisper_decode.py applies to its beam decisions -- a decision whose margin is
below the fp32 reference's own error flips between the two runs).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


BEAMS = (1, 3, 10)
CTC_BEAM = 5
RESCORE_CTC_WEIGHT = 1.0


def _decode_alone(model, feats, dtype):
    """decode() of every utterance alone -> {method/beam: [token list per utterance]}."""
    out = {}
    with torch.no_grad():
        for beam in BEAMS:
            out[f'attention/{beam}'] = [
                list(map(int, model.decode(['attention'], f.unsqueeze(0).to(dtype),
                                           torch.tensor([f.shape[0]]),
                                           beam_size=beam)['attention'][0].tokens))
                for f in feats]
        for name, beam in (('ctc_greedy_search', 1), ('ctc_prefix_beam_search', CTC_BEAM)):
            out[name] = [
                list(map(int, model.decode([name], f.unsqueeze(0).to(dtype),
                                           torch.tensor([f.shape[0]]),
                                           beam_size=beam)[name][0].tokens))
                for f in feats]
        res = [model.decode(['ctc_prefix_beam_search', 'attention_rescoring'],
                            f.unsqueeze(0).to(dtype), torch.tensor([f.shape[0]]),
                            beam_size=CTC_BEAM, ctc_weight=RESCORE_CTC_WEIGHT) for f in feats]
        out['attention_rescoring'] = [list(map(int, r['attention_rescoring'][0].tokens))
                                      for r in res]
    return out


def _scores(model, feats, toks, dtype, eos, sos):
    """What decode() does not return (attention_beam_search builds its DecodeResult from the
    token list alone): the decoder's teacher-forced log-probability of every recorded attention
    list followed by <eos> -- forward_attention_decoder on the utterance's own encoder output --
    and the attention_rescoring / ctc_prefix_beam_search scores."""
    out = {f'attention/{b}': [] for b in BEAMS}
    out.update(attention_rescoring=[], ctc_prefix_beam_search=[])
    with torch.no_grad():
        for i, f in enumerate(feats):
            n = torch.tensor([f.shape[0]])
            enc, _ = model._forward_encoder(f.unsqueeze(0).to(dtype), n)
            for b in BEAMS:
                u = toks[f'attention/{b}'][i]
                hyp = torch.tensor([[sos] + u], dtype=torch.long)
                logp, _ = model.forward_attention_decoder(hyp, torch.tensor([len(u) + 1]), enc,
                                                          0.0)
                tgt = torch.tensor(u + [eos])
                out[f'attention/{b}'].append(float(logp[0, torch.arange(len(tgt)), tgt].sum()))
            r = model.decode(['ctc_prefix_beam_search', 'attention_rescoring'],
                             f.unsqueeze(0).to(dtype), n, beam_size=CTC_BEAM,
                             ctc_weight=RESCORE_CTC_WEIGHT)
            out['attention_rescoring'].append(float(r['attention_rescoring'][0].score))
            out['ctc_prefix_beam_search'].append(float(r['ctc_prefix_beam_search'][0].score))
    return out


def try_seed(wseed):
    """The model fixture of one weight seed, or the reason it is rejected."""
    import firered_refs as FR
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(FR.TINY['config'])
    sd = S.make_state_dict(configs, wseed)
    feats = FR.tiny_features()
    m32 = build_reference_model(configs, sd)
    toks = _decode_alone(m32, feats, torch.float32)
    caps = [FR.firered_out_len(f.shape[0]) for f in feats]
    for i in range(len(feats)):
        if len(set(t for b in BEAMS for t in toks[f'attention/{b}'][i])) < 3:
            return 'an utterance whose attention lists hold fewer than 3 distinct tokens', None
    if not any(0 < len(u) < caps[i] for b in BEAMS
               for i, u in enumerate(toks[f'attention/{b}'])):
        return 'no utterance reaches eos before the length cap', None
    if not any(len(u) > 0 for u in toks['ctc_prefix_beam_search']):
        return 'every CTC result is empty', None
    m64 = build_reference_model(configs, sd).double()
    if _decode_alone(m64, feats, torch.float64) != toks:
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    arrays, e_enc, enc_lens = {}, [], []
    with torch.no_grad():
        for f in feats:
            n = f.shape[0]
            e64, mk = m64._forward_encoder(f.unsqueeze(0).double(), torch.tensor([n]))
            e32, _ = m32._forward_encoder(f.unsqueeze(0), torch.tensor([n]))
            assert int(mk.sum()) == e64.shape[1] == FR.firered_out_len(n)
            e_enc.append(float((e32[0].double() - e64[0]).abs().max()))
            enc_lens.append(int(e64.shape[1]))
            if n in FR.RECORDED_ENC:
                arrays[f'enc64_{n}'] = e64[0].numpy()
            if n == FR.RECORDED_ENC_3TILE:
                arrays3 = {f'enc64_{n}': e64[0].numpy()}
    st = configs['tokenizer_conf']['special_tokens']
    s64 = _scores(m64, feats, toks, torch.float64, st['eos'], st['sos'])
    s32 = _scores(m32, feats, toks, torch.float32, st['eos'], st['sos'])
    e_score = {k: [abs(a - b) for a, b in zip(s32[k], s64[k])] for k in s64}
    meta = dict(FR.TINY, wseed=wseed, beams=list(BEAMS), ctc_beam=CTC_BEAM, tokens=toks,
                e_enc=e_enc, enc_lens=enc_lens, scores=s64, e_score=e_score,
                rescore_ctc_weight=RESCORE_CTC_WEIGHT, special_tokens=st)
    return None, (meta, arrays, arrays3)


def write_model_fixture():
    for wseed in range(200):
        why, got = try_seed(wseed)
        if got is None:
            print(f'seed {wseed}: rejected: {why}')
            continue
        meta, arrays, arrays3 = got
        np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'firered',
                                         'firered_tiny_enc3.npz'),
                            meta=np.frombuffer(json.dumps(dict(wseed=wseed)).encode(),
                                               dtype=np.uint8), **arrays3)
        path = os.path.join(ROOT, 'tests', 'golden', 'firered', 'firered_tiny.npz')
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                            **arrays)
        print(f'seed {wseed}: accepted -> {path} ({os.path.getsize(path)} bytes); lengths',
              {k: [len(u) for u in v] for k, v in meta['tokens'].items()}, 'of', meta['enc_lens'],
              'e_enc', meta['e_enc'])
        return 0
    print('no seed met the conditions')
    return 1


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    import firered_refs as FR
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    from wenet.models.firered.attention import (FiredRelPositionMultiHeadedAttention,
                                                FireRedRelPositionalEncoding)
    from wenet.models.firered.subsampling import FireRedConv2dSubsampling4
    from wenet.utils.mask import make_pad_mask

    arrays, meta = {}, {}
    with torch.no_grad():
        # ---- the attention module
        x, sd = FR.attn_module_inputs()
        T, d, H = FR.ATTN_MODULE['T'], FR.ATTN_MODULE['d'], FR.ATTN_MODULE['H']
        att = FiredRelPositionMultiHeadedAttention(H, d, 0.0, False, False, False).double().eval()
        att.load_state_dict(sd, strict=True)
        pos = FireRedRelPositionalEncoding(d, 0.0).double().eval()
        xb = x.unsqueeze(0)
        _, pos_emb = pos(xb)
        mask = torch.ones(1, 1, T, dtype=torch.bool)
        out, _ = att(xb, xb, xb, mask, pos_emb)
        arrays['attn_out'] = out[0].numpy()
        assert pos_emb.shape[1] == 2 * T - 1
        arrays['pos_emb_rows'] = pos_emb[0][FR.POS_ROWS].numpy()
        meta['attn'] = dict(FR.ATTN_MODULE)

        # ---- the front end
        c, w_out, b_out = FR.frontend_module_inputs()
        m = FR.FRONT_MODULE
        sub = FireRedConv2dSubsampling4(m['F'], m['d'], 0.0,
                                        FireRedRelPositionalEncoding(m['d'], 0.0),
                                        odim=m['C']).double().eval()
        missing, unexpected = sub.load_state_dict(
            {'conv.0.weight': c['w1'].double(), 'conv.0.bias': c['b1'].double(),
             'conv.2.weight': c['w2'].double(), 'conv.2.bias': c['b2'].double(),
             'out.0.weight': w_out.double(), 'out.0.bias': b_out.double()}, strict=False)
        assert not unexpected and set(missing) <= {'pos_enc.pe'}, (missing, unexpected)
        feats = c['feats'].double()
        for b, n in enumerate(m['lens']):
            y, _, mk = sub(feats[b:b + 1, :n], torch.ones(1, 1, n, dtype=torch.bool))
            assert int(mk.sum()) == y.shape[1]
            arrays[f'front_alone_{n}'] = y[0].numpy()
        lens = torch.tensor(m['lens'])
        _, _, mk = sub(feats, ~make_pad_mask(lens, feats.shape[1]).unsqueeze(1))
        meta['front'] = dict(m)
        meta['batched_lens'] = [int(v) for v in mk.squeeze(1).sum(1)]
        meta['alone_lens'] = [int(arrays[f'front_alone_{n}'].shape[0]) for n in m['lens']]
    out_dir = os.path.join(ROOT, 'tests', 'golden', 'firered')
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'firered_modules.npz')
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        **arrays)
    print(f'{path}: {os.path.getsize(path)} bytes; {meta}')
    return write_model_fixture()


if __name__ == '__main__':
    sys.exit(main())
