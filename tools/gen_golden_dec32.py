#!/usr/bin/env python3
"""Record what the REAL reference computes on models whose decoders have heads of 32, for
tests/test_attention_d32_host.py and tests/test_gpu_dec32.py.

    python tools/gen_golden_dec32.py        # CPU only; needs the reference tree

tests/golden/dec32/<model>*.npz -- the reference model (init_model + the synthetic state dict,
loaded strictly) of attention_d32_refs.MODELS on their utterances, every utterance decoded ALONE
with decoding_chunk_size -1, in fp32 and as .double():
  enc64_<n>          the fp64 encoder output
  meta.e_enc         per utterance, the fp32 reference's own max abs error against fp64
  meta.tokens        ctc_prefix_beam_search (beam 5), attention_rescoring (beam 5, ctc_weight 0.5,
                     reverse_weight 0.3), attention_b1 / attention_b5 (`attention`, beams 1 and 5)
  meta.scores / e_score   the fp64 scores of the two beam modes and |fp32 - fp64| of them (the
                     reference's `attention` results carry no score)
A weight seed is REJECTED unless the fp64 and the fp32 reference decode the same tokens in every
mode, at least three utterances have non-empty CTC results, at least three attention_rescoring
winners differ from the CTC best (otherwise the decoder decides nothing) and -- where the encoder
leaves more than 64 frames to decode over (tiny_dec32: 72 of 291; the Efficient Conformer's rate
of 8 leaves 36) -- at least one `attention` result is longer than 64 tokens: the second key block
of the step kernel.

tests/golden/dec32/<width model>.npz -- forward_attention_decoder of the one-block model at the
shipped widths (256, 8 decoder heads) on the five padded hypotheses of
attention_d32_refs.width_inputs: the fp64 log-probs of both directions (logp_l, logp_r) and
meta.e_logp, the fp32 reference's distance from them.

Arrays are cut into row blocks and dealt into files as tools/gen_golden_efficonformer.py does,
under the same file-size assertion.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_golden_efficonformer as GE  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'dec32')


def _decode_alone(model, feats, dtype, reverse_weight):
    toks, scores = {}, {}
    with torch.no_grad():
        for f in feats:
            x, ln = f.unsqueeze(0).to(dtype), torch.tensor([f.shape[0]])
            r = model.decode(list(D.BEAM_METHODS), x, ln, beam_size=D.CTC_BEAM,
                             decoding_chunk_size=-1, ctc_weight=D.RESCORE_CTC_WEIGHT,
                             reverse_weight=reverse_weight)
            got = {m: r[m][0] for m in D.BEAM_METHODS}
            for b in D.ATTENTION_BEAMS:
                got[f'attention_b{b}'] = model.decode(['attention'], x, ln, beam_size=b,
                                                      decoding_chunk_size=-1)['attention'][0]
            for m, res in got.items():
                toks.setdefault(m, []).append(list(map(int, res.tokens)))
                if m in D.BEAM_METHODS:      # the reference's `attention` result carries no score
                    scores.setdefault(m, []).append(float(res.score))
    return toks, scores


def try_seed(name, wseed):
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, wseed)
    feats = D.model_features(name)
    spec = D.MODELS[name]
    rw = spec['reverse_weight']
    m32 = build_reference_model(configs, sd)
    t32, s32 = _decode_alone(m32, feats, torch.float32, rw)
    ctc, res = t32['ctc_prefix_beam_search'], t32['attention_rescoring']
    if sum(len(u) > 0 for u in ctc) < 3:
        return 'fewer than three utterances with a non-empty CTC result', None
    if sum(a != b for a, b in zip(ctc, res)) < 3:
        return 'fewer than three rescoring winners differ from the CTC best', None
    if spec['long_attention'] and not any(
            len(u) > 64 for b in D.ATTENTION_BEAMS for u in t32[f'attention_b{b}']):
        return 'no attention result longer than 64 tokens', None
    m64 = build_reference_model(configs, sd).double()
    t64, s64 = _decode_alone(m64, feats, torch.float64, rw)
    if t64 != t32:
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    arrays, e_enc, enc_lens = {}, [], []
    with torch.no_grad():
        for f in feats:
            n = f.shape[0]
            ln = torch.tensor([n])
            e64, _ = m64._forward_encoder(f.unsqueeze(0).double(), ln)
            e32, _ = m32._forward_encoder(f.unsqueeze(0), ln)
            arrays[f'enc64_{n}'] = e64[0].numpy()
            e_enc.append(float((e32[0].double() - e64[0]).abs().max()))
            enc_lens.append(int(e64.shape[1]))
    e_score = {k: [abs(a - b) for a, b in zip(s32[k], s64[k])] for k in s64}
    meta = dict(frames=spec['frames'], fseed=spec['fseed'], reverse_weight=rw, config=name,
                wseed=wseed, ctc_beam=D.CTC_BEAM, tokens=t64, e_enc=e_enc, enc_lens=enc_lens,
                scores=s64, e_score=e_score, rescore_ctc_weight=D.RESCORE_CTC_WEIGHT)
    return None, (meta, arrays)


def write_model_fixture(name):
    for wseed in range(1, 200):
        why, got = try_seed(name, wseed)
        if got is None:
            print(f'{name} seed {wseed}: rejected: {why}')
            continue
        meta, arrays = got
        print(f'{name} seed {wseed}: accepted; lengths',
              {k: [len(u) for u in v] for k, v in meta['tokens'].items()}, 'of',
              meta['enc_lens'], 'e_enc', meta['e_enc'], 'e_score', meta['e_score'])
        GE.save_split(name, meta, arrays)
        return 0
    print(f'{name}: no seed met the conditions')
    return 1


def write_width_fixture():
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(D.WIDTH_MODEL)
    sd = S.make_state_dict(configs, D.WIDTH_WSEED)
    hyps, lens, enc = D.width_inputs(configs)
    rw = configs['model_conf']['reverse_weight']
    m32 = build_reference_model(configs, sd)
    m64 = build_reference_model(configs, sd).double()
    with torch.no_grad():
        l32, r32 = m32.forward_attention_decoder(hyps, lens, enc, rw)
        l64, r64 = m64.forward_attention_decoder(hyps, lens, enc.double(), rw)
    assert r64.dim() == 3
    e_logp = dict(l=float((l32.double() - l64).abs().max()),
                  r=float((r32.double() - r64).abs().max()))
    print(f'{D.WIDTH_MODEL}: e_logp', e_logp)
    meta = dict(config=D.WIDTH_MODEL, wseed=D.WIDTH_WSEED, reverse_weight=rw, e_logp=e_logp,
                hyps=hyps.tolist(), lens=lens.tolist())
    V = l64.shape[-1]
    GE.save_split(D.WIDTH_MODEL, meta, dict(logp_l=l64.reshape(-1, V).numpy(),
                                            logp_r=r64.reshape(-1, V).numpy()))


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    GE.accept_tuple_cache()
    global D
    import attention_d32_refs as D
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    os.makedirs(OUT, exist_ok=True)
    GE.OUT = OUT
    write_width_fixture()
    return max(write_model_fixture(n) for n in D.MODELS)


if __name__ == '__main__':
    sys.exit(main())
