#!/usr/bin/env python3
"""Record what the REAL reference computes for the rotary Conformer models, for
tests/test_gpu_rope_model.py.

    python tools/gen_golden_rope.py        # CPU only; needs the reference tree

tests/golden/rope/<config>.npz for the wenet_amd.synthetic configurations `tiny_rope` and
`tiny_rope_mqa`: the reference ASRModel (init_model + the synthetic state dict, loaded strictly)
on the utterances of rope_refs.MODELS, every utterance decoded ALONE, in fp32 and as .double():
  enc64_<s>_<i>   the fp64 encoder output of utterance i under setting s: 0 = full context, then
                  the (decoding_chunk_size, num_decoding_left_chunks) pairs of MODELS[config]
  meta.e_enc      per setting and utterance, |fp32 - fp64| of the reference itself on it
  meta.tokens / meta.scores / meta.e_score   ctc_greedy_search, ctc_prefix_beam_search and
                  attention_rescoring (full context) from the fp64 reference, and |fp32 - fp64| of
                  the reference's own scores
A weight seed is rejected when the fp32 and the fp64 reference decode different tokens (a
near-tie).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'rope')
METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring')


def _decode(model, f, dtype, T):
    r = model.decode(list(METHODS), f.unsqueeze(0).to(dtype), torch.tensor([f.shape[0]]),
                     beam_size=T['beam'], ctc_weight=T['ctc_weight'],
                     reverse_weight=T['reverse_weight'])
    return ({m: list(map(int, r[m][0].tokens)) for m in METHODS},
            {m: float(r[m][0].score) for m in METHODS})


def try_seed(name, wseed):
    import rope_refs as RR
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    T = RR.MODELS[name]
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, wseed)
    m32 = build_reference_model(configs, sd)
    m64 = build_reference_model(configs, sd).double()
    settings = [(-1, -1)] + [tuple(c) for c in T['chunks']]
    arrays, e_enc, toks, scores, e_score = {}, [[] for _ in settings], [], [], []
    with torch.no_grad():
        for i, f in enumerate(RR.model_features(name)):
            n = torch.tensor([f.shape[0]])
            for s, (chunk, left) in enumerate(settings):
                e64, _ = m64._forward_encoder(f.unsqueeze(0).double(), n, chunk, left)
                e32, _ = m32._forward_encoder(f.unsqueeze(0), n, chunk, left)
                arrays[f'enc64_{s}_{i}'] = e64[0].numpy()
                e_enc[s].append(float((e32[0].double() - e64[0]).abs().max()))
            t64, s64 = _decode(m64, f, torch.float64, T)
            t32, s32 = _decode(m32, f, torch.float32, T)
            if t64 != t32:
                return f'utterance {i}: fp64 and fp32 decode different tokens (near-tie)', None
            toks.append(t64); scores.append(s64)
            e_score.append({m: abs(s64[m] - s32[m]) for m in METHODS})
    if not any(t['attention_rescoring'] for t in toks):
        return 'every result is empty', None
    meta = dict(T, config=name, wseed=wseed, settings=settings, tokens=toks, scores=scores,
                e_score=e_score, e_enc=e_enc)
    return None, (meta, arrays)


def main():
    import rope_refs as RR
    from oracle import _ref_harness
    _ref_harness.install()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    os.makedirs(OUT, exist_ok=True)
    for name in RR.MODELS:
        for wseed in range(50):
            why, got = try_seed(name, wseed)
            if got is None:
                print(f'{name} seed {wseed}: rejected: {why}')
                continue
            meta, arrays = got
            path = os.path.join(OUT, f'{name}.npz')
            np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(),
                                                         dtype=np.uint8), **arrays)
            print(f'{name} seed {wseed}: accepted -> {path} ({os.path.getsize(path)} bytes)',
                  [{m: len(u) for m, u in t.items()} for t in meta['tokens']],
                  'e_enc', meta['e_enc'])
            break
        else:
            print(f'{name}: no seed met the conditions')
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
