#!/usr/bin/env python3
"""Record what the REAL reference's hybrid transducer decodes with its greedy search behind a
chunk-masked encoder pass -- Transducer.greedy_search(decoding_chunk_size=c,
num_decoding_left_chunks=l), wenet/models/transducer/transducer.py:398-442 -- for the streaming
transducer sessions (tests/test_transducer_stream_formulation.py,
tests/test_gpu_transducer_stream.py).

    python tools/gen_golden_transducer_stream.py        # CPU only; needs the reference tree

Model: wenet_amd.synthetic `tiny_rnnt`, built by the reference's own init_model and loaded
strictly with the synthetic state dict.  Inputs: make_features(3, (60, 150), seed=77), one
utterance at a time, as the reference requires.

Recorded in tests/golden/rnnt/rnnt_stream_tiny.npz, for (c, l) in {(4, -1), (3, 2)}: the
reference's chunk-masked encoder output (`enc_c{c}_l{l}`, padded to the longest utterance) and
its greedy token lists for n_steps 64 and 3.

A weight seed is REJECTED unless
  1. the reference in fp64 decodes the same tokens on every path;
  2. the fp64 formulation (tests/transducer_formulation.py) on the recorded encoder output
     decodes the same tokens, and at every joint evaluation that decides something the gap of
     the top two logits is >= 4 x the fp32 dot-product bound (dot_bound), in fp64;
  3. some chunk of some utterance that is not its last ends on a frame that hits the
     n_steps = 3 cap: a session fed chunk by chunk walks the `stale` path there;
  4. some result is non-empty.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONFIG = 'tiny_rnnt'
BATCH, FRAMES, FSEED = 3, (60, 150), 77
CHUNKS = ((4, -1), (3, 2))
N_STEPS = (64, 3)


def key(c, l):
    return f'c{c}_l{l}'


def build(configs, sd, double=False):
    from oracle.gen_golden import build_reference_model
    model = build_reference_model(configs, sd)
    return model.double() if double else model


def ref_run(model, feats, lens, double=False):
    """{key: ({n_steps: token lists}, [encoder output (T', d) per utterance])}"""
    out = {}
    with torch.no_grad():
        for c, l in CHUNKS:
            toks = {k: [] for k in N_STEPS}
            encs = []
            for b in range(feats.size(0)):
                n = int(lens[b])
                x = feats[b:b + 1, :n].double() if double else feats[b:b + 1, :n]
                enc, mask = model.encoder(x, lens[b:b + 1], c, l)
                assert int(mask.squeeze(1).sum()) == enc.size(1)
                encs.append(enc[0])
                for k in N_STEPS:
                    got = model.greedy_search(x, lens[b:b + 1], decoding_chunk_size=c,
                                              num_decoding_left_chunks=l, n_steps=k)
                    toks[k].append([int(v) for v in got[0]])
            out[key(c, l)] = (toks, encs)
    return out


def ref_run64(configs, sd, feats, lens):
    torch.set_default_dtype(torch.float64)     # init_state allocates with the default dtype
    try:
        return ref_run(build(configs, sd, double=True), feats, lens, double=True)
    finally:
        torch.set_default_dtype(torch.float32)


def try_seed(wseed):
    import transducer_formulation as TF
    from wenet_amd import synthetic as S
    configs = S.make_configs(CONFIG)
    blank = configs['tokenizer_conf']['special_tokens']['<blank>']
    feats, lens = S.make_features(BATCH, FRAMES, seed=FSEED)
    sd = S.make_state_dict(configs, wseed)
    model = build(configs, sd)
    got = ref_run(model, feats, lens)
    if not any(len(u) for toks, _ in got.values() for k in N_STEPS for u in toks[k]):
        return 'every result is empty', None
    W = TF.weights64({k: v.numpy() for k, v in sd.items() if k.startswith(('predictor.', 'joint.'))},
                     configs['predictor_conf']['num_layers'])
    J = configs['joint_conf']['join_dim']
    ratio, bound, stale_at = np.inf, 0.0, []
    arrays = {}
    enc_lens = None
    for c, l in CHUNKS:
        toks, encs = got[key(c, l)]
        n_enc = [int(e.size(0)) for e in encs]
        assert enc_lens in (None, n_enc)
        enc_lens = n_enc
        enc = np.zeros((BATCH, max(n_enc), encs[0].size(1)), dtype=np.float32)
        for b, e in enumerate(encs):
            enc[b, :n_enc[b]] = e.numpy()
        arrays['enc_' + key(c, l)] = enc
        for k in N_STEPS:
            emitted = [np.zeros(n, dtype=np.int64) for n in n_enc]
            worst = [np.inf, 0.0]

            def on_row(b, t, hrow, logits):
                if int(logits.argmax()) != blank:
                    emitted[b][t] += 1
                gap, bd = TF.dot_bound(hrow, logits, W['ffn_out'][0], J)
                if gap / bd < worst[0]:
                    worst[0], worst[1] = gap / bd, bd
            ftoks, _ = TF.lookahead_greedy_search(enc, n_enc, W, blank, k, 1, on_row)
            if ftoks != toks[k]:
                return f'the fp64 formulation differs from the reference at {key(c, l)} n_steps {k}', None
            if worst[0] < ratio:
                ratio, bound = worst
            if k == 3:
                stale_at += [(key(c, l), b, t) for b in range(BATCH) for t in range(n_enc[b])
                             if emitted[b][t] >= 3 and (t + 1) % c == 0 and t + 1 < n_enc[b]]
    if ratio < 4.0:
        return f'gap / bound {ratio:.2f} < 4', None
    if not stale_at:
        return 'n_steps 3: the cap is never hit on the last frame of a chunk', None
    got64 = ref_run64(configs, sd, feats, lens)
    if any(got64[k][0] != got[k][0] for k in got):
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    meta = dict(config=CONFIG, wseed=wseed, batch=BATCH, frames=list(FRAMES), fseed=FSEED,
                blank=blank, blank_bias=S.RNNT_BLANK_BIAS, n_steps=list(N_STEPS),
                chunks=[list(cl) for cl in CHUNKS], enc_lens=enc_lens,
                feat_lens=[int(v) for v in lens],
                tokens={kk: {str(k): v[0][k] for k in N_STEPS} for kk, v in got.items()},
                min_gap_over_bound=float(ratio), bound=float(bound),
                stale_at=[[kk, int(b), int(t)] for kk, b, t in stale_at])
    return None, (meta, arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for wseed in range(200):
        why, got = try_seed(wseed)
        if got is None:
            print(f'seed {wseed}: rejected: {why}', flush=True)
            continue
        meta, arrays = got
        out = os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_stream_tiny.npz')
        os.makedirs(os.path.dirname(out), exist_ok=True)
        np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                            **arrays)
        print(f'seed {wseed}: accepted -> {out} ({os.path.getsize(out)} bytes); lengths',
              {kk: {k: [len(u) for u in v] for k, v in t.items()} for kk, t in meta['tokens'].items()},
              f"gap / bound {meta['min_gap_over_bound']:.1f}, stale at", meta['stale_at'])
        return 0
    print('no seed met the conditions')
    return 1


if __name__ == '__main__':
    sys.exit(main())
