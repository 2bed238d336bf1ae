#!/usr/bin/env python3
"""Record what the REAL reference's hybrid transducer (wenet/models/transducer/transducer.py)
decodes with its greedy search -- basic_greedy_search, search/greedy_search.py:6-54 -- for
tests/test_transducer_formulation.py and tests/test_gpu_transducer.py.

    python tools/gen_golden_transducer.py        # CPU only; needs the reference tree

Model: wenet_amd.synthetic `tiny_rnnt` (tiny_causal + an LSTM predictor 64 / 80 / 96, two layers,
and a joint of 160), built by the reference's own init_model and loaded strictly with the
synthetic state dict.  Inputs: make_features(3, (60, 150), seed=77): T' = 29, 16, 15.

Recorded in tests/golden/rnnt/rnnt_tiny.npz: the reference encoder output and lengths; the greedy
token lists of every utterance (run one at a time, as the reference requires) for n_steps 64, 3
and 1; ctc_greedy_search of the same model; four predictor steps (token, state in, out, state
out) with the joint logits of one frame each; the token lists of a second model, `blank_heavy`
(a larger blank bias), with at least one empty result.

A weight seed is REJECTED unless
  1. with n_steps 64 some frame emits >= 2 symbols, some frame none, and >= 4 blank frames follow
     one another somewhere;
  2. with n_steps 3 the cap is hit on a frame;
  3. the reference in fp64 (model.double() under a float64 default dtype) decodes the same tokens;
  4. at every joint evaluation that decides something, on every path (n_steps 64 / 3 / 1, both
     models), the gap of the top two logits is >= 4 x the fp32 dot-product bound
     (tests/transducer_formulation.dot_bound), in fp64.
The smallest gap / bound ratio and the bound go into the fixture's meta.
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
N_STEPS = (64, 3, 1)
HEAVY_BIASES = (9.0, 10.0, 12.0, 15.0)
STEP_AT = (0, 1, 2, 5)          # the recorded predictor steps of utterance 0


def ref_tokens(model, enc, enc_lens, n_steps):
    from wenet.models.transducer.search.greedy_search import basic_greedy_search
    out = []
    with torch.no_grad():
        for b in range(enc.size(0)):
            n = int(enc_lens[b])
            out.append([int(v) for v in basic_greedy_search(
                model, enc[b:b + 1, :n], torch.tensor(n), n_steps=n_steps)[0]])
    return out


def build(configs, sd, double=False):
    from oracle.gen_golden import build_reference_model
    model = build_reference_model(configs, sd)
    return model.double() if double else model


def tokens64(configs, sd, feats, lens):
    torch.set_default_dtype(torch.float64)     # init_state allocates with the default dtype
    try:
        model = build(configs, sd, double=True)
        with torch.no_grad():
            enc, mask = model._forward_encoder(feats.double(), lens, -1, -1)
        return {n: ref_tokens(model, enc, mask.squeeze(1).sum(1), n) for n in N_STEPS}
    finally:
        torch.set_default_dtype(torch.float32)


def walk(enc, enc_lens, sd, configs, blank, n_steps):
    """The fp64 formulation at lookahead 1 over the recorded encoder output: its tokens, the
    symbols per frame and the smallest gap / bound ratio of the deciding joint rows."""
    import transducer_formulation as TF
    W = TF.weights64({k: v.numpy() for k, v in sd.items() if k.startswith(('predictor.', 'joint.'))},
                     configs['predictor_conf']['num_layers'])
    J = configs['joint_conf']['join_dim']
    emitted = [np.zeros(int(n), dtype=np.int64) for n in enc_lens]
    worst = [np.inf, 0.0]

    def on_row(b, t, hrow, logits):
        if int(logits.argmax()) != blank:
            emitted[b][t] += 1
        gap, bound = TF.dot_bound(hrow, logits, W['ffn_out'][0], J)
        if gap / bound < worst[0]:
            worst[0], worst[1] = gap / bound, bound
    toks, _ = TF.lookahead_greedy_search(enc.numpy(), enc_lens, W, blank, n_steps, 1, on_row)
    return toks, emitted, worst


def longest_zero_run(v):
    best = run = 0
    for x in v:
        run = run + 1 if x == 0 else 0
        best = max(best, run)
    return best


def try_seed(wseed):
    from wenet_amd import synthetic as S
    configs = S.make_configs(CONFIG)
    blank = configs['tokenizer_conf']['special_tokens']['<blank>']
    feats, lens = S.make_features(BATCH, FRAMES, seed=FSEED)
    sd = S.make_state_dict(configs, wseed)
    model = build(configs, sd)
    assert model.blank == blank
    with torch.no_grad():
        enc, mask = model._forward_encoder(feats, lens, -1, -1)
        enc_lens = mask.squeeze(1).sum(1)
    toks = {n: ref_tokens(model, enc, enc_lens, n) for n in N_STEPS}
    ratio, bound = np.inf, 0.0
    for n in N_STEPS:
        ftoks, emitted, worst = walk(enc, enc_lens, sd, configs, blank, n)
        if ftoks != toks[n]:
            return f'the fp64 formulation differs from the reference at n_steps {n}', None
        if worst[0] < ratio:
            ratio, bound = worst
        if n == 64:
            if not any((e >= 2).any() for e in emitted):
                return 'no frame emits two symbols', None
            if not any((e == 0).any() for e in emitted):
                return 'no frame without a symbol', None
            if max(longest_zero_run(e) for e in emitted) < 4:
                return 'no run of four blank frames', None
        if n == 3 and not any((e >= 3).any() for e in emitted):
            return 'n_steps 3: the cap is never hit', None
    if ratio < 4.0:
        return f'gap / bound {ratio:.2f} < 4', None
    # the reference's own entry point, one utterance at a time through its own encoder pass
    with torch.no_grad():
        for b in range(BATCH):
            n = int(lens[b])
            got = model.greedy_search(feats[b:b + 1, :n], lens[b:b + 1], n_steps=64)[0]
            if [int(v) for v in got] != toks[64][b]:
                return 'greedy_search of an utterance alone differs from the batch encoder', None
    if tokens64(configs, sd, feats, lens) != toks:
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    # the blank-heavy model
    heavy = None
    for bias in HEAVY_BIASES:
        sdh = S.make_state_dict(configs, wseed, rnnt_blank_bias=bias)
        mh = build(configs, sdh)
        th = ref_tokens(mh, enc, enc_lens, 64)
        if not any(len(u) == 0 for u in th):
            continue
        fth, _, worst = walk(enc, enc_lens, sdh, configs, blank, 64)
        if fth != th or worst[0] < 4.0:
            continue
        if tokens64(configs, sdh, feats, lens)[64] != th:
            continue
        heavy = dict(bias=bias, tokens=th, ratio=float(worst[0]))
        break
    if heavy is None:
        return 'no blank-heavy model with an empty result and clear gaps', None
    with torch.no_grad():
        ctc = model.decode(['ctc_greedy_search'], feats, lens)['ctc_greedy_search']
    # four predictor steps of utterance 0 along its n_steps-64 path, with the joint logits of the
    # frame of the same number
    arrays = {}
    seq = [blank] + toks[64][0]
    with torch.no_grad():
        cache = model.predictor.init_state(1, method='zero', device=enc.device)
        padding = torch.zeros(1, 1)
        for k, tok in enumerate(seq[:max(STEP_AT) + 1]):
            out, new = model.predictor.forward_step(torch.tensor([[tok]]), padding, cache)
            if k in STEP_AT:
                logits = model.joint(enc[0:1, k:k + 1], out)
                arrays[f'step{k}_h_in'] = cache[0][:, 0].numpy()
                arrays[f'step{k}_c_in'] = cache[1][:, 0].numpy()
                arrays[f'step{k}_out'] = out[0, 0].numpy()
                arrays[f'step{k}_h'] = new[0][:, 0].numpy()
                arrays[f'step{k}_c'] = new[1][:, 0].numpy()
                arrays[f'step{k}_logits'] = logits.reshape(-1).numpy()
            cache = new
    if len(seq) <= max(STEP_AT):
        return 'utterance 0 is too short for the recorded steps', None
    meta = dict(config=CONFIG, wseed=wseed, batch=BATCH, frames=list(FRAMES), fseed=FSEED,
                blank=blank, blank_bias=S.RNNT_BLANK_BIAS, n_steps=list(N_STEPS),
                tokens={str(n): toks[n] for n in N_STEPS}, enc_lens=[int(v) for v in enc_lens],
                ctc_greedy=[[int(v) for v in r.tokens] for r in ctc],
                min_gap_over_bound=float(ratio), bound=float(bound), heavy=heavy,
                step_at=list(STEP_AT), step_tokens=[int(seq[k]) for k in STEP_AT])
    arrays['enc'] = enc.numpy().astype(np.float32)
    return None, (meta, {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()})


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for wseed in range(200):
        why, got = try_seed(wseed)
        if got is None:
            print(f'seed {wseed}: rejected: {why}')
            continue
        meta, arrays = got
        out = os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_tiny.npz')
        os.makedirs(os.path.dirname(out), exist_ok=True)
        np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                            **arrays)
        print(f'seed {wseed}: accepted -> {out} ({os.path.getsize(out)} bytes); lengths',
              {k: [len(u) for u in v] for k, v in meta['tokens'].items()},
              f"gap / bound {meta['min_gap_over_bound']:.1f}, bound {meta['bound']:.2e}, heavy",
              meta['heavy']['bias'], [len(u) for u in meta['heavy']['tokens']])
        return 0
    print('no seed met the conditions')
    return 1


if __name__ == '__main__':
    sys.exit(main())
