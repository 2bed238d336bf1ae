#!/usr/bin/env python3
"""Timing record of the SenseVoice path: `sensevoice_small` (the released widths: 50 + 20 blocks
at d 512 with 4 heads of 128, 2048 units, vocabulary 25055; synthetic weights), B = 32 utterances
of 8-12 s, fp32, after warm-up.

    python tools/bench_sensevoice.py [--steps 5 --warmup 2 --batch 32 --out-dir DIR]

Records: the encoder (query rows + LFR front end, 50 blocks, after_norm, 20 tp blocks, tp_norm),
`decode(['ctc_greedy_search'])` as a whole in audio-s/s, and `sv_front` alone through its operator
hook on the same batch (the library's launch plus the hook's descriptor upload, so an upper
bound).  Beside it, in the same process, the encoder of `paraformer_large` (50 blocks of the same
widths) on the same features: a record of two different models, not a ratio.  One run, untuned.
Writes profiles/sensevoice_small.json and docs/LOG_round28.md (or both into --out-dir).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def front_hook(sd, feats, lens, steps, warmup):
    """sv_front on the batch through wn_op_sv_front, with the model's own tables."""
    from wenet_amd import _lib
    from wenet_amd.sensevoice import out_len, query_ids
    L = _lib.lib()
    B, T, F = feats.shape
    D, ld = 7 * F, 576
    ln = np.ascontiguousarray(lens.numpy().astype(np.int32))
    rows = np.asarray([out_len(int(n)) for n in ln], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int32)
    M = int(rows.sum())
    half = D // 2
    inc = math.log(10000.0) / (half - 1)
    st_ = torch.arange(int(rows.max()) + 1, dtype=torch.float64)[:, None] * \
        torch.exp(-inc * torch.arange(half, dtype=torch.float64))[None, :]
    pe = torch.cat([torch.sin(st_), torch.cos(st_)], dim=1).float().cuda()
    dev = {k: sd[k].float().contiguous().cuda() for k in (
        'global_cmvn.mean', 'global_cmvn.istd', 'embed.weight',
        'encoder.encoders0.0.norm1.weight', 'encoder.encoders0.0.norm1.bias')}
    out = torch.empty(M, ld, device='cuda')
    qid = np.ascontiguousarray(query_ids(None, B))
    out_rows = np.zeros(B, dtype=np.int32)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        _lib.check(L.wn_op_sv_front(
            feats.data_ptr(), dev['global_cmvn.mean'].data_ptr(),
            dev['global_cmvn.istd'].data_ptr(), dev['embed.weight'].data_ptr(), pe.data_ptr(),
            pe.shape[0], dev['encoder.encoders0.0.norm1.weight'].data_ptr(),
            dev['encoder.encoders0.0.norm1.bias'].data_ptr(), out.data_ptr(), ld, M,
            _lib.i32p(ln), _lib.i32p(off), _lib.i32p(qid), _lib.i32p(out_rows), B, T, F, 7, 6,
            math.sqrt(512.0), 1e-5, st), 'sv_front')

    return timed(run, steps * 4, warmup), M


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out-dir', default=None)
    args = ap.parse_args(argv)
    from wenet_amd import Paraformer, SenseVoiceSmall
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('sensevoice_small')
    sd = S.make_state_dict(configs, 0)
    model = SenseVoiceSmall(configs, sd, device='cuda:0')
    print(f'sensevoice_small built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    B = feats.shape[0]
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    _, mask = model._forward_encoder(feats, lens)
    enc_frames = int(mask.sum())
    ctc_ms = timed(lambda: model.decode(['ctc_greedy_search'], feats, lens), args.steps,
                   args.warmup)
    res0 = model.decode(['ctc_greedy_search'], feats, lens)['ctc_greedy_search']
    tokens = sum(len(r.tokens) for r in res0)
    front_ms, front_rows = front_hook(sd, feats, lens, args.steps, args.warmup)
    assert front_rows == enc_frames
    del model, sd
    torch.cuda.empty_cache()
    t0 = time.time()
    pconfigs = S.make_configs('paraformer_large')
    pmodel = Paraformer(pconfigs, S.make_state_dict(pconfigs, 0), device='cuda:0')
    print(f'paraformer_large built in {time.time() - t0:.1f} s', flush=True)
    pf_ms = timed(lambda: pmodel._forward_encoder(feats, lens), args.steps, args.warmup)
    _, pmask = pmodel._forward_encoder(feats, lens)
    res = dict(status='measured, one run, untuned', config='sensevoice_small', batch=B,
               audio_s=audio_s, steps=args.steps, warmup=args.warmup, dtype='fp32',
               enc_frames=enc_frames, tokens=tokens, encoder_ms=enc_ms, ctc_greedy_ms=ctc_ms,
               ctc_greedy_audio_s_per_s=audio_s / (ctc_ms * 1e-3), sv_front_hook_ms=front_ms,
               paraformer_large_encoder_ms=pf_ms, paraformer_large_enc_frames=int(pmask.sum()),
               ffn='linear() pairs with ReLU / residual epilogues; ffn_fused was not tried',
               kernel_split='not collected')
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'sensevoice_small.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round28.md'), 'w') as f:
        f.write(LOG.format(**res))
    print(json.dumps(res))
    return 0


LOG = """# Round 28: SenseVoice Small models

`tools/bench_sensevoice.py`: `sensevoice_small` (synthetic weights), B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {enc_frames} encoder frames with the four query frames of every
utterance, {tokens} tokens), fp32, {steps} steps after {warmup}.  One run, untuned.

| what | ms |
| --- | --- |
| encoder (`sv_front`, 50 blocks, `after_norm`, 20 tp blocks, `tp_norm`) | {encoder_ms:.2f} |
| `decode(['ctc_greedy_search'])`, encoder included | {ctc_greedy_ms:.2f} |
| `sv_front` alone (`wn_op_sv_front`, with the hook's descriptor upload: an upper bound) | {sv_front_hook_ms:.3f} |
| beside it: the encoder of `paraformer_large` (50 blocks, {paraformer_large_enc_frames} frames), same features, same process | {paraformer_large_encoder_ms:.2f} |

{ctc_greedy_audio_s_per_s:.0f} audio-s/s through `ctc_greedy_search`.  The two encoder rows are
a record of two different models (70 blocks against 50, four more frames per utterance), not a
ratio.  Feed-forward modules: {ffn}.  Kernel split: {kernel_split}.
"""

if __name__ == '__main__':
    sys.exit(main())
