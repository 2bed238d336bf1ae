#!/usr/bin/env python3
"""Measure the FireRedASR-AED-L path: `firered_aed_l` (d 1280, 20 heads, ffn 5120, 16 + 16 blocks,
vocabulary 7832, synthetic weights), B = 16 utterances of 8-12 s.

    python tools/bench_firered.py [--steps 5] [--warmup 2] [--out-dir DIR]

Writes profiles/firered_aed_l.json and docs/LOG_round20.md (or both into --out-dir):
  encoder_ms        wn_encode of the batch (front end + 16 layers), HIP events
  attention_ms      decode(['attention'], beam 3) of the batch, encoder included
  audio_s_per_s     audio seconds of the batch / attention_ms
  relshift_ms / plain_ms   one layer's rel-shift attention (wn_op_attention_relshift) beside
                    attention_kernel without a position term (wn_op_attention) on the same packed
                    Q / K / V rows in the same process: what the second contraction and the skew
                    cost
No number is a pass condition.  A kernel split comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_firered.py --steps 1 --warmup 1
"""
import argparse
import ctypes
import json
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


def attention_pair(enc_lens, H, steps, warmup):
    """One layer's attention on the batch's packed rows: rel-shift against plain."""
    from wenet_amd import _lib
    L = _lib.lib()
    d = H * 64
    lens = np.asarray(enc_lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M, T = int(lens.sum()), int(lens.max())
    g = torch.Generator(device='cuda').manual_seed(0)
    qkv = torch.randn(M, 3 * d, device='cuda', generator=g)
    P = torch.randn(2 * T - 1, d, device='cuda', generator=g)
    bu = torch.randn(H, 64, device='cuda', generator=g) * 0.5
    bv = torch.randn(H, 64, device='cuda', generator=g) * 0.5
    O = torch.empty(M, d, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d

    def relshift():
        _lib.check(L.wn_op_attention_relshift(q, k, v, 3 * d, 3 * d, 3 * d, M, P.data_ptr(), d,
                                              2 * T - 1, T - 1, bu.data_ptr(), bv.data_ptr(),
                                              O.data_ptr(), d, _lib.i32p(off), _lib.i32p(lens),
                                              len(lens), H, 0.125, st), 'attention_relshift')

    op = _lib.WnAttentionOp()
    op.Q, op.K, op.V = q, k, v
    op.ldq = op.ldk = op.ldv = 3 * d
    op.q_rows = op.kv_rows = M
    op.O, op.ldo = O.data_ptr(), d
    op.q_off = op.kv_off = _lib.i32p(off)
    op.q_len = op.kv_len = _lib.i32p(lens)
    op.n_seq, op.n_heads, op.mask_mode, op.left_chunks, op.scale = len(lens), H, 0, -1, 0.125
    form = ctypes.c_int32(0)

    def plain():
        _lib.check(L.wn_op_attention(ctypes.byref(op), ctypes.byref(form), st), 'attention')

    return timed(relshift, steps * 4, warmup), timed(plain, steps * 4, warmup), hex(form.value)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--out-dir', default=None)
    args = ap.parse_args(argv)
    from wenet_amd import FireRed
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('firered_aed_l')
    model = FireRed(configs, S.make_state_dict(configs, 0), device='cuda:0')
    print(f'model built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    att_ms = timed(lambda: model.decode(['attention'], feats, lens, beam_size=3), args.steps,
                   args.warmup)
    _, mask = model._forward_encoder(feats, lens)
    enc_lens = mask.squeeze(1).sum(1).tolist()
    rs_ms, pl_ms, form = attention_pair(enc_lens, configs['encoder_conf']['attention_heads'],
                                        args.steps, args.warmup)
    res = dict(status='measured', config='firered_aed_l', batch=args.batch, audio_s=audio_s,
               steps=args.steps, warmup=args.warmup, encoder_ms=enc_ms, attention_ms=att_ms,
               audio_s_per_s=audio_s / (att_ms * 1e-3), encoder_audio_s_per_s=audio_s /
               (enc_ms * 1e-3), relshift_ms=rs_ms, plain_ms=pl_ms, plain_form=form,
               enc_frames=int(sum(enc_lens)), dtype='fp32', kernel_split='not collected')
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'firered_aed_l.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round20.md'), 'w') as f:
        f.write(LOG.format(**res))
    print(json.dumps(res))
    return 0


LOG = """# Round 20: FireRedASR-AED models

`tools/bench_firered.py`: `firered_aed_l` (synthetic weights), B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {enc_frames} encoder frames), fp32, {steps} steps after {warmup}.

| what | ms |
| --- | --- |
| encoder (front end + 16 layers) | {encoder_ms:.2f} |
| `decode(['attention'], beam 3)`, encoder included | {attention_ms:.2f} |
| rel-shift attention, one layer (`wn_op_attention_relshift`) | {relshift_ms:.3f} |
| `attention_kernel`, no position term, same rows (form {plain_form}) | {plain_ms:.3f} |

{audio_s_per_s:.0f} audio-s/s through `attention` decoding ({encoder_audio_s_per_s:.0f} for the
encoder alone).  The path is the plain fp32 one, untuned; the `attention` search runs one call
per distinct encoder length of the batch.  Kernel split: {kernel_split}.
"""

if __name__ == '__main__':
    sys.exit(main())
