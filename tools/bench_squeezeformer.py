#!/usr/bin/env python3
"""Measure the Squeezeformer path: `librispeech_squeezeformer` (train_squeezeformer.yaml at its
real widths: d 256, 4 heads, FFN 1024, K 31, 12 blocks, reduction in front of block 5, recovery in
front of block 11, the wrapped shift; synthetic weights), B = 32 utterances of 8-12 s, beside the
Conformer of BASELINE.json configs[1] (`aishell_u2pp`) on the same batch in the same process --
two models side by side, not a ratio.

    python tools/bench_squeezeformer.py [--steps 10] [--warmup 3] [--out-dir DIR]

Writes profiles/squeezeformer_librispeech.json and docs/LOG_round24.md (or both into --out-dir):
  encoder_ms / conformer_encoder_ms   wn_encode of the batch, HIP events around `steps` calls
  attention_*_us    one launch on the batch's packed full-rate rows (4 heads) through the operator
                    hooks, HIP events around 4 x `steps` calls: attention_sqshift, attention_kernel
                    with the rel-pos term (ATTN_RELPOS, no fold) and attention_relshift.  The
                    hook's descriptor upload (one small host-to-device copy) is inside every
                    bracket, the same for the three.
  time_reduce_us / time_recover_us    likewise, with the bytes the kernels must move
The path is untuned and every figure comes from ONE run of this tool: a record, not a pass mark.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29


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


def hook_launches(enc_lens, H, steps, warmup):
    """us per launch of the three attention kernels and the two time kernels on the same rows."""
    from wenet_amd import _lib
    L = _lib.lib()
    d = H * 64
    lens = np.asarray(enc_lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    lens2 = (lens + 1) // 2
    off2 = np.concatenate([[0], np.cumsum(lens2)[:-1]]).astype(np.int32)
    M, M2, tmax = int(lens.sum()), int(lens2.sum()), int(lens.max())
    g = torch.Generator(device='cuda').manual_seed(0)
    qkv = torch.randn(M, 3 * d, device='cuda', generator=g)
    P = torch.randn(2 * tmax - 1, d, device='cuda', generator=g)
    bu = torch.randn(H, 64, device='cuda', generator=g) * 0.5
    bv = torch.randn(H, 64, device='cuda', generator=g) * 0.5
    O = torch.empty(M, d, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d

    def sqshift():
        _lib.check(L.wn_op_attention_sqshift(q, k, v, 3 * d, 3 * d, 3 * d, M, P.data_ptr(), d,
                                             tmax, bu.data_ptr(), bv.data_ptr(), O.data_ptr(), d,
                                             _lib.i32p(off), _lib.i32p(lens), len(lens), H, 0.125,
                                             st), 'attention_sqshift')

    def relshift():
        _lib.check(L.wn_op_attention_relshift(q, k, v, 3 * d, 3 * d, 3 * d, M, P.data_ptr(), d,
                                              2 * tmax - 1, tmax - 1, bu.data_ptr(), bv.data_ptr(),
                                              O.data_ptr(), d, _lib.i32p(off), _lib.i32p(lens),
                                              len(lens), H, 0.125, st), 'attention_relshift')

    op = _lib.WnAttentionOp()
    op.Q, op.K, op.V = q, k, v
    op.ldq = op.ldk = op.ldv = 3 * d
    op.q_rows = op.kv_rows = M
    op.P, op.ldp, op.p_rows = P.data_ptr(), d, tmax
    op.bias_u, op.bias_v = bu.data_ptr(), bv.data_ptr()
    op.O, op.ldo = O.data_ptr(), d
    op.q_off = op.kv_off = _lib.i32p(off)
    op.q_len = op.kv_len = _lib.i32p(lens)
    op.n_seq, op.n_heads = len(lens), H
    op.mask_mode, op.chunk_size, op.left_chunks, op.scale = 0, 0, -1, 0.125
    op.flags, op.precision, op.x6_galign = 0, 0, 0
    form = np.zeros(1, dtype=np.int32)

    def relpos():
        _lib.check(L.wn_op_attention(op, _lib.i32p(form), st), 'attention')

    x = torch.randn(M, d, device='cuda', generator=g)
    wt = torch.randn(5, d, device='cuda', generator=g)
    bias = torch.zeros(d, device='cuda')
    y2 = torch.empty(M2, d, device='cuda')
    z = torch.randn(M2, d, device='cuda', generator=g)
    y = torch.empty(M, d, device='cuda')

    def reduce_():
        _lib.check(L.wn_op_time_reduce(x.data_ptr(), d, M, d, wt.data_ptr(), bias.data_ptr(), 5, 3,
                                       y2.data_ptr(), d, M2, _lib.i32p(off), _lib.i32p(lens),
                                       _lib.i32p(off2), len(lens), st), 'time_reduce')

    def recover():
        _lib.check(L.wn_op_time_recover(x.data_ptr(), d, z.data_ptr(), d, M2, y.data_ptr(), d, M,
                                        d, _lib.i32p(off), _lib.i32p(lens), _lib.i32p(off2),
                                        len(lens), st), 'time_recover')

    n = steps * 4
    out = dict(attention_sqshift_us=timed(sqshift, n, warmup) * 1e3,
               attention_relpos_us=timed(relpos, n, warmup) * 1e3,
               attention_relshift_us=timed(relshift, n, warmup) * 1e3,
               time_reduce_us=timed(reduce_, n, warmup) * 1e3,
               time_recover_us=timed(recover, n, warmup) * 1e3,
               attention_relpos_form=int(form[0]),
               # reads every row once (the 5-tap halo: 67 / 64 of it) and writes half as many;
               # reads the skip and half as many z rows, writes the full rows
               time_reduce_bytes=int(4 * d * (M * 67 / 64 + M2)),
               time_recover_bytes=int(4 * d * (2 * M + M2)), rows=M, half_rows=M2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out-dir', default=None)
    args = ap.parse_args(argv)
    from wenet_amd import ASRModel, Squeezeformer
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('librispeech_squeezeformer')
    model = Squeezeformer(configs, S.make_state_dict(configs, 0), device='cuda:0')
    cconf = S.make_configs('aishell_u2pp')
    conformer = ASRModel(cconf, S.make_state_dict(cconf, 0), device='cuda:0')
    print(f'models built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    cenc_ms = timed(lambda: conformer._forward_encoder(feats, lens), args.steps, args.warmup)
    _, mask = model._forward_encoder(feats, lens)
    enc_lens = mask.squeeze(1).sum(1).tolist()
    res = dict(status='measured', config='librispeech_squeezeformer',
               conformer_config='aishell_u2pp', batch=args.batch, audio_s=audio_s,
               steps=args.steps, warmup=args.warmup, dtype='fp32', runs=1, tuned=False,
               encoder_ms=enc_ms, conformer_encoder_ms=cenc_ms,
               encoder_audio_s_per_s=audio_s / (enc_ms * 1e-3),
               conformer_encoder_audio_s_per_s=audio_s / (cenc_ms * 1e-3),
               hbm_spec_tb_per_s=HBM_SPEC_TBS, hbm_copy_tb_per_s=HBM_COPY_TBS)
    res.update(hook_launches(enc_lens, configs['encoder_conf']['attention_heads'], args.steps,
                             args.warmup))
    res['time_reduce_tb_per_s'] = res['time_reduce_bytes'] / (res['time_reduce_us'] * 1e-6) * 1e-12
    res['time_recover_tb_per_s'] = res['time_recover_bytes'] / (res['time_recover_us'] * 1e-6) * 1e-12
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'squeezeformer_librispeech.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round24.md'), 'w') as f:
        f.write(LOG.format(mb_reduce=res['time_reduce_bytes'] / 1e6,
                           mb_recover=res['time_recover_bytes'] / 1e6, **res))
    print(json.dumps(res))
    return 0


LOG = """# Round 24: Squeezeformer encoders

`tools/bench_squeezeformer.py`: `{config}` (synthetic weights) beside the Conformer
`{conformer_config}` of BASELINE.json configs[1], same process, same batch: B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {rows} encoder frames, {half_rows} at the half rate), fp32, {steps}
steps after {warmup}.  All numbers: profiles/squeezeformer_librispeech.json.  The path is
UNTUNED and every figure comes from ONE run: a record, not a pass mark.

| what | ms | audio-s/s |
| --- | --- | --- |
| Squeezeformer encoder (front end + 12 blocks, 6 of them at the half rate) | {encoder_ms:.2f} | {encoder_audio_s_per_s:.0f} |
| Conformer encoder (front end + 12 blocks, tuned routes) | {conformer_encoder_ms:.2f} | {conformer_encoder_audio_s_per_s:.0f} |

One launch on the batch's packed full-rate rows (4 heads of 64) through the operator hooks, HIP
events around {steps} x 4 calls; the hook's descriptor upload is inside every bracket:

| kernel | us / launch |
| --- | --- |
| `attention_sqshift` (the wrapped shift) | {attention_sqshift_us:.1f} |
| `attention_kernel`, rel-pos term without a shift (form code {attention_relpos_form}) | {attention_relpos_us:.1f} |
| `attention_relshift` (FireRed's Transformer-XL shift) | {attention_relshift_us:.1f} |

| kernel | us / launch | MB it must move | TB/s |
| --- | --- | --- | --- |
| `time_reduce_dwconv` (5 taps) | {time_reduce_us:.1f} | {mb_reduce:.1f} | {time_reduce_tb_per_s:.2f} |
| `time_recover_add` | {time_recover_us:.1f} | {mb_recover:.1f} | {time_recover_tb_per_s:.2f} |

The HBM figures of the hardware guide are {hbm_spec_tb_per_s} TB/s (spec) and {hbm_copy_tb_per_s}
TB/s (measured copy); at these sizes the tensors are cache resident and the launch itself is a
large part of the two time kernels' figures.  Not measured: a kernel trace of the encoder (the
per-launch times inside the layer stack), the `stream` reduction, the batch_norm recipe at d 512,
occupancy or LDS-bank counters of `attention_sqshift`.
"""

if __name__ == '__main__':
    sys.exit(main())
