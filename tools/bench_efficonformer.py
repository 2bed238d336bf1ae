#!/usr/bin/env python3
"""Measure the Efficient Conformer path: `aishell_efficonformer_v1`
(train_u2++_efficonformer_v1.yaml at its encoder's widths: d 256, 8 heads, FFN 2048, K 15 -> 7,
12 blocks, grouped layers 0-3, stride layer 3; a decoder of 4 heads; synthetic weights), B = 32
utterances of 8-12 s, beside the Conformer of BASELINE.json configs[1] (`aishell_u2pp`) on the
same batch in the same process -- two models side by side, not a ratio.

    python tools/bench_efficonformer.py [--steps 10] [--warmup 3] [--out-dir DIR]

Writes profiles/efficonformer_aishell.json and docs/LOG_round26.md (or both into --out-dir):
  encoder_ms / conformer_encoder_ms   wn_encode of the batch, HIP events around `steps` calls
  attention_grouped_us   one launch on the batch's packed rate-4 rows (8 heads, W = 96, g = 3)
                    through the operator hook, HIP events around 4 x `steps` calls
  attention_relpos_us    attention_kernel with the rel-pos term on the same rows as the plain
                    layers of this model run it: 8 heads of 32 laid out as 64 columns each
  stride_dwconv_us / avgpool_residual_us   likewise, with the bytes the kernels must move
The hook's descriptor upload (one small host-to-device copy) is inside every bracket.  The path
is untuned and every figure comes from ONE run of this tool: a record, not a pass mark.

    python tools/bench_efficonformer.py --leg dec8 [--steps 10] [--warmup 3] [--out-dir DIR]

The decoder leg (dec8_leg below): `aishell_efficonformer_v1_dec8`, the recipe with its own 8-head
decoders, beside the 4-head `aishell_efficonformer_v1`; writes
profiles/efficonformer_aishell_dec8.json and docs/LOG_round27.md.
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


def hook_launches(lens0, H, d, K, steps, warmup):
    """us per launch of the two attention kernels and the two stride kernels on the same rows."""
    from wenet_amd import _lib
    L = _lib.lib()
    g, W, dq = 3, 3 * d // H, H * 64
    lens = np.asarray(lens0, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    lens2 = (lens + 1) // 2
    off2 = np.concatenate([[0], np.cumsum(lens2)[:-1]]).astype(np.int32)
    M, M2, tmax = int(lens.sum()), int(lens2.sum()), int(lens.max())
    gen = torch.Generator(device='cuda').manual_seed(0)
    qkv = torch.randn(M, 3 * d, device='cuda', generator=gen)
    P = torch.randn(tmax, d, device='cuda', generator=gen)
    bu = torch.randn(H, W, device='cuda', generator=gen) * 0.5
    bv = torch.randn(H, W, device='cuda', generator=gen) * 0.5
    O = torch.empty(M, d, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d

    def grouped():
        _lib.check(L.wn_op_attention_grouped(q, k, v, 3 * d, 3 * d, 3 * d, M, P.data_ptr(), d,
                                             tmax, None, bu.data_ptr(), bv.data_ptr(),
                                             O.data_ptr(), d, _lib.i32p(off), _lib.i32p(lens),
                                             len(lens), H, g, W, g, 0, -1, W ** -0.5, st),
                   'attention_grouped')

    # the plain layers' attention: heads of 32 as 64 columns, the upper 32 zero
    qkv2 = torch.zeros(M, 3 * dq, device='cuda')
    qkv2.view(M, 3 * H, 64)[:, :, :32] = torch.randn(M, 3 * H, 32, device='cuda', generator=gen)
    P2 = torch.zeros(tmax, dq, device='cuda')
    P2.view(tmax, H, 64)[:, :, :32] = torch.randn(tmax, H, 32, device='cuda', generator=gen)
    bu2 = torch.zeros(H, 64, device='cuda')
    bv2 = torch.zeros(H, 64, device='cuda')
    bu2[:, :32] = bu[:, :32]
    bv2[:, :32] = bv[:, :32]
    O2 = torch.empty(M, dq, device='cuda')
    op = _lib.WnAttentionOp()
    op.Q, op.K, op.V = qkv2.data_ptr(), qkv2.data_ptr() + 4 * dq, qkv2.data_ptr() + 8 * dq
    op.ldq = op.ldk = op.ldv = 3 * dq
    op.q_rows = op.kv_rows = M
    op.P, op.ldp, op.p_rows = P2.data_ptr(), dq, tmax
    op.bias_u, op.bias_v = bu2.data_ptr(), bv2.data_ptr()
    op.O, op.ldo = O2.data_ptr(), dq
    op.q_off = op.kv_off = _lib.i32p(off)
    op.q_len = op.kv_len = _lib.i32p(lens)
    op.n_seq, op.n_heads = len(lens), H
    op.mask_mode, op.chunk_size, op.left_chunks, op.scale = 0, 0, -1, 32 ** -0.5
    op.flags, op.precision, op.x6_galign = 0, 0, 0
    form = np.zeros(1, dtype=np.int32)

    def relpos():
        _lib.check(L.wn_op_attention(op, _lib.i32p(form), st), 'attention')

    x = torch.randn(M, d, device='cuda', generator=gen)
    wt = torch.randn(K, d, device='cuda', generator=gen)
    bias = torch.zeros(d, device='cuda')
    lw, lb = torch.ones(d, device='cuda'), torch.zeros(d, device='cuda')
    y2 = torch.empty(M2, d, device='cuda')
    z = torch.randn(M2, d, device='cuda', generator=gen)

    def strided():
        _lib.check(L.wn_op_stride_dwconv_ln_silu(
            x.data_ptr(), d, M, d, wt.data_ptr(), bias.data_ptr(), None, lw.data_ptr(),
            lb.data_ptr(), 0, 1e-5, K, 0, 2, y2.data_ptr(), d, M2, _lib.i32p(off), _lib.i32p(lens),
            _lib.i32p(off2), len(lens), st), 'stride_dwconv_ln_silu')

    def pooled():
        _lib.check(L.wn_op_avgpool_residual_add(
            x.data_ptr(), d, M, z.data_ptr(), d, z.data_ptr(), d, M2, d, 2, _lib.i32p(off),
            _lib.i32p(lens), _lib.i32p(off2), len(lens), st), 'avgpool_residual_add')

    n = steps * 4
    return dict(attention_grouped_us=timed(grouped, n, warmup) * 1e3,
                attention_relpos_us=timed(relpos, n, warmup) * 1e3,
                stride_dwconv_us=timed(strided, n, warmup) * 1e3,
                avgpool_residual_us=timed(pooled, n, warmup) * 1e3,
                attention_relpos_form=int(form[0]),
                # reads every row once and writes half as many; reads x and z, writes z
                stride_dwconv_bytes=int(4 * d * (M + M2)),
                avgpool_residual_bytes=int(4 * d * (M + 2 * M2)), rows=M, half_rows=M2)


def wall_ms(fn, steps, warmup):
    """Wall time per call of a decode (host work and result copies included)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def dec8_leg(args):
    """The decoder leg: `aishell_efficonformer_v1_dec8` (the recipe as shipped: two decoders of 8
    heads of 32 on attention_d32 and the d_k = 32 step kernel) beside the 4-head
    `aishell_efficonformer_v1` (heads of 64 on attention_kernel), same process, same batch:
    model.decode wall time of `attention_rescoring` and of `attention`, both at beam 10.  Two
    different models (the same weight matrices cut into 8 or 4 heads: other functions, other
    hypotheses): a record of one run, gating nothing.  Writes
    profiles/efficonformer_aishell_dec8.json and docs/LOG_round27.md."""
    from wenet_amd import EfficientConformer
    from wenet_amd import synthetic as S
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    res = dict(status='measured', batch=args.batch, audio_s=float(lens.sum()) * 0.01,
               steps=args.steps, warmup=args.warmup, dtype='fp32', runs=1, tuned=False, beam=10)
    for key, name in (('dec8', 'aishell_efficonformer_v1_dec8'),
                      ('dec4', 'aishell_efficonformer_v1')):
        configs = S.make_configs(name)
        model = EfficientConformer(configs, S.make_state_dict(configs, 0), device='cuda:0')
        res[key + '_config'] = name
        res[key + '_heads'] = configs['decoder_conf']['attention_heads']
        for mode in ('attention_rescoring', 'attention'):
            kw = dict(beam_size=10, ctc_weight=0.5, reverse_weight=0.3) \
                if mode == 'attention_rescoring' else dict(beam_size=10)
            out = model.decode([mode], feats, lens, **kw)[mode]
            res[f'{key}_{mode}_ms'] = wall_ms(lambda: model.decode([mode], feats, lens, **kw),
                                              args.steps, args.warmup)
            res[f'{key}_{mode}_tokens'] = int(sum(len(r.tokens) for r in out))
        del model
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'efficonformer_aishell_dec8.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round27.md'), 'w') as f:
        f.write(LOG_DEC8.format(**res))
    print(json.dumps(res))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out-dir', default=None)
    ap.add_argument('--leg', choices=('encoder', 'dec8'), default='encoder',
                    help='encoder: the encoder and its kernels; dec8: the 8-head decoders')
    args = ap.parse_args(argv)
    if args.leg == 'dec8':
        return dec8_leg(args)
    from wenet_amd import ASRModel, EfficientConformer
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('aishell_efficonformer_v1')
    model = EfficientConformer(configs, S.make_state_dict(configs, 0), device='cuda:0')
    cconf = S.make_configs('aishell_u2pp')
    conformer = ASRModel(cconf, S.make_state_dict(cconf, 0), device='cuda:0')
    print(f'models built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    cenc_ms = timed(lambda: conformer._forward_encoder(feats, lens), args.steps, args.warmup)
    lens0 = [(int(n) - 7) // 4 + 1 for n in lens]
    ec = configs['encoder_conf']
    res = dict(status='measured', config='aishell_efficonformer_v1',
               conformer_config='aishell_u2pp', batch=args.batch, audio_s=audio_s,
               steps=args.steps, warmup=args.warmup, dtype='fp32', runs=1, tuned=False,
               encoder_ms=enc_ms, conformer_encoder_ms=cenc_ms,
               encoder_audio_s_per_s=audio_s / (enc_ms * 1e-3),
               conformer_encoder_audio_s_per_s=audio_s / (cenc_ms * 1e-3),
               hbm_spec_tb_per_s=HBM_SPEC_TBS, hbm_copy_tb_per_s=HBM_COPY_TBS)
    res.update(hook_launches(lens0, ec['attention_heads'], ec['output_size'],
                             ec['cnn_module_kernel'], args.steps, args.warmup))
    for k in ('stride_dwconv', 'avgpool_residual'):
        res[k + '_tb_per_s'] = res[k + '_bytes'] / (res[k + '_us'] * 1e-6) * 1e-12
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'efficonformer_aishell.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round26.md'), 'w') as f:
        f.write(LOG.format(mb_stride=res['stride_dwconv_bytes'] / 1e6,
                           mb_pool=res['avgpool_residual_bytes'] / 1e6, **res))
    print(json.dumps(res))
    return 0


LOG = """# Round 26: Efficient Conformer encoders

`tools/bench_efficonformer.py`: `{config}` (synthetic weights) beside the Conformer
`{conformer_config}` of BASELINE.json configs[1], same process, same batch: B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {rows} encoder frames behind the front end, {half_rows} behind the
stride layer), fp32, {steps} steps after {warmup}.  All numbers: profiles/efficonformer_aishell.json.
The path is UNTUNED and every figure comes from ONE run: a record, not a pass mark.

| what | ms | audio-s/s |
| --- | --- | --- |
| Efficient Conformer encoder (front end + 12 blocks: 4 grouped, 8 at the half rate) | {encoder_ms:.2f} | {encoder_audio_s_per_s:.0f} |
| Conformer encoder (front end + 12 blocks, tuned routes) | {conformer_encoder_ms:.2f} | {conformer_encoder_audio_s_per_s:.0f} |

One launch on the batch's packed rows behind the front end through the operator hooks, HIP events
around {steps} x 4 calls; the hook's descriptor upload is inside every bracket:

| kernel | us / launch |
| --- | --- |
| `attention_grouped`, 8 heads, W = 96, g = 3, full context | {attention_grouped_us:.1f} |
| `attention_kernel`, rel-pos term, 8 heads of 32 laid out as 64 columns (form code {attention_relpos_form}) | {attention_relpos_us:.1f} |

| kernel | us / launch | MB it must move | TB/s |
| --- | --- | --- | --- |
| `stride_dwconv_ln_silu` (K 15, LayerNorm) | {stride_dwconv_us:.1f} | {mb_stride:.1f} | {stride_dwconv_tb_per_s:.2f} |
| `avgpool_residual_add` | {avgpool_residual_us:.1f} | {mb_pool:.1f} | {avgpool_residual_tb_per_s:.2f} |

The HBM figures of the hardware guide are {hbm_spec_tb_per_s} TB/s (spec) and {hbm_copy_tb_per_s}
TB/s (measured copy); at these sizes the tensors are cache resident and the launch itself is a
large part of `avgpool_residual_add`'s figure.  `stride_dwconv_ln_silu` is a wave-per-frame kernel
that reads its taps from global memory: far from the bytes it must move, and where its time goes
has not been measured.  Not measured either: a kernel trace of the encoder (the
per-launch times inside the layer stack), W = 192, chunk masks, the causal and batch_norm
variants, the conv2d2 front end, occupancy or LDS-bank counters of `attention_grouped` (the
compiler reports 264 registers at W = 96 and 404 at W = 192, one wave per SIMD, no scratch).
"""

LOG_DEC8 = """# Round 27: decoder heads of 32

`tools/bench_efficonformer.py --leg dec8`: `{dec8_config}` (the recipe as
shipped: two decoders of {dec8_heads} heads of 32 on `attention_d32` and the d_k = 32 step kernel) beside `{dec4_config}`
({dec4_heads} heads of 64 on `attention_kernel`), synthetic weights, same process, same batch:
B = {batch} x 8-12 s ({audio_s:.1f} s of audio), fp32, beam {beam}, wall time of `model.decode`
per call over {steps} calls after {warmup}.  All numbers: profiles/efficonformer_aishell_dec8.json.
Two DIFFERENT models (the same synthetic weight matrices cut into 8 or 4 heads: other functions,
other hypotheses), ONE run, untuned: a record, not a pass mark and not a ratio.

| mode | 8 heads of 32: ms | tokens out | 4 heads of 64: ms | tokens out |
| --- | --- | --- | --- | --- |
| `attention_rescoring` | {dec8_attention_rescoring_ms:.2f} | {dec8_attention_rescoring_tokens} | {dec4_attention_rescoring_ms:.2f} | {dec4_attention_rescoring_tokens} |
| `attention` | {dec8_attention_ms:.2f} | {dec8_attention_tokens} | {dec4_attention_ms:.2f} | {dec4_attention_tokens} |

Not measured: a kernel trace of either decode (the share of the attention launches in these wall
times), `attention_d32` per launch, more than one wave per block, LDS-bank counters.
"""

if __name__ == '__main__':
    sys.exit(main())
