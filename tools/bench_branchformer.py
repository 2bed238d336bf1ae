#!/usr/bin/env python3
"""Measure the E-Branchformer path: `aishell_ebranchformer` (the shipped aishell recipe's widths:
d 256, 8 heads of 32, FFN 1024, cgMLP 1024 units, both convs 31 taps, 17 blocks; synthetic
weights), B = 32 utterances of 8-12 s, beside the Conformer of BASELINE.json configs[1]
(`aishell_u2pp`) on the same batch in the same process -- two models side by side, not a ratio.

    python tools/bench_branchformer.py [--steps 10] [--warmup 3] [--out-dir DIR]
                                       [--kernel-stats DIR]

Writes profiles/ebranchformer_aishell.json and docs/LOG_round22.md (or both into --out-dir):
  encoder_ms / conformer_encoder_ms   wn_encode of the batch, HIP events around `steps` calls
  rescoring_ms      decode(['attention_rescoring'], beam 10) of the batch, encoder included
  csgu_gate_us / merge_dwconv_us      one launch on the batch's packed rows through the operator
                    hooks, HIP events: the hook's descriptor upload is inside the bracket
  kernels           with --kernel-stats DIR (the output directory of a run of its own,
                    `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_branchformer.py
                    --steps 2 --warmup 1 --out-dir /tmp/x`): the average time per launch of
                    csgu_stats_kernel and the two dwconv_tile_kernel instantiations from its
                    kernel_stats file, and the bytes/s they reach: the bytes are what the
                    algorithm must move per row (kernel comments in csrc/branchformer.hip), the
                    HBM figures beside them are the guide's (8.0 TB/s spec, 6.29 TB/s measured copy)
No number is a pass condition.
"""
import argparse
import csv
import glob
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


def kernel_bytes(M, C, d2, tile, K, Km):
    """Bytes the two kernels must move for M rows (fp32): the pre-pass reads the gate half; the
    gate kernel reads the gate half ((tile + K - 1) / tile times: the halo), r and the 8-byte
    statistics and writes C floats; the merge reads 2 d (with its halo) and writes 2 d."""
    stats = M * (4 * C + 8)
    gate = M * (4 * C * (tile + K - 1) / tile + 8 + 4 * C + 4 * C)
    merge = M * (4 * d2 * (tile + Km - 1) / tile + 4 * d2)
    return dict(csgu_stats_kernel=stats, csgu_gate=gate, merge_dwconv=merge)


def hook_launches(enc_lens, C, d2, K, Km, steps, warmup):
    from wenet_amd import _lib
    L = _lib.lib()
    lens = np.asarray(enc_lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = int(lens.sum())
    g = torch.Generator(device='cuda').manual_seed(0)
    h = torch.randn(M, 2 * C, device='cuda', generator=g)
    ln_w, ln_b = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    wt = torch.randn(K, C, device='cuda', generator=g) / K ** 0.5
    bias = torch.zeros(C, device='cuda')
    y = torch.empty(M, C, device='cuda')
    cat = torch.randn(M, d2, device='cuda', generator=g)
    wm = torch.randn(Km, d2, device='cuda', generator=g) / Km ** 0.5
    bm = torch.zeros(d2, device='cuda')
    ym = torch.empty(M, d2, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def gate():
        _lib.check(L.wn_op_csgu_gate(h.data_ptr(), 2 * C, M, C, ln_w.data_ptr(), ln_b.data_ptr(),
                                     wt.data_ptr(), bias.data_ptr(), K, 0, 1, y.data_ptr(), C,
                                     _lib.i32p(off), _lib.i32p(lens), len(lens), st), 'csgu_gate')

    def merge():
        _lib.check(L.wn_op_merge_dwconv(cat.data_ptr(), d2, M, d2, wm.data_ptr(), bm.data_ptr(),
                                        Km, 0, ym.data_ptr(), d2, _lib.i32p(off), _lib.i32p(lens),
                                        len(lens), st), 'merge_dwconv')

    return timed(gate, steps * 4, warmup) * 1e3, timed(merge, steps * 4, warmup) * 1e3


def read_kernel_stats(path, nbytes):
    """Average ns per launch of the three kernels from rocprofv3's kernel_stats csv under `path`
    -> {name: dict(avg_us, calls, tb_per_s)}."""
    files = glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {path}')
    want = {'csgu_stats_kernel': 'csgu_stats_kernel', 'dwconv_tile_kernel<0>': 'csgu_gate',
            'dwconv_tile_kernel<1>': 'merge_dwconv'}
    out = {}
    with open(files[0], newline='') as f:
        for row in csv.DictReader(f):
            for pat, name in want.items():
                if pat in row['Name']:
                    us = float(row['AverageNs']) * 1e-3
                    out[name] = dict(avg_us=us, calls=int(row['Calls']),
                                     tb_per_s=nbytes[name] / (us * 1e-6) * 1e-12)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out-dir', default=None)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args(argv)
    from wenet_amd import ASRModel, Branchformer, _lib
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('aishell_ebranchformer')
    model = Branchformer(configs, S.make_state_dict(configs, 0), device='cuda:0')
    cconf = S.make_configs('aishell_u2pp')
    conformer = ASRModel(cconf, S.make_state_dict(cconf, 0), device='cuda:0')
    print(f'models built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    cenc_ms = timed(lambda: conformer._forward_encoder(feats, lens), args.steps, args.warmup)
    res_ms = timed(lambda: model.decode(['attention_rescoring'], feats, lens, beam_size=10),
                   args.steps, args.warmup)
    _, mask = model._forward_encoder(feats, lens)
    enc_lens = mask.squeeze(1).sum(1).tolist()
    ec = configs['encoder_conf']
    C, d2 = ec['cgmlp_linear_units'] // 2, 2 * ec['output_size']
    K, Km = ec['cgmlp_conv_kernel'], ec['merge_conv_kernel']
    gate_us, merge_us = hook_launches(enc_lens, C, d2, K, Km, args.steps, args.warmup)
    M = int(sum(enc_lens))
    nbytes = kernel_bytes(M, C, d2, _lib.lib().wn_csgu_time_tile(), K, Km)
    res = dict(status='measured', config='aishell_ebranchformer', conformer_config='aishell_u2pp',
               batch=args.batch, audio_s=audio_s, steps=args.steps, warmup=args.warmup,
               enc_frames=M, dtype='fp32', encoder_ms=enc_ms, conformer_encoder_ms=cenc_ms,
               rescoring_ms=res_ms, encoder_audio_s_per_s=audio_s / (enc_ms * 1e-3),
               conformer_encoder_audio_s_per_s=audio_s / (cenc_ms * 1e-3),
               rescoring_audio_s_per_s=audio_s / (res_ms * 1e-3), csgu_gate_hook_us=gate_us,
               merge_dwconv_hook_us=merge_us, kernel_bytes=nbytes, hbm_spec_tb_per_s=HBM_SPEC_TBS,
               hbm_copy_tb_per_s=HBM_COPY_TBS, kernels='not collected')
    if args.kernel_stats:
        res['kernels'] = read_kernel_stats(args.kernel_stats, nbytes)
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'ebranchformer_aishell.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    k = res['kernels']
    rows = ''
    if isinstance(k, dict):
        rows = ''.join(f'| `{n}` | {v["avg_us"]:.1f} | {nbytes[n] / 1e6:.1f} | '
                       f'{v["tb_per_s"]:.2f} |\n' for n, v in sorted(k.items()))
    with open(os.path.join(ldir, 'LOG_round22.md'), 'w') as f:
        f.write(LOG.format(kernel_rows=rows or '| not collected | | | |\n', **res))
    print(json.dumps(res))
    return 0


LOG = """# Round 22: Branchformer and E-Branchformer encoders

`tools/bench_branchformer.py`: `{config}` (synthetic weights) beside the Conformer
`{conformer_config}` of BASELINE.json configs[1], same process, same batch: B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {enc_frames} encoder frames), fp32, {steps} steps after {warmup}.
All numbers: profiles/ebranchformer_aishell.json.

| what | ms | audio-s/s |
| --- | --- | --- |
| E-Branchformer encoder (front end + 17 blocks) | {encoder_ms:.2f} | {encoder_audio_s_per_s:.0f} |
| Conformer encoder (front end + 12 blocks, tuned routes) | {conformer_encoder_ms:.2f} | {conformer_encoder_audio_s_per_s:.0f} |
| E-Branchformer `decode(['attention_rescoring'], beam 10)`, encoder included | {rescoring_ms:.2f} | {rescoring_audio_s_per_s:.0f} |

One launch on the batch's packed rows through the operator hooks (HIP events; the hook's
descriptor upload is inside the bracket): `csgu_gate` {csgu_gate_hook_us:.1f} us, `merge_dwconv`
{merge_dwconv_hook_us:.1f} us.

Per launch inside the encoder, from a kernel trace of its own (average over the run), with the
bytes the algorithm must move and the rate that gives; the HBM figures of the hardware guide are
{hbm_spec_tb_per_s} TB/s (spec) and {hbm_copy_tb_per_s} TB/s (measured copy).  A record, not a
pass mark: at these sizes the tensors are cache resident.

| kernel | us / launch | MB / launch | TB/s |
| --- | --- | --- | --- |
{kernel_rows}
The Branchformer path is the plain fp32 one (no six-product, row-block or fused feed-forward
routes), untuned, and its d_k = 32 heads run zero-padded on the d_k = 64 attention kernel.
"""

if __name__ == '__main__':
    sys.exit(main())
