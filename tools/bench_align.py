#!/usr/bin/env python3
"""Time of CTC forced alignment on the BASELINE.json configs[1] batch (AIShell u2++ 256d,
B = 32 x 8-12 s), next to the prefix beam search of the same batch.

Labels = the batch's own greedy tokens (L 66-100, adjacent repeats included).  Every variant
is a host clock around work that ends in a device synchronise; the variants run in alternating
blocks in one process (warm-up first), the reported number is the median over all timed
iterations:

  align              ASRModel.align(): encoder + CTC head + emission gather + trellis + copy + the
                     host's token groups / intervals
  encoder            wn_encode of the batch
  align_tail         wn_ctc_force_align on the encoded batch: CTC GEMM + emission gather +
                     trellis + backtrace + result copy
  trellis_copy       the same call in its log-prob form on the batch's (B, T', V) log-probs: its
                     gather only reads L + 1 values per row, so this is trellis + backtrace +
                     copy; align_tail - trellis_copy = CTC GEMM + fused emission gather
  decode_prefix      decode(['ctc_prefix_beam_search'], beam 10), the whole call
  prefix_head        wn_ctc_logprobs(top-10): CTC GEMM + log-softmax / top-k pass
  prefix_search      wn_ctc_prefix_beam_search: search kernel + result copy (the "prefix beam
                     tail" the alignment tail is held against)

    python tools/bench_align.py [--iters 30] [--warmup 5] [--blocks 4] [--out profiles/align_config2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='config2')
    ap.add_argument('--iters', type=int, default=30, help='timed iterations per block')
    ap.add_argument('--blocks', type=int, default=4, help='alternating blocks per variant')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'align_config2.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_align: needs the GPU (no CPU fallback, nothing is estimated)')
    from wenet_amd import _lib
    from wenet_amd import synthetic as S
    from wenet_amd.align import _call, align_current_batch, force_align_batch
    from wenet_amd.model import ASRModel
    from wenet_amd.search import _prefix_beam, _stream_ptr
    dev = torch.device('cuda', 0)
    wl = S.BENCH_WORKLOADS[args.workload]
    config_name = wl['config'] if isinstance(wl, dict) else wl[0]
    configs = S.make_configs(config_name)
    model = ASRModel(configs, S.make_state_dict(configs, 0), device=dev)
    feats, lens = S.make_bench_batch(args.workload, 1)
    fd = feats.to(dev)
    B = fd.size(0)
    audio_s = float(lens.sum()) * 0.01
    L = model._L
    sp = lambda: _stream_ptr(model.device)   # noqa: E731

    greedy = model.decode(['ctc_greedy_search'], fd, lens)['ctc_greedy_search']
    labels = [list(r.tokens) for r in greedy]
    enc, mask = model._forward_encoder(fd, lens)
    enc_lens_t = mask.squeeze(1).sum(1).cpu()
    logp = model.ctc_logprobs(enc, encoder_lens=enc_lens_t)
    del enc
    speech, lens_np = model._prep(fd, lens)
    state = {}

    def encoder():
        _, state['enc_lens'], state['Tp'] = model._encode(speech, lens_np, -1, -1, False)
        torch.cuda.synchronize()

    def align_tail():
        state['raw'] = align_current_batch(model, labels, state['enc_lens'], state['Tp'])

    def prefix_head():
        _lib.check(L.wn_ctc_logprobs(model._h, args.beam, 0, 0.0, None, state['Tp'], sp()),
                   'wn_ctc_logprobs')
        torch.cuda.synchronize()

    def prefix_search():
        _prefix_beam(model._h, B, int(state['enc_lens'].max()), args.beam, 0, model.device)

    variants = [
        ('align', lambda: model.align(fd, lens, labels)),
        ('decode_prefix', lambda: model.decode(['ctc_prefix_beam_search'], fd, lens,
                                               beam_size=args.beam)),
        ('encoder', encoder),
        ('prefix_head', prefix_head),
        ('prefix_search', prefix_search),
        ('align_tail', align_tail),
        ('trellis_copy', lambda: force_align_batch(logp, enc_lens_t, labels, return_raw=False)),
    ]
    times = {name: [] for name, _ in variants}
    for name, fn in variants:
        for _ in range(args.warmup):
            fn()
    for _ in range(args.blocks):
        for name, fn in variants:
            for _ in range(args.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    p10 = {k: float(np.percentile(v, 10)) for k, v in times.items()}
    p90 = {k: float(np.percentile(v, 90)) for k, v in times.items()}
    raw = state['raw']
    assert (raw['status'] == 0).all()
    frames = int(state['enc_lens'].sum())
    rep = dict(
        workload=args.workload, config=config_name, batch=B, audio_seconds=round(audio_s, 2),
        encoder_frames=frames, longest_frames=int(state['enc_lens'].max()),
        label_lens=[min(map(len, labels)), max(map(len, labels))],
        adjacent_repeats=sum(sum(y[i] == y[i - 1] for i in range(1, len(y))) for y in labels),
        iterations=args.iters * args.blocks, warmup=args.warmup,
        median_ms={k: round(v, 4) for k, v in med.items()},
        p10_ms={k: round(v, 4) for k, v in p10.items()},
        p90_ms={k: round(v, 4) for k, v in p90.items()},
        align_split_ms=dict(
            encoder=round(med['encoder'], 4),
            ctc_gemm_plus_emission_gather=round(med['align_tail'] - med['trellis_copy'], 4),
            trellis_backtrace_copy=round(med['trellis_copy'], 4)),
        align_audio_seconds_per_second=round(audio_s / (med['align'] * 1e-3), 1),
        decode_prefix_audio_seconds_per_second=round(audio_s / (med['decode_prefix'] * 1e-3), 1),
        prefix_beam_tail_ms=round(med['prefix_search'], 4),
        align_tail_ms=round(med['align_tail'], 4),
        align_tail_over_prefix_beam_tail=round(med['align_tail'] / med['prefix_search'], 4),
        trellis_copy_us_per_longest_frame=round(
            med['trellis_copy'] * 1e3 / int(state['enc_lens'].max()), 3),
        note='host clock around calls that end in a device synchronise; variants alternate in '
             'blocks in one process; align_tail = CTC GEMM + emission gather + trellis + copy, '
             'prefix_beam_tail = search kernel + copy only (its CTC GEMM + top-k pass is '
             'prefix_head)')
    print(json.dumps(rep))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rep, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
