#!/usr/bin/env python3
"""Time the batched RNN-T greedy search (wn_transducer_greedy_search) on the GPU and write
profiles/transducer_greedy.json.

    python tools/bench_transducer.py                      # aishell_u2pp_rnnt, 32 x 8-12 s
    python tools/bench_transducer.py --layers 2 --repeats 2          # a quick look

Workload: `aishell_u2pp_rnnt` with synthetic weights on the batch of BASELINE.json configs[1]
(wenet_amd.synthetic.make_bench_group('config2'): 32 utterances of 8-12 s).  A random joint
emits what its blank bias lets it: the tool tries the biases of --blank-bias in turn and keeps
the first with 30-60 symbols per utterance on average (recorded in the file; a real model's
rate).  The encoder runs once; the search is then timed on that encoder output for every
`rnnt_lookahead`, the settings ALTERNATING in one process, each search a host clock around a
call that ends in a device synchronise.  Reported per lookahead: median / min / max search time,
lock-step steps, time per step; then `greedy_search()` as a whole (encoder + search) in seconds
of audio per second, and `decode(['ctc_prefix_beam_search'], beam 10)` of the same model and
batch beside it for scale.

The per-kernel split (enc_proj / predictor / joint / advance) comes from a kernel trace in a run
of its own, because the handle's launch brackets (wn_profile_enable) time the GEMM launchers
only and a traced run is not a timed one:

    rocprofv3 --kernel-trace --stats -d profiles/transducer_trace -- \
        python tools/bench_transducer.py --layers 2 --searches-only 3

In its kernel statistics rnnt_linear_kernel + rnnt_cell_kernel are the predictor with joint.pred_ffn (6 launches
per step at the recipe's two layers), rnnt_joint_kernel the joint, rnnt_advance_kernel the advance;
enc_proj is the one tile-GEMM launch per search with N = join_dim.  Nothing here reads counters.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOOKAHEADS = (1, 2, 4, 8, 16)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--config', default='aishell_u2pp_rnnt')
    p.add_argument('--layers', type=int, default=None, help='encoder blocks (a quick look)')
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--n-steps', type=int, default=64)
    p.add_argument('--blank-bias', type=float, nargs='+', default=[8.5, 8.0, 9.0, 7.0, 6.0])
    p.add_argument('--searches-only', type=int, default=0,
                   help='profiler runs: N searches per lookahead, no JSON')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transducer_greedy.json'))
    args = p.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_transducer: needs the GPU (no CPU fallback)')
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import basic_greedy_search

    configs = S.make_configs(args.config)
    if args.layers is not None:
        configs['encoder_conf']['num_blocks'] = args.layers
    feats, lens = S.make_bench_group('config2')
    feats = feats.cuda()
    audio_s = float(lens.sum()) * 0.01
    sync = torch.cuda.synchronize

    model = enc = enc_lens = None
    picked = None
    for bias in args.blank_bias:
        sd = S.make_state_dict(configs, 0, rnnt_blank_bias=bias)
        model = Transducer(configs, sd, device='cuda')
        enc, mask = model._forward_encoder(feats, lens)
        enc_lens = mask.squeeze(1).sum(1).cpu()
        toks = basic_greedy_search(model, enc, enc_lens, args.n_steps)
        mean = sum(len(u) for u in toks) / len(toks)
        print(f'blank bias {bias}: {mean:.1f} symbols per utterance', flush=True)
        picked = dict(blank_bias=bias, mean_symbols=mean, in_range=30 <= mean <= 60,
                      symbols=[len(u) for u in toks])
        if picked['in_range']:
            break
    ref_tokens = basic_greedy_search(model, enc, enc_lens, args.n_steps)

    def one_search(F):
        model.tune('rnnt_lookahead', F)
        sync()
        t0 = time.perf_counter()
        toks = basic_greedy_search(model, enc, enc_lens, args.n_steps)
        dt = time.perf_counter() - t0
        assert toks == ref_tokens, f'lookahead {F} decodes other tokens'
        return dt, model.last_rnnt_steps

    for F in LOOKAHEADS:          # warm up every shape
        one_search(F)
    if args.searches_only:
        for _ in range(args.searches_only):
            for F in LOOKAHEADS:
                one_search(F)
        return 0
    times = {F: [] for F in LOOKAHEADS}
    steps = {}
    for _ in range(args.repeats):
        for F in LOOKAHEADS:
            dt, steps[F] = one_search(F)
            times[F].append(dt)
    table = {}
    for F in LOOKAHEADS:
        med = statistics.median(times[F])
        table[str(F)] = dict(search_ms=dict(median=med * 1e3, min=min(times[F]) * 1e3,
                                            max=max(times[F]) * 1e3),
                             steps=steps[F], us_per_step=med * 1e6 / max(steps[F], 1))
        print(f'lookahead {F:2d}: {med * 1e3:8.2f} ms  ({steps[F]} steps, '
              f'{med * 1e6 / max(steps[F], 1):.1f} us / step)', flush=True)
    best = min(LOOKAHEADS, key=lambda F: table[str(F)]['search_ms']['median'])
    model.tune('rnnt_lookahead', best)

    def timed(fn):
        fn(); sync()
        ts = []
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_rnnt = timed(lambda: model.greedy_search(feats, lens, n_steps=args.n_steps))
    t_ctc = timed(lambda: model.decode(['ctc_prefix_beam_search'], feats, lens, beam_size=10))
    out = dict(config=args.config, encoder_blocks=configs['encoder_conf']['num_blocks'],
               batch=int(feats.shape[0]), audio_seconds=audio_s, n_steps=args.n_steps,
               weights=picked, lookahead=table, fastest_lookahead=best,
               greedy_search=dict(lookahead=best, seconds=t_rnnt, audio_s_per_s=audio_s / t_rnnt),
               ctc_prefix_beam_search_beam10=dict(seconds=t_ctc, audio_s_per_s=audio_s / t_ctc),
               kernel_split='from a kernel trace in a run of its own: see the command in this '
                            'tool\'s docstring (--searches-only)',
               method='host clock around calls that end in a device synchronise; settings '
                      'alternate in one process; median of --repeats')
    print(json.dumps(out['greedy_search']), json.dumps(out['ctc_prefix_beam_search_beam10']))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
