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

    python tools/bench_transducer.py --beam              # the prefix beam search instead

--beam times the batched prefix beam search (wn_transducer_beam_search) on the same model, batch
and fixed encoder output and writes profiles/transducer_beam.json: beam 5 and 10 with
(ctc_weight, transducer_weight) = (0.3, 0.7) and (0.0, 1.0), the settings alternating, median of
--repeats; per setting the search time, the time per step (a step is one frame: `longest T'`
steps), the launches per step (2 per LSTM layer, the projection, joint.pred_ffn, the joint, the
fusion + top-k, the beam step, the state gather) and the rows per step that ran the LSTM step
(`advance`) against the B x beam rows rnnt_linear_kernel walks.  Beside it, in the same process:
the greedy search at its shipped lookahead and decode(['ctc_prefix_beam_search'], beam 10).

    python tools/bench_transducer.py --rescore           # transducer + attention rescoring

--rescore times the parts of Transducer.transducer_attention_rescoring on the same model, batch and
fixed encoder output and writes profiles/transducer_rescore.json: beams 5 and 10, search weights
(0.3, 0.7), rescoring weights (ctc 0.3, attn 0.4, transducer 0.3, reverse 0.3), the beams
alternating, median of --repeats.  Per beam: the search, wn_transducer_score (and, from a call of
their own under wn_profile_enable, by events on its stream: joint.enc_ffn, the predictor over the
trie, the gather GEMM and the lattices), the attention scores (wn_rescore); the GEMM rows computed
against the rows without prefix sharing; `transducer_attention_rescoring()` as a whole in seconds
of audio per second beside `beam_search()`.

    python tools/bench_transducer.py --predictor embedding     # a stateless predictor

--predictor embedding | conv times the searches of a model with a stateless predictor
(`aishell_u2pp_rnnt_embed`: examples/aishell/rnnt/conf/example_embedding_predictor.yaml's 320 /
320, 4 heads, history 5, join 320; conv: the same widths with a ConvPredictor) and of the LSTM
model (`aishell_u2pp_rnnt`) beside it in the same process, on the same batch, each on its own
fixed encoder output, and writes profiles/transducer_stateless.json: the greedy search at
lookahead 1 / 4 / 16 and the prefix beam search with beam 5 / 10 at (0.3, 0.7), the models and
settings alternating, median of --repeats; per setting the search time, the steps, the time per
step and the launches per step (beam: 2 per LSTM layer + 6 = 10 for the LSTM model; one
rnnt_stateless_step, the joint, the fusion + top-k, the beam step and the gather = 5 for a
stateless one).  Each model gets the first blank bias of --blank-bias with 30-60 symbols per
utterance (for the stateless model 10.0 .. 12.0 are tried after them: a random joint emits
more under such a predictor).

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
    p.add_argument('--beam', action='store_true', help='time the prefix beam search')
    p.add_argument('--rescore', action='store_true',
                   help='time transducer + attention rescoring')
    p.add_argument('--predictor', choices=('rnn', 'embedding', 'conv'), default='rnn',
                   help='embedding / conv: time a stateless predictor beside the LSTM model')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    if args.predictor != 'rnn':
        return bench_stateless(args)
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'transducer_rescore.json' if args.rescore
                                else 'transducer_beam.json' if args.beam
                                else 'transducer_greedy.json')

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
    if args.beam:
        return bench_beam(args, model, configs, feats, lens, enc, enc_lens, audio_s, picked)
    if args.rescore:
        return bench_rescore(args, model, configs, feats, lens, enc, enc_lens, audio_s, picked)

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


STATELESS_LOOKAHEADS = (1, 4, 16)
STATELESS_BEAMS = ((5, 0.3, 0.7), (10, 0.3, 0.7))


def bench_stateless(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_transducer: needs the GPU (no CPU fallback)')
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import basic_greedy_search, prefix_beam_search
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'transducer_stateless.json')
    sync = torch.cuda.synchronize
    feats, lens = S.make_bench_group('config2')
    feats = feats.cuda()
    B = int(feats.shape[0])
    audio_s = float(lens.sum()) * 0.01
    if args.predictor == 'embedding':
        stateless = S.make_configs('aishell_u2pp_rnnt_embed')
    else:
        S.CONFIGS['aishell_u2pp_rnnt_conv'] = S._rnnt_stateless(
            'aishell_u2pp_rnnt', 'conv', 320, 320, history_size=5, activation='relu', bias=True)
        stateless = S.make_configs('aishell_u2pp_rnnt_conv')
    models = {}
    for kind, configs in (('rnn', S.make_configs('aishell_u2pp_rnnt')), (args.predictor, stateless)):
        if args.layers is not None:
            configs['encoder_conf']['num_blocks'] = args.layers
        # (a random joint emits more under a stateless predictor: larger biases are tried too)
        for bias in list(args.blank_bias) + ([] if kind == 'rnn' else [10.0, 10.5, 11.0, 11.5, 12.0]):
            model = Transducer(configs, S.make_state_dict(configs, 0, rnnt_blank_bias=bias),
                               device='cuda')
            enc, mask = model._forward_encoder(feats, lens)
            enc_lens = mask.squeeze(1).sum(1).cpu()
            toks = basic_greedy_search(model, enc, enc_lens, args.n_steps)
            mean = sum(len(u) for u in toks) / len(toks)
            print(f'{kind}: blank bias {bias}: {mean:.1f} symbols per utterance', flush=True)
            picked = dict(blank_bias=bias, mean_symbols=mean, in_range=30 <= mean <= 60)
            if picked['in_range']:
                break
        layers = configs['predictor_conf'].get('num_layers', 0)
        models[kind] = dict(model=model, enc=enc, enc_lens=enc_lens, weights=picked, tokens=toks,
                            beam_launches=2 * layers + 6 if kind == 'rnn' else 5,
                            greedy_launches=2 * layers + 4 if kind == 'rnn' else 3)

    def greedy(kind, F):
        m = models[kind]
        m['model'].tune('rnnt_lookahead', F)
        sync()
        t0 = time.perf_counter()
        toks = basic_greedy_search(m['model'], m['enc'], m['enc_lens'], args.n_steps)
        dt = time.perf_counter() - t0
        assert toks == m['tokens'], f'{kind}: lookahead {F} decodes other tokens'
        return dt, m['model'].last_rnnt_steps

    def beam(kind, setting):
        m = models[kind]
        sync()
        t0 = time.perf_counter()
        nbest = prefix_beam_search(m['model'], m['enc'], m['enc_lens'], *setting)
        dt = time.perf_counter() - t0
        return dt, m['model'].last_rnnt_steps, nbest

    runs = [(kind, 'greedy', F) for F in STATELESS_LOOKAHEADS for kind in models] + \
        [(kind, 'beam', s) for s in STATELESS_BEAMS for kind in models]
    first = {}
    for r in runs:                    # warm up every shape
        first[r] = greedy(r[0], r[2]) if r[1] == 'greedy' else beam(r[0], r[2])
    times = {r: [] for r in runs}
    for _ in range(args.repeats):
        for r in runs:
            got = greedy(r[0], r[2]) if r[1] == 'greedy' else beam(r[0], r[2])
            assert r[1] == 'greedy' or got[2] == first[r][2], f'{r}: another result on a repeat'
            times[r].append(got[0])
    out = dict(batch=B, audio_seconds=audio_s, n_steps=args.n_steps, models={},
               method='host clock around calls that end in a device synchronise; models and '
                      'settings alternate in one process; median of --repeats')
    for kind, m in models.items():
        table = dict(weights=m['weights'], greedy={}, beam=[])
        for r in runs:
            if r[0] != kind:
                continue
            med = statistics.median(times[r])
            steps = first[r][1]
            row = dict(search_ms=dict(median=med * 1e3, min=min(times[r]) * 1e3,
                                      max=max(times[r]) * 1e3),
                       steps=steps, us_per_step=med * 1e6 / max(steps, 1))
            if r[1] == 'greedy':
                row['launches_per_step'] = m['greedy_launches']
                table['greedy'][str(r[2])] = row
                what = f'greedy lookahead {r[2]:2d}'
            else:
                row.update(beam=r[2][0], ctc_weight=r[2][1], transducer_weight=r[2][2],
                           launches_per_step=m['beam_launches'], rows=B * r[2][0])
                table['beam'].append(row)
                what = f'beam {r[2][0]:2d} {r[2][1:]}'
            print(f"{kind:9s} {what}: {med * 1e3:8.2f} ms  ({steps} steps, "
                  f"{row['us_per_step']:.1f} us / step, {row['launches_per_step']} launches / step)",
                  flush=True)
        out['models'][kind] = table
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)
    return 0


BEAM_SETTINGS = ((5, 0.3, 0.7), (5, 0.0, 1.0), (10, 0.3, 0.7), (10, 0.0, 1.0))


def bench_beam(args, model, configs, feats, lens, enc, enc_lens, audio_s, picked):
    import torch
    from wenet_amd.transducer import basic_greedy_search, prefix_beam_search
    sync = torch.cuda.synchronize
    B = int(feats.shape[0])
    n_layers = configs['predictor_conf']['num_layers']
    launches = 2 * n_layers + 6

    def one(setting):
        beam, cw, tw = setting
        sync()
        t0 = time.perf_counter()
        nbest = prefix_beam_search(model, enc, enc_lens, beam, cw, tw)
        dt = time.perf_counter() - t0
        return dt, nbest

    first, stats = {}, {}
    for s in BEAM_SETTINGS:          # warm up every shape
        first[s] = one(s)[1]
        stats[s] = (model.last_rnnt_steps, model.last_rnnt_advance_rows)
    if args.searches_only:
        for _ in range(args.searches_only):
            for s in BEAM_SETTINGS:
                one(s)
        return 0
    times = {s: [] for s in BEAM_SETTINGS}
    for _ in range(args.repeats):
        for s in BEAM_SETTINGS:
            dt, nbest = one(s)
            assert nbest == first[s], f'{s}: another result on a repeat'
            times[s].append(dt)
    table = []
    for s in BEAM_SETTINGS:
        beam, cw, tw = s
        med = statistics.median(times[s])
        steps, adv = stats[s]
        row = dict(beam=beam, ctc_weight=cw, transducer_weight=tw,
                   search_ms=dict(median=med * 1e3, min=min(times[s]) * 1e3,
                                  max=max(times[s]) * 1e3),
                   steps=steps, us_per_step=med * 1e6 / max(steps, 1), launches_per_step=launches,
                   rows=B * beam, advancing_rows_per_step=adv / max(steps, 1),
                   mean_best_len=sum(len(u[0][0]) for u in first[s]) / B)
        table.append(row)
        print(f'beam {beam:2d} ({cw}, {tw}): {med * 1e3:8.2f} ms  ({steps} steps, '
              f"{row['us_per_step']:.1f} us / step, {launches} launches / step, "
              f"{row['advancing_rows_per_step']:.1f} of {B * beam} rows advance)", flush=True)

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

    F = model.tune('rnnt_lookahead')
    t_greedy = timed(lambda: basic_greedy_search(model, enc, enc_lens, args.n_steps))
    greedy_steps = model.last_rnnt_steps
    t_ctc = timed(lambda: model.decode(['ctc_prefix_beam_search'], feats, lens, beam_size=10))
    t_e2e = timed(lambda: model.beam_search(feats, lens, beam_size=10))
    out = dict(config=args.config, encoder_blocks=configs['encoder_conf']['num_blocks'], batch=B,
               audio_seconds=audio_s, weights=picked, beam_search=table,
               greedy_search_on_the_same_encoder_output=dict(
                   lookahead=F, search_ms=t_greedy * 1e3, steps=greedy_steps,
                   us_per_step=t_greedy * 1e6 / max(greedy_steps, 1)),
               beam_search_beam10_with_encoder=dict(seconds=t_e2e, audio_s_per_s=audio_s / t_e2e),
               ctc_prefix_beam_search_beam10_with_encoder=dict(seconds=t_ctc,
                                                               audio_s_per_s=audio_s / t_ctc),
               method='host clock around calls that end in a device synchronise; settings '
                      'alternate in one process; median of --repeats')
    print(json.dumps(out['greedy_search_on_the_same_encoder_output']),
          json.dumps(out['beam_search_beam10_with_encoder']),
          json.dumps(out['ctc_prefix_beam_search_beam10_with_encoder']))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)
    return 0


RESCORE_BEAMS = (5, 10)
RESCORE_SEARCH = (0.3, 0.7)                  # (ctc, transducer) of the search
RESCORE_WEIGHTS = (0.3, 0.4, 0.3, 0.3)       # (ctc, attn, transducer, reverse) of the rescoring


def bench_rescore(args, model, configs, feats, lens, enc, enc_lens, audio_s, picked):
    import ctypes
    import torch
    from wenet_amd import _lib
    from wenet_amd import transducer as T
    sync = torch.cuda.synchronize
    B = int(feats.shape[0])
    cw, aw, tw, rw = RESCORE_WEIGHTS

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return time.perf_counter() - t0, out

    def one(beam):
        t_search, nbest = clock(lambda: T.prefix_beam_search(model, enc, enc_lens, beam,
                                                             *RESCORE_SEARCH))
        hyps = [[t for t, _ in u] for u in nbest]
        t_score, td = clock(lambda: T._score_current(model, hyps))
        rows_stat = model.last_rnnt_score_rows
        # the stages, in a call of their own under the handle's launch brackets (event marks
        # inside wn_transducer_score); the timed call above records none
        _lib.check(model._L.wn_profile_enable(model._h, 1), 'wn_profile_enable')
        try:
            td_marked = T._score_current(model, hyps)
            ms = (ctypes.c_float * 4)()
            _lib.check(model._L.wn_transducer_score_times(model._h, ms),
                       'wn_transducer_score_times')
        finally:
            _lib.check(model._L.wn_profile_enable(model._h, 0), 'wn_profile_enable')
        assert td_marked == td
        t_attn, attn = clock(lambda: T._attn_scores_current(model, hyps, rw))
        return dict(search=t_search, score=t_score, attn=t_attn, enc_proj=ms[0] * 1e-3,
                    predictor=ms[1] * 1e-3, gather=ms[2] * 1e-3, lattice=ms[3] * 1e-3), \
            (nbest, td, attn, rows_stat)

    first = {beam: one(beam)[1] for beam in RESCORE_BEAMS}      # warm up every shape
    if args.searches_only:
        for _ in range(args.searches_only):
            for beam in RESCORE_BEAMS:
                one(beam)
        return 0
    times = {beam: [] for beam in RESCORE_BEAMS}
    for _ in range(args.repeats):
        for beam in RESCORE_BEAMS:
            t, got = one(beam)
            assert got[:3] == first[beam][:3], f'beam {beam}: another result on a repeat'
            times[beam].append(t)

    def timed(fn):
        fn(); sync()
        ts = [clock(fn)[0] for _ in range(args.repeats)]
        return statistics.median(ts)

    J, V = configs['joint_conf']['join_dim'], configs['output_dim']
    table = []
    for beam in RESCORE_BEAMS:
        med = {k: statistics.median(t[k] for t in times[beam]) for k in times[beam][0]}
        nbest, _, _, (rows, unshared, nodes) = first[beam]
        t_e2e = timed(lambda: model.transducer_attention_rescoring(
            feats, lens, beam, reverse_weight=rw, ctc_weight=cw, attn_weight=aw,
            transducer_weight=tw, search_ctc_weight=RESCORE_SEARCH[0],
            search_transducer_weight=RESCORE_SEARCH[1]))
        t_bs = timed(lambda: model.beam_search(feats, lens, beam_size=beam,
                                               ctc_weight=RESCORE_SEARCH[0],
                                               transducer_weight=RESCORE_SEARCH[1]))
        row = dict(beam=beam, ms={k: v * 1e3 for k, v in med.items()},
                   rows=rows, rows_unshared=unshared, trie_nodes=nodes,
                   gather_tflops=rows * 2.0 * J * V / max(med['gather'], 1e-9) * 1e-12,
                   mean_hyp_len=sum(len(t) for u in nbest for t, _ in u)
                   / max(sum(len(u) for u in nbest), 1),
                   transducer_attention_rescoring=dict(seconds=t_e2e, audio_s_per_s=audio_s / t_e2e),
                   beam_search=dict(seconds=t_bs, audio_s_per_s=audio_s / t_bs))
        table.append(row)
        print(f"beam {beam:2d}: search {med['search'] * 1e3:7.2f} ms, score {med['score'] * 1e3:7.2f} "
              f"ms (enc_proj {med['enc_proj'] * 1e3:.2f}, predictor {med['predictor'] * 1e3:.2f}, "
              f"gather {med['gather'] * 1e3:.2f}, "
              f"lattice {med['lattice'] * 1e3:.2f}), attention "
              f"{med['attn'] * 1e3:7.2f} ms; rows {rows} of {unshared} unshared, "
              f"{row['gather_tflops']:.1f} TFLOP/s; rescoring {audio_s / t_e2e:.0f} audio-s/s, "
              f'beam_search {audio_s / t_bs:.0f}', flush=True)
    out = dict(config=args.config, encoder_blocks=configs['encoder_conf']['num_blocks'], batch=B,
               audio_seconds=audio_s, weights=picked, search_weights=list(RESCORE_SEARCH),
               rescore_weights=dict(ctc=cw, attn=aw, transducer=tw, reverse=rw), rescoring=table,
               method='host clock around calls that end in a device synchronise (search, score, '
                      'attention, the whole calls); enc_proj / predictor / gather / lattice: '
                      'device time between events inside a wn_transducer_score call of their '
                      'own under wn_profile_enable; beams alternate '
                      'in one process; median of --repeats')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
