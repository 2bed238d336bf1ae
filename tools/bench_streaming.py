#!/usr/bin/env python3
"""Latency / throughput of BATCHED cache streaming (SURVEY.md section 8 row f2,
`ASRModel.forward_encoder_chunk_batch` = wn_encode_chunk_batch; the reference's batched
formulation: wenet/bin/export_onnx_gpu.py:83-232; published context for the reference's own
GPU streaming server: runtime/gpu/README.md:140-186).

N concurrent sessions of the WenetSpeech u2++ conformer (12L / 8 heads / 512d, causal,
chunk-trained: BASELINE.json configs[3]'s model), decoding_chunk_size 16 (= 0.64 s of audio per
step and session), num_decoding_left_chunks L (required_cache_size = 16 L; -1 = all history
up to --max-cache frames).  One STEP = every session advances by one chunk: the encoder chunk
forward for all N sessions in one call + the CTC head on the N x 16 new frames (log-softmax +
top-10, what a streaming prefix beam consumes).  Reported per N: median / p99 step latency in
steady state (caches full) and audio-seconds per second = N x 0.64 / step.

    python tools/bench_streaming.py [--sessions 16,32,64] [--left 4] [--steps 200]

--search: the step also runs the resumable prefix beam search of the streaming recognizer
(wenet_amd.streaming.StreamSearch.advance_encoded: CTC head + search in one call, 1-best
partials) and the line reports the step latency with it (`search_step_ms_*`) next to the one
without it, measured in the same process in alternating blocks.  `--utt-seconds 5,20,60`: the
sessions have that much audio behind them when the measurement starts (the search state is
brought there first).  `--requadratic`: also time what a caller had to do before the
resumable search existed to get a partial after every chunk -- search.ctc_prefix_beam_search
over ALL log-probs received so far (`rerun_step_ms_*`).

--rnnt: the same question for the hybrid transducer's streaming sessions.  Model
`aishell_u2pp_rnnt` (conformer_u2pp_rnnt.yaml at full width), N sessions with 5 s of audio
behind them (put back there before every block of the resumable search), chunk 16, the window `rnnt_lookahead` 1 / 4 / 16 set on the handle.  Per N and
window the step latency of (a) the encoder chunk alone, (b) the chunk + the resumable RNN-T
greedy search (wenet_amd.streaming.RnntStreamSearch.advance_encoded) and (c) the chunk + the
one-shot wn_transducer_greedy_search over the 5 s of history and the new chunk -- what a caller
had to run for a partial before the sessions existed; blocks of 10 steps of each kind in turn.
Host clock around work that ends in a device synchronise.  Writes
profiles/streaming_rnnt_sessions.json (or --out).

--rnnt-beam: the same for the resumable RNN-T prefix beam search
(wenet_amd.streaming.RnntBeamStreamSearch.advance_encoded, fusion weights 0.3 / 0.7) at the beams
of --beams (5,10): (a) the encoder chunk alone, (b) the chunk + the session step, (c) the chunk +
the one-shot transducer.prefix_beam_search over the 5 s of history and the new chunk, on the same
process and encoder output; plus the kernel launches of one session step, counted from the
model's shape.  Writes profiles/streaming_rnnt_beam_sessions.json (or --out).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', default='1,16,32,64')
    ap.add_argument('--left', type=int, default=4, help='num_decoding_left_chunks (-1: all)')
    ap.add_argument('--chunk', type=int, default=16)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--max-cache', type=int, default=512)
    ap.add_argument('--config', default='wenetspeech_u2pp')
    ap.add_argument('--out', default='')
    ap.add_argument('--search', action='store_true',
                    help='also measure the step with the resumable prefix beam search')
    ap.add_argument('--utt-seconds', default='5',
                    help='--search: audio seconds every session has consumed before timing')
    ap.add_argument('--requadratic', action='store_true',
                    help='--search: also time the one-shot search over everything so far')
    ap.add_argument('--nbest', action='store_true', help='--search: n-best partials')
    ap.add_argument('--rnnt', action='store_true',
                    help='streaming transducer sessions: resumable vs one-shot RNN-T greedy search')
    ap.add_argument('--lookahead', default='1,4,16', help='--rnnt: rnnt_lookahead values')
    ap.add_argument('--rnnt-beam', action='store_true',
                    help='streaming transducer sessions: resumable vs one-shot RNN-T prefix beam '
                         'search')
    ap.add_argument('--beams', default='5,10', help='--rnnt-beam: beam sizes')
    args = ap.parse_args()
    if args.rnnt_beam:
        return rnnt_beam_main(args)
    if args.rnnt:
        return rnnt_main(args)
    from wenet_amd import synthetic as S
    from wenet_amd.model import ASRModel
    dev = torch.device('cuda', 0)
    configs = S.make_configs(args.config)
    model = ASRModel(configs, S.make_state_dict(configs, 0), device=dev)
    chunk = args.chunk
    window = (chunk - 1) * 4 + 7          # feature frames per step (encoder.py:337-352)
    req = chunk * args.left if args.left >= 0 else -1
    rows = []
    for n in [int(x) for x in args.sessions.split(',')]:
        feats, _ = S.make_features(n, window, seed=5, feat_dim=configs['input_dim'])
        xs = feats.to(dev)
        att = [None] * n
        cnn = [None] * n
        offsets = [0] * n
        lat = []
        for it in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ys, att, cnn = model.forward_encoder_chunk_batch(xs, offsets, req, att, cnn)
            logp = model.ctc_logprobs(ys)                  # (n, chunk, V) log-softmax
            top = logp.topk(10, dim=-1)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            offsets = [o + chunk for o in offsets]
            if args.left < 0 and att[0].size(2) > args.max_cache:
                att = [a[:, :, -args.max_cache:].contiguous() for a in att]
            if it >= args.warmup:
                lat.append(dt)
        lat = np.asarray(lat) * 1e3
        audio = n * chunk * 0.04
        row = dict(sessions=n, chunk=chunk, left_chunks=args.left,
                   cache_frames=int(att[0].size(2)),
                   step_ms_median=round(float(np.median(lat)), 3),
                   step_ms_p99=round(float(np.percentile(lat, 99)), 3),
                   audio_s_per_s=round(audio / (float(np.median(lat)) * 1e-3), 1),
                   audio_s_per_step=round(audio, 2))
        if args.search:
            row['search'] = [search_rows(args, model, dev, n, xs, att, cnn, offsets, req, secs)
                             for secs in [float(x) for x in args.utt_seconds.split(',')]]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del top
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(model=args.config, note='encoder chunk forward for all sessions + '
                           'CTC head (log-softmax, top-10) per step, host-synchronous; one '
                           'MI355X', rows=rows), f, indent=1)


def search_rows(args, model, dev, n, xs, att, cnn, offsets, req, secs):
    """Step latency without / with the resumable search (/ with the one-shot search over all
    frames so far) for sessions that have `secs` of audio behind them: blocks of 10 steps of
    each kind in turn, so that all three see the same clocks and cache state."""
    from wenet_amd import search as SR
    from wenet_amd.streaming import StreamSearch
    chunk = args.chunk
    hist = int(round(secs / 0.04))                 # encoder frames already consumed
    total = hist + chunk * (args.warmup + args.steps + 8)
    ss = StreamSearch(model._h, dev, n, 10, total)
    slots = list(range(n))
    ys, att, cnn = model.forward_encoder_chunk_batch(xs, offsets, req, att, cnn)
    logp1 = model.ctc_logprobs(ys)                 # one chunk of realistic posteriors ...
    fill = logp1.repeat(1, (hist + chunk - 1) // chunk, 1)[:, :hist].contiguous()
    for t in range(0, hist, 256):                  # ... repeated: the sessions' history
        k = min(256, hist - t)
        ss.advance(slots, fill[:, t:t + k].contiguous(), [k] * n)
    sofar = fill

    def step(kind):
        nonlocal att, cnn, sofar
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys, att, cnn = model.forward_encoder_chunk_batch(xs, offsets, req, att, cnn)
        if kind == 'none':
            logp = model.ctc_logprobs(ys)
            top = logp.topk(10, dim=-1)
            del top
        elif kind == 'search':
            ss.advance_encoded(slots, ys, nbest=args.nbest)
        else:
            logp = model.ctc_logprobs(ys)
            sofar = torch.cat([sofar, logp], 1)
            SR.ctc_prefix_beam_search(sofar, torch.full((n, ), sofar.size(1)), 10)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.left < 0 and att[0].size(2) > args.max_cache:
            att = [a[:, :, -args.max_cache:].contiguous() for a in att]
        return dt

    kinds = ['none', 'search'] + (['rerun'] if args.requadratic else [])
    lat = {k: [] for k in kinds}
    for k in kinds:
        for _ in range(max(args.warmup // 2, 3)):
            step(k)
    blocks = max(args.steps // 10, 1)
    for _ in range(blocks):
        for k in kinds:
            for _ in range(10):
                if k == 'search' and ss.frames[0] + chunk > total:
                    break
                lat[k].append(step(k))
    ss.close()
    out = dict(utt_seconds=secs, history_frames=hist, nbest=bool(args.nbest))
    names = dict(none='step_ms', search='search_step_ms', rerun='rerun_step_ms')
    for k in kinds:
        a = np.asarray(lat[k]) * 1e3
        out[names[k] + '_median'] = round(float(np.median(a)), 3)
        out[names[k] + '_p99'] = round(float(np.percentile(a, 99)), 3)
    out['search_minus_step_ms'] = round(out['search_step_ms_median'] - out['step_ms_median'], 3)
    return out


def rnnt_main(args):
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import RnntStreamSearch
    from wenet_amd.transducer import basic_greedy_search
    dev = torch.device('cuda', 0)
    config = 'aishell_u2pp_rnnt' if args.config == 'wenetspeech_u2pp' else args.config
    configs = S.make_configs(config)
    model = Transducer(configs, S.make_state_dict(configs, 0), device=dev)
    tc = model._tcfg
    chunk = args.chunk
    window = (chunk - 1) * 4 + 7
    req = chunk * args.left if args.left >= 0 else -1
    secs = float(args.utt_seconds.split(',')[0])
    hist = int(round(secs / 0.04))
    n_hist = (hist + chunk - 1) // chunk
    n_steps = 64
    rows = []
    for n in [int(x) for x in args.sessions.split(',')]:
        feats, _ = S.make_features(n, window, seed=5, feat_dim=configs['input_dim'])
        xs = feats.to(dev)
        for F in [int(x) for x in args.lookahead.split(',')]:
            assert model.tune('rnnt_lookahead', F) == F
            att, cnn, offsets = [None] * n, [None] * n, [0] * n
            total = chunk * (n_hist + max(args.warmup // 2, 3) + 12)
            rs = RnntStreamSearch(model._h, dev, n, total, total * n_steps, n_steps,
                                  dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))
            slots = list(range(n))
            past = []
            for _ in range(n_hist):            # the sessions' history: 5 s of encoder output
                ys, att, cnn = model.forward_encoder_chunk_batch(xs, offsets, req, att, cnn)
                offsets = [o + chunk for o in offsets]
                rs.advance_encoded(slots, ys)
                past.append(ys)
            past_chunks = past
            past = torch.cat(past, 1)[:, -hist:].contiguous()
            state = dict(att=att, cnn=cnn, offsets=offsets, steps=[], rerun_steps=[])

            def step(kind):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ys, state['att'], state['cnn'] = model.forward_encoder_chunk_batch(
                    xs, state['offsets'], req, state['att'], state['cnn'])
                if kind == 'search':
                    state['steps'].append(rs.advance_encoded(slots, ys).steps)
                elif kind == 'rerun':
                    sofar = torch.cat([past, ys], 1)
                    basic_greedy_search(model, sofar, [sofar.size(1)] * n, n_steps)
                    state['rerun_steps'].append(model.last_rnnt_steps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0      # (the offset stays at 5 s, as in --search)
                if args.left < 0 and state['att'][0].size(2) > args.max_cache:
                    state['att'] = [a[:, :, -args.max_cache:].contiguous() for a in state['att']]
                return dt

            kinds = ['none', 'search', 'rerun']
            lat = {k: [] for k in kinds}
            for k in kinds:
                for _ in range(max(args.warmup // 2, 3)):
                    step(k)
            state['steps'], state['rerun_steps'] = [], []
            for _ in range(max(args.steps // 10, 1)):
                for k in kinds:
                    if k == 'search':      # back to 5 s of audio behind every session (untimed)
                        rs.reset(slots)
                        for ys in past_chunks:
                            rs.advance_encoded(slots, ys)
                    for _ in range(10):
                        lat[k].append(step(k))
            row = dict(sessions=n, chunk=chunk, left_chunks=args.left, rnnt_lookahead=F,
                       history_frames=hist, n_steps=n_steps,
                       tokens_per_session=round(float(np.mean(rs.n_tok)), 1),
                       frames_per_session=int(rs.frames[0]),
                       lockstep_steps_per_call=round(float(np.mean(state['steps'])), 1),
                       rerun_lockstep_steps=round(float(np.mean(state['rerun_steps'])), 1))
            names = dict(none='step_ms', search='stream_step_ms', rerun='rerun_step_ms')
            for k in kinds:
                a = np.asarray(lat[k]) * 1e3
                row[names[k] + '_median'] = round(float(np.median(a)), 3)
                row[names[k] + '_p99'] = round(float(np.percentile(a, 99)), 3)
            row['stream_minus_step_ms'] = round(row['stream_step_ms_median'] - row['step_ms_median'], 3)
            row['rerun_minus_step_ms'] = round(row['rerun_step_ms_median'] - row['step_ms_median'], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            rs.close()
            model.tune('rnnt_lookahead', 'inherit')
    out = args.out or os.path.join(ROOT, 'profiles', 'streaming_rnnt_sessions.json')
    with open(out, 'w') as f:
        json.dump(dict(
            model=config, steps=args.steps, warmup=args.warmup,
            note='step latency, host clock around a device synchronise, one MI355X; blocks of 10 '
                 'steps of each kind in turn',
            step_ms='(a) encoder chunk forward for all sessions',
            stream_step_ms='(b) encoder chunk + wn_rnnt_stream_advance_encoded (joint.enc_ffn over '
                           'the chunk + resumable greedy search, tokens and times to the host)',
            rerun_step_ms='(c) encoder chunk + wn_transducer_greedy_search over the history and '
                          'the new chunk (history_frames + chunk frames per session)',
            rows=rows), f, indent=1)


def rnnt_beam_main(args):
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import RnntBeamStreamSearch
    from wenet_amd.transducer import prefix_beam_search
    dev = torch.device('cuda', 0)
    config = 'aishell_u2pp_rnnt' if args.config == 'wenetspeech_u2pp' else args.config
    configs = S.make_configs(config)
    model = Transducer(configs, S.make_state_dict(configs, 0), device=dev)
    tc = model._tcfg
    chunk = args.chunk
    window = (chunk - 1) * 4 + 7
    req = chunk * args.left if args.left >= 0 else -1
    secs = float(args.utt_seconds.split(',')[0])
    hist = int(round(secs / 0.04))
    n_hist = (hist + chunk - 1) // chunk
    cw, tw = 0.3, 0.7
    # one session step: joint.enc_ffn, the CTC head, its log-softmax, begin, end, and per frame
    # two launches per LSTM layer, the projection, joint.pred_ffn, the joint rows, the fusion +
    # top-k, the beam step and the gather
    per_frame = 2 * tc.pred_layers + 6
    launches = 5 + chunk * per_frame
    rows = []
    for n in [int(x) for x in args.sessions.split(',')]:
        feats, _ = S.make_features(n, window, seed=5, feat_dim=configs['input_dim'])
        xs = feats.to(dev)
        for beam in [int(x) for x in args.beams.split(',')]:
            att, cnn, offsets = [None] * n, [None] * n, [0] * n
            total = chunk * (n_hist + max(args.warmup // 2, 3) + 12)
            rs = RnntBeamStreamSearch(model._h, dev, n, beam, total, cw, tw,
                                      dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))
            slots = list(range(n))
            past = []
            for _ in range(n_hist):            # the sessions' history: 5 s of encoder output
                ys, att, cnn = model.forward_encoder_chunk_batch(xs, offsets, req, att, cnn)
                offsets = [o + chunk for o in offsets]
                rs.advance_encoded(slots, ys)
                past.append(ys)
            past_chunks = past
            past = torch.cat(past, 1)[:, -hist:].contiguous()
            state = dict(att=att, cnn=cnn, offsets=offsets, tokens=[])

            def step(kind):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ys, state['att'], state['cnn'] = model.forward_encoder_chunk_batch(
                    xs, state['offsets'], req, state['att'], state['cnn'])
                if kind == 'search':
                    res = rs.advance_encoded(slots, ys)
                    state['tokens'].append(float(np.mean([len(r.tokens) for r in res])))
                elif kind == 'rerun':
                    sofar = torch.cat([past, ys], 1)
                    prefix_beam_search(model, sofar, [sofar.size(1)] * n, beam, cw, tw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0      # (the offset stays at 5 s, as in --search)
                if args.left < 0 and state['att'][0].size(2) > args.max_cache:
                    state['att'] = [a[:, :, -args.max_cache:].contiguous() for a in state['att']]
                return dt

            kinds = ['none', 'search', 'rerun']
            lat = {k: [] for k in kinds}
            for k in kinds:
                for _ in range(max(args.warmup // 2, 3)):
                    step(k)
            state['tokens'] = []
            for _ in range(max(args.steps // 10, 1)):
                for k in kinds:
                    if k == 'search':      # back to 5 s of audio behind every session (untimed)
                        rs.reset(slots)
                        for ys in past_chunks:
                            rs.advance_encoded(slots, ys)
                    for _ in range(10):
                        lat[k].append(step(k))
            row = dict(sessions=n, chunk=chunk, left_chunks=args.left, beam=beam,
                       ctc_weight=cw, transducer_weight=tw, history_frames=hist,
                       best_tokens_per_session=round(float(np.mean(state['tokens'])), 1),
                       frames_per_session=int(rs.frames[0]),
                       lockstep_steps_per_call=chunk, launches_per_step=launches,
                       launches_per_frame=per_frame, rerun_lockstep_steps=hist + chunk)
            names = dict(none='step_ms', search='stream_step_ms', rerun='rerun_step_ms')
            for k in kinds:
                a = np.asarray(lat[k]) * 1e3
                row[names[k] + '_median'] = round(float(np.median(a)), 3)
                row[names[k] + '_p99'] = round(float(np.percentile(a, 99)), 3)
            row['stream_minus_step_ms'] = round(row['stream_step_ms_median'] - row['step_ms_median'], 3)
            row['rerun_minus_step_ms'] = round(row['rerun_step_ms_median'] - row['step_ms_median'], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            rs.close()
    out = args.out or os.path.join(ROOT, 'profiles', 'streaming_rnnt_beam_sessions.json')
    with open(out, 'w') as f:
        json.dump(dict(
            model=config, steps=args.steps, warmup=args.warmup,
            note='step latency, host clock around a device synchronise, one MI355X; blocks of 10 '
                 'steps of each kind in turn',
            step_ms='(a) encoder chunk forward for all sessions',
            stream_step_ms='(b) encoder chunk + wn_rnnt_beam_stream_advance_encoded (joint.enc_ffn '
                           'and the CTC head over the chunk + resumable prefix beam search, the '
                           'n-best to the host)',
            rerun_step_ms='(c) encoder chunk + wn_transducer_beam_search over the history and '
                          'the new chunk (history_frames + chunk frames per session)',
            launches_per_step='kernel launches of one session step, counted from the model shape: '
                              '5 + chunk x (2 x LSTM layers + 6)',
            rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
