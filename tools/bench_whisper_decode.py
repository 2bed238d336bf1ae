#!/usr/bin/env python3
"""Time the Whisper `attention` decode (wn_attention_beam_search_prompt) on the GPU and write
profiles/whisper_decode.json.

    python tools/bench_whisper_decode.py                 # whisper_largev3_dec, 16 x 30 s, beam 10
    python tools/bench_whisper_decode.py --layers 4 --repeats 3                   # a quick look

Workload: synthetic weights (they rarely emit <eot>, so every decode runs to the positional cap
and the step count is fixed), B utterances of 30 s, T' = 1500.  Per precision (fp32, bf16) the
encoder + CTC head is timed once, the first decode (it also projects the cross-attention K / V of
the batch, once) is reported on its own, and then decodes with the step GEMMs on linear()
(dec_skinny = 0: the kernels the classic search runs) and on the skinny kernel (dec_skinny = 1)
ALTERNATE in the same process; each decode is a host clock around a call that ends in a device
synchronise.  Reported: median / min / max per setting, ms per step, and the weight bytes a step
streams -- computed from the shapes here -- over the step time, beside the 6.3 TB/s the HBM
delivers to a streaming read.  A per-kernel split needs a separate profiler run
(`--decodes-only N` keeps such a run short); nothing here reads counters.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STREAM_BYTES_PER_S = 6.3e12


def step_weight_elems(d, ffn, layers, vocab):
    """Weight elements one decoder step reads: six GEMMs per layer + the output layer."""
    per_layer = 3 * d * d + d * d + d * d + d * d + 2 * d * ffn
    return layers * per_layer, vocab * d


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--config', default='whisper_largev3_dec')
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--seconds', type=float, default=30.0)
    p.add_argument('--beam', type=int, default=10)
    p.add_argument('--layers', type=int, default=None, help='decoder AND encoder blocks')
    p.add_argument('--vocab', type=int, default=None)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--dtypes', nargs='+', default=['fp32', 'bf16'])
    p.add_argument('--decodes-only', type=int, default=0,
                   help='profiler runs: N decodes per setting, no JSON')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'whisper_decode.json'))
    args = p.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_whisper_decode: needs the GPU (no CPU fallback)')
    from wenet_amd import synthetic as S
    from wenet_amd.model import ASRModel
    from wenet_amd.search import attention_beam_search

    t0 = time.perf_counter()
    configs = S.make_configs(args.config)
    if args.layers is not None:
        configs['encoder_conf']['num_blocks'] = args.layers
        configs['decoder_conf']['num_blocks'] = args.layers
    if args.vocab is not None:
        if args.vocab <= max(configs['tokenizer_conf']['special_tokens'].values()):
            raise SystemExit('--vocab must keep the special tokens inside the vocabulary')
        configs['output_dim'] = args.vocab
    sd = S.make_state_dict(configs, 0)
    model = ASRModel(configs, sd, device='cuda')
    del sd
    setup_s = time.perf_counter() - t0
    ec, dc = configs['encoder_conf'], configs['decoder_conf']
    d, V = ec['output_size'], configs['output_dim']
    frames = int(args.seconds * 100)
    feats, lens = S.make_features(args.batch, (frames, frames), seed=5,
                                  feat_dim=configs['input_dim'])
    feats = feats.cuda()
    layer_elems, out_elems = step_weight_elems(d, dc['linear_units'], dc['num_blocks'], V)
    report = dict(config=args.config, batch=args.batch, seconds=args.seconds, beam=args.beam,
                  enc_blocks=ec['num_blocks'], dec_blocks=dc['num_blocks'], d_model=d, vocab=V,
                  rows_per_step=args.batch * args.beam, setup_s=round(setup_s, 1),
                  device=torch.cuda.get_device_name(0), dtypes={})

    def sync():
        torch.cuda.synchronize()

    for dtype in args.dtypes:
        model.set_compute_dtype(dtype)
        wbytes = (layer_elems + out_elems) * (4 if dtype == 'fp32' else 2)
        sync()
        t = time.perf_counter()
        st = model._decode_begin(['attention'], feats, lens, args.beam)
        sync()
        enc_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()                      # second encode: warm
        st = model._decode_begin(['attention'], feats, lens, args.beam)
        sync()
        enc_ms = min(enc_ms, (time.perf_counter() - t) * 1e3)
        B, Tp = st['B'], st['Tp']

        def decode(skinny):
            model.tune('dec_skinny', skinny)
            sync()
            t = time.perf_counter()
            res = attention_beam_search(model, B, Tp, args.beam, 0.0, None)
            sync()
            return (time.perf_counter() - t) * 1e3, res

        first_ms, res = decode(1)                    # + the cross-attention K / V of the batch
        dmax = model._cfg.dec_max_pos
        steps = min(Tp, dmax) - 4 + 1
        full = bool(model.last_attention_truncated) or min(len(r.tokens) for r in res) >= steps
        decode(0)                                    # warm-up of the other setting
        n = args.decodes_only or args.repeats
        times = {0: [], 1: []}
        for _ in range(n):
            for skinny in (0, 1):
                times[skinny].append(decode(skinny)[0])
        if args.decodes_only:
            continue
        entry = dict(encoder_ctc_ms=round(enc_ms, 2), first_decode_ms=round(first_ms, 2),
                     T_prime=Tp, steps=steps, ran_to_the_cap=full,
                     weight_bytes_per_step=wbytes, settings={})
        for skinny in (0, 1):
            ts = times[skinny]
            med = statistics.median(ts)
            entry['settings'][f'dec_skinny={skinny}'] = dict(
                decode_ms_median=round(med, 2), decode_ms_min=round(min(ts), 2),
                decode_ms_max=round(max(ts), 2), n=len(ts),
                ms_per_step=round(med / steps, 4),
                weight_bytes_per_s=round(wbytes / (med / steps * 1e-3), 0),
                share_of_hbm_stream=round(wbytes / (med / steps * 1e-3) / HBM_STREAM_BYTES_PER_S,
                                          4))
        a, b = (entry['settings'][f'dec_skinny={k}'] for k in (0, 1))
        spread = max(a['decode_ms_max'] - a['decode_ms_min'], b['decode_ms_max'] - b['decode_ms_min'])
        entry['skinny_gain_ms'] = round(a['decode_ms_median'] - b['decode_ms_median'], 2)
        entry['run_to_run_spread_ms'] = round(spread, 2)
        entry['skinny_wins'] = entry['skinny_gain_ms'] > spread
        report['dtypes'][dtype] = entry
        print(dtype, json.dumps(entry), flush=True)
    model.tune('dec_skinny', 'inherit')
    if not args.decodes_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(report, f, indent=1)
            f.write('\n')
        print('wrote', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
