#!/usr/bin/env python3
"""Conv2dSubsampling6 front end on gigaspeech_conformer (d 512, rate 6) and on the same recipe at
d 256, B = 32 x 8-12 s, fp32.  Three modes, each a run of its own:

    python tools/bench_conv2d6.py --out FILE.json
        host brackets (a device synchronise inside each) of the front end -- conv2d6_patch + the
        projection + descriptor uploads, through wn_op_conv2d6 -- for every (d, frames per tile,
        column split), the variants ALTERNATED inside every round; then, with the shipped
        constants, the encoder and decode(['ctc_prefix_beam_search']); as a side record the
        Conv2dSubsampling4 front end of a d-256 handle on the same audio (another convolution,
        not a ratio).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
            python tools/bench_conv2d6.py --profile D,FT,WIDE
        `--reps` launches of one variant and nothing else, for the kernel's own time; samples the
        shader clock the driver reports while they run and prints it as one JSON line.
    python tools/bench_conv2d6.py --merge DIR --out FILE.json
        folds the conv2d6_patch rows of the *kernel_stats.csv files under DIR/<D>_<FT>_<WIDE>/ and
        the clock lines DIR/<D>_<FT>_<WIDE>.clock into FILE.json with the share of the six-product
        ceiling (256 CUs x 4096 bf16 FLOP per clock / 6) at the clock held.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [(512, 5, 1), (512, 8, 1), (512, 10, 1), (512, 5, 2), (512, 8, 2),
            (256, 5, 0), (256, 8, 0), (256, 10, 0)]
SPLIT = {0: 'four waves', 1: 'two column halves', 2: 'eight waves'}


def batch():
    lens = np.random.default_rng(5).integers(800, 1201, size=32).astype(np.int32)
    g = torch.Generator().manual_seed(7)
    return (torch.randn(32, int(lens.max()), 80, generator=g) * 3.0 + 11.0).cuda(), lens


def make(d, blocks):
    from wenet_amd import synthetic as S
    from wenet_amd.model import ASRModel
    configs = S.make_configs('gigaspeech_conformer')
    configs['encoder_conf'].update(num_blocks=blocks, output_size=d, attention_heads=d // 64)
    configs['decoder_conf']['attention_heads'] = d // 64
    return ASRModel(configs, S.make_state_dict(configs, 0), device='cuda')


def front_fn(model, dev, lens, d):
    from wenet_amd import _lib
    L = _lib.lib()
    M = int(sum(L.wn_conv2d6_frames(int(n)) for n in lens))
    c2 = torch.empty(M * 12 * d, device='cuda')

    def front():
        _lib.check(L.wn_op_conv2d6(model._h, dev.data_ptr(), _lib.i32p(lens), 32, dev.shape[1],
                                   c2.data_ptr(), None, None, None), 'wn_op_conv2d6')
    return front, M


def bracket(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), n=len(ts))


def set_variant(ft, wide):
    from wenet_amd import _lib
    L = _lib.lib()
    _lib.check(L.wn_tune_set(b'conv2d6_ft', ft), 'tune')
    _lib.check(L.wn_tune_set(b'conv2d6_wide', wide), 'tune')


def sclk_mhz():
    """The current shader clock of the busiest card as the driver's pp_dpm_sclk reports it."""
    best = None
    for p in glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk'):
        try:
            for line in open(p):
                m = re.search(r'(\d+)\s*Mhz\s*\*', line, re.I)
                if m:
                    best = max(best or 0, int(m.group(1)))
        except OSError:
            pass
    return best


def run_profile(spec, reps):
    d, ft, wide = map(int, spec.split(','))
    dev, lens = batch()
    front, _ = front_fn(make(d, 1), dev, lens, d)
    set_variant(ft, wide)
    front()
    samples, stop = [], threading.Event()

    def sample():
        while not stop.is_set():
            v = sclk_mhz()
            if v:
                samples.append(v)
            time.sleep(0.01)
    th = threading.Thread(target=sample)
    th.start()
    for _ in range(reps):
        front()
    stop.set()
    th.join()
    samples = samples[len(samples) // 2:]             # (the clock ramps up over the first launches)
    print(json.dumps(dict(clock_mhz_median=float(np.median(samples)) if samples else None,
                          clock_mhz_min=min(samples) if samples else None,
                          clock_samples=len(samples))), flush=True)


def run_host(a):
    from wenet_amd import _lib, synthetic as S
    from wenet_amd.model import ASRModel
    L = _lib.lib()
    dev, lens = batch()
    lt = torch.as_tensor(lens)
    res = dict(workload='gigaspeech_conformer B=32 x 8-12 s fp32', front_end_host=[])
    models = {512: make(512, a.blocks), 256: make(256, 1)}
    fronts = {d: front_fn(m, dev, lens, d) for d, m in models.items()}
    res['output_frames'] = fronts[512][1]
    ts = {v: [] for v in VARIANTS}
    for r in range(a.brackets + 1):                  # round 0 warms every variant up
        for v in VARIANTS:
            set_variant(v[1], v[2])
            t = bracket(fronts[v[0]][0])
            if r:
                ts[v].append(t)
    for v in VARIANTS:
        res['front_end_host'].append(dict(d=v[0], ft=v[1], split=SPLIT[v[2]], **stats(ts[v])))
        print(res['front_end_host'][-1], flush=True)
    set_variant(0, 0)
    m = models[512]
    for name, fn in (('front_end_shipped', fronts[512][0]),
                     ('encoder', lambda: m._forward_encoder(dev, lt)),
                     ('decode_ctc_prefix_beam_search',
                      lambda: m.decode(['ctc_prefix_beam_search'], dev, lt, beam_size=10))):
        fn()
        res[name] = stats([bracket(fn) for _ in range(a.brackets)])
    res['encoder_blocks'] = a.blocks
    c4 = S.make_configs('aishell_u2pp')
    c4['encoder_conf']['num_blocks'] = 1
    m4 = ASRModel(c4, S.make_state_dict(c4, 0), device='cuda')
    c24 = torch.empty(int(sum((int(n) - 7) // 4 + 1 for n in lens)) * 19 * 256, device='cuda')
    code = np.zeros(1, np.int32)

    def front4():
        _lib.check(L.wn_op_conv2d4(m4._h, dev.data_ptr(), _lib.i32p(lens), 32, dev.shape[1], None,
                                   c24.data_ptr(), None, None, _lib.i32p(code), None), 'conv2d4')
    front4()
    res['side_record_conv2d4_front_end_d256'] = stats([bracket(front4) for _ in range(a.brackets)])
    return res


def merge(res, root):
    rows = []
    for d, ft, wide in VARIANTS:
        stem = os.path.join(root, f'{d}_{ft}_{wide}')
        row = dict(d=d, ft=ft, split=SPLIT[wide])
        for path in glob.glob(os.path.join(stem, '**', '*kernel_stats.csv'), recursive=True):
            for r in csv.DictReader(open(path)):
                if 'conv2d6_patch_kernel' in r.get('Name', ''):
                    row['kernel_stats'] = {k: v for k, v in r.items() if k != 'Name'}
        if os.path.exists(stem + '.clock'):
            for line in open(stem + '.clock'):
                if line.startswith('{'):
                    row.update(json.loads(line))
        ks = row.get('kernel_stats', {})
        avg = float(ks['AverageNs']) if 'AverageNs' in ks else None
        if avg:
            flop = 2.0 * res['output_frames'] * 12 * 25 * d * d
            row['kernel_ms'] = avg / 1e6
            row['tflops'] = flop / avg / 1e3
            if row.get('clock_mhz_median'):
                ceiling = 256 * 4096 * row['clock_mhz_median'] * 1e6 / 6
                row['share_of_six_product_ceiling'] = flop / (avg * 1e-9) / ceiling
        rows.append(row)
        print(row, flush=True)
    res['conv2d6_patch_kernel_trace'] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--brackets', type=int, default=9)
    ap.add_argument('--blocks', type=int, default=12)
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--profile')
    ap.add_argument('--merge')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv2d6_gigaspeech.json'))
    a = ap.parse_args()
    if a.profile:
        return run_profile(a.profile, a.reps)
    if a.merge:
        res = json.load(open(a.out))
        merge(res, a.merge)
    else:
        res = run_host(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
