#!/usr/bin/env python3
"""Record what the REAL reference's `get_frames_timestamp` / `get_labformat`
(wenet/bin/alignment.py:55-123) return, for tests/test_align_host.py.

    python tools/gen_golden_align.py        # CPU only; needs the reference tree

Inputs: the reference `ctc_logp` of the committed goldens tiny_sym_full / tiny_causal_full /
tiny_bn_full; label lists = every utterance's greedy tokens and n-best entries 1-5; the
alignment of each is the plain fp32 rule (tests/align_formulation.py ctc_align; lists that do
not fit into the frames are left out); threshold pairs (0.999999, 1e-6), (0.999, 1e-10) and
(0.6, 0.05).  The reference functions read `configs` / `char_dict` as script globals: they are
set on the imported module (conv2d subsampling = 4, symbol "t<id>").  Their prints are
swallowed.  Output: tests/golden/align/frames_labformat.json.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CASES = ('tiny_sym_full', 'tiny_causal_full', 'tiny_bn_full')
PAIRS = ((0.999999, 1e-6), (0.999, 1e-10), (0.6, 0.05))


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    import wenet.bin.alignment as ref
    import align_formulation as AF
    import golden_util as G
    ref.configs = {'encoder_conf': {'input_layer': 'conv2d'}}
    records = []
    for case in CASES:
        meta, arr = G.load_case(case)
        logp, lens = arr['ctc_logp'], arr['enc_lens']
        ref.char_dict = {i: f't{i}' for i in range(logp.shape[-1])}
        prefix = meta['prefix']
        for b in range(len(lens)):
            lists = [('greedy', meta['greedy'][b])]
            lists += [(f'nbest{i}', y) for i, y in enumerate(prefix[b]['nbest']) if 1 <= i <= 5]
            lp = logp[b, :lens[b]]
            for what, y in lists:
                y = [int(t) for t in y]
                got = AF.ctc_align(lp, y)
                if got is None or not y:
                    continue
                path = got[0].tolist()
                rec = dict(case=case, utt=b, what=what, labels=y, alignment=path, pairs=[])
                for bt, th in PAIRS:
                    with contextlib.redirect_stdout(io.StringIO()):
                        ts = ref.get_frames_timestamp(list(path), lp, bt, th)
                        lab = ref.get_labformat(ts, 4)
                    rec['pairs'].append(dict(blank_thres=bt, thres=th,
                                             timestamp=[[int(v) for v in g] for g in ts],
                                             labformat=lab))
                records.append(rec)
    out = os.path.join(ROOT, 'tests', 'golden', 'align', 'frames_labformat.json')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(dict(subsample=4, records=records), f, separators=(',', ':'))
    n_blank = sum(any(0 in g[:-1] or g[0] == 0 for g in p['timestamp'])
                  for r in records for p in r['pairs'])
    print(f'{len(records)} alignments x {len(PAIRS)} threshold pairs -> {out} '
          f'({os.path.getsize(out)} bytes); groups that keep blanks: {n_blank}')


if __name__ == '__main__':
    main()
