#!/usr/bin/env python3
"""Record the final beams of the REAL reference's transducer prefix beam search --
PrefixBeamSearch.prefix_beam_search, wenet/models/transducer/search/prefix_beam_search.py:42-148,
what Transducer.beam_search (transducer.py:216-260) runs -- for
tests/test_transducer_beam_formulation.py and tests/test_gpu_transducer_beam.py.

    python tools/gen_golden_transducer_beam.py        # CPU only; needs the reference tree

Model: wenet_amd.synthetic `tiny_rnnt`; inputs make_features(3, (60, 150), seed=77): T' = 29, 16,
15.  The reference's own PrefixBeamSearch object decodes one utterance at a time from the
RECORDED encoder output (its `encoder` is a function that returns the recorded rows, so that
every side starts from the same numbers), in fp32 and as model.double() under a float64 default
dtype, for (ctc_weight, transducer_weight) in WEIGHTS and every beam in BEAMS.

The reference's prefix fusion calls log_add([a, b]) although log_add takes its values one by one
(wenet/utils/common.py:302), so the first fusion raises a TypeError.  Every run is tried
unmodified first; where it raises it is repeated with that one call mended IN THIS PROCESS
(`search.log_add = lambda xs: common.log_add(*xs)`), and the fixture says per run which of the
two it holds (`unmodified`).  Nothing in the reference tree changes.

While a run decodes, this process looks on: a subclass of the reference's Sequence notes every
candidate that is created (and, at the end, the score the fusion left it with) and a wrapper of
Tensor.topk notes the fused rows.  From them, per frame: the top beam + 1 values of every live
row, the fusion list and the number of fusions.

Recorded in tests/golden/rnnt/rnnt_beam_tiny.npz: the encoder output and its lengths, the fp32
CTC log-probs, and in `meta` the final beams (token lists and scores, in order) of every run in
fp32 and fp64.

A weight seed (0..199) is REJECTED unless for every recorded run
  1. the fp32 and the fp64 reference give the same token lists in the same order;
  2. the fp64 restatement (tests/transducer_beam_formulation.py) gives the fp64 reference's
     lists, scores within 1e-9;
  3. some run has a fusion in at least five frames; some utterance's best hypothesis differs
     between beam 1 and beam 5; some final beam contains the empty hypothesis;
  4. with e_row = the largest |f32 - f64| over the top beam + 1 fused values of every live row
     and e_score = the largest |score32 - score64| over the fusion lists of all frames (both
     runs must hold the same candidates in the same places):
       every top-k membership gap (value beam against value beam + 1 of a row) >= 8 e_row + 2e-6,
       every cut gap (entry beam against entry beam + 1 of the sorted fusion list) and every gap
       between neighbours of a final beam >= 8 e_score + 2e-6
     (twice the GPU tolerance of 4 e + 1e-6, once for each side of a comparison), gaps measured
     on the fp64 side.
e_row, e_score and the smallest gap of each kind go into the meta.  The largest beam is 10; if no
seed passes with it, 8 and then 6 are tried in its place and the meta says so.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONFIG = 'tiny_rnnt'
BATCH, FRAMES, FSEED = 3, (60, 150), 77
WEIGHTS = ((0.3, 0.7), (0.0, 1.0), (1.0, 0.0))
BEAMS = (1, 3, 5)
LARGE = (10, 8, 6)


class Onlooker:
    """Notes, while the reference decodes, the fused rows and the candidates of every frame."""

    def __init__(self, search):
        self.search = search
        self.frames = []          # dict(rows=tensor (N, V), seqs=[Sequence, ...])

    def __enter__(self):
        me = self
        self._seq, self._topk = self.search.Sequence, torch.Tensor.topk

        class Noted(self._seq):
            def __init__(s, hyp, score, cache):
                super().__init__(hyp, score, cache)
                if me.frames:
                    me.frames[-1]['seqs'].append(s)

        def topk(t, *a, **k):
            me.frames.append(dict(rows=t.detach().clone(), seqs=[]))
            return me._topk(t, *a, **k)

        self.search.Sequence = Noted
        torch.Tensor.topk = topk
        return self

    def __exit__(self, *exc):
        self.search.Sequence = self._seq
        torch.Tensor.topk = self._topk

    def digest(self, beam):
        """Per frame: (top beam + 1 values of every row, descending; the fusion list as
        [(hyp, score)] in list order; the number of fusions)."""
        out = []
        for f in self.frames:
            rows = torch.sort(f['rows'].double(), dim=-1, descending=True)[0][:, :beam + 1].numpy()
            fusion, seen, n_fused = [], set(), 0
            for s in f['seqs']:
                key = tuple(int(v) for v in s.hyp)
                if key in seen:
                    n_fused += 1
                    continue
                seen.add(key)
                fusion.append((key, float(s.score)))
            out.append((rows, fusion, n_fused))
        return out


def run_reference(model, enc_b, beam, cw, tw):
    """One utterance through the reference's own PrefixBeamSearch on the recorded encoder rows.
    Returns (final beam [(tokens, score)], per-frame digest, ran unmodified)."""
    import wenet.models.transducer.search.prefix_beam_search as search
    from wenet.utils import common
    bs = search.PrefixBeamSearch(lambda *a: (enc_b, None), model.predictor, model.joint, model.ctc,
                                 model.blank)
    speech = torch.zeros(1, 1, 1)
    args = (speech, torch.tensor([1]), -1, beam, -1, False, cw, tw)
    saved = search.log_add
    for unmodified in (True, False):
        if not unmodified:
            search.log_add = lambda xs: common.log_add(*xs)      # the one mended call
        try:
            with Onlooker(search) as look, torch.no_grad():
                final, _ = bs.prefix_beam_search(*args)
        except TypeError:
            if not unmodified:
                raise
            continue
        finally:
            search.log_add = saved
        return ([([int(v) for v in s.hyp[1:]], float(s.score)) for s in final],
                look.digest(beam), unmodified)


def try_seed(wseed, beams):
    import transducer_beam_formulation as BF
    import transducer_formulation as TF
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(CONFIG)
    blank = configs['tokenizer_conf']['special_tokens']['<blank>']
    feats, lens = S.make_features(BATCH, FRAMES, seed=FSEED)
    sd = S.make_state_dict(configs, wseed)
    model = build_reference_model(configs, sd)
    with torch.no_grad():
        enc, mask = model._forward_encoder(feats, lens, -1, -1)
        enc_lens = [int(v) for v in mask.squeeze(1).sum(1)]
        ctc32 = model.ctc.log_softmax(enc)
    torch.set_default_dtype(torch.float64)        # init_state allocates with the default dtype
    try:
        model64 = build_reference_model(configs, sd).double()
        with torch.no_grad():
            ctc64 = model64.ctc.log_softmax(enc.double()).numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    W = TF.weights64({k: v.numpy() for k, v in sd.items() if k.startswith(('predictor.', 'joint.'))},
                     configs['predictor_conf']['num_layers'])

    runs = {}
    e_row = e_score = 0.0
    gaps = dict(member=[], cut=[], final=[])
    fusion_frames = 0
    for cw, tw in WEIGHTS:
        for beam in beams:
            b32, b64, unmod = [], [], True
            for b in range(BATCH):
                n = enc_lens[b]
                f32, d32, u32 = run_reference(model, enc[b:b + 1, :n], beam, cw, tw)
                torch.set_default_dtype(torch.float64)
                try:
                    f64, d64, _ = run_reference(model64, enc[b:b + 1, :n].double(), beam, cw, tw)
                finally:
                    torch.set_default_dtype(torch.float32)
                if [t for t, _ in f32] != [t for t, _ in f64]:
                    return f'({cw}, {tw}) beam {beam}: fp32 and fp64 final beams differ', None
                unmod = unmod and u32
                b32.append(f32)
                b64.append(f64)
                fusion_frames = max(fusion_frames, sum(1 for _, _, nf in d64 if nf > 0))
                for (r32, l32, _), (r64, l64, _) in zip(d32, d64):
                    if [h for h, _ in l32] != [h for h, _ in l64]:
                        return f'({cw}, {tw}) beam {beam}: candidate sets differ', None
                    e_row = max(e_row, float(np.abs(r32 - r64).max()))
                    e_score = max(e_score, max(abs(a - c) for (_, a), (_, c) in zip(l32, l64)))
                    if r64.shape[1] > beam:
                        gaps['member'].append(float((r64[:, beam - 1] - r64[:, beam]).min()))
                    srt = sorted((s for _, s in l64), reverse=True)
                    if len(srt) > beam:
                        gaps['cut'].append(srt[beam - 1] - srt[beam])
                sc = [s for _, s in f64]
                gaps['final'] += [a - c for a, c in zip(sc, sc[1:])]
            # the fp64 restatement, the whole batch at once
            mine = BF.prefix_beam_search(enc.numpy(), enc_lens, ctc64, W, blank, beam, cw, tw,
                                         score_dtype=np.float64)
            for b in range(BATCH):
                if [t for t, _ in mine[b]] != [t for t, _ in b64[b]]:
                    return f'({cw}, {tw}) beam {beam}: the restatement differs from fp64', None
                if max(abs(a - c) for (_, a), (_, c) in zip(mine[b], b64[b])) > 1e-9:
                    return f'({cw}, {tw}) beam {beam}: restatement scores off by > 1e-9', None
            runs[f'{cw}_{tw}_{beam}'] = dict(ctc_weight=cw, transducer_weight=tw, beam=beam,
                                            unmodified=unmod, fp32=b32, fp64=b64)
    if fusion_frames < 5:
        return 'no run with a fusion in five frames', None
    if 5 in beams and not any(
            runs[f'{cw}_{tw}_1']['fp64'][b][0][0] != runs[f'{cw}_{tw}_5']['fp64'][b][0][0]
            for cw, tw in WEIGHTS for b in range(BATCH)):
        return 'beam 1 and beam 5 agree on every best hypothesis', None
    if not any(t == [] for r in runs.values() for u in r['fp64'] for t, _ in u):
        return 'no final beam holds the empty hypothesis', None
    need_row, need_score = 8 * e_row + 2e-6, 8 * e_score + 2e-6
    mins = {k: (min(v) if v else float('inf')) for k, v in gaps.items()}
    if mins['member'] < need_row:
        return f"membership gap {mins['member']:.2e} < {need_row:.2e}", None
    if mins['cut'] < need_score:
        return f"cut gap {mins['cut']:.2e} < {need_score:.2e}", None
    if mins['final'] < need_score:
        return f"final-beam gap {mins['final']:.2e} < {need_score:.2e}", None
    meta = dict(config=CONFIG, wseed=wseed, batch=BATCH, frames=list(FRAMES), fseed=FSEED,
                blank=blank, enc_lens=enc_lens, weights=[list(w) for w in WEIGHTS],
                beams=list(beams), runs=runs, e_row=e_row, e_score=e_score,
                min_member_gap=mins['member'], min_cut_gap=mins['cut'],
                min_final_gap=mins['final'], most_fusion_frames=fusion_frames,
                mend='search.log_add = lambda xs: common.log_add(*xs)')
    arrays = dict(enc=enc.numpy().astype(np.float32), ctc_logp=ctc32.numpy().astype(np.float32))
    return None, (meta, arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    passed_small = []
    for large in LARGE:
        seeds = range(200) if large == LARGE[0] else passed_small
        for wseed in seeds:
            if large == LARGE[0]:
                why, got = try_seed(wseed, BEAMS)
                if got is None:
                    print(f'seed {wseed}: rejected: {why}', flush=True)
                    continue
                passed_small.append(wseed)
            why, got = try_seed(wseed, BEAMS + (large, ))
            if got is None:
                print(f'seed {wseed}: beams 1 / 3 / 5 pass, rejected with {large}: {why}', flush=True)
                continue
            meta, arrays = got
            meta['largest_beam_tried'] = list(LARGE[:LARGE.index(large) + 1])
            out = os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_beam_tiny.npz')
            np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                                **arrays)
            print(f'seed {wseed}: accepted with beams {meta["beams"]} -> {out} '
                  f'({os.path.getsize(out)} bytes); e_row {meta["e_row"]:.2e}, e_score '
                  f'{meta["e_score"]:.2e}, gaps member {meta["min_member_gap"]:.2e} cut '
                  f'{meta["min_cut_gap"]:.2e} final {meta["min_final_gap"]:.2e}, fusion frames '
                  f'{meta["most_fusion_frames"]}, unmodified runs',
                  [k for k, r in meta['runs'].items() if r['unmodified']])
            return 0
    print('no seed met the conditions')
    return 1


if __name__ == '__main__':
    sys.exit(main())
