#!/usr/bin/env python3
"""Record the final beams of the REAL reference's transducer prefix beam search behind a
chunk-masked encoder pass -- model.bs.prefix_beam_search(..., decoding_chunk_size=c,
num_decoding_left_chunks=l, ...), wenet/models/transducer/search/prefix_beam_search.py:42-148 --
for the streaming transducer beam sessions (tests/test_transducer_beam_stream_formulation.py,
tests/test_gpu_transducer_beam_stream.py).

    python tools/gen_golden_transducer_beam_stream.py        # CPU only; needs the reference tree

Model: wenet_amd.synthetic `tiny_rnnt`, built by the reference's own init_model; inputs
make_features(3, (60, 150), seed=77), one utterance at a time, as the reference requires.  What
tools/gen_golden_transducer_beam.py does for the one-shot search is done here per (c, l) in
{(4, -1), (3, 2)}: the reference's own search object decodes from its own chunk-masked encoder
pass, in fp32 and as model.double(), for beams 1 / 5 and (ctc_weight, transducer_weight) in
{(0.3, 0.7), (0.0, 1.0)}; every run is tried unmodified first and repeated with the one log_add
call mended in this process where it raises (see that tool); an Onlooker notes the fused rows and
the fusion lists.

Recorded in tests/golden/rnnt/rnnt_beam_stream_tiny.npz: per (c, l) the chunk-masked encoder
output (`enc_c{c}_l{l}`, padded to the longest utterance) and in `meta` the full final beams of
every run in fp32 and fp64 (model.double() decodes from the recorded fp32 rows, so that every side
starts from the same numbers).

A weight seed is REJECTED unless
  * rules 1, 2 and 4 of tools/gen_golden_transducer_beam.py hold on this fixture (fp32 and fp64
    agree on the lists; the fp64 restatement gives the fp64 lists, scores within 1e-9; every
    membership, cut and final-beam gap is >= 8 e + 2e-6), e_row, e_score and the smallest gaps
    going into the meta;
  * some utterance appends a token to a surviving hypothesis on a frame that is the last of a
    chunk and not the last of the utterance (the `pending` path of a session fed chunk by chunk);
  * some fusion falls on such a frame.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

CONFIG = 'tiny_rnnt'
BATCH, FRAMES, FSEED = 3, (60, 150), 77
CHUNKS = ((4, -1), (3, 2))
WEIGHTS = ((0.3, 0.7), (0.0, 1.0))
BEAMS = (1, 5)


def key(c, l):
    return f'c{c}_l{l}'


def run_reference(model, x, xlen, c, l, beam, cw, tw):
    """One utterance through model.bs.prefix_beam_search behind the chunk-masked encoder.
    Returns (final beam [(tokens, score)], per-frame digest, ran unmodified, encoder output)."""
    import wenet.models.transducer.search.prefix_beam_search as search
    from wenet.utils import common
    from gen_golden_transducer_beam import Onlooker
    saved = search.log_add
    for unmodified in (True, False):
        if not unmodified:
            search.log_add = lambda xs: common.log_add(*xs)      # the one mended call
        try:
            with Onlooker(search) as look, torch.no_grad():
                final, enc = model.bs.prefix_beam_search(
                    x, xlen, decoding_chunk_size=c, beam_size=beam, num_decoding_left_chunks=l,
                    simulate_streaming=False, ctc_weight=cw, transducer_weight=tw)
        except TypeError:
            if not unmodified:
                raise
            continue
        finally:
            search.log_add = saved
        return ([([int(v) for v in s.hyp[1:]], float(s.score)) for s in final],
                look.digest(beam), unmodified, enc[0])


def try_seed(wseed):
    import transducer_beam_stream_formulation as SF
    import transducer_formulation as TF
    from gen_golden_transducer_beam import run_reference as run_on_rows
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(CONFIG)
    blank = configs['tokenizer_conf']['special_tokens']['<blank>']
    feats, lens = S.make_features(BATCH, FRAMES, seed=FSEED)
    sd = S.make_state_dict(configs, wseed)
    model = build_reference_model(configs, sd)
    model.init_bs()       # (transducer.py:156: what beam_search does before it calls model.bs)
    torch.set_default_dtype(torch.float64)       # init_state allocates with the default dtype
    try:
        model64 = build_reference_model(configs, sd).double()
    finally:
        torch.set_default_dtype(torch.float32)
    W = TF.weights64({k: v.numpy() for k, v in sd.items() if k.startswith(('predictor.', 'joint.'))},
                     configs['predictor_conf']['num_layers'])

    runs, arrays = {}, {}
    e_row = e_score = 0.0
    gaps = dict(member=[], cut=[], final=[])
    pending_at, fusion_at = [], []
    enc_lens = None
    for c, l in CHUNKS:
        encs = [None] * BATCH
        for cw, tw in WEIGHTS:
            for beam in BEAMS:
                b32, b64, unmod = [], [], True
                for b in range(BATCH):
                    n = int(lens[b])
                    x, xl = feats[b:b + 1, :n], lens[b:b + 1]
                    f32, d32, u32, enc = run_reference(model, x, xl, c, l, beam, cw, tw)
                    if encs[b] is None:
                        encs[b] = enc.numpy().astype(np.float32)
                    assert np.array_equal(encs[b], enc.numpy())
                    rows = encs[b]
                    # model.double() decodes from the RECORDED rows (as in the one-shot tool):
                    # every side starts from the same numbers
                    torch.set_default_dtype(torch.float64)
                    try:
                        f64, d64, _ = run_on_rows(model64, torch.from_numpy(rows).double()[None],
                                                  beam, cw, tw)
                    finally:
                        torch.set_default_dtype(torch.float32)
                    if [t for t, _ in f32] != [t for t, _ in f64]:
                        return f'{key(c, l)} ({cw}, {tw}) beam {beam}: fp32 and fp64 final beams differ', None
                    unmod = unmod and u32
                    b32.append(f32)
                    b64.append(f64)
                    for (r32, l32, _), (r64, l64, _) in zip(d32, d64):
                        if [h for h, _ in l32] != [h for h, _ in l64]:
                            return f'{key(c, l)} ({cw}, {tw}) beam {beam}: candidate sets differ', None
                        e_row = max(e_row, float(np.abs(r32 - r64).max()))
                        e_score = max(e_score, max(abs(a - d) for (_, a), (_, d) in zip(l32, l64)))
                        if r64.shape[1] > beam:
                            gaps['member'].append(float((r64[:, beam - 1] - r64[:, beam]).min()))
                        srt = sorted((s for _, s in l64), reverse=True)
                        if len(srt) > beam:
                            gaps['cut'].append(srt[beam - 1] - srt[beam])
                    sc = [s for _, s in f64]
                    gaps['final'] += [a - d for a, d in zip(sc, sc[1:])]
                    # the fp64 restatement as a session fed chunk by chunk
                    with torch.no_grad():
                        ctc64 = model64.ctc.log_softmax(torch.from_numpy(rows).double()[None])[0].numpy()
                    ses = SF.run_splits(rows, ctc64, (c, ), W, blank, beam, cw, tw)
                    mine = ses.result()
                    if [t for t, _ in mine] != [t for t, _ in f64]:
                        return f'{key(c, l)} ({cw}, {tw}) beam {beam}: the restatement differs from fp64', None
                    if max(abs(a - d) for (_, a), (_, d) in zip(mine, f64)) > 1e-9:
                        return f'{key(c, l)} ({cw}, {tw}) beam {beam}: restatement scores off by > 1e-9', None
                    T = rows.shape[0]
                    for e in ses.events:
                        t = e['frame']
                        if (t + 1) % c == 0 and t + 1 < T:
                            if e['appended'] > 0:
                                pending_at.append([key(c, l), cw, tw, beam, b, t])
                            if e['n_fused'] > 0:
                                fusion_at.append([key(c, l), cw, tw, beam, b, t])
                runs[f'{key(c, l)}_{cw}_{tw}_{beam}'] = dict(
                    chunk=c, left=l, ctc_weight=cw, transducer_weight=tw, beam=beam,
                    unmodified=unmod, fp32=b32, fp64=b64)
        n_enc = [int(e.shape[0]) for e in encs]
        assert enc_lens in (None, n_enc)
        enc_lens = n_enc
        enc = np.zeros((BATCH, max(n_enc), encs[0].shape[1]), dtype=np.float32)
        for b, e in enumerate(encs):
            enc[b, :n_enc[b]] = e
        arrays['enc_' + key(c, l)] = enc
    if not pending_at:
        return 'no token is appended on the last frame of a chunk inside an utterance', None
    if not fusion_at:
        return 'no fusion falls on the last frame of a chunk inside an utterance', None
    need_row, need_score = 8 * e_row + 2e-6, 8 * e_score + 2e-6
    mins = {k: (min(v) if v else float('inf')) for k, v in gaps.items()}
    if mins['member'] < need_row:
        return f"membership gap {mins['member']:.2e} < {need_row:.2e}", None
    if mins['cut'] < need_score:
        return f"cut gap {mins['cut']:.2e} < {need_score:.2e}", None
    if mins['final'] < need_score:
        return f"final-beam gap {mins['final']:.2e} < {need_score:.2e}", None
    meta = dict(config=CONFIG, wseed=wseed, batch=BATCH, frames=list(FRAMES), fseed=FSEED,
                blank=blank, enc_lens=enc_lens, feat_lens=[int(v) for v in lens],
                chunks=[list(cl) for cl in CHUNKS], weights=[list(w) for w in WEIGHTS],
                beams=list(BEAMS), runs=runs, e_row=e_row, e_score=e_score,
                min_member_gap=mins['member'], min_cut_gap=mins['cut'],
                min_final_gap=mins['final'], pending_at=pending_at[:16], fusion_at=fusion_at[:16],
                n_pending_at=len(pending_at), n_fusion_at=len(fusion_at),
                fp64_runs='model.double() on the recorded fp32 encoder rows',
                mend='search.log_add = lambda xs: common.log_add(*xs)')
    return None, (meta, arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for wseed in range(200):
        why, got = try_seed(wseed)
        if got is None:
            print(f'seed {wseed}: rejected: {why}', flush=True)
            continue
        meta, arrays = got
        out = os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_beam_stream_tiny.npz')
        np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                            **arrays)
        print(f'seed {wseed}: accepted -> {out} ({os.path.getsize(out)} bytes); e_row '
              f'{meta["e_row"]:.2e}, e_score {meta["e_score"]:.2e}, gaps member '
              f'{meta["min_member_gap"]:.2e} cut {meta["min_cut_gap"]:.2e} final '
              f'{meta["min_final_gap"]:.2e}; pending frames {meta["n_pending_at"]}, fusion '
              f'frames {meta["n_fusion_at"]}')
        return 0
    print('no seed met the conditions')
    return 1


if __name__ == '__main__':
    sys.exit(main())
