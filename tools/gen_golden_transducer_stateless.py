#!/usr/bin/env python3
"""Record what the REAL reference's hybrid transducer decodes with its two stateless predictors
-- EmbeddingPredictor and ConvPredictor, wenet/models/transducer/predictor.py:209-495 -- for
tests/test_transducer_stateless_formulation.py and tests/test_gpu_transducer_stateless.py.

    python tools/gen_golden_transducer_stateless.py [first seed]   # CPU only; needs the reference

Models: wenet_amd.synthetic `tiny_rnnt_embed` and `tiny_rnnt_conv`, built by the reference's own
init_model and loaded strictly with the synthetic state dict, each with a weight seed of its own.
Inputs: make_features(3, (60, 150), seed=77): T' = 29, 16, 15.  The helpers of the LSTM fixtures'
generators run the reference (tools/gen_golden_transducer*.py): one utterance at a time from the
recorded encoder rows, in fp32 and as model.double() under a float64 default dtype, with the same
names bound in this process only (search.log_add mended, torchaudio's rnnt_loss by its published
definition); nothing in the reference tree changes.

Recorded in tests/golden/rnnt/rnnt_stateless_tiny.npz, per model (meta[config]):
  * greedy token lists for n_steps 64 / 3 / 1;
  * the final beams of beams 1 / 3 / 5 at (ctc_weight, transducer_weight) (0.3, 0.7), (0, 1),
    (1, 0), fp32 and fp64;
  * transducer_attention_rescoring after the (0.3, 0.7) transducer search with beams 1 / 5 and
    the rescoring weights of RESCORE_WEIGHTS: n-best, the parts of every score, the winner;
  * six forward_step calls along utterance 0's n_steps-64 path: the window ids, the fp64 output
    and the fp64 joint logits of the frame of the same number (arrays `<config>_step<k>_*`), and
    e_step, the fp32 module's max abs error of joint.pred_ffn(forward_step) against fp64 on them;
and the model's encoder output (`<config>_enc`, zero behind an utterance's last frame).

A model's weight seed (first seed .. 199) is REJECTED unless
  1. the fp64 reference and the fp64 restatement (tests/transducer_stateless_formulation.py
     driven through the existing formulation searches) decode what the fp32 reference decodes;
  2. greedy, n_steps 64: some frame emits >= 2 symbols, some frame none, >= 4 blank frames follow
     one another somewhere; n_steps 3: the cap is hit on a frame;
  3. at every joint row that decides something on a greedy path the top-two gap is >= 4 x
         dot_bound + 4 e_pp sum_k |W[i, k] - W[j, k]|
     -- transducer_formulation.dot_bound is the fp32 bound of the joint row itself; the second
     term carries the predictor: the GPU may be 4 e_pp off in every element of pred_proj
     (e_pp: the fp32 reference's largest error of joint.pred_ffn(forward_step) against fp64 over
     every window of the greedy paths), tanh is 1-Lipschitz, and the gap moves by at most
     sum_k |W[i, k] - W[j, k]| times that;
  4. the beam fixture's conditions (tools/gen_golden_transducer_beam.py, 1. - 4.) and the
     rescoring fixture's (tools/gen_golden_transducer_rescore.py, 1. - 4.) on the runs recorded
     here;
  5. some greedy decision is taken while the window still holds a pre-start zero (the first one
     is, with a context above 1); some greedy hypothesis is longer than the context, so the
     window slides off the leading blank; with beam 5 some frame holds two live hypotheses
     with the same window (their last C tokens) that differ earlier.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

CONFIGS = ('tiny_rnnt_embed', 'tiny_rnnt_conv')
BATCH, FRAMES, FSEED = 3, (60, 150), 77
N_STEPS = (64, 3, 1)
WEIGHTS = ((0.3, 0.7), (0.0, 1.0), (1.0, 0.0))
BEAMS = (1, 3, 5)
RESCORE_BEAMS = (1, 5)
RESCORE_SEARCH = (0.3, 0.7)
RESCORE_WEIGHTS = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.3, 0.4, 0.3, 0.3),
                   (0.5, 0.5, 0.0, 0.0))     # (ctc, attn, transducer, reverse)
STEP_AT = (0, 1, 2, 4, 5, 7)     # the recorded forward_step calls of utterance 0
OUT = os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_stateless_tiny.npz')


def build_pair(configs, sd):
    """(fp32 reference model, fp64 reference model)."""
    from oracle.gen_golden import build_reference_model
    model = build_reference_model(configs, sd)
    torch.set_default_dtype(torch.float64)       # init_state allocates with the default dtype
    try:
        model64 = build_reference_model(configs, sd).double()
    finally:
        torch.set_default_dtype(torch.float32)
    return model, model64


class Double:
    def __enter__(self):
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)


def module_pp(model, ctx, dtype):
    """joint.pred_ffn(forward_step) of the reference module for one window (ids, -1: zero)."""
    emb = model.predictor.embed.weight
    hist = torch.stack([emb[i] if i >= 0 else torch.zeros_like(emb[0]) for i in ctx[:-1]]) \
        if len(ctx) > 1 else torch.zeros(0, emb.shape[1], dtype=dtype)
    out, _ = model.predictor.forward_step(torch.tensor([[int(ctx[-1])]]), torch.zeros(1, 1, dtype=dtype),
                                          [hist.unsqueeze(0).to(dtype)])
    return out[0, 0], model.joint.pred_ffn(out)[0, 0]


def greedy_part(name, configs, sd, model, model64, enc, enc_lens, blank):
    import gen_golden_transducer as GG
    import transducer_formulation as TF
    import transducer_stateless_formulation as SF
    W = SF.weights64({k: v.numpy() for k, v in sd.items() if k.startswith(('predictor.', 'joint.'))},
                     configs)
    C, J = W['context'], configs['joint_conf']['join_dim']
    toks = {n: GG.ref_tokens(model, enc, enc_lens, n) for n in N_STEPS}
    with Double():
        toks64 = {n: GG.ref_tokens(model64, enc.double(), enc_lens, n) for n in N_STEPS}
    if toks64 != toks:
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    # e_pp over every window of the greedy paths
    wins = {tuple(w) for n in N_STEPS for u in toks[n]
            for w in SF.windows([u[:k] for k in range(len(u) + 1)], C, blank).tolist()}
    e_pp = 0.0
    with torch.no_grad():
        for w in sorted(wins):
            p32 = module_pp(model, w, torch.float32)[1].double().numpy()
            with Double():
                p64 = module_pp(model64, w, torch.float64)[1].numpy()
            e_pp = max(e_pp, float(np.abs(p32 - p64).max()))
            mine = SF.pred_proj(np.asarray([w]), W)[0]
            if np.abs(mine - p64).max() > 1e-11:
                return 'the fp64 restatement of the predictor differs from the reference', None
    ratio = np.inf
    w_out = W['ffn_out'][0]
    for n in N_STEPS:
        emitted = [np.zeros(int(v), dtype=np.int64) for v in enc_lens]
        worst = [np.inf]

        def on_row(b, t, hrow, logits):
            if int(logits.argmax()) != blank:
                emitted[b][t] += 1
            gap, bound = TF.dot_bound(hrow, logits, w_out, J)
            order = np.argsort(-logits, kind='stable')
            bound += 4 * e_pp * float(np.abs(w_out[order[0]] - w_out[order[1]]).sum())
            worst[0] = min(worst[0], gap / bound)
        ftoks, _ = TF.lookahead_greedy_search(enc.numpy(), enc_lens, W, blank, n, 1, on_row)
        if ftoks != toks[n]:
            return f'the fp64 restatement differs from the reference at n_steps {n}', None
        ratio = min(ratio, worst[0])
        if n == 64:
            if not any((e >= 2).any() for e in emitted):
                return 'no frame emits two symbols', None
            if not any((e == 0).any() for e in emitted):
                return 'no frame without a symbol', None
            if max(GG.longest_zero_run(e) for e in emitted) < 4:
                return 'no run of four blank frames', None
        if n == 3 and not any((e >= 3).any() for e in emitted):
            return 'n_steps 3: the cap is never hit', None
    if ratio < 4.0:
        return f'greedy gap / extended bound {ratio:.2f} < 4', None
    if C > 1 and not any(len(u) > 0 for u in toks[64]):
        return 'no decision under a window with a pre-start zero', None
    if not any(len(u) > C for u in toks[64]):
        return 'no hypothesis longer than the context', None
    seq = toks[64][0]
    if len(seq) < max(STEP_AT):
        return 'utterance 0 is too short for the recorded steps', None
    arrays, e_step = {}, 0.0
    with torch.no_grad():
        for k in STEP_AT:
            ctx = SF.windows([seq[:k]], C, blank)[0].tolist()
            p32 = module_pp(model, ctx, torch.float32)[1].double().numpy()
            with Double():
                out64, p64 = module_pp(model64, ctx, torch.float64)
                logits = model64.joint(enc[0:1, k:k + 1].double(), out64.reshape(1, 1, -1))
            e_step = max(e_step, float(np.abs(p32 - p64.numpy()).max()))
            arrays[f'{name}_step{k}_ctx'] = np.asarray(ctx, dtype=np.int32)
            arrays[f'{name}_step{k}_out'] = out64.numpy().astype(np.float64)
            arrays[f'{name}_step{k}_logits'] = logits.reshape(-1).numpy().astype(np.float64)
    meta = dict(tokens={str(n): toks[n] for n in N_STEPS}, min_gap_over_bound=float(ratio),
                e_pp=e_pp, e_step=e_step, step_at=list(STEP_AT), context=C)
    return None, (meta, arrays, W)


def beam_part(configs, model, model64, enc, enc_lens, blank, W):
    """The beam fixture's runs and conditions (gen_golden_transducer_beam.try_seed) on this
    model, and the shared-window condition."""
    import gen_golden_transducer_beam as GB
    import transducer_beam_formulation as BF
    with torch.no_grad():
        with Double():
            ctc64 = model64.ctc.log_softmax(enc.double()).numpy()
    runs = {}
    e_row = e_score = 0.0
    gaps = dict(member=[], cut=[], final=[])
    fusion_frames, shared = 0, False
    for cw, tw in WEIGHTS:
        for beam in BEAMS:
            b32, b64, unmod = [], [], True
            for b in range(BATCH):
                n = enc_lens[b]
                f32, d32, u32 = GB.run_reference(model, enc[b:b + 1, :n], beam, cw, tw)
                with Double():
                    f64, d64, _ = GB.run_reference(model64, enc[b:b + 1, :n].double(), beam, cw, tw)
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
            trace = []
            mine = BF.prefix_beam_search(enc.numpy(), enc_lens, ctc64, W, blank, beam, cw, tw,
                                         score_dtype=np.float64, trace=trace)
            for b in range(BATCH):
                if [t for t, _ in mine[b]] != [t for t, _ in b64[b]]:
                    return f'({cw}, {tw}) beam {beam}: the restatement differs from fp64', None
                if max(abs(a - c) for (_, a), (_, c) in zip(mine[b], b64[b])) > 1e-9:
                    return f'({cw}, {tw}) beam {beam}: restatement scores off by > 1e-9', None
            if beam == 5:
                # live hypotheses are distinct token lists: two slots of one utterance with the
                # same pred_proj row (a function of the window alone) share their last C tokens
                # and differ earlier
                for fr in trace:
                    pp = fr['pred_proj']
                    for (b, j), row in pp.items():
                        shared = shared or any(b2 == b and j2 < j and np.array_equal(row, r2)
                                               for (b2, j2), r2 in pp.items())
            runs[f'{cw}_{tw}_{beam}'] = dict(ctc_weight=cw, transducer_weight=tw, beam=beam,
                                            unmodified=unmod, fp32=b32, fp64=b64)
    if fusion_frames < 5:
        return 'no run with a fusion in five frames', None
    if not any(runs[f'{cw}_{tw}_1']['fp64'][b][0][0] != runs[f'{cw}_{tw}_5']['fp64'][b][0][0]
               for cw, tw in WEIGHTS for b in range(BATCH)):
        return 'beam 1 and beam 5 agree on every best hypothesis', None
    if not any(t == [] for r in runs.values() for u in r['fp64'] for t, _ in u):
        return 'no final beam holds the empty hypothesis', None
    if not shared:
        return 'beam 5: no two live hypotheses share a window', None
    need_row, need_score = 8 * e_row + 2e-6, 8 * e_score + 2e-6
    mins = {k: (min(v) if v else float('inf')) for k, v in gaps.items()}
    if mins['member'] < need_row:
        return f"membership gap {mins['member']:.2e} < {need_row:.2e}", None
    if mins['cut'] < need_score:
        return f"cut gap {mins['cut']:.2e} < {need_score:.2e}", None
    if mins['final'] < need_score:
        return f"final-beam gap {mins['final']:.2e} < {need_score:.2e}", None
    meta = dict(weights=[list(w) for w in WEIGHTS], beams=list(BEAMS), runs=runs, e_row=e_row,
                e_score=e_score, min_member_gap=mins['member'], min_cut_gap=mins['cut'],
                min_final_gap=mins['final'], most_fusion_frames=fusion_frames)
    return None, meta


def rescore_part(model, model64, enc, enc_lens, blank, W):
    """The rescoring fixture's conditions (gen_golden_transducer_rescore.try_seed) on the runs
    recorded here."""
    import gen_golden_transducer_rescore as GR
    import transducer_score_formulation as SCF
    runs = {}
    e = dict(td=0.0, attn=0.0, score=0.0)
    gaps = []
    not_first = False
    sw = RESCORE_SEARCH
    for beam in RESCORE_BEAMS:
        for wi, rw_set in enumerate(RESCORE_WEIGHTS):
            u32, u64 = [], []
            for b in range(BATCH):
                n = enc_lens[b]
                try:
                    r32 = GR.run_reference(model, enc[b:b + 1, :n], beam, 'transducer', sw, rw_set)
                    with Double():
                        r64 = GR.run_reference(model64, enc[b:b + 1, :n].double(), beam,
                                               'transducer', sw, rw_set)
                except (AssertionError, RuntimeError, IndexError) as ex:
                    return f'rescoring beam {beam} set {wi}: the reference raised {ex!r}', None
                if [t for t, _ in r32['nbest']] != [t for t, _ in r64['nbest']]:
                    return f'rescoring beam {beam}: fp32 and fp64 n-bests differ', None
                if r32['tokens'] != r64['tokens']:
                    return f'rescoring beam {beam} set {wi}: winners differ', None
                for k in ('td', 'attn'):
                    e[k] = max(e[k], max(abs(a - c) for a, c in zip(r32[k], r64[k])))
                e['score'] = max(e['score'], abs(r32['score'] - r64['score']),
                                 max(abs(a - c) for a, c in zip(r32['final'], r64['final'])))
                srt = sorted(r64['final'], reverse=True)
                if len(srt) > 1:
                    gaps.append(srt[0] - srt[1])
                not_first = not_first or r64['winner'] != 0
                if wi == 0:
                    mine = SCF.transducer_scores(enc[b, :n].numpy(), [t for t, _ in r64['nbest']],
                                                 W, blank)
                    if max(abs(a - c) for a, c in zip(mine, r64['td'])) > 1e-9:
                        return f'rescoring beam {beam}: restatement td off by > 1e-9', None
                u32.append(r32)
                u64.append(r64)
            runs[f'{beam}_{wi}'] = dict(beam=beam, weights=list(rw_set), fp32=u32, fp64=u64)
    if not not_first:
        return 'rescoring: the winner is the first hypothesis in every run', None
    differs = any(a['tokens'] != c['tokens']
                  for beam in RESCORE_BEAMS for wi in range(1, len(RESCORE_WEIGHTS))
                  for a, c in zip(runs[f'{beam}_0']['fp64'], runs[f'{beam}_{wi}']['fp64']))
    if not differs:
        return 'rescoring: no winner differs between two weight sets', None
    if not any(t == [] for r in runs.values() for u in r['fp64'] for t, _ in u['nbest']):
        return 'rescoring: no n-best holds the empty hypothesis', None
    need = 8 * e['score'] + 2e-6
    if min(gaps) < need:
        return f'rescoring: winner gap {min(gaps):.2e} < {need:.2e}', None
    return None, dict(search_weights=list(sw), beams=list(RESCORE_BEAMS),
                      rescore_weights=[list(w) for w in RESCORE_WEIGHTS], runs=runs,
                      e_td=e['td'], e_attn=e['attn'], e_score=e['score'], min_gap=min(gaps))


def try_config(name, wseed):
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    blank = configs['tokenizer_conf']['special_tokens']['<blank>']
    feats, lens = S.make_features(BATCH, FRAMES, seed=FSEED)
    sd = S.make_state_dict(configs, wseed)
    model, model64 = build_pair(configs, sd)
    assert model.blank == blank
    with torch.no_grad():
        enc, mask = model._forward_encoder(feats, lens, -1, -1)
        enc_lens = [int(v) for v in mask.squeeze(1).sum(1)]
    why, got = greedy_part(name, configs, sd, model, model64, enc, enc_lens, blank)
    if got is None:
        return why, None
    gmeta, arrays, W = got
    why, got = beam_part(configs, model, model64, enc, enc_lens, blank, W)
    if got is None:
        return why, None
    bmeta = got
    why, rmeta = rescore_part(model, model64, enc, enc_lens, blank, W)
    if rmeta is None:
        return why, None
    meta = dict(greedy=gmeta, beam=bmeta, rescore=rmeta, blank=blank, enc_lens=enc_lens)
    enc = enc.numpy().astype(np.float32).copy()
    for b, n in enumerate(enc_lens):      # (no search reads a row behind an utterance's end)
        enc[b, n:] = 0.0
    return None, (meta, arrays, enc)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    import gen_golden_transducer_rescore as GR
    import wenet.models.transducer.transducer as T
    T.torchaudio = types.SimpleNamespace(functional=types.SimpleNamespace(rnnt_loss=GR.rnnt_loss_fp64))
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    meta = dict(configs=list(CONFIGS), batch=BATCH, frames=list(FRAMES), fseed=FSEED,
                bound=['torchaudio.functional.rnnt_loss = rnnt_loss_fp64 of '
                       'tools/gen_golden_transducer_rescore.py',
                       'search.log_add = lambda xs: common.log_add(*xs)'])
    arrays = {}
    for name in CONFIGS:
        for wseed in range(first, 200):
            why, got = try_config(name, wseed)
            if got is None:
                print(f'{name} seed {wseed}: rejected: {why}', flush=True)
                continue
            meta[name], arr, enc = got
            meta[name]['wseed'] = wseed
            arrays.update(arr)
            arrays[f'{name}_enc'] = enc
            print(f'{name} seed {wseed}: accepted', flush=True)
            break
        else:
            print(f'{name}: no seed met the conditions')
            return 1
    np.savez_compressed(OUT, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        **arrays)
    print(f'-> {OUT} ({os.path.getsize(OUT)} bytes)')
    for name in CONFIGS:
        m = meta[name]
        print(f"  {name} (seed {m['wseed']}): greedy lengths "
              f"{[len(u) for u in m['greedy']['tokens']['64']]}, gap / bound "
              f"{m['greedy']['min_gap_over_bound']:.1f}, e_pp {m['greedy']['e_pp']:.2e}, e_step "
              f"{m['greedy']['e_step']:.2e}; beam e_row {m['beam']['e_row']:.2e} e_score "
              f"{m['beam']['e_score']:.2e}; rescore e_td {m['rescore']['e_td']:.2e} e_score "
              f"{m['rescore']['e_score']:.2e}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
