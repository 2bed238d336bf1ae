"""NumPy fp64 restatement of the batched RNN-T prefix beam search
(wenet_amd/csrc/transducer_beam.hip; the reference: PrefixBeamSearch.prefix_beam_search,
wenet/models/transducer/search/prefix_beam_search.py:66-148): the fusion + top-k of a joint row
(`ref_fuse_topk`), one frame of the beam step on a batch of slots (`ref_beam_step`) and the whole
search over a padded encoder output (`prefix_beam_search`).  What the kernels are checked against
on the GPU (tests/test_gpu_transducer_beam.py) and, on the CPU, against the reference's recorded
final beams (tests/test_transducer_beam_formulation.py, tests/golden/rnnt/rnnt_beam_tiny.npz).

Per utterance: one hypothesis [blank], score 0.0, on a zero LSTM state; per frame and live
hypothesis j the predictor output of hyp_j, logp_j = log_softmax(joint(enc[i], pred_j)),
f_j = log(tw exp(logp_j) + cw exp(ctc_logp[i])), its `beam` largest entries (lower index on equal
values); candidates j-major and rank-minor with score `score_dtype(score_j) + value` held as a
double; a blank candidate keeps hyp_j, another token appends; a candidate whose token list equals
that of an earlier entry adds its score into it with log_add (the entry keeps its place); a
stable sort by score, descending, keeps `beam`.

The reference's fusion calls log_add with a list although the function takes its values one by
one, and raises; this restates the intent, log_add of the two scores.

The predictor state and pred_out of a hypothesis are functions of its token sequence alone, so a
slot keeps the state reached after its WHOLE hypothesis and its joint.pred_ffn row: a
blank-extended or fused-into-blank slot copies them, only a slot that appended a token steps the
LSTM.  (The reference keeps the state after hyp[:-1] and steps every hypothesis every frame.)
"""
import math

import numpy as np

import transducer_formulation as TF

NEG_INF = -float('inf')


def log_add2(a, b):
    """wenet/utils/common.py:302-310 for two values.  A NaN gives NaN, two -inf give -inf."""
    if a != a or b != b:
        return float('nan')
    if a == NEG_INF and b == NEG_INF:
        return NEG_INF
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def rank_key(x):
    """A NaN ranks as -inf (the rule of the attention beam's update kernel)."""
    return NEG_INF if x != x else x


def ref_fuse_topk(logits, ctc_logp, cw, tw, k):
    """One joint row (V) -> (fused row, top-k values, top-k indices).  The selection order is
    larger value first, the lower index on equal values; a NaN ranks, and is returned, as -inf,
    so the indices are always k distinct columns.  cw == 0: the CTC row is not read."""
    x = np.asarray(logits)
    with np.errstate(all='ignore'):
        ok = x[~np.isnan(x)]
        mx = ok.max() if ok.size else x.dtype.type(NEG_INF)     # (fmaxf skips a NaN)
        lp = (x - mx) - np.log(np.exp(x - mx).sum())
        p = x.dtype.type(tw) * np.exp(lp)
        if cw != 0:
            p = p + x.dtype.type(cw) * np.exp(np.asarray(ctc_logp, dtype=x.dtype))
        f = np.log(p)
    key = np.where(np.isnan(f), x.dtype.type(NEG_INF), f)
    order = np.argsort(-key, kind='stable')[:k]
    return f, key[order], order.astype(np.int64)


def ref_beam_step(slots, top_val, top_idx, frame, lens, blank, beam, score_dtype=np.float32,
                  trace=None):
    """One frame of the beam step on a batch.
    slots[b]: the live hypotheses of utterance b in rank order, [(token list, score), ...]
    (tokens without the leading blank); top_val / top_idx [b][j]: the top-k pairs of slot j.
    Returns (new slots, src, tok, advance, row_enc), the last four (B, beam) int arrays over the
    new slots: the slot b * beam + j of the whole batch whose predictor state the new slot takes
    (-1: none -- an empty slot, or the utterance has no further frame), the token it appended
    (else blank), whether the predictor steps on it, and its joint row of the next frame (the
    utterances' rows packed in order; -1: inert).  An utterance with frame >= its length moves on
    unchanged.  trace (a list): gets per stepped utterance
    dict(b, sorted=[scores of the sorted fusion list], n_fused, fused=[whether that entry is a
    log_add of two])."""
    B = len(slots)
    src = np.full((B, beam), -1, dtype=np.int64)
    tok = np.full((B, beam), blank, dtype=np.int64)
    advance = np.zeros((B, beam), dtype=np.int64)
    row_enc = np.full((B, beam), -1, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = []
    for b in range(B):
        live = slots[b]
        if frame >= lens[b]:
            out.append([(list(h), s) for h, s in live])
            continue
        # beam_A: j-major, top-k-rank-minor
        cand = []
        for j, (hyp, score) in enumerate(live):
            for r in range(beam):
                k = int(top_idx[b][j][r])
                s = float(score_dtype(score) + score_dtype(top_val[b][j][r]))
                if k == blank:
                    cand.append(dict(hyp=list(hyp), score=s, src=j, tok=None))
                else:
                    cand.append(dict(hyp=list(hyp) + [k], score=s, src=j, tok=k))
        # prefix fusion: identity is the token sequence; the entry keeps its place.  Live
        # hypotheses are distinct, so a pair is always one blank and one token candidate: the
        # fused entry copies the blank candidate's slot (no LSTM step)
        fusion, n_fused = [], 0
        for c in cand:
            for e in fusion:
                if e['hyp'] == c['hyp']:
                    e['score'] = log_add2(e['score'], c['score'])
                    e['fused'] = True
                    if c['tok'] is None:
                        e['src'], e['tok'] = c['src'], None
                    n_fused += 1
                    break
            else:
                fusion.append(c)
        fusion.sort(key=lambda e: -rank_key(e['score']))      # stable
        if trace is not None:
            trace.append(dict(b=b, sorted=[e['score'] for e in fusion], n_fused=n_fused,
                              fused=[e.get('fused', False) for e in fusion]))
        more = frame + 1 < lens[b]
        new = []
        for s, e in enumerate(fusion[:beam]):
            new.append((e['hyp'], e['score']))
            if more:
                src[b, s] = b * beam + e['src']
                row_enc[b, s] = off[b] + frame + 1
            if e['tok'] is not None:
                tok[b, s] = e['tok']
                advance[b, s] = 1 if more else 0
        out.append(new)
    return out, src, tok, advance, row_enc


def prefix_beam_search(enc, enc_lens, ctc_logp, W, blank, beam, cw, tw, score_dtype=np.float64,
                       trace=None):
    """The search over a padded (B, T', d) encoder output in fp64; ctc_logp (B, T', V) or None
    with cw == 0.  Returns per utterance the final beam [(tokens, score), ...], best first.
    score_dtype: what the scores are rounded to when a frame starts (the reference rebuilds a
    tensor of the default dtype from its Python floats: float32, or float64 for model.double()).
    trace (a list): gets per frame dict(frame, rows={(b, j): the top beam + 1 fused values},
    pred_proj={(b, j): the joint.pred_ffn row of slot j}, steps=[ref_beam_step's trace])."""
    enc = np.asarray(enc, dtype=np.float64)
    lens = [int(v) for v in np.asarray(enc_lens).reshape(-1)]
    B = enc.shape[0]
    L, H = len(W['rnn']), W['rnn'][0][1].shape[1]
    enc_proj = enc @ W['enc_ffn'][0].T + W['enc_ffn'][1]
    V = W['ffn_out'][0].shape[0]

    def step_state(state, token):
        h, c = (np.zeros((L, 1, H)), np.zeros((L, 1, H))) if state is None else state[:2]
        out, h, c = TF.predictor_step([token], h, c, W)
        return h, c, out @ W['pred_ffn'][0].T + W['pred_ffn'][1]

    slots = [[([], 0.0)] for _ in range(B)]
    # state[b][j]: (h, c, pred_proj) after [blank] + hyp_j
    state = [[step_state(None, blank)] for _ in range(B)]
    for i in range(max(lens + [0])):
        top_val = [None] * B
        top_idx = [None] * B
        rows, pps = {}, {}
        for b in range(B):
            if i >= lens[b]:
                continue
            top_val[b], top_idx[b] = [], []
            for j in range(len(slots[b])):
                logits = TF.joint_logits(enc_proj[b, i], state[b][j][2][0], W)
                crow = None if cw == 0 else ctc_logp[b, i]
                f, val, idx = ref_fuse_topk(logits, crow, cw, tw, beam)
                val = list(val) + [NEG_INF] * (beam - len(val))
                top_val[b].append(val)
                top_idx[b].append(list(idx))
                if trace is not None:
                    key = np.where(np.isnan(f), NEG_INF, f)
                    rows[(b, j)] = np.sort(key)[::-1][:min(beam + 1, V)].copy()
                    pps[(b, j)] = state[b][j][2][0]
        steps = [] if trace is not None else None
        slots, src, tok, advance, _ = ref_beam_step(slots, top_val, top_idx, i, lens, blank, beam,
                                                    score_dtype, steps)
        if trace is not None:
            trace.append(dict(frame=i, rows=rows, pred_proj=pps, steps=steps))
        new_state = []
        for b in range(B):
            if i >= lens[b]:
                new_state.append(state[b])
                continue
            row = []
            for s in range(len(slots[b])):
                if src[b, s] < 0:
                    row.append(None)           # the utterance is finished: never read again
                    continue
                st = state[b][src[b, s] - b * beam]
                row.append(step_state(st, int(tok[b, s])) if advance[b, s] else st)
            new_state.append(row)
        state = new_state
    return slots


# ---- hand-written beam-step cases ------------------------------------------------------------
def add32(score, value):
    """A candidate's score: the fp32 add of the fp32-rounded score and the fp32 value, as a double."""
    return float(np.float32(score) + np.float32(value))


def hand_cases():
    """Chains of beam-step frames whose results were worked out by hand (blank = 0, V = 16):
    dict(name, beam, lens, frame0, slots, frames=[dict(top_val, top_idx, want, src, tok, advance,
    row_enc)]); `want` etc. are what ref_beam_step and the kernel must return for that frame, and
    the next frame starts from `want`."""
    nan, inf = float('nan'), float('inf')
    cases = []
    # a blank / token fusion, the blank candidate earlier in the list: [5] of slot 0 (blank)
    # meets [] + [5] of slot 1; the entry keeps place 0 and copies slot 0
    cases.append(dict(
        name='fusion_blank_first', beam=2, lens=[3], frame0=1,
        slots=[[([5], -1.0), ([], -2.0)]],
        frames=[dict(top_val=[[[-0.5, -1.5], [-0.25, -3.0]]], top_idx=[[[0, 7], [5, 0]]],
                     want=[[([5], log_add2(add32(-1.0, -0.5), add32(-2.0, -0.25))),
                            ([5, 7], add32(-1.0, -1.5))]],
                     src=[[0, 0]], tok=[[0, 7]], advance=[[0, 1]], row_enc=[[2, 2]])]))
    # the same with the token candidate earlier: the entry keeps place 0 and copies slot 1, the
    # blank candidate's slot (no LSTM step)
    cases.append(dict(
        name='fusion_token_first', beam=2, lens=[3], frame0=1,
        slots=[[([], -1.0), ([5], -2.0)]],
        frames=[dict(top_val=[[[-0.5, -1.0], [-0.25, -4.0]]], top_idx=[[[5, 0], [0, 9]]],
                     want=[[([5], log_add2(add32(-1.0, -0.5), add32(-2.0, -0.25))),
                            ([], add32(-1.0, -1.0))]],
                     src=[[1, 0]], tok=[[0, 0]], advance=[[0, 0]], row_enc=[[2, 2]])]))
    # a re-created prefix: [5] (slot 0) begets [5, 7] and leaves the beam in frame 0, is created
    # again from [] in frame 1 and now sits in slot 1; in frame 2 the blank candidate of [5, 7]
    # must fuse with ([5], 7) although the [5] alive now is not the object [5, 7] came from --
    # an identity by creation id misses it and keeps [5, 7] twice
    f0 = [([5, 7], add32(-1.0, -0.1)), ([], add32(-1.2, -0.2))]
    f1 = [([5, 7], add32(f0[0][1], -0.1)), ([5], add32(f0[1][1], -0.1))]
    f2 = [([5, 7], log_add2(add32(f1[0][1], -0.3), add32(f1[1][1], -0.2))),
          ([5], add32(f1[1][1], -0.4))]
    cases.append(dict(
        name='recreated_prefix', beam=2, lens=[4], frame0=0,
        slots=[[([5], -1.0), ([], -1.2)]],
        frames=[dict(top_val=[[[-0.1, -3.0], [-0.2, -4.0]]], top_idx=[[[7, 0], [0, 5]]],
                     want=[f0], src=[[0, 1]], tok=[[7, 0]], advance=[[1, 0]], row_enc=[[1, 1]]),
                dict(top_val=[[[-0.1, -5.0], [-0.1, -5.0]]], top_idx=[[[0, 9], [5, 0]]],
                     want=[f1], src=[[0, 1]], tok=[[0, 5]], advance=[[0, 1]], row_enc=[[2, 2]]),
                dict(top_val=[[[-0.3, -6.0], [-0.2, -0.4]]], top_idx=[[[0, 9], [7, 0]]],
                     want=[f2], src=[[0, 1]], tok=[[0, 0]], advance=[[0, 0]], row_enc=[[3, 3]])]))
    # equal scores keep list order
    cases.append(dict(
        name='equal_scores', beam=2, lens=[5], frame0=2,
        slots=[[([], -1.0), ([3], -1.0)]],
        frames=[dict(top_val=[[[-1.0, -1.0], [-1.0, -1.0]]], top_idx=[[[4, 0], [0, 6]]],
                     want=[[([4], -2.0), ([], -2.0)]],
                     src=[[0, 0]], tok=[[4, 0]], advance=[[1, 0]], row_enc=[[3, 3]])]))
    # a -inf and a NaN candidate: both rank as -inf, in list order, behind every number
    cases.append(dict(
        name='inf_and_nan', beam=3, lens=[2], frame0=0,
        slots=[[([], 0.0), ([2], -1.0)]],
        frames=[dict(top_val=[[[nan, -1.0, -inf], [-0.5, -inf, nan]]],
                     top_idx=[[[1, 0, 3], [0, 4, 5]]],
                     want=[[([], -1.0), ([2], -1.5), ([1], nan)]],
                     src=[[0, 1, 0]], tok=[[0, 0, 1]], advance=[[0, 0, 1]], row_enc=[[1, 1, 1]])]))
    # the first frame: one live slot fills the beam
    cases.append(dict(
        name='first_frame', beam=3, lens=[2], frame0=0,
        slots=[[([], 0.0)]],
        frames=[dict(top_val=[[[-0.1, -2.5, -3.0]]], top_idx=[[[0, 8, 2]]],
                     want=[[([], add32(0.0, -0.1)), ([8], -2.5), ([2], -3.0)]],
                     src=[[0, 0, 0]], tok=[[0, 8, 2]], advance=[[0, 1, 1]],
                     row_enc=[[1, 1, 1]])]))
    # beam 1, three utterances: one goes on, one sees its last frame (no state is handed on),
    # one is finished and moves on unchanged
    cases.append(dict(
        name='beam_1', beam=1, lens=[3, 2, 1], frame0=1,
        slots=[[([4], -0.5)], [([], -1.0)], [([6], -0.75)]],
        frames=[dict(top_val=[[[-0.25]], [[-0.5]], [[-9.0]]], top_idx=[[[9]], [[0]], [[3]]],
                     want=[[([4, 9], -0.75)], [([], -1.5)], [([6], -0.75)]],
                     src=[[0], [-1], [-1]], tok=[[9], [0], [0]], advance=[[1], [0], [0]],
                     row_enc=[[2], [-1], [-1]])]))
    return cases


def same_score(a, b, ulps=0):
    """NaN equals NaN; otherwise within `ulps` fp64 ulps (0: the same bits up to the sign of 0)."""
    if a != a or b != b:
        return a != a and b != b
    if a == b:
        return True
    return abs(a - b) <= ulps * np.spacing(max(abs(a), abs(b)))
