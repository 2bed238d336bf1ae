"""Shared helpers of the GPU parity tests."""
import numpy as np
import torch

from golden_util import build_inputs, load_case


def make_model(configs, sd):
    from wenet_amd.model import ASRModel
    return ASRModel(configs, sd, device='cuda')


_MODEL_CACHE = {}


def cached_model(config_name, wseed):
    from wenet_amd import synthetic as S
    key = (config_name, wseed)
    if key not in _MODEL_CACHE:
        configs = S.make_configs(config_name)
        sd = S.make_state_dict(configs, wseed)
        _MODEL_CACHE[key] = (configs, sd, make_model(configs, sd))
    return _MODEL_CACHE[key]


def refusal_text(exc):
    """The library's message of a refused call, whole: the RuntimeError of wenet_amd._lib.check
    without its '<entry point> failed (<status>): ' head and without the '<source file>:<line>: '
    that most refusals carry in front of the message (it moves with every edit of the file)."""
    import re
    m = re.fullmatch(r'\w+ failed \(-?\d+\): (?:[^\n]*?\.(?:hip|h):\d+: )?(.*)', str(exc), re.S)
    assert m, str(exc)
    return m.group(1)


def compare_nbest(got, ref_nbest, ref_scores, ref_times, score_atol=2e-3,
                  what=''):
    """n-best lists produced from slightly different log-probs: every reference
    hypothesis that is clear of the pruning boundary must be present with a
    matching score and identical time stamps; order may differ only between
    hypotheses whose scores are closer than the tolerance."""
    g_nbest = [list(x) for x in got.nbest]
    r_nbest = [list(x) for x in ref_nbest]
    assert len(g_nbest) == len(r_nbest), what
    cutoff = ref_scores[-1] + 4 * score_atol
    for i, h in enumerate(r_nbest):
        if ref_scores[i] < cutoff and i > 0:
            continue  # too close to the beam edge to be stable
        assert h in g_nbest, f'{what}: reference hyp #{i} {h} missing'
        j = g_nbest.index(h)
        assert abs(got.nbest_scores[j] - ref_scores[i]) < score_atol, \
            (what, i, got.nbest_scores[j], ref_scores[i])
        assert list(got.nbest_times[j]) == list(ref_times[i]), (what, i)
        if j != i:
            assert abs(ref_scores[i] - ref_scores[j]) < 2 * score_atol, \
                f'{what}: order differs beyond tolerance ({i} vs {j})'
    if len(ref_scores) < 2 or ref_scores[0] - ref_scores[1] > 2 * score_atol:
        assert list(got.tokens) == r_nbest[0], what


def frame_margins(logp: torch.Tensor):
    top2 = logp.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1])


# ---------------------------------------------------------------------------
# Margin-aware parity rules (north_star: identical CTC 1-best tokens for greedy,
# rescoring scores within 1e-3).  The reference's and the GPU's log-probs differ by
# fp32 summation order (<= LOGP_TOL); a frame whose reference top-1 margin is
# below FRAME_EPS may legitimately flip to the reference's second choice.  The
# rules are per FRAME, never per utterance, and every check reports how much it
# actually compared.
FRAME_EPS = 1e-3     # top-1 margin under which a frame may flip to the runner-up
LOGP_TOL = 2.5e-4    # |GPU - reference| on the top-k CTC log-probs (measured 4.8e-5 .. 6.6e-5
                     # on the BASELINE batches, r02a) -- FRAME_EPS = 4 x this
NBEST_TOL = 2e-3     # fp64 prefix-beam score, sum of ~T' log-probs
RESCORE_TOL = 1e-3   # north_star: attention-rescoring scores within 1e-3


def collapse(path, blank=0):
    """ctc_utils.remove_duplicates_and_blank (ctc_utils.py:23-33)."""
    out, prev = [], None
    for t in path:
        t = int(t)
        if t != prev and t != blank:
            out.append(t)
        prev = t
    return out


def greedy_frame_check(got_top1, ref_topk_idx, ref_topk_val, got_tokens, ref_tokens,
                       what='', eps=FRAME_EPS):
    """Per-frame greedy rule for ONE utterance.
    got_top1 [n] GPU arg-max per frame; ref_topk_idx/val [n][>=2] of the reference.
      * every frame with reference margin > eps: identical arg-max (strict);
      * a frame under eps: the GPU arg-max is the reference's top-1 or top-2;
      * the GPU token list is the collapse of its own arg-max path, and with no
        flipped frame it IS the reference's token list.
    Returns (n_frames, n_strict, n_flips)."""
    got_top1 = np.asarray(got_top1).astype(np.int64)
    idx = np.asarray(ref_topk_idx).astype(np.int64)
    val = np.asarray(ref_topk_val)
    n = len(got_top1)
    assert idx.shape[0] == n, (what, idx.shape, n)
    margin = val[:, 0] - val[:, 1]
    strict = margin > eps
    bad = strict & (got_top1 != idx[:, 0])
    assert not bad.any(), (f'{what}: arg-max differs on frames with reference margin > '
                           f'{eps}', np.nonzero(bad)[0][:8].tolist(),
                           margin[bad][:8].tolist())
    loose = ~strict
    ok2 = (got_top1 == idx[:, 0]) | (got_top1 == idx[:, 1])
    assert ok2[loose].all(), f'{what}: low-margin frame outside the reference top-2'
    flips = int((got_top1 != idx[:, 0]).sum())
    assert list(got_tokens) == collapse(got_top1), f'{what}: tokens != collapse(arg-max)'
    if flips == 0:
        assert list(got_tokens) == list(ref_tokens), f'{what}: greedy tokens differ'
    return n, int(strict.sum()), flips


def nbest_check(got, ref_nbest, ref_scores, ref_times, what='', tol=NBEST_TOL):
    """Prefix-beam n-best of one utterance against the reference's (from slightly
    different log-probs).  A reference hypothesis may be absent from the GPU list
    only if it sits within 2*tol of the reference's pruning edge (its last score);
    present ones must carry the reference's score (tol) and identical time stamps;
    the 1-best is the reference's unless the reference's top-2 gap is under 2*tol.
    Returns (n_ref_hyps, n_compared)."""
    g_nbest = [list(x) for x in got.nbest]
    r_nbest = [list(x) for x in ref_nbest]
    assert len(g_nbest) == len(r_nbest), (what, len(g_nbest), len(r_nbest))
    compared = 0
    for i, h in enumerate(r_nbest):
        if h not in g_nbest:
            assert ref_scores[i] - ref_scores[-1] < 2 * tol, \
                f'{what}: reference hyp #{i} missing, {ref_scores[i] - ref_scores[-1]:.2e} above the beam edge'
            continue
        j = g_nbest.index(h)
        assert abs(got.nbest_scores[j] - ref_scores[i]) < tol, \
            (what, i, got.nbest_scores[j], ref_scores[i])
        if ref_times is not None and len(ref_times) > i:
            assert list(got.nbest_times[j]) == list(ref_times[i]), (what, i)
        if j != i:
            lo, hi = min(i, j), max(i, j)
            assert abs(ref_scores[lo] - ref_scores[hi]) < 2 * tol, \
                f'{what}: order differs beyond tolerance ({i} vs {j})'
        compared += 1
    if len(ref_scores) < 2 or ref_scores[0] - ref_scores[1] > 2 * tol:
        assert list(got.tokens) == r_nbest[0], f'{what}: 1-best differs'
    else:
        assert list(got.tokens) in r_nbest[:2], f'{what}: 1-best outside the tied pair'
    return len(r_nbest), compared


def rescoring_check(got, got_pre, ref, ref_pre_nbest, what='', tol=RESCORE_TOL):
    """attention_rescoring of one utterance: the score of EVERY hypothesis both
    n-best lists hold within `tol` ABSOLUTE of the reference's
    (`ref['all_scores'][i]` belongs to `ref_pre_nbest[i]`); the winner is the
    reference's whenever the reference's top-2 rescoring gap exceeds 2*tol.
    Returns (n_hyps_compared, max_abs_err)."""
    g_nbest = [list(x) for x in got_pre.nbest]
    r_nbest = [list(x) for x in ref_pre_nbest]
    errs = []
    for i, h in enumerate(r_nbest):
        if h in g_nbest:
            errs.append(abs(got.all_scores[g_nbest.index(h)] - ref['all_scores'][i]))
    assert errs, f'{what}: no common hypothesis'
    assert max(errs) < tol, (f'{what}: rescoring score off by {max(errs):.3e}', errs)
    rs = sorted(ref['all_scores'], reverse=True)
    if len(rs) < 2 or rs[0] - rs[1] > 2 * tol:
        assert list(got.tokens) == list(ref['tokens']), f'{what}: rescoring winner differs'
        assert abs(got.score - ref['score']) < tol, (what, got.score, ref['score'])
    return len(errs), max(errs)


def pruning_tie_check(got, logp_b, beam, what='', tol=NBEST_TOL):
    """Fallback for an utterance whose n-best list differs from the reference's beyond the
    direct rules: the reference's search and the GPU's start from log-probs that differ by
    up to LOGP_TOL, so a pruning decision taken by a smaller margin may legitimately go the
    other way -- and everything downstream of it (which alignments a prefix's score sums)
    then differs by far more than the tolerance.  Accepted only if BOTH hold:
      * the GPU search is EXACT on its own inputs: the oracle's prefix beam search
        (search.py:127-249 restated) on the GPU's own log-probs reproduces the GPU n-best
        list -- tokens, order, time stamps, scores;
      * that search really passes through a near-tie: its smallest pruning margin is below
        2 x tol.
    Returns the margin."""
    from oracle import wenet_oracle as O
    import torch
    gaps = []
    lp = torch.as_tensor(logp_b, dtype=torch.float32).unsqueeze(0)
    ref = O.ctc_prefix_beam_search(lp, torch.tensor([lp.shape[1]]), beam, edge_gaps=gaps)[0]
    assert [list(x) for x in got.nbest] == [list(x) for x in ref.nbest], \
        f'{what}: GPU n-best differs from the oracle search on the GPU\'s own log-probs'
    for a, b in zip(got.nbest_scores, ref.nbest_scores):
        assert abs(a - b) < 1e-6 * max(1.0, abs(b)), (what, a, b)
    assert [list(x) for x in got.nbest_times] == [list(x) for x in ref.nbest_times], what
    assert gaps[0] < 2 * tol, (f'{what}: n-best differs from the reference although no '
                               f'pruning decision was closer than {gaps[0]:.2e}')
    return gaps[0]


def rescoring_attention_part_check(got, got_pre, ref, ref_pre_nbest, ref_pre_scores,
                                   ctc_weight, what='', tol=RESCORE_TOL):
    """rescoring_check for an utterance whose CTC prefix scores took the other side of a
    pruning tie (pruning_tie_check): the attention-decoder part of every common hypothesis'
    score -- score - ctc_weight * ctc_score -- within `tol` of the reference's."""
    g_nbest = [list(x) for x in got_pre.nbest]
    r_nbest = [list(x) for x in ref_pre_nbest]
    errs = []
    for i, h in enumerate(r_nbest):
        if h in g_nbest:
            j = g_nbest.index(h)
            errs.append(abs((got.all_scores[j] - ctc_weight * got_pre.nbest_scores[j]) -
                            (ref['all_scores'][i] - ctc_weight * ref_pre_scores[i])))
    assert errs, f'{what}: no common hypothesis'
    assert max(errs) < tol, (f'{what}: attention part of the rescoring score off by '
                             f'{max(errs):.3e}', errs)
    return len(errs), max(errs)


def rescore_replay(hyps_per_utt, ctc_scores_per_utt, l2r, r2l, ctc_weight, reverse_weight,
                   use_r2l):
    """The scalar tail of attention_rescoring (search.py:424-457) replayed on gathered
    per-token log-probs with the reference's dtypes (np.float32 scalars, left-to-right sums,
    Python floats rounded where they meet the fp32 tensor): the checker wn_rescore's reduce
    kernel must agree with BIT FOR BIT.  -> per utterance (best_index, all_scores fp32,
    confidences, tokens_confidences)."""
    import math
    f32 = np.float32
    out = []
    for b, hyps in enumerate(hyps_per_utt):
        best_score, best_index = -float('inf'), 0
        confs, tcs, scores = [], [], []
        for i, hyp in enumerate(hyps):
            L = len(hyp)
            s_l = l2r[b, i, :L + 1].astype(f32)
            score = f32(0.0)
            for j in range(L):
                score = f32(score + s_l[j])
            tc = [math.exp(float(s_l[j])) for j in range(L)]
            score = f32(score + s_l[L])
            if reverse_weight > 0 and use_r2l:
                s_r = r2l[b, i, :L + 1].astype(f32)
                r_score = f32(0.0)
                for j in range(L):
                    s = s_r[L - j - 1]
                    r_score = f32(r_score + s)
                    tc[j] = (tc[j] + math.exp(float(s))) / 2
                r_score = f32(r_score + s_r[L])
                score = f32(f32(score * f32(1 - reverse_weight)) +
                            f32(r_score * f32(reverse_weight)))
            confs.append(math.exp(float(f32(score / f32(L + 1)))))
            score = f32(score + f32(ctc_scores_per_utt[b][i] * ctc_weight))
            scores.append(score)
            if float(score) > best_score:
                best_score, best_index = float(score), i
            tcs.append(tc)
        out.append((best_index, scores, confs, tcs))
    return out
