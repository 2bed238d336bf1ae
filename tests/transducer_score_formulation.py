"""NumPy fp64 restatement of the teacher-forced transducer score
(wenet_amd/csrc/transducer_score.hip, rnnt_trie.h) and of the score combination of
Transducer.transducer_attention_rescoring (wenet/models/transducer/transducer.py:262-396): the
prefix trie of an utterance's hypotheses, the predictor run over the trie, the joint log-probs
gathered at a node's blank and child columns, Graves' forward algorithm over the lattice and the
weighted sum.  What the kernels are checked against on the GPU (tests/test_gpu_transducer_score.py)
and, on the CPU, against the reference's recorded scores (tests/test_transducer_score_formulation.py,
tests/golden/rnnt/rnnt_rescore_tiny.npz).

The score is pinned to the published definition (Graves 2012): with lp = log_softmax of the joint
logits of (frame t, prefix y[:u]),
    alpha(0, 0) = 0
    alpha(t, u) = log_add(alpha(t-1, u) + lp(t-1, u)[blank], alpha(t, u-1) + lp(t, u-1)[y[u-1]])
    log P(y | x) = alpha(T-1, U) + lp(T-1, U)[blank]
"""
import numpy as np

import transducer_formulation as TF


def build_trie(hyps, blank):
    """Prefix trie of token lists.  Node 0 is the empty prefix; nodes are in level order, within
    a level in order of first appearance over the hypotheses in their given order.  Returns a
    dict: parent, token, depth, slot (place of the node's token in its parent's column list),
    paths (per hypothesis its len + 1 node ids), col_off / cols (per node: blank, then its
    children's tokens in node order)."""
    parent, token, depth, slot, kids = [-1], [blank], [0], [0], [[]]
    cur = [0] * len(hyps)
    paths = [[0] for _ in hyps]
    for d in range(1, max([len(h) for h in hyps] + [0]) + 1):
        for k, h in enumerate(hyps):
            if len(h) < d:
                continue
            tok, p = int(h[d - 1]), cur[k]
            c = next((i for i in kids[p] if token[i] == tok), None)
            if c is None:
                c = len(parent)
                parent.append(p); token.append(tok); depth.append(d)
                slot.append(len(kids[p]) + 1)
                kids[p].append(c)
                kids.append([])
            cur[k] = c
            paths[k].append(c)
    col_off, cols = [0], []
    for i in range(len(parent)):
        cols += [blank] + [token[c] for c in kids[i]]
        col_off.append(len(cols))
    return dict(parent=parent, token=token, depth=depth, slot=slot, paths=paths,
                col_off=col_off, cols=cols)


def trie_pred_proj(trie, W):
    """joint.pred_ffn(predictor(prefix)) of every node, (N, J): a node steps the LSTM from its
    parent's state on its own token (node 0: on the blank, from the zero state) -- the last
    output of RNNPredictor.forward on [blank] + prefix."""
    L, H = len(W['rnn']), W['rnn'][0][1].shape[1]
    N = len(trie['parent'])
    hs, cs, out = [None] * N, [None] * N, []
    for i in range(N):              # parents precede children
        p = trie['parent'][i]
        h = np.zeros((L, 1, H)) if p < 0 else hs[p]
        c = np.zeros((L, 1, H)) if p < 0 else cs[p]
        o, hs[i], cs[i] = TF.predictor_step([trie['token'][i]], h, c, W)
        out.append(o[0] @ W['pred_ffn'][0].T + W['pred_ffn'][1])
    return np.stack(out)


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def gathered_logp(enc_proj, pred_proj, trie, W):
    """(T, entries): for every frame the log-probs of every node at its listed columns, in the
    order of trie['cols']."""
    T, N = enc_proj.shape[0], pred_proj.shape[0]
    ent_node = np.repeat(np.arange(N), np.diff(trie['col_off']))
    cols = np.asarray(trie['cols'])
    out = np.empty((T, len(cols)))
    for t in range(T):
        lp = log_softmax(TF.joint_logits(enc_proj[t][None, :], pred_proj, W))     # (N, V)
        out[t] = lp[ent_node, cols]
    return out


def log_add(a, b):
    """wenet/utils/common.py:302-310 for two values; two -inf give -inf."""
    if a == -np.inf and b == -np.inf:
        return -np.inf
    m, n = (a, b) if a > b else (b, a)
    return m + np.log(1.0 + np.exp(n - m))


def lattice(lp_blank, lp_label):
    """Forward algorithm: lp_blank (T, U + 1), lp_label (T, U) -> log P.  T == 0: -inf."""
    lp_blank = np.asarray(lp_blank, dtype=np.float64)
    T, U1 = lp_blank.shape
    if T == 0:
        return -np.inf
    lp_label = np.asarray(lp_label, dtype=np.float64).reshape(T, U1 - 1)
    alpha = np.full((T, U1), -np.inf)
    alpha[0, 0] = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(T):
            for u in range(U1):
                if t == 0 and u == 0:
                    continue
                x = alpha[t - 1, u] + lp_blank[t - 1, u] if t > 0 else -np.inf
                y = alpha[t, u - 1] + lp_label[t, u - 1] if u > 0 else -np.inf
                alpha[t, u] = log_add(x, y)
    return float(alpha[T - 1, U1 - 1] + lp_blank[T - 1, U1 - 1])


def lattice_emissions(logp, trie, k):
    """The two emission arrays of hypothesis k out of gathered_logp's (T, entries)."""
    path = trie['paths'][k]
    off = trie['col_off']
    ub = [off[n] for n in path]
    ul = [off[path[u]] + trie['slot'][path[u + 1]] for u in range(len(path) - 1)]
    return logp[:, ub], logp[:, ul]


def transducer_scores(enc, hyps, W, blank):
    """-RNN-T loss of every hypothesis of one utterance: enc (T, d) encoder rows."""
    enc = np.asarray(enc, dtype=np.float64)
    if enc.shape[0] == 0:
        return [-np.inf] * len(hyps)
    trie = build_trie(hyps, blank)
    enc_proj = enc @ W['enc_ffn'][0].T + W['enc_ffn'][1]
    logp = gathered_logp(enc_proj, trie_pred_proj(trie, W), trie, W)
    return [lattice(*lattice_emissions(logp, trie, k)) for k in range(len(hyps))]


def combine(attn, beam_score, td, attn_weight, ctc_weight, transducer_weight):
    """transducer.py:389-394: (index of the first maximum, every hypothesis' score); a NaN never
    wins."""
    scores = [float(attn[i]) * attn_weight + float(beam_score[i]) * ctc_weight
              + float(td[i]) * transducer_weight for i in range(len(attn))]
    best, best_score = 0, -np.inf
    for i, s in enumerate(scores):
        if s > best_score:
            best, best_score = i, s
    return best, scores
