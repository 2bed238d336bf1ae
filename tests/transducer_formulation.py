"""NumPy fp64 restatement of the batched RNN-T greedy search with frame lookahead
(wenet_amd/csrc/transducer.hip): the LSTM predictor step, the joint network and the advance
rule, in lock-step over a batch.  What the kernels are checked against on the GPU
(tests/test_gpu_transducer.py) and, on the CPU, against the reference's recorded token lists
(tests/test_transducer_formulation.py, tests/golden/rnnt/rnnt_tiny.npz).

The reference (greedy_search.py:6-54) walks one utterance a symbol at a time.  The joint output
depends on the predictor only through pred_out, which changes only when a non-blank symbol is
emitted, so the next F frames can be evaluated under the current pred_out at once; the window is
consumed up to and including its first non-blank frame.
"""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def weights64(sd, n_layers):
    """predictor.* / joint.* of a state dict (name -> array-like) as fp64 arrays."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)   # noqa: E731
    return dict(
        embed=g('predictor.embed.weight'),
        rnn=[(g(f'predictor.rnn.weight_ih_l{l}'), g(f'predictor.rnn.weight_hh_l{l}'),
              g(f'predictor.rnn.bias_ih_l{l}'), g(f'predictor.rnn.bias_hh_l{l}'))
             for l in range(n_layers)],
        proj=(g('predictor.projection.weight'), g('predictor.projection.bias')),
        enc_ffn=(g('joint.enc_ffn.weight'), g('joint.enc_ffn.bias')),
        pred_ffn=(g('joint.pred_ffn.weight'), g('joint.pred_ffn.bias')),
        ffn_out=(g('joint.ffn_out.weight'), g('joint.ffn_out.bias')))


def lstm_step(x, h, c, rnn):
    """One time step of torch.nn.LSTM (gate order i, f, g, o).  x (B, E); h, c (L, B, H).
    Returns (top layer's h, new h, new c)."""
    h, c = h.copy(), c.copy()
    inp = x
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(rnn):
        H = w_hh.shape[1]
        gates = inp @ w_ih.T + b_ih + h[l] @ w_hh.T + b_hh
        i, f = sigmoid(gates[:, :H]), sigmoid(gates[:, H:2 * H])
        g, o = np.tanh(gates[:, 2 * H:3 * H]), sigmoid(gates[:, 3 * H:])
        c[l] = f * c[l] + i * g
        h[l] = o * np.tanh(c[l])
        inp = h[l]
    return inp, h, c


def predictor_step(tokens, h, c, W):
    """RNNPredictor.forward_step (predictor.py:185-206): (out (B, P), h, c)."""
    top, h, c = lstm_step(W['embed'][np.asarray(tokens)], h, c, W['rnn'])
    return top @ W['proj'][0].T + W['proj'][1], h, c


def joint_logits(enc_proj_rows, pred_proj_rows, W):
    """TransducerJoint.forward behind its prejoin linears (joint.py:84-92): rows (M, J)."""
    return np.tanh(enc_proj_rows + pred_proj_rows) @ W['ffn_out'][0].T + W['ffn_out'][1]


def argmax_rows(logits):
    """The arg-max rule of the search, torch.argmax's: the lowest index among equal maxima, and
    a NaN counts as larger than any number, so a row with NaNs returns its FIRST NaN (a row of
    nothing but NaNs returns 0).  The result is therefore always a column in [0, V) -- the
    kernels must keep it so, because the winning index is the row of the embedding table that
    the predictor reads next.  (np.argmax follows the same rule.)"""
    logits = np.asarray(logits)
    out = np.empty(logits.shape[0], dtype=np.int64)
    for r, row in enumerate(logits):
        nan = np.flatnonzero(np.isnan(row))
        out[r] = nan[0] if nan.size else np.flatnonzero(row == row.max())[0]
    return out


def dot_bound(hrow, logits, w_out, J):
    """The fp32 dot-product bound of the top-two gap of one joint row:
    (J + 2) 2^-24 (sum_k |h_k| (|W[i,k]| + |W[j,k]|) + 2 max|logit|)."""
    order = np.argsort(-logits, kind='stable')
    i, j = int(order[0]), int(order[1])
    gap = float(logits[i] - logits[j])
    bound = (J + 2) * 2.0 ** -24 * (float(np.abs(hrow) @ (np.abs(w_out[i]) + np.abs(w_out[j])))
                                    + 2.0 * float(np.abs(logits).max()))
    return gap, bound


def lookahead_greedy_search(enc, enc_lens, W, blank, n_steps=64, lookahead=4, on_row=None):
    """Lock-step search over a padded (B, T', d) encoder output.  Returns (token lists, steps).
    on_row(b, t, h_row, logits_row): called for every joint row that takes part in a decision
    (frame t of utterance b under its current predictor output)."""
    enc = np.asarray(enc, dtype=np.float64)
    lens = [int(v) for v in np.asarray(enc_lens).reshape(-1)]
    B = enc.shape[0]
    L, H = len(W['rnn']), W['rnn'][0][1].shape[1]
    enc_proj = enc @ W['enc_ffn'][0].T + W['enc_ffn'][1]
    h = np.zeros((L, B, H)); c = np.zeros((L, B, H))
    P, J = W['proj'][0].shape[0], W['pred_ffn'][0].shape[0]
    pred_proj = np.zeros((B, J))
    t = [0] * B; cnt = [0] * B
    last = [blank] * B
    advance = [n > 0 for n in lens]
    hyps = [[] for _ in range(B)]
    steps = 0
    bound = max(lens + [0]) * (n_steps + 1) + 1
    while any(t[b] < lens[b] for b in range(B)):
        assert steps < bound, 'the search ran past its step bound'
        steps += 1
        out, h2, c2 = predictor_step(last, h, c, W)
        pp2 = out @ W['pred_ffn'][0].T + W['pred_ffn'][1]
        for b in range(B):          # rows without `advance` keep their state
            if advance[b]:
                h[:, b], c[:, b], pred_proj[b] = h2[:, b], c2[:, b], pp2[b]
        for b in range(B):
            advance[b] = False
            if t[b] >= lens[b]:
                continue
            n = min(lookahead, lens[b] - t[b])
            hrows = np.tanh(enc_proj[b, t[b]:t[b] + n] + pred_proj[b])
            logits = hrows @ W['ffn_out'][0].T + W['ffn_out'][1]
            best = argmax_rows(logits)
            nb = [f for f in range(n) if best[f] != blank]
            if on_row is not None:
                for f in range(n if not nb else nb[0] + 1):
                    on_row(b, t[b] + f, hrows[f], logits[f])
            if not nb:
                t[b] += n; cnt[b] = 0
                continue
            f = nb[0]
            if f > 0:
                cnt[b] = 0
            t[b] += f
            hyps[b].append(int(best[f]))
            cnt[b] += 1
            if cnt[b] >= n_steps:
                t[b] += 1; cnt[b] = 0
            last[b] = int(best[f])
            advance[b] = t[b] < lens[b]
    return hyps, steps
