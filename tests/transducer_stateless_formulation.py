"""NumPy fp64 restatement of the reference's two stateless predictors -- EmbeddingPredictor and
ConvPredictor, wenet/models/transducer/predictor.py:209-495 -- followed by joint.pred_ffn: what
rnnt_stateless_step (wenet_amd/csrc/transducer_stateless.hip) is checked against on the GPU
(tests/test_gpu_transducer_stateless.py) and, on the CPU, against the reference's recorded steps,
token lists and beams (tests/test_transducer_stateless_formulation.py,
tests/golden/rnnt/rnnt_stateless_tiny.npz).

A stateless predictor's output is a function of the last C = history_size + 1 tokens of
[blank] + hypothesis, the window; before the leading blank the reference's history is zero
vectors, written here as the id -1.

`weights64` returns a dict the existing formulation searches (transducer_formulation.
lookahead_greedy_search, transducer_beam_formulation.prefix_beam_search) run on unchanged: they
keep a predictor "state" h of shape (L, B, H) that they zero, copy and gather but never look
into.  Here L = 1, H = C and h[0, b] holds the window of row b as id + 1 (so the zero state is
the all -1 window); importing this module wraps transducer_formulation.predictor_step so that
such a dict takes this predictor instead of the LSTM.  Every other dict goes to the LSTM step as
before.
"""
import numpy as np

import transducer_formulation as TF

KINDS = {'embedding': 1, 'conv': 2}


def weights64(sd, configs):
    """predictor.* / joint.* of a state dict (name -> array-like) of a `predictor: embedding` or
    `predictor: conv` configuration as fp64 arrays."""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)   # noqa: E731
    pc = configs['predictor_conf']
    kind = configs['predictor']
    E, C = pc['embed_size'], pc.get('history_size', 2) + 1
    W = dict(stateless=kind, context=C, embed=g('predictor.embed.weight'),
             eps=float(pc.get('layer_norm_epsilon', 1e-5)),
             act=pc.get('activation', 'swish' if kind == 'embedding' else 'relu'),
             norm=(g('predictor.norm.weight'), g('predictor.norm.bias')),
             enc_ffn=(g('joint.enc_ffn.weight'), g('joint.enc_ffn.bias')),
             pred_ffn=(g('joint.pred_ffn.weight'), g('joint.pred_ffn.bias')),
             ffn_out=(g('joint.ffn_out.weight'), g('joint.ffn_out.bias')))
    if kind == 'embedding':
        W['heads'] = pc['n_head']
        # (pos_embed.bias, if the state dict has one, is never read: predictor.py:308, :355)
        W['pos'] = g('predictor.pos_embed.weight').reshape(pc['n_head'], E, C)
        W['ffn'] = (g('predictor.ffn.weight'), g('predictor.ffn.bias'))
    else:
        W['conv'] = g('predictor.conv.weight').reshape(E, C)
        W['conv_bias'] = g('predictor.conv.bias') if pc.get('bias', False) else None
    # what the searches read of an LSTM dict: L = len(rnn), H = rnn[0][1].shape[1],
    # P = proj[0].shape[0]
    W['rnn'] = [(None, np.zeros((1, C)), None, None)]
    W['proj'] = (np.zeros((E, 1)), None)
    return W


def windows(hyps, C, blank):
    """The window of every hypothesis (token lists without the leading blank): (M, C) ids, oldest
    first, the last C of [-1] * C + [blank] + hyp."""
    return np.asarray([([-1] * C + [blank] + [int(t) for t in h])[-C:] for h in hyps],
                      dtype=np.int64).reshape(len(hyps), C)


def predictor_out(ctx, W):
    """forward_step of either predictor for the windows ctx (M, C): (M, E)."""
    ctx = np.asarray(ctx, dtype=np.int64)
    C = W['context']
    assert ctx.ndim == 2 and ctx.shape[1] == C
    dt = W['embed'].dtype
    x = np.where((ctx >= 0)[..., None], W['embed'][np.maximum(ctx, 0)], dt.type(0))   # (M, C, E)
    if W['stateless'] == 'embedding':
        w = np.einsum('mce,hec->mhc', x, W['pos'])
        mix = np.einsum('mc,mce->me', w.sum(axis=1), x) / dt.type(W['heads'] * C)
        y = mix @ W['ffn'][0].T + W['ffn'][1]
    else:
        y = np.einsum('mce,ec->me', x, W['conv'])
        if W['conv_bias'] is not None:
            y = y + W['conv_bias']
    mean = y.mean(axis=1, keepdims=True)
    var = ((y - mean) ** 2).mean(axis=1, keepdims=True)
    y = (y - mean) / np.sqrt(var + dt.type(W['eps'])) * W['norm'][0] + W['norm'][1]
    if W['act'] == 'swish':
        return y / (1.0 + np.exp(-y))
    assert W['act'] == 'relu'
    return np.maximum(y, 0.0)


def pred_proj(ctx, W):
    """joint.pred_ffn of the predictor output: the row of pred_proj (M, J)."""
    return predictor_out(ctx, W) @ W['pred_ffn'][0].T + W['pred_ffn'][1]


def cast(W, dtype):
    """The weight dict with every array in `dtype` (the fp32 restatement of the GPU tests)."""
    def conv(v):
        if isinstance(v, np.ndarray):
            return v.astype(dtype)
        if isinstance(v, tuple):
            return tuple(conv(u) for u in v)
        return v
    return {k: (v if k in ('rnn', 'proj') else conv(v)) for k, v in W.items()}


_lstm_step = TF.predictor_step


def _predictor_step(tokens, h, c, W):
    """transducer_formulation.predictor_step for both kinds of dict (module docstring)."""
    if 'stateless' not in W:
        return _lstm_step(tokens, h, c, W)
    win = np.concatenate([h[0, :, 1:], np.asarray(tokens, dtype=np.float64).reshape(-1, 1) + 1.0],
                         axis=1)
    return predictor_out(np.rint(win).astype(np.int64) - 1, W), win[None], c


if getattr(TF.predictor_step, '__name__', '') != '_predictor_step':
    TF.predictor_step = _predictor_step
