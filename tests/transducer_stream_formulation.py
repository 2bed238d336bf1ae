"""NumPy fp64 restatement of the resumable RNN-T greedy search (wenet_amd/csrc/transducer_stream.hip,
wn_rnnt_stream_*): `lookahead_greedy_search` of tests/transducer_formulation.py for ONE session
that receives its encoder frames in pieces.

State that survives a call: the LSTM's h / c, the projected predictor output pred_proj, the last
token, `stale` (pred_proj does not belong to last_tok yet), the tokens with the absolute encoder
frame of each, the frames consumed and the trailing-blank count.

A call with n_t > 0 frames runs the one-shot rule over its frames 0 .. n_t - 1.  The one-shot
search drops the predictor step behind a token that the n_steps cap emits on the LAST frame
(nothing follows there); here a later call may follow, so that case sets `stale` and the next
call with frames runs the step first.  A call ends only after a blank or a cap, so the
symbols-per-frame counter is 0 at every boundary and is not part of the state.
"""
import numpy as np

import transducer_formulation as TF


class StreamSession:
    def __init__(self, W, blank, n_steps=64, lookahead=4, stale_step=True):
        """stale_step=False: the variant that forgets the predictor step behind a token emitted by
        the cap on a call's last frame (what the one-shot kernel may do, wrong here)."""
        self.W, self.blank, self.n_steps, self.F = W, blank, n_steps, lookahead
        self.stale_step = stale_step
        self.L, self.H = len(W['rnn']), W['rnn'][0][1].shape[1]
        self.J = W['pred_ffn'][0].shape[0]
        self.boundary_cnt = []      # the symbols-per-frame counter at the end of every call
        self.steps = 0              # lock-step steps of the last call
        self.reset()

    def reset(self):
        self.h = np.zeros((self.L, 1, self.H))
        self.c = np.zeros((self.L, 1, self.H))
        self.pred_proj = np.zeros((self.J, ))
        self.last_tok, self.stale = self.blank, 1
        self.tokens, self.times = [], []
        self.frames = 0
        self.trailing_blank = 0

    def _predictor(self):
        out, self.h, self.c = TF.predictor_step([self.last_tok], self.h, self.c, self.W)
        self.pred_proj = (out @ self.W['pred_ffn'][0].T + self.W['pred_ffn'][1])[0]

    def advance(self, chunk, on_row=None):
        """chunk: (n_t, d) encoder frames.  on_row(t_abs, h_row, logits_row) for every joint row
        that takes part in a decision.  Returns the tokens so far."""
        chunk = np.asarray(chunk, dtype=np.float64)
        n_t = chunk.shape[0]
        self.steps = 0
        if n_t == 0:
            return list(self.tokens)
        W = self.W
        enc_proj = chunk @ W['enc_ffn'][0].T + W['enc_ffn'][1]
        t = cnt = 0
        advance, self.stale = bool(self.stale), 0
        bound = n_t * (self.n_steps + 1) + 1
        while t < n_t:
            assert self.steps < bound, 'the call ran past its step bound'
            self.steps += 1
            if advance:
                self._predictor()
            advance = False
            n = min(self.F, n_t - t)
            hrows = np.tanh(enc_proj[t:t + n] + self.pred_proj)
            logits = hrows @ W['ffn_out'][0].T + W['ffn_out'][1]
            best = TF.argmax_rows(logits)
            nb = [f for f in range(n) if best[f] != self.blank]
            if on_row is not None:
                for f in range(n if not nb else nb[0] + 1):
                    on_row(self.frames + t + f, hrows[f], logits[f])
            if not nb:
                t += n
                cnt = 0
                continue
            f = nb[0]
            if f > 0:
                cnt = 0
            t += f
            self.tokens.append(int(best[f]))
            self.times.append(self.frames + t)
            cnt += 1
            capped = cnt >= self.n_steps
            if capped:
                t += 1
                cnt = 0
            self.last_tok = int(best[f])
            if t < n_t:
                advance = True
            else:
                # only the cap moves t past the last frame behind a token
                assert capped
                self.stale = 1 if self.stale_step else 0
        self.boundary_cnt.append(cnt)
        self.frames += n_t
        self.trailing_blank = self.frames - 1 - self.times[-1] if self.times else self.frames
        return list(self.tokens)


def pieces(total, split):
    """The lengths of the calls that feed `total` frames with `split` repeated cyclically (a 0 in
    the split is an empty call)."""
    out, fed, i = [], 0, 0
    while fed < total:
        n = min(split[i % len(split)], total - fed)
        out.append(n)
        fed += n
        i += 1
    return out


def run_session(enc, n_frames, W, blank, n_steps, lookahead, split, stale_step=True,
                on_row=None):
    """One utterance's (T', d) encoder output through a session in the pieces of `split`.
    Returns (session, the token list after every call)."""
    s = StreamSession(W, blank, n_steps, lookahead, stale_step)
    after, at = [], 0
    for n in pieces(n_frames, split):
        after.append(s.advance(enc[at:at + n], on_row))
        at += n
    return s, after
