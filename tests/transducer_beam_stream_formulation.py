"""NumPy fp64 restatement of the resumable RNN-T prefix beam search
(wenet_amd/csrc/transducer_beam_stream.hip, wn_rnnt_beam_stream_*): one session whose encoder
frames arrive in pieces.

The state of a session is what the kernels keep in a slot between calls: the live hypotheses in
rank order with their scores, and per hypothesis the last token, `pending` (the predictor step on
the last token is still owed), `last_time` (the absolute frame of its last token, -1: none) and
the predictor state (h, c, joint.pred_ffn row).  `advance(rows)` consumes the next frames with
transducer_beam_formulation.ref_beam_step, one frame per step, plus the carry rule: on the last
frame of a call the one-shot step hands no state on (`more` is false: nothing follows); here a
later call may follow, so the new slots take their source slots' state as on any other frame and
a slot that appended a token is marked `pending` -- the next call with frames runs that step
first.  (ref_beam_step is asked with one frame more than the call has, which makes it answer
`src` / `advance` as usual on the call's last frame; that frame's `advance` is the `pending`.)

The search is causal, so after any calls the beam equals
transducer_beam_formulation.prefix_beam_search on the frames consumed so far.
`drop_pending=True` is the variant that forgets the owed step, as the one-shot kernel does on an
utterance's last frame: a wrong search once a token lands on the last frame of a call.
"""
import numpy as np

import transducer_beam_formulation as BF
import transducer_formulation as TF


class BeamSession:
    def __init__(self, W, blank, beam, cw, tw, score_dtype=np.float64, drop_pending=False):
        self.W, self.blank, self.beam, self.cw, self.tw = W, blank, beam, cw, tw
        self.score_dtype, self.drop_pending = score_dtype, drop_pending
        self.L, self.H = len(W['rnn']), W['rnn'][0][1].shape[1]
        self.J = W['pred_ffn'][0].shape[0]
        self.reset()

    def reset(self):
        """What rnnt_beam_init gives an utterance: [] with score 0.0 on a zero state, the
        predictor's first step (blank) owed."""
        self.hyps = [([], 0.0)]
        self.frames = 0
        self.last_tok = [self.blank]
        self.pending = [1]
        self.last_time = [-1]
        self.state = [(np.zeros((self.L, 1, self.H)), np.zeros((self.L, 1, self.H)),
                       np.zeros((1, self.J)))]
        self.events = []      # per consumed frame: dict(frame, appended, n_fused, last_of_call)

    def _step_state(self, st, token):
        out, h, c = TF.predictor_step([token], st[0], st[1], self.W)
        return h, c, out @ self.W['pred_ffn'][0].T + self.W['pred_ffn'][1]

    def advance(self, rows, ctc_rows=None):
        """rows (k, d): the next k encoder frames; ctc_rows (k, V): their CTC log-probs (cw > 0).
        k == 0 changes nothing.  Returns the beam."""
        W, beam, blank = self.W, self.beam, self.blank
        rows = np.asarray(rows, dtype=np.float64)
        k = rows.shape[0]
        if k == 0:
            return self.result()
        enc_proj = rows @ W['enc_ffn'][0].T + W['enc_ffn'][1]
        # begin: the steps the previous call owed
        for j in range(len(self.hyps)):
            if self.pending[j]:
                self.state[j] = self._step_state(self.state[j], self.last_tok[j])
                self.pending[j] = 0
        for f in range(k):
            top_val, top_idx = [], []
            for j in range(len(self.hyps)):
                logits = TF.joint_logits(enc_proj[f], self.state[j][2][0], W)
                crow = None if self.cw == 0 else ctc_rows[f]
                _, val, idx = BF.ref_fuse_topk(logits, crow, self.cw, self.tw, beam)
                top_val.append(list(val) + [BF.NEG_INF] * (beam - len(val)))
                top_idx.append(list(idx))
            trace = []
            # lens = k + 1: `src` and `advance` as on a frame that another one follows
            new, src, tok, adv, _ = BF.ref_beam_step([self.hyps], [top_val], [top_idx], f, [k + 1],
                                                     blank, beam, self.score_dtype, trace)
            last = f + 1 == k
            state, last_tok, pending, last_time = [], [], [], []
            for s in range(len(new[0])):
                sj = int(src[0, s])
                appended = bool(adv[0, s])
                st = self.state[sj]
                if appended and not last:
                    st = self._step_state(st, int(tok[0, s]))
                state.append(st)
                last_tok.append(int(tok[0, s]))
                pending.append(1 if appended and last and not self.drop_pending else 0)
                last_time.append(self.frames + f if appended else self.last_time[sj])
            self.events.append(dict(frame=self.frames + f, appended=int(adv[0].sum()),
                                    n_fused=trace[0]['n_fused'], last_of_call=last))
            self.hyps = [(list(h), s) for h, s in new[0]]
            self.state, self.last_tok, self.pending, self.last_time = (state, last_tok, pending,
                                                                       last_time)
        self.frames += k
        return self.result()

    def result(self):
        """[(tokens, score), ...], best first."""
        return [(list(h), s) for h, s in self.hyps]

    def trailing_blank(self):
        """Frames consumed behind the last token of the best hypothesis; all of them without one."""
        return self.frames - 1 - self.last_time[0]


def run_splits(enc_rows, ctc_rows, split, W, blank, beam, cw, tw, score_dtype=np.float64,
               drop_pending=False, after=None):
    """Feed one utterance's frames (T', d) to a BeamSession in pieces: `split` is cycled until
    the frames are used up (a 0 is an empty call).  after(session, frames so far): called behind
    every call.  Returns the session."""
    s = BeamSession(W, blank, beam, cw, tw, score_dtype, drop_pending)
    t, i, n = 0, 0, len(enc_rows)
    while t < n:
        k = min(split[i % len(split)], n - t)
        i += 1
        s.advance(enc_rows[t:t + k], None if ctc_rows is None else ctc_rows[t:t + k])
        t += k
        if after is not None:
            after(s, t)
    return s
