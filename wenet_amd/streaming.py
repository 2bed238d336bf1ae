"""Streaming recognition: N independent sessions, each fed feature frames as they arrive,
each returning a partial result after every chunk and a final (optionally attention-rescored)
result at the end -- the reference runtime's streaming decoder
(runtime/core/decoder/asr_decoder.cc:87-132 AdvanceDecoding, :217-243 rescoring at the end;
ctc_prefix_beam_search.cc:84-186 Search() resuming from cur_hyps_; ctc_endpoint.cc:36-77) on
the chunk-cache encoder (`ASRModel.forward_encoder_chunk_batch`) and the resumable HIP prefix
beam search (`wn_stream_*`, csrc/ctc.hip).

Layers, bottom up:

* `StreamSearch`: a set of search sessions on the device (`wn_stream_create`), advanced by
  (n, T, V) log-probs or directly by encoder output;
* `ChunkWindower`: which feature windows a session has to run, a pure host-side restatement
  of `BaseEncoder.forward_chunk_by_chunk`'s loop (encoder.py:287-362) for frames that arrive
  in pieces;
* `CtcEndpointConfig` / `CtcEndpointRule` / `endpoint_rule`: the reference's endpoint rules
  evaluated on the host from the two counters the search kernel keeps;
* `RnntStreamSearch`: the same for a hybrid transducer -- resumable RNN-T greedy searches
  (`wn_rnnt_stream_create`, csrc/transducer_stream.hip), advanced by encoder output;
* `RnntBeamStreamSearch`: resumable RNN-T prefix beam searches (`wn_rnnt_beam_stream_create`,
  csrc/transducer_beam_stream.hip): an n-best per session after every chunk;
* `StreamingRecognizer`: open / accept / step / finish / close, with either search;
* `RnntBeamStreamingRecognizer`: the same on the resumable RNN-T prefix beam search, with the
  transducer + attention rescoring of the final beam in `finish`.
"""
import ctypes
from typing import Dict, List, Optional, Tuple

import numpy as np

from wenet_amd import _lib


# --------------------------------------------------------------------------- endpoint rules
class CtcEndpointRule:
    """ctc_endpoint.h:27-38 (times in ms)."""

    def __init__(self, must_decoded_sth: bool = True, min_trailing_silence: int = 1000,
                 min_utterance_length: int = 0):
        self.must_decoded_sth = must_decoded_sth
        self.min_trailing_silence = min_trailing_silence
        self.min_utterance_length = min_utterance_length


class CtcEndpointConfig:
    """ctc_endpoint.h:40-60: rule1 times out after 5000 ms of silence even if nothing was
    decoded, rule2 after 1000 ms of silence once something was decoded, rule3 when the
    utterance is 20000 ms long."""

    def __init__(self, blank: int = 0, blank_scale: float = 1.0, blank_threshold: float = 0.8,
                 rule1: Optional[CtcEndpointRule] = None,
                 rule2: Optional[CtcEndpointRule] = None,
                 rule3: Optional[CtcEndpointRule] = None):
        self.blank = blank
        self.blank_scale = blank_scale
        self.blank_threshold = blank_threshold
        self.rule1 = rule1 or CtcEndpointRule(False, 5000, 0)
        self.rule2 = rule2 or CtcEndpointRule(True, 1000, 0)
        self.rule3 = rule3 or CtcEndpointRule(False, 0, 20000)


def endpoint_rule(config: CtcEndpointConfig, frames_decoded: int, trailing_blank: int,
                  decoded_something: bool, frame_shift_ms: int) -> Optional[str]:
    """CtcEndpoint::IsEndpoint's rule arithmetic (ctc_endpoint.cc:36-46,62-77) on the two
    frame counters: the name of the first rule that fires, or None."""
    assert frame_shift_ms > 0 and frames_decoded >= trailing_blank >= 0
    utterance_length = frames_decoded * frame_shift_ms
    trailing_silence = trailing_blank * frame_shift_ms
    for name in ('rule1', 'rule2', 'rule3'):
        r = getattr(config, name)
        if ((decoded_something or not r.must_decoded_sth)
                and trailing_silence >= r.min_trailing_silence
                and utterance_length >= r.min_utterance_length):
            return name
    return None


# --------------------------------------------------------------------------- windowing
class ChunkWindower:
    """The feature windows of one streaming session.

    `forward_chunk_by_chunk` cuts an utterance of n frames into the windows
    `(cur, min(cur + window, n)) for cur in range(0, n - context + 1, stride)` with
    `stride = subsampling * chunk`, `context = right_context + 1`,
    `window = (chunk - 1) * subsampling + context`.  Here the frames arrive in pieces:
    `push(k)` announces k more frames, `pop()` gives the next FULL window once all of its
    frames are there (a full window is the same whatever n turns out to be), and
    `flush()` -- the utterance is over, n is known -- gives the remaining windows, the last
    one possibly shorter.  Frame indices are absolute; nothing here touches a tensor."""

    def __init__(self, chunk: int, subsampling: int, right_context: int):
        assert chunk > 0 and subsampling > 0 and right_context >= 0
        self.context = right_context + 1
        self.stride = subsampling * chunk
        self.window = (chunk - 1) * subsampling + self.context
        self.received = 0      # frames announced so far
        self.start = 0         # first frame of the next window
        self.finished = False

    def push(self, n_frames: int):
        assert not self.finished and n_frames >= 0
        self.received += n_frames

    def ready(self) -> bool:
        return not self.finished and self.start + self.window <= self.received

    def pop(self) -> Tuple[int, int]:
        assert self.ready()
        w = (self.start, self.start + self.window)
        self.start += self.stride
        return w

    def flush(self) -> List[Tuple[int, int]]:
        self.finished = True
        out = []
        while self.start + self.context <= self.received:
            out.append((self.start, min(self.start + self.window, self.received)))
            self.start += self.stride
        return out

    def keep_from(self) -> int:
        """Frames before this index are never needed again."""
        return self.start


# --------------------------------------------------------------------------- device search
class StreamSearch:
    """`n_slots` resumable CTC prefix beam searches on the device (wn_stream_create).

    `advance(slots, logp, n_t)` feeds session slots[i] the first n_t[i] rows of logp[i] and
    returns one DecodeResult per session for everything that session has consumed so far --
    what `search.ctc_prefix_beam_search` returns for those frames in one call.  With
    `nbest=False` only the 1-best is walked out of the node pools (tokens, times, score);
    `nbest=True` gives the whole list.  Extra attributes of every result: `viterbi_score`,
    `frames_decoded`, `trailing_blank`; `.raw` of the returned list holds the call's arrays."""

    def __init__(self, handle: int, device, n_slots: int, beam_size: int, max_frames: int,
                 blank_id: int = 0, blank_threshold: float = 0.8, blank_scale: float = 1.0):
        self._L = _lib.lib()
        self.device = device
        self.n_slots, self.beam, self.max_frames = n_slots, beam_size, max_frames
        self.frames = [0] * n_slots         # frames every slot has consumed
        self._set = None
        h = ctypes.c_void_p()
        _lib.check(self._L.wn_stream_create(handle, n_slots, beam_size, max_frames, blank_id,
                                            ctypes.byref(h), self._stream()),
                   'wn_stream_create')
        self._set = h
        _lib.check(self._L.wn_stream_set_endpoint(self._set, blank_threshold, blank_scale),
                   'wn_stream_set_endpoint')

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if self._set is not None:
            self._L.wn_stream_destroy(self._set)
            self._set = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def reset(self, slots):
        ids = np.asarray(list(slots), dtype=np.int32)
        _lib.check(self._L.wn_stream_reset(self._set, len(ids), _lib.i32p(ids), self._stream()),
                   'wn_stream_reset')
        for s in ids.tolist():
            self.frames[s] = 0

    def _outputs(self, slots, n_t):
        n, beam = len(slots), self.beam
        max_len = max([self.frames[s] + t for s, t in zip(slots, n_t)] + [1])
        a = dict(n_hyps=np.zeros((n, ), np.int32), hyp_lens=np.zeros((n, beam), np.int32),
                 hyp_tlens=np.zeros((n, beam), np.int32),
                 hyp_tokens=np.zeros((n, beam, max_len), np.int32),
                 hyp_times=np.zeros((n, beam, max_len), np.int32),
                 hyp_scores=np.zeros((n, beam), np.float64),
                 hyp_viterbi=np.zeros((n, beam), np.float64),
                 frames_decoded=np.zeros((n, ), np.int32),
                 trailing_blank=np.zeros((n, ), np.int32), max_len=max_len)
        r = _lib.WnStreamResult(
            _lib.i32p(a['n_hyps']), _lib.i32p(a['hyp_lens']), _lib.i32p(a['hyp_tlens']),
            _lib.i32p(a['hyp_tokens']), _lib.i32p(a['hyp_times']), _lib.f64p(a['hyp_scores']),
            _lib.f64p(a['hyp_viterbi']), _lib.i32p(a['frames_decoded']),
            _lib.i32p(a['trailing_blank']), max_len)
        return a, r

    def _results(self, slots, n_t, a):
        from wenet_amd.search import DecodeResult, _NBestBatch
        for s, t in zip(slots, n_t):
            self.frames[s] += int(t)
        batch = _NBestBatch(a['n_hyps'], a['hyp_lens'], a['hyp_tlens'], a['hyp_tokens'],
                            a['hyp_times'], a['hyp_scores'])
        out = _Results()
        for b in range(len(slots)):
            have = a['n_hyps'][b] > 0
            nl = int(a['hyp_lens'][b, 0]) if have else 0
            ntl = int(a['hyp_tlens'][b, 0]) if have else 0
            r = DecodeResult(tokens=tuple(a['hyp_tokens'][b, 0, :nl].tolist()),
                             score=float(a['hyp_scores'][b, 0]),
                             times=a['hyp_times'][b, 0, :ntl].tolist())
            r._lazy, r._b = batch, b
            r.viterbi_score = float(a['hyp_viterbi'][b, 0])
            r.frames_decoded = int(a['frames_decoded'][b])
            r.trailing_blank = int(a['trailing_blank'][b])
            out.append(r)
        out.raw = a
        return out

    def advance(self, slots, logp, n_t, nbest: bool = False):
        """logp: (n, T, V) float32 log-probs on the device."""
        assert logp.is_cuda and logp.dim() == 3 and logp.size(0) == len(slots)
        import torch
        logp = logp.detach().to(torch.float32).contiguous()
        ids = np.asarray(list(slots), dtype=np.int32)
        nt = np.asarray(list(n_t), dtype=np.int32)
        assert len(ids) == len(nt)
        a, r = self._outputs(ids.tolist(), nt.tolist())
        _lib.check(self._L.wn_stream_advance(
            self._set, len(ids), _lib.i32p(ids), logp.data_ptr(), _lib.i32p(nt), logp.size(1),
            logp.size(2), 1 if nbest else 0, ctypes.byref(r), self._stream()),
            'wn_stream_advance')
        return self._results(ids.tolist(), nt.tolist(), a)

    def advance_encoded(self, slots, enc_out, n_t=None, nbest: bool = False):
        """enc_out: (n, chunk, d_model) float32 encoder output on the device; the CTC head of
        the set's model runs in the same call."""
        assert enc_out.is_cuda and enc_out.dim() == 3 and enc_out.size(0) == len(slots)
        import torch
        enc_out = enc_out.detach().to(torch.float32).contiguous()
        ids = np.asarray(list(slots), dtype=np.int32)
        nt = np.asarray(list(n_t) if n_t is not None else [enc_out.size(1)] * len(ids),
                        dtype=np.int32)
        a, r = self._outputs(ids.tolist(), nt.tolist())
        _lib.check(self._L.wn_stream_advance_encoded(
            self._set, len(ids), _lib.i32p(ids), enc_out.data_ptr(), _lib.i32p(nt),
            enc_out.size(1), 1 if nbest else 0, ctypes.byref(r), self._stream()),
            'wn_stream_advance_encoded')
        return self._results(ids.tolist(), nt.tolist(), a)


class _Results(list):
    raw = None


class RnntStreamSearch:
    """`n_slots` resumable RNN-T greedy searches on the device (wn_rnnt_stream_create; the
    handle must be a `wenet_amd.Transducer`'s).

    `advance_encoded(slots, enc_out, n_t)` feeds session slots[i] the first n_t[i] frames of
    enc_out[i] and returns one DecodeResult per session for everything that session has
    consumed so far -- what `transducer.basic_greedy_search` returns for those frames in one
    call: `tokens`, `times` (the encoder frame of each token) and the extra attributes
    `frames_decoded`, `trailing_blank`; `.raw` of the returned list holds the call's arrays and
    `.steps` its lock-step steps.  `dims` = (predictor layers, hidden size, join_dim) is what
    `state(slot)` needs to size its arrays."""

    def __init__(self, handle: int, device, n_slots: int, max_frames: int, max_tokens: int,
                 n_steps: int = 64, dims=None):
        self._L = _lib.lib()
        self.device = device
        self.n_slots, self.max_frames, self.max_tokens = n_slots, max_frames, max_tokens
        self.n_steps, self.dims = n_steps, dims
        self.frames = [0] * n_slots         # frames every slot has consumed
        self.n_tok = [0] * n_slots          # tokens every slot has emitted
        self._set = None
        h = ctypes.c_void_p()
        _lib.check(self._L.wn_rnnt_stream_create(handle, n_slots, max_frames, max_tokens,
                                                 n_steps, ctypes.byref(h), self._stream()),
                   'wn_rnnt_stream_create')
        self._set = h

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if self._set is not None:
            self._L.wn_rnnt_stream_destroy(self._set)
            self._set = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def reset(self, slots):
        ids = np.asarray(list(slots), dtype=np.int32)
        _lib.check(self._L.wn_rnnt_stream_reset(self._set, len(ids), _lib.i32p(ids),
                                                self._stream()), 'wn_rnnt_stream_reset')
        for s in ids.tolist():
            self.frames[s] = self.n_tok[s] = 0

    def advance_encoded(self, slots, enc_out, n_t=None, max_len=None):
        """enc_out: (n, chunk, d_model) float32 encoder output on the device.  `max_len`: the
        row pitch of the result arrays (default: what the call can need)."""
        assert enc_out.is_cuda and enc_out.dim() == 3 and enc_out.size(0) == len(slots)
        import torch
        from wenet_amd.search import DecodeResult
        enc_out = enc_out.detach().to(torch.float32).contiguous()
        ids = np.asarray(list(slots), dtype=np.int32)
        nt = np.asarray(list(n_t) if n_t is not None else [enc_out.size(1)] * len(ids),
                        dtype=np.int32)
        assert len(ids) == len(nt)
        n = len(ids)
        if max_len is None:
            max_len = max([min(self.n_tok[s] + max(int(t), 0) * self.n_steps, self.max_tokens)
                           for s, t in zip(ids.tolist(), nt.tolist())
                           if 0 <= s < self.n_slots] + [1])
        a = dict(tok_lens=np.zeros((n, ), np.int32), tokens=np.zeros((n, max_len), np.int32),
                 times=np.zeros((n, max_len), np.int32),
                 frames_decoded=np.zeros((n, ), np.int32),
                 trailing_blank=np.zeros((n, ), np.int32), max_len=max_len,
                 steps=np.zeros((1, ), np.int32))
        r = _lib.WnRnntStreamResult(_lib.i32p(a['tok_lens']), _lib.i32p(a['tokens']),
                                    _lib.i32p(a['times']), _lib.i32p(a['frames_decoded']),
                                    _lib.i32p(a['trailing_blank']), max_len, _lib.i32p(a['steps']))
        st = self._L.wn_rnnt_stream_advance_encoded(
            self._set, n, _lib.i32p(ids), enc_out.data_ptr(), _lib.i32p(nt), enc_out.size(1),
            ctypes.byref(r), self._stream())
        if st != 0 and b'token buffer overflow' in self._L.wn_last_error():
            # the sessions did advance; the device keeps counting past max_tokens
            for s, t in zip(ids.tolist(), nt.tolist()):
                self.frames[s] += int(t)
                self.n_tok[s] = self.max_tokens
        _lib.check(st, 'wn_rnnt_stream_advance_encoded')
        out = _Results()
        for b, s in enumerate(ids.tolist()):
            self.frames[s] = int(a['frames_decoded'][b])
            self.n_tok[s] = nl = int(a['tok_lens'][b])
            res = DecodeResult(tokens=tuple(a['tokens'][b, :nl].tolist()),
                               times=a['times'][b, :nl].tolist())
            res.frames_decoded = int(a['frames_decoded'][b])
            res.trailing_blank = int(a['trailing_blank'][b])
            out.append(res)
        out.raw = a
        out.steps = int(a['steps'][0])
        return out

    def state(self, slot: int):
        """wn_rnnt_stream_state: (h, c (layers, H), pred_proj (J), dict of the counters)."""
        assert self.dims is not None, 'RnntStreamSearch.state needs dims=(layers, hidden, join_dim)'
        L_, H, J = self.dims
        h = np.zeros((L_, H), np.float32)
        c = np.zeros((L_, H), np.float32)
        pp = np.zeros((J, ), np.float32)
        sc = np.zeros((5, ), np.int32)
        _lib.check(self._L.wn_rnnt_stream_state(self._set, slot, _lib.f32p(h), _lib.f32p(c),
                                                _lib.f32p(pp), _lib.i32p(sc), self._stream()),
                   'wn_rnnt_stream_state')
        names = ('last_tok', 'stale', 'n_tok', 'frames', 'trailing_blank')
        return h, c, pp, dict(zip(names, sc.tolist()))


class RnntBeamStreamSearch:
    """`n_slots` resumable RNN-T prefix beam searches on the device
    (wn_rnnt_beam_stream_create; the handle must be a `wenet_amd.Transducer`'s).  The beam and
    the fusion weights of `transducer.prefix_beam_search` are fixed for the set.

    `advance_encoded(slots, enc_out, n_t)` feeds session slots[i] the first n_t[i] frames of
    enc_out[i] and returns one DecodeResult per session for everything that session has
    consumed so far -- what `transducer.prefix_beam_search` returns for those frames in one
    call: `tokens` and `score` of the best hypothesis, `nbest`, `nbest_scores`, and the extra
    attributes `frames_decoded`, `trailing_blank` (frames consumed behind the last token of the
    best hypothesis: this project's definition); `.raw` of the returned list holds the call's
    arrays.  `dims` = (predictor layers, hidden size, join_dim) is what `state(slot)` needs to
    size its arrays."""

    def __init__(self, handle: int, device, n_slots: int, beam_size: int, max_frames: int,
                 ctc_weight: float = 0.3, transducer_weight: float = 0.7, dims=None):
        self._L = _lib.lib()
        self.device = device
        self.n_slots, self.beam, self.max_frames = n_slots, int(beam_size), max_frames
        self.ctc_weight, self.transducer_weight = float(ctc_weight), float(transducer_weight)
        self.dims = dims
        self.frames = [0] * n_slots         # frames every slot has consumed
        self._set = None
        h = ctypes.c_void_p()
        _lib.check(self._L.wn_rnnt_beam_stream_create(
            handle, n_slots, self.beam, max_frames, self.ctc_weight, self.transducer_weight,
            ctypes.byref(h), self._stream()), 'wn_rnnt_beam_stream_create')
        self._set = h

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if self._set is not None:
            self._L.wn_rnnt_beam_stream_destroy(self._set)
            self._set = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def reset(self, slots):
        ids = np.asarray(list(slots), dtype=np.int32)
        _lib.check(self._L.wn_rnnt_beam_stream_reset(self._set, len(ids), _lib.i32p(ids),
                                                     self._stream()), 'wn_rnnt_beam_stream_reset')
        for s in ids.tolist():
            self.frames[s] = 0

    def advance_encoded(self, slots, enc_out, n_t=None, max_len=None):
        """enc_out: (n, chunk, d_model) float32 encoder output on the device.  `max_len`: the
        row pitch of the result arrays (default: what the call can need)."""
        assert enc_out.is_cuda and enc_out.dim() == 3 and enc_out.size(0) == len(slots)
        import torch
        from wenet_amd.search import DecodeResult
        enc_out = enc_out.detach().to(torch.float32).contiguous()
        ids = np.asarray(list(slots), dtype=np.int32)
        nt = np.asarray(list(n_t) if n_t is not None else [enc_out.size(1)] * len(ids),
                        dtype=np.int32)
        assert len(ids) == len(nt)
        n, beam = len(ids), self.beam
        if max_len is None:
            max_len = max([self.frames[s] + max(int(t), 0) for s, t in zip(ids.tolist(), nt.tolist())
                           if 0 <= s < self.n_slots] + [1])
        a = dict(n_hyps=np.zeros((n, ), np.int32), hyp_lens=np.zeros((n, beam), np.int32),
                 hyp_tokens=np.zeros((n, beam, max(max_len, 1)), np.int32),
                 hyp_scores=np.full((n, beam), -np.inf, np.float64),
                 frames_decoded=np.zeros((n, ), np.int32),
                 trailing_blank=np.zeros((n, ), np.int32), max_len=max_len)
        r = _lib.WnRnntBeamStreamResult(
            _lib.i32p(a['n_hyps']), _lib.i32p(a['hyp_lens']), _lib.i32p(a['hyp_tokens']),
            _lib.f64p(a['hyp_scores']), _lib.i32p(a['frames_decoded']),
            _lib.i32p(a['trailing_blank']), max_len)
        _lib.check(self._L.wn_rnnt_beam_stream_advance_encoded(
            self._set, n, _lib.i32p(ids), enc_out.data_ptr(), _lib.i32p(nt), enc_out.size(1),
            ctypes.byref(r), self._stream()), 'wn_rnnt_beam_stream_advance_encoded')
        out = _Results()
        for b, s in enumerate(ids.tolist()):
            self.frames[s] = int(a['frames_decoded'][b])
            nbest = [a['hyp_tokens'][b, k, :a['hyp_lens'][b, k]].tolist()
                     for k in range(int(a['n_hyps'][b]))]
            scores = a['hyp_scores'][b, :len(nbest)].tolist()
            res = DecodeResult(nbest[0], score=scores[0], nbest=nbest, nbest_scores=scores)
            res.frames_decoded = int(a['frames_decoded'][b])
            res.trailing_blank = int(a['trailing_blank'][b])
            out.append(res)
        out.raw = a
        return out

    def state(self, slot: int):
        """wn_rnnt_beam_stream_state: the session's whole state as a dict of host arrays:
        n_live, frames, score (beam), tok_len / last_tok / pending / last_time (beam), tokens
        (beam, max_frames), h / c (beam, layers, H), pred_proj (beam, J)."""
        assert self.dims is not None, 'RnntBeamStreamSearch.state needs dims=(layers, hidden, join_dim)'
        L_, H, J = self.dims
        beam = self.beam
        cnt = np.zeros((2, ), np.int32)
        score = np.zeros((beam, ), np.float64)
        ints = np.zeros((4, beam), np.int32)
        tokens = np.zeros((beam, self.max_frames), np.int32)
        h = np.zeros((beam, L_, H), np.float32)
        c = np.zeros((beam, L_, H), np.float32)
        pp = np.zeros((beam, J), np.float32)
        _lib.check(self._L.wn_rnnt_beam_stream_state(
            self._set, slot, _lib.i32p(cnt), _lib.f64p(score), _lib.i32p(ints), _lib.i32p(tokens),
            _lib.f32p(h), _lib.f32p(c), _lib.f32p(pp), self._stream()),
            'wn_rnnt_beam_stream_state')
        return dict(n_live=int(cnt[0]), frames=int(cnt[1]), score=score, tok_len=ints[0],
                    last_tok=ints[1], pending=ints[2], last_time=ints[3], tokens=tokens, h=h, c=c,
                    pred_proj=pp)


# --------------------------------------------------------------------------- recognizer
class _Session:
    __slots__ = ('slot', 'win', 'feats', 'base', 'att', 'cnn', 'offset', 'enc', 'last')

    def __init__(self, slot, win):
        self.slot, self.win = slot, win
        self.feats = None     # pending feature frames (k, mel) on the device ...
        self.base = 0         # ... the first of which is frame `base` of the utterance
        self.att = self.cnn = None
        self.offset = 0       # encoder frames emitted
        self.enc = []         # encoder output, chunk by chunk (the final rescoring's input)
        self.last = None      # the last partial result


class StreamingRecognizer:
    """Batched streaming recognition on one model.

        rec = StreamingRecognizer(model, n_sessions=16, decoding_chunk_size=16)
        sid = rec.open()
        rec.accept(sid, feats)          # any number of new (k, mel) frames, on the GPU
        partials = rec.step()           # {sid: DecodeResult} of the sessions that advanced
        final = rec.finish(sid)         # flushes the tail, n-best (+ attention rescoring)
        rec.close(sid)

    `step()` advances every session that has a full window by one chunk in ONE
    `forward_encoder_chunk_batch` and ONE search call; its results carry `is_endpoint`
    (the endpoint rule that fired, or None) next to the search's counters.  Only causal,
    chunk-trained Conformers are accepted (`ASRModel._check_simulate_streaming`).

    `search='ctc_prefix_beam_search'` (default) is the CTC prefix beam search above.
    `search='rnnt_greedy_search'` needs a `wenet_amd.Transducer` and runs the resumable RNN-T
    greedy search (`RnntStreamSearch`, at most `n_steps` symbols per frame): partial and final
    results are the greedy token lists with `times`; `beam_size` and `nbest` are not read,
    and attention `rescoring` is NOT applied in this mode (finish() ignores it).  The endpoint
    rules are fed with that search's counters: `trailing_blank` counts the frames consumed
    behind the frame of the last token (this project's definition: the reference has no RNN-T
    endpointing).  A session may store `max_tokens` tokens (default: 8 per encoder frame of
    `max_seconds`, fewer if n_steps is smaller); one that emits more raises and must be closed."""

    SEARCHES = ('ctc_prefix_beam_search', 'rnnt_greedy_search')

    def __init__(self, model, n_sessions: int, decoding_chunk_size: int,
                 num_decoding_left_chunks: int = -1, beam_size: int = 10,
                 max_seconds: float = 60.0, endpoint: Optional[CtcEndpointConfig] = None,
                 blank_id: int = 0, search: str = 'ctc_prefix_beam_search', n_steps: int = 64,
                 max_tokens: Optional[int] = None):
        if search not in self.SEARCHES:
            raise ValueError(f'search={search!r}: expected one of {self.SEARCHES}')
        self.rnnt = search == 'rnnt_greedy_search'
        max_frames = self._setup(model, n_sessions, decoding_chunk_size, num_decoding_left_chunks,
                                 max_seconds, endpoint, blank_id, search if self.rnnt else None)
        if self.rnnt:
            tc = model._tcfg
            if max_tokens is None:
                max_tokens = max_frames * min(n_steps, 8)
            self.search = RnntStreamSearch(model._h, model.device, n_sessions, max_frames,
                                           max_tokens, n_steps,
                                           dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))
        else:
            self.search = StreamSearch(model._h, model.device, n_sessions, beam_size, max_frames,
                                       blank_id, self.endpoint.blank_threshold,
                                       self.endpoint.blank_scale)

    def _setup(self, model, n_sessions, decoding_chunk_size, num_decoding_left_chunks,
               max_seconds, endpoint, blank_id, transducer_search):
        """Everything of __init__ but the search object; returns max_frames.
        transducer_search: the name of a search that needs a `wenet_amd.Transducer`, or None."""
        import torch
        assert decoding_chunk_size > 0, 'decoding_chunk_size must be positive'
        if transducer_search is not None:
            from wenet_amd.transducer import Transducer
            if not isinstance(model, Transducer):
                raise TypeError(f"search='{transducer_search}' needs a wenet_amd.Transducer, got "
                                f'{type(model).__name__}')
        model._check_simulate_streaming(torch.empty((1, 0, 0)))
        ctx = getattr(model, '_ctx_graph', None)
        if ctx is not None:
            raise NotImplementedError('context biasing is not supported in streaming '
                                      'sessions (its finalize() mutates the beam)')
        self.model = model
        self.chunk = decoding_chunk_size
        self.required = decoding_chunk_size * num_decoding_left_chunks
        self.subsampling = model.subsampling_rate()
        self.right_context = model.right_context()
        self.endpoint = endpoint or CtcEndpointConfig(blank=blank_id)
        self.frame_shift_ms = 10 * self.subsampling
        self._free = list(range(n_sessions - 1, -1, -1))
        self._sessions: Dict[int, _Session] = {}
        self._next_sid = 0
        return int(np.ceil(max_seconds * 1000.0 / self.frame_shift_ms)) + decoding_chunk_size

    # ---- session life cycle
    def open(self) -> int:
        if not self._free:
            raise RuntimeError('StreamingRecognizer: every session slot is in use')
        slot = self._free.pop()
        self.search.reset([slot])
        sid = self._next_sid
        self._next_sid += 1
        self._sessions[sid] = _Session(
            slot, ChunkWindower(self.chunk, self.subsampling, self.right_context))
        return sid

    def close(self, sid: int):
        s = self._sessions.pop(sid)
        self._free.append(s.slot)

    def accept(self, sid: int, feats):
        """feats: (k, mel) float32 feature frames on the device, k >= 0."""
        import torch
        s = self._sessions[sid]
        assert feats.is_cuda and feats.dim() == 2, 'accept: (frames, mel) on the GPU'
        feats = feats.detach().to(torch.float32)
        s.feats = feats if s.feats is None else torch.cat([s.feats, feats], 0)
        s.win.push(feats.size(0))

    # ---- decoding
    def _run(self, sids: List[int], windows, nbest: bool):
        """One encoder chunk call + one search call for sessions whose windows have one length."""
        import torch
        ss = [self._sessions[i] for i in sids]
        xs = torch.stack([s.feats[a - s.base:b - s.base] for s, (a, b) in zip(ss, windows)])
        ys, att, cnn = self.model.forward_encoder_chunk_batch(
            xs, [s.offset for s in ss], self.required, [s.att for s in ss],
            [s.cnn for s in ss])
        if self.rnnt:
            res = self.search.advance_encoded([s.slot for s in ss], ys)
        else:
            res = self.search.advance_encoded([s.slot for s in ss], ys, nbest=nbest)
        for b, s in enumerate(ss):
            s.att, s.cnn = att[b], cnn[b]
            s.offset += ys.size(1)
            s.enc.append(ys[b])
            keep = s.win.keep_from()
            if keep > s.base:
                s.feats = s.feats[keep - s.base:]
                s.base = keep
            r = res[b]
            r.is_endpoint = endpoint_rule(self.endpoint, r.frames_decoded, r.trailing_blank,
                                          len(r.tokens) > 0, self.frame_shift_ms)
            s.last = r
        return res

    def step(self, nbest: bool = False) -> Dict[int, object]:
        sids = [i for i, s in self._sessions.items() if s.win.ready()]
        if not sids:
            return {}
        windows = [self._sessions[i].win.pop() for i in sids]
        res = self._run(sids, windows, nbest)
        return dict(zip(sids, res))

    def encoder_out(self, sid: int):
        """(1, T', d_model): the encoder output session `sid` has produced so far."""
        import torch
        s = self._sessions[sid]
        d = self.model._cfg.d_model
        if not s.enc:
            return torch.zeros((1, 0, d), dtype=torch.float32, device=self.model.device)
        return torch.cat(s.enc, 0).unsqueeze(0)

    def finish(self, sid: int, rescoring: bool = True, ctc_weight: float = 0.5,
               reverse_weight: float = 0.0):
        """No more frames for `sid`: run the windows that are left (the last may be shorter),
        return the n-best like `ctc_prefix_beam_search`, attention-rescored when asked for and
        the model has a decoder.  The session stays open (closed by `close`) but takes no more
        frames.  With search='rnnt_greedy_search' the result is the greedy token list of the
        whole utterance; rescoring is not applied."""
        import torch
        from wenet_amd import search
        s = self._sessions[sid]
        res = None
        for w in s.win.flush():
            res = self._run([sid], [w], True)[0]
        if self.rnnt:
            if res is None:
                # nothing left to run: what has been consumed (an n_t = 0 advance)
                d = self.model._cfg.d_model
                res = self.search.advance_encoded(
                    [s.slot], torch.zeros((1, 1, d), dtype=torch.float32,
                                          device=self.model.device), [0])[0]
                res.is_endpoint = s.last.is_endpoint if s.last is not None else None
            return res
        if res is None:
            # nothing left to run: the n-best of what has been consumed (an n_t = 0 advance)
            V = self.model.vocab_size
            res = self.search.advance(
                [s.slot], torch.zeros((1, 1, V), dtype=torch.float32, device=self.model.device),
                [0], nbest=True)[0]
            res.is_endpoint = s.last.is_endpoint if s.last is not None else None
        if rescoring and self.model._cfg.dec_layers > 0 and s.offset > 0:
            enc = self.encoder_out(sid)
            out = search.attention_rescoring(
                self.model, [res], enc, torch.tensor([enc.size(1)], dtype=torch.int32),
                ctc_weight, reverse_weight)[0]
            out.is_endpoint = res.is_endpoint
            return out
        return res


class RnntBeamStreamingRecognizer(StreamingRecognizer):
    """`StreamingRecognizer` on the resumable RNN-T prefix beam search (`RnntBeamStreamSearch`):
    the same open / accept / step / finish / close / encoder_out on a `wenet_amd.Transducer`.

        rec = RnntBeamStreamingRecognizer(model, n_sessions=16, decoding_chunk_size=16,
                                          beam_size=5)

    Every partial result is the n-best `transducer.prefix_beam_search` gives for the frames so
    far (`tokens`, `score`, `nbest`, `nbest_scores`), fused with the CTC head's log-probs by
    `search_ctc_weight` / `search_transducer_weight`.  The endpoint rules read
    `trailing_blank` = the frames consumed behind the last token of the best hypothesis (this
    project's definition: the reference has no RNN-T endpointing).  A separate class, not a
    third entry of `StreamingRecognizer.SEARCHES`: the constructor and `finish` take the
    transducer's arguments."""

    SEARCH = 'rnnt_prefix_beam_search'

    def __init__(self, model, n_sessions: int, decoding_chunk_size: int,
                 num_decoding_left_chunks: int = -1, beam_size: int = 5,
                 search_ctc_weight: float = 0.3, search_transducer_weight: float = 0.7,
                 max_seconds: float = 60.0, endpoint: Optional[CtcEndpointConfig] = None,
                 blank_id: int = 0):
        self.rnnt = True          # (_run: the search takes no `nbest` switch)
        max_frames = self._setup(model, n_sessions, decoding_chunk_size, num_decoding_left_chunks,
                                 max_seconds, endpoint, blank_id, self.SEARCH)
        tc = model._tcfg
        self.beam_size = int(beam_size)
        self.search_ctc_weight = float(search_ctc_weight)
        self.search_transducer_weight = float(search_transducer_weight)
        self.search = RnntBeamStreamSearch(model._h, model.device, n_sessions, self.beam_size,
                                           max_frames, self.search_ctc_weight,
                                           self.search_transducer_weight,
                                           dims=(tc.pred_layers, tc.pred_hidden, tc.join_dim))

    def finish(self, sid: int, rescoring: bool = True, attn_weight: float = 0.0,
               transducer_weight: float = 0.0, ctc_weight: float = 0.0,
               reverse_weight: float = 0.0):
        """No more frames for `sid`: run the windows that are left (the last may be shorter) and
        return the final beam.  With `rescoring` on a model with a decoder, the beam is rescored
        as `Transducer.transducer_attention_rescoring` rescores the one-shot search's (per
        hypothesis attn * attn_weight + beam score * ctc_weight + td * transducer_weight; the
        defaults are that method's) on the session's encoder output, WITHOUT running the search
        again: `tokens` / `score` of the winner, `nbest` in search order, `nbest_scores` the
        rescored score of each.  The session stays open (closed by `close`) but takes no more
        frames."""
        import torch
        from wenet_amd import transducer
        s = self._sessions[sid]
        res = None
        for w in s.win.flush():
            res = self._run([sid], [w], True)[0]
        if res is None:
            # nothing left to run: the beam of what has been consumed (an n_t = 0 advance)
            d = self.model._cfg.d_model
            res = self.search.advance_encoded(
                [s.slot], torch.zeros((1, 1, d), dtype=torch.float32, device=self.model.device),
                [0])[0]
            res.is_endpoint = s.last.is_endpoint if s.last is not None else None
        if rescoring and self.model._cfg.dec_layers > 0 and s.offset > 0:
            if reverse_weight > 0.0:
                assert self.model._cfg.dec_r_layers > 0
            enc = self.encoder_out(sid)
            self.model._set_encoder_out(enc, torch.tensor([enc.size(1)], dtype=torch.int32))
            out = transducer._rescore_current(
                self.model, [list(zip(res.nbest, res.nbest_scores))], reverse_weight, ctc_weight,
                attn_weight, transducer_weight)[0]
            out.is_endpoint = res.is_endpoint
            out.frames_decoded, out.trailing_blank = res.frames_decoded, res.trailing_blank
            return out
        return res
