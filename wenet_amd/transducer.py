"""The hybrid transducer (`model: transducer`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * Transducer.greedy_search                  wenet/models/transducer/transducer.py:398-442
  * basic_greedy_search                       wenet/models/transducer/search/greedy_search.py:6-54
  * Transducer.beam_search                    wenet/models/transducer/transducer.py:216-260
  * PrefixBeamSearch.prefix_beam_search       transducer/search/prefix_beam_search.py:42-148
  * RNNPredictor / TransducerJoint            transducer/predictor.py:60-206, joint.py:62-92
  * how init_model builds the model           wenet/utils/init_model.py:137-154

The reference decodes one utterance and one symbol at a time; here the whole batch runs in
lock-step on the GPU with a frame lookahead (csrc/transducer.hip), for any batch size, with the
same token lists.  The prefix beam search likewise runs the batch in lock-step, one frame per
step (csrc/transducer_beam.hip); a fused hypothesis' score is log_add of the two, which is what
the reference's prefix fusion means to compute (its call raises a TypeError).
The encoder, the CTC head and the attention decoder are the ones of `ASRModel`, so its decode
modes and `align` work on a `Transducer` unchanged.
"""
import copy
import ctypes
from typing import Dict, List, Tuple

import numpy as np
import torch

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml
from wenet_amd.search import DecodeResult, _stream_ptr

RNNT_METHOD = 'rnnt_greedy_search'   # wenet/bin/recognize.py:86
RNNT_BEAM_METHOD = 'rnnt_beam_search'


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the transducer kernels need {want!r})')


def transducer_config_from_yaml(configs: dict):
    """train.yaml dict of a `model: transducer` recipe -> (wn_config, wn_transducer_config): the
    encoder / decoder keys as `config_from_yaml` reads them for an `asr_model`, and the
    predictor and joint widths.
    Has kernels: `predictor: rnn` with an LSTM and biases, `joint: transducer_joint` with
    prejoin linears, 'add', tanh, no postjoin linear and no HAT head; anything else is refused."""
    model_type = configs.get('model', 'asr_model')
    if model_type != 'transducer':
        _refuse('model', model_type, 'transducer')
    pred = configs.get('predictor', 'rnn')
    if pred != 'rnn':          # 'embedding' / 'conv' predictors (predictor.py:209-)
        _refuse('predictor', pred, 'rnn')
    joint = configs.get('joint', 'transducer_joint')
    if joint != 'transducer_joint':
        _refuse('joint', joint, 'transducer_joint')
    pc = configs.get('predictor_conf') or {}
    jc = configs.get('joint_conf') or {}
    for k, want in (('rnn_type', 'lstm'), ('bias', True)):      # RNNPredictor defaults
        if pc.get(k, want) != want:
            _refuse(f'predictor_conf.{k}', pc.get(k), want)
    for k, want in (('joint_mode', 'add'), ('prejoin_linear', True), ('postjoin_linear', False),
                    ('activation', 'tanh'), ('hat_joint', False)):   # TransducerJoint defaults
        if jc.get(k, want) != want:
            _refuse(f'joint_conf.{k}', jc.get(k), want)
    for k in ('embed_size', 'output_size', 'hidden_size', 'num_layers'):
        if k not in pc:
            raise KeyError(f'predictor_conf.{k}')
    as_asr = copy.copy(configs)
    as_asr['model'] = 'asr_model'
    c = config_from_yaml(as_asr)
    if c.encoder_type != 0:
        _refuse('encoder', configs.get('encoder'), 'conformer')
    if jc.get('enc_output_size', c.d_model) != c.d_model:
        _refuse('joint_conf.enc_output_size', jc.get('enc_output_size'), c.d_model)
    if jc.get('pred_output_size', pc['output_size']) != pc['output_size']:
        _refuse('joint_conf.pred_output_size', jc.get('pred_output_size'), pc['output_size'])
    join_dim = jc['join_dim']
    if join_dim % 32 != 0 or not 32 <= join_dim <= 1024:
        _refuse('joint_conf.join_dim', join_dim, 'a multiple of 32 in [32, 1024]')
    for k in ('embed_size', 'output_size', 'hidden_size'):
        if not 1 <= pc[k] <= 1024:
            _refuse(f'predictor_conf.{k}', pc[k], 'at most 1024')
    tc = _lib.WnTransducerConfig()
    tc.pred_embed = pc['embed_size']
    tc.pred_hidden = pc['hidden_size']
    tc.pred_layers = pc['num_layers']
    tc.pred_out = pc['output_size']
    tc.join_dim = join_dim
    # init_model.py:137-160: the blank of the CTC head and of the transducer is one id
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    tc.blank = st.get('<blank>', (configs.get('ctc_conf') or {}).get('ctc_blank_id', 0))
    return c, tc


def _search_current(model, B: int, max_frames: int, n_steps: int):
    """wn_transducer_greedy_search on the handle's current batch -> (token lists, steps)."""
    max_len = max(max_frames, 1) * n_steps
    tokens = np.empty((B, max_len), dtype=np.int32)
    lens = np.zeros((B, ), dtype=np.int32)
    steps = ctypes.c_int32(0)
    _lib.check(
        model._L.wn_transducer_greedy_search(model._h, n_steps, _lib.i32p(tokens),
                                             _lib.i32p(lens), max_len, ctypes.byref(steps),
                                             _stream_ptr(model.device)),
        'wn_transducer_greedy_search')
    model.last_rnnt_steps = int(steps.value)
    return [tokens[b, :lens[b]].tolist() for b in range(B)]


def basic_greedy_search(model, encoder_out: torch.Tensor, encoder_out_lens,
                        n_steps: int = 64) -> List[List[int]]:
    """greedy_search.py:6-54 on a caller's padded (B, T', d) encoder output, any B."""
    lens = torch.as_tensor(encoder_out_lens).reshape(-1)
    B, Tp = model._set_encoder_out(encoder_out, lens)
    return _search_current(model, B, Tp, n_steps)


def _beam_current(model, B: int, max_frames: int, beam_size: int, ctc_weight: float,
                  transducer_weight: float):
    """wn_transducer_beam_search on the handle's current batch -> per utterance the n-best
    [(tokens, score), ...] in rank order."""
    beam_size = int(beam_size)
    max_len = max(max_frames, 1)        # one symbol per frame at most
    n_hyps = np.zeros((B, ), dtype=np.int32)
    lens = np.zeros((B, max(beam_size, 1)), dtype=np.int32)
    tokens = np.empty((B, max(beam_size, 1), max_len), dtype=np.int32)
    scores = np.empty((B, max(beam_size, 1)), dtype=np.float64)
    _lib.check(
        model._L.wn_transducer_beam_search(model._h, beam_size, float(ctc_weight),
                                           float(transducer_weight), _lib.i32p(n_hyps),
                                           _lib.i32p(lens), _lib.i32p(tokens), _lib.f64p(scores),
                                           max_len, _stream_ptr(model.device)),
        'wn_transducer_beam_search')
    steps, adv = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.check(model._L.wn_transducer_beam_stats(model._h, ctypes.byref(steps), ctypes.byref(adv)),
               'wn_transducer_beam_stats')
    model.last_rnnt_steps = int(steps.value)
    model.last_rnnt_advance_rows = int(adv.value)
    return [[(tokens[b, k, :lens[b, k]].tolist(), float(scores[b, k]))
             for k in range(n_hyps[b])] for b in range(B)]


def prefix_beam_search(model, encoder_out: torch.Tensor, encoder_out_lens, beam_size: int = 5,
                       ctc_weight: float = 0.3, transducer_weight: float = 0.7
                       ) -> List[List[Tuple[List[int], float]]]:
    """prefix_beam_search.py:66-148 on a caller's padded (B, T', d) encoder output, any B: the
    final beam of every utterance as [(tokens, score), ...], best first, tokens without the
    leading blank."""
    lens = torch.as_tensor(encoder_out_lens).reshape(-1)
    B, Tp = model._set_encoder_out(encoder_out, lens)
    return _beam_current(model, B, Tp, beam_size, ctc_weight, transducer_weight)


def _beam_results(nbest) -> List[DecodeResult]:
    return [DecodeResult(u[0][0], score=u[0][1], nbest=[t for t, _ in u],
                         nbest_scores=[s for _, s in u]) for u in nbest]


class Transducer(ASRModel):
    """Hybrid transducer + CTC + attention model with the reference's inference API."""

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        super().__init__(configs, state_dict, device)
        self.blank = self._tcfg.blank
        self.last_rnnt_steps = 0     # lock-step steps of the last transducer search
        self.last_rnnt_advance_rows = 0   # beam search: rows that ran the LSTM step, all steps

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._tcfg = transducer_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_transducer(ctypes.byref(self._cfg), ctypes.byref(self._tcfg),
                                            tensors, n, self.device.index, ctypes.byref(h))

    def greedy_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor,
                      decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                      simulate_streaming: bool = False, n_steps: int = 64) -> List[List[int]]:
        """transducer.py:398-442, for any batch size."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        _ = simulate_streaming      # (the reference ignores it here too)
        speech, lens = self._prep(speech, speech_lengths)
        _, enc_lens, _ = self._encode(speech, lens, decoding_chunk_size,
                                      num_decoding_left_chunks, False)
        return _search_current(self, speech.shape[0], int(enc_lens.max()), n_steps)

    def beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor,
                    decoding_chunk_size: int = -1, beam_size: int = 5,
                    num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                    ctc_weight: float = 0.3, transducer_weight: float = 0.7
                    ) -> Tuple[List[List[int]], List[float]]:
        """transducer.py:216-260, for any batch size: (token lists, scores), one entry per
        utterance -- the best hypothesis of its final beam.  The reference takes one utterance
        and returns that utterance's single pair (`best_hyp, best_score`); with B == 1 that is
        `(out[0][0], out[1][0])` here."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        _ = simulate_streaming
        speech, lens = self._prep(speech, speech_lengths)
        _, enc_lens, _ = self._encode(speech, lens, decoding_chunk_size,
                                      num_decoding_left_chunks, False)
        nbest = _beam_current(self, speech.shape[0], int(enc_lens.max()), beam_size, ctc_weight,
                              transducer_weight)
        return [u[0][0] for u in nbest], [u[0][1] for u in nbest]

    def decode(self, methods: List[str], speech: torch.Tensor, speech_lengths: torch.Tensor,
               beam_size: int = 1, decoding_chunk_size: int = -1,
               num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
               simulate_streaming: bool = False, reverse_weight: float = 0.0,
               context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
               length_penalty: float = 0.0, infos=None, n_steps: int = 64,
               search_ctc_weight: float = 0.3, search_transducer_weight: float = 0.7
               ) -> Dict[str, List[DecodeResult]]:
        """ASRModel.decode, which additionally knows 'rnnt_greedy_search' and 'rnnt_beam_search':
        one encoder pass serves every requested mode.  The beam search takes `beam_size` and its
        fusion weights `search_ctc_weight` / `search_transducer_weight`; `ctc_weight` stays the
        rescoring weight and is not read by it.  Its results carry `tokens`, `score`, `nbest`
        and `nbest_scores`."""
        others = [m for m in methods if m not in (RNNT_METHOD, RNNT_BEAM_METHOD)]
        st = self._decode_begin(others, speech, speech_lengths, beam_size, decoding_chunk_size,
                                num_decoding_left_chunks, simulate_streaming, context_graph,
                                blank_id, blank_penalty)
        results = {}
        if RNNT_METHOD in methods:
            # first: the search reads the encoder output, which the non-blank filter of
            # attention_rescoring may replace
            B, enc_lens = st['B'], st['enc_lens']
            toks = _search_current(self, B, int(enc_lens.max()) if B > 0 else 0, n_steps)
            results[RNNT_METHOD] = [DecodeResult(t) for t in toks]
        if RNNT_BEAM_METHOD in methods:      # (before _decode_end, for the same reason)
            B, enc_lens = st['B'], st['enc_lens']
            results[RNNT_BEAM_METHOD] = _beam_results(_beam_current(
                self, B, int(enc_lens.max()) if B > 0 else 0, beam_size, search_ctc_weight,
                search_transducer_weight))
        results.update(self._decode_end(st, ctc_weight, reverse_weight, length_penalty, infos))
        return results
