"""The hybrid transducer (`model: transducer`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * Transducer.greedy_search                  wenet/models/transducer/transducer.py:398-442
  * basic_greedy_search                       wenet/models/transducer/search/greedy_search.py:6-54
  * Transducer.beam_search                    wenet/models/transducer/transducer.py:216-260
  * PrefixBeamSearch.prefix_beam_search       transducer/search/prefix_beam_search.py:42-148
  * Transducer.transducer_attention_rescoring wenet/models/transducer/transducer.py:262-396
  * _cal_transducer_score / _cal_attn_score   wenet/models/transducer/transducer.py:161-214
  * RNNPredictor / TransducerJoint            transducer/predictor.py:60-206, joint.py:62-92
  * EmbeddingPredictor / ConvPredictor        transducer/predictor.py:209-495
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
RNNT_RESCORE_METHOD = 'rnnt_beam_attn_rescoring'


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
    if c.encoder_type != 0 or configs.get('encoder', 'conformer') != 'conformer':
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


STATELESS_PREDICTORS = {'embedding': 1, 'conv': 2}      # wn_stateless_predictor_config.kind


def stateless_transducer_config_from_yaml(configs: dict):
    """train.yaml dict of a `model: transducer` recipe with `predictor: embedding` or
    `predictor: conv` (predictor.py:209-495) -> (wn_config, wn_transducer_config,
    WnStatelessPredictorConfig).  The encoder / decoder keys and the joint are read as
    `transducer_config_from_yaml` reads them; the handle has pred_embed == pred_out ==
    embed_size and no LSTM layers.  Has kernels: swish or relu, a window of at most 16 tokens,
    at most 16 heads, embed_size at most 1024; anything else is refused."""
    model_type = configs.get('model', 'asr_model')
    if model_type != 'transducer':
        _refuse('model', model_type, 'transducer')
    pred = configs.get('predictor', 'rnn')
    if pred not in STATELESS_PREDICTORS:
        _refuse('predictor', pred, 'embedding or conv')
    joint = configs.get('joint', 'transducer_joint')
    if joint != 'transducer_joint':
        _refuse('joint', joint, 'transducer_joint')
    pc = configs.get('predictor_conf') or {}
    jc = configs.get('joint_conf') or {}
    for k, want in (('joint_mode', 'add'), ('prejoin_linear', True), ('postjoin_linear', False),
                    ('activation', 'tanh'), ('hat_joint', False)):   # TransducerJoint defaults
        if jc.get(k, want) != want:
            _refuse(f'joint_conf.{k}', jc.get(k), want)
    for k in ('embed_size', 'output_size') + (('n_head', ) if pred == 'embedding' else ()):
        if k not in pc:
            raise KeyError(f'predictor_conf.{k}')
    embed = pc['embed_size']
    if pc['output_size'] != embed:      # predictor.py:230 / :392 assert it
        _refuse('predictor_conf.output_size', pc['output_size'], embed)
    if not 1 <= embed <= 1024:
        _refuse('predictor_conf.embed_size', embed, 'at most 1024')
    act = pc.get('activation', 'swish' if pred == 'embedding' else 'relu')
    if act not in ('swish', 'relu'):
        _refuse('predictor_conf.activation', act, 'swish or relu')
    history = pc.get('history_size', 2)
    if not 0 <= history <= 15:
        _refuse('predictor_conf.history_size', history, 'at most 15 (a window of 16 tokens)')
    heads = pc['n_head'] if pred == 'embedding' else 1
    if not 1 <= heads <= 16:
        _refuse('predictor_conf.n_head', heads, 'at most 16')
    as_asr = copy.copy(configs)
    as_asr['model'] = 'asr_model'
    c = config_from_yaml(as_asr)
    if c.encoder_type != 0 or configs.get('encoder', 'conformer') != 'conformer':
        _refuse('encoder', configs.get('encoder'), 'conformer')
    if jc.get('enc_output_size', c.d_model) != c.d_model:
        _refuse('joint_conf.enc_output_size', jc.get('enc_output_size'), c.d_model)
    if jc.get('pred_output_size', embed) != embed:
        _refuse('joint_conf.pred_output_size', jc.get('pred_output_size'), embed)
    join_dim = jc['join_dim']
    if join_dim % 32 != 0 or not 32 <= join_dim <= 1024:
        _refuse('joint_conf.join_dim', join_dim, 'a multiple of 32 in [32, 1024]')
    tc = _lib.WnTransducerConfig()
    tc.pred_embed = tc.pred_out = embed
    tc.pred_hidden = tc.pred_layers = 0
    tc.join_dim = join_dim
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    tc.blank = st.get('<blank>', (configs.get('ctc_conf') or {}).get('ctc_blank_id', 0))
    sc = _lib.WnStatelessPredictorConfig()
    sc.kind = STATELESS_PREDICTORS[pred]
    sc.context = history + 1
    sc.heads = heads
    sc.activation = 0 if act == 'swish' else 1
    sc.conv_bias = int(pred == 'conv' and bool(pc.get('bias', False)))
    sc.norm_eps = pc.get('layer_norm_epsilon', 1e-5)
    return c, tc, sc


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


def _hyp_arrays(hyps: List[List[List[int]]]):
    """Per-utterance lists of token lists -> (beam, n_hyps, hyp_lens, hyp_tokens, max_len) laid
    out as wn_rescore / wn_transducer_score read them."""
    B = len(hyps)
    beam = max(max((len(u) for u in hyps), default=0), 1)
    max_len = max(max((len(h) for u in hyps for h in u), default=0), 1)
    n_hyps = np.zeros((B, ), dtype=np.int32)
    lens = np.zeros((B, beam), dtype=np.int32)
    tokens = np.zeros((B, beam, max_len), dtype=np.int32)
    for b, u in enumerate(hyps):
        n_hyps[b] = len(u)
        for i, h in enumerate(u):
            lens[b, i] = len(h)
            tokens[b, i, :len(h)] = np.asarray(h, dtype=np.int32).reshape(-1)
    return beam, n_hyps, lens, tokens, max_len


def _score_current(model, hyps: List[List[List[int]]]) -> List[List[float]]:
    """wn_transducer_score on the handle's current batch: per utterance the -RNN-T loss of each
    of its hypotheses (fp64)."""
    beam, n_hyps, lens, tokens, max_len = _hyp_arrays(hyps)
    td = np.empty((len(hyps), beam), dtype=np.float64)
    _lib.check(
        model._L.wn_transducer_score(model._h, beam, _lib.i32p(n_hyps), _lib.i32p(lens),
                                     _lib.i32p(tokens), max_len, _lib.f64p(td),
                                     _stream_ptr(model.device)), 'wn_transducer_score')
    rows, unshared, nodes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
    _lib.check(model._L.wn_transducer_score_stats(model._h, ctypes.byref(rows),
                                                  ctypes.byref(unshared), ctypes.byref(nodes)),
               'wn_transducer_score_stats')
    model.last_rnnt_score_rows = (int(rows.value), int(unshared.value), int(nodes.value))
    return [td[b, :n_hyps[b]].tolist() for b in range(len(hyps))]


def transducer_score(model, encoder_out: torch.Tensor, encoder_out_lens,
                     hyps: List[List[List[int]]]) -> List[List[float]]:
    """Transducer._cal_transducer_score (transducer.py:161-186) on a caller's padded (B, T', d)
    encoder output, any B: per utterance the -RNN-T loss of each of its hypotheses (token lists
    without the leading blank), fp64.  An utterance of zero frames scores -inf."""
    lens = torch.as_tensor(encoder_out_lens).reshape(-1)
    B, _ = model._set_encoder_out(encoder_out, lens)
    if len(hyps) != B:
        raise ValueError(f'transducer_score: {len(hyps)} n-bests for a batch of {B} utterances')
    return _score_current(model, hyps)


def _attn_scores_current(model, hyps: List[List[List[int]]], reverse_weight: float):
    """The attention decoder's score of every hypothesis (transducer.py:188-214 + :376-387)
    through wn_rescore with explicit host hypotheses and ctc_weight = 0: its all_scores."""
    beam, n_hyps, lens, tokens, max_len = _hyp_arrays(hyps)
    B = len(hyps)
    best = np.zeros((B, ), dtype=np.int32)
    score = np.zeros((B, ), dtype=np.float32)
    all_scores = np.zeros((B, beam), dtype=np.float32)
    zeros = np.zeros((B, beam), dtype=np.float64)
    null_d = ctypes.POINTER(ctypes.c_double)()
    _lib.check(
        model._L.wn_rescore(model._h, beam, _lib.i32p(n_hyps), _lib.i32p(lens), _lib.i32p(tokens),
                            _lib.f64p(zeros), max_len, 0.0, float(reverse_weight),
                            _lib.i32p(best), _lib.f32p(score), null_d, null_d,
                            _lib.f32p(all_scores), _stream_ptr(model.device)), 'wn_rescore')
    return [all_scores[b, :n_hyps[b]].astype(np.float64).tolist() for b in range(B)]


def combine_scores(attn, beam_score, td, attn_weight: float, ctc_weight: float,
                   transducer_weight: float):
    """transducer.py:389-394 for one utterance, in fp64: (index of the winner, the rescored
    score of every hypothesis).  The first maximum wins; a NaN never wins (`score > best` is
    false for it, as in the reference)."""
    scores, best, best_score = [], 0, -float('inf')
    for i in range(len(attn)):
        s = float(attn[i]) * attn_weight + float(beam_score[i]) * ctc_weight
        if transducer_weight != 0.0:
            s += float(td[i]) * transducer_weight
        scores.append(s)
        if s > best_score:
            best, best_score = i, s
    return best, scores


BEAM_SEARCH_TYPES = ('transducer', 'ctc')


def _check_search_type(beam_search_type):
    if beam_search_type not in BEAM_SEARCH_TYPES:
        raise ValueError(f'beam_search_type={beam_search_type!r}: expected one of '
                         f'{BEAM_SEARCH_TYPES}')


def _rescore_current(model, nbest, reverse_weight, ctc_weight, attn_weight, transducer_weight
                     ) -> List[DecodeResult]:
    """Steps 2.1 - 2.2 and the combination of transducer_attention_rescoring on the handle's
    current batch, for an n-best [(tokens, score), ...] per utterance."""
    hyps = [[list(t) for t, _ in u] for u in nbest]
    # the transducer score first: it reads the encoder output as the search left it
    td = _score_current(model, hyps) if transducer_weight != 0.0 else [None] * len(hyps)
    attn = _attn_scores_current(model, hyps, reverse_weight)
    out = []
    for b, u in enumerate(nbest):
        best, scores = combine_scores(attn[b], [s for _, s in u], td[b], attn_weight, ctc_weight,
                                      transducer_weight)
        r = DecodeResult(hyps[b][best], score=scores[best], nbest=hyps[b], nbest_scores=scores)
        r.attn_scores, r.td_scores = attn[b], td[b]     # extra: the parts of every score
        out.append(r)
    return out


def _ctc_nbest_current(model, B: int, Tp: int, max_frames: int, beam_size: int, blank_id: int,
                       head: bool):
    """This project's CTC prefix beam search on the handle's current batch as
    [(tokens, score), ...] per utterance.  `head`: run the CTC head first (top-k = beam_size);
    otherwise its rows are in place already."""
    from wenet_amd.search import _prefix_beam
    if head:
        _lib.check(model._L.wn_ctc_logprobs(model._h, beam_size, blank_id, 0.0, None, Tp,
                                            _stream_ptr(model.device)), 'wn_ctc_logprobs')
    res, _ = _prefix_beam(model._h, B, max_frames, beam_size, blank_id, model.device)
    return [[(list(t), float(s)) for t, s in zip(r.nbest, r.nbest_scores)] for r in res]


def attention_rescoring(model, encoder_out: torch.Tensor, encoder_out_lens, beam_size: int,
                        reverse_weight: float = 0.0, ctc_weight: float = 0.0,
                        attn_weight: float = 0.0, transducer_weight: float = 0.0,
                        search_ctc_weight: float = 1.0, search_transducer_weight: float = 0.0,
                        beam_search_type: str = 'transducer') -> List[DecodeResult]:
    """transducer.py:316-396 on a caller's padded (B, T', d) encoder output, any B: one record
    per utterance with `tokens`, `score`, `nbest` (in search order) and `nbest_scores` (the
    rescored score of each).  Every utterance needs at least one encoder frame: the attention
    scores come from wn_rescore, which refuses an utterance without frames (only
    `transducer_score` serves that case, with -inf)."""
    _check_search_type(beam_search_type)
    if reverse_weight > 0.0:
        assert model._cfg.dec_r_layers > 0
    lens = torch.as_tensor(encoder_out_lens).reshape(-1)
    B, Tp = model._set_encoder_out(encoder_out, lens)
    max_frames = int(lens.max()) if B > 0 else 0
    if beam_search_type == 'transducer':
        nbest = _beam_current(model, B, max_frames, beam_size, search_ctc_weight,
                              search_transducer_weight)
    else:
        nbest = _ctc_nbest_current(model, B, Tp, max_frames, beam_size, model.blank, True)
    return _rescore_current(model, nbest, reverse_weight, ctc_weight, attn_weight,
                            transducer_weight)


class Transducer(ASRModel):
    """Hybrid transducer + CTC + attention model with the reference's inference API."""

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        super().__init__(configs, state_dict, device)
        self.blank = self._tcfg.blank
        self.last_rnnt_steps = 0     # lock-step steps of the last transducer search
        self.last_rnnt_advance_rows = 0   # beam search: rows that ran the LSTM step, all steps
        # transducer score: (joint rows computed, rows without prefix sharing, trie nodes)
        self.last_rnnt_score_rows = (0, 0, 0)

    def _config(self, configs: dict) -> _lib.WnConfig:
        self._scfg = None       # WnStatelessPredictorConfig of an embedding / conv predictor
        if configs.get('predictor', 'rnn') in STATELESS_PREDICTORS:
            cfg, self._tcfg, self._scfg = stateless_transducer_config_from_yaml(configs)
        else:
            cfg, self._tcfg = transducer_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        if self._scfg is not None:
            return L.wn_model_create_transducer_stateless(
                ctypes.byref(self._cfg), ctypes.byref(self._tcfg), ctypes.byref(self._scfg),
                tensors, n, self.device.index, ctypes.byref(h))
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

    def transducer_attention_rescoring(
            self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
            decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
            simulate_streaming: bool = False, reverse_weight: float = 0.0,
            ctc_weight: float = 0.0, attn_weight: float = 0.0, transducer_weight: float = 0.0,
            search_ctc_weight: float = 1.0, search_transducer_weight: float = 0.0,
            beam_search_type: str = 'transducer') -> Tuple[List[List[int]], List[float]]:
        """transducer.py:262-396, for any batch size: (token lists, scores), one entry per
        utterance.  One encoder pass; the n-best of the RNN-T prefix beam search with the search
        weights ('transducer') or of the CTC prefix beam search ('ctc'); per hypothesis
        `attn * attn_weight + beam_score * ctc_weight + td * transducer_weight` in fp64, where
        td = -RNN-T loss (wn_transducer_score, skipped when transducer_weight == 0) and attn the
        attention decoder's score (blended with the right-to-left decoder's by reverse_weight).
        The reference takes one utterance; with B == 1 its pair is `(out[0][0], out[1][0])`.
        Every utterance needs at least one encoder frame (wn_rescore refuses one without)."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        if reverse_weight > 0.0:
            # decoder should be a bitransformer decoder if reverse_weight > 0.0
            assert self._cfg.dec_r_layers > 0
        _check_search_type(beam_search_type)
        _ = simulate_streaming
        speech, lens = self._prep(speech, speech_lengths)
        B = speech.shape[0]
        _, enc_lens, Tp = self._encode(speech, lens, decoding_chunk_size,
                                       num_decoding_left_chunks, False)
        max_frames = int(enc_lens.max()) if B > 0 else 0
        if beam_search_type == 'transducer':
            nbest = _beam_current(self, B, max_frames, beam_size, search_ctc_weight,
                                  search_transducer_weight)
        else:
            nbest = _ctc_nbest_current(self, B, Tp, max_frames, beam_size, self.blank, True)
        res = _rescore_current(self, nbest, reverse_weight, ctc_weight, attn_weight,
                               transducer_weight)
        return [list(r.tokens) for r in res], [r.score for r in res]

    def decode(self, methods: List[str], speech: torch.Tensor, speech_lengths: torch.Tensor,
               beam_size: int = 1, decoding_chunk_size: int = -1,
               num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
               simulate_streaming: bool = False, reverse_weight: float = 0.0,
               context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
               length_penalty: float = 0.0, infos=None, n_steps: int = 64,
               search_ctc_weight: float = 0.3, search_transducer_weight: float = 0.7,
               attn_weight: float = 0.0, transducer_weight: float = 0.0,
               beam_search_type: str = 'transducer') -> Dict[str, List[DecodeResult]]:
        """ASRModel.decode, which additionally knows 'rnnt_greedy_search', 'rnnt_beam_search' and
        'rnnt_beam_attn_rescoring': one encoder pass serves every requested mode.  The beam
        search takes `beam_size` and its fusion weights `search_ctc_weight` /
        `search_transducer_weight`; `ctc_weight` stays the rescoring weight and is not read by
        it.  Its results carry `tokens`, `score`, `nbest` and `nbest_scores`.
        'rnnt_beam_attn_rescoring' (transducer_attention_rescoring) rescores the n-best of that
        search (computed once when both modes are asked for), or with beam_search_type='ctc' of
        the CTC prefix beam search, with `attn_weight`, `ctc_weight`, `transducer_weight` and
        `reverse_weight`; its results carry `tokens`, `score`, `nbest` in search order and
        `nbest_scores`, the rescored score of each."""
        rescoring = RNNT_RESCORE_METHOD in methods
        if rescoring:
            _check_search_type(beam_search_type)
            if reverse_weight > 0.0:
                assert self._cfg.dec_r_layers > 0
        ctc_nbest = rescoring and beam_search_type == 'ctc'
        others = [m for m in methods
                  if m not in (RNNT_METHOD, RNNT_BEAM_METHOD, RNNT_RESCORE_METHOD)]
        # (the CTC n-best of the rescoring needs the CTC head's top-k at beam_size)
        st = self._decode_begin(others, speech, speech_lengths, beam_size, decoding_chunk_size,
                                num_decoding_left_chunks, simulate_streaming, context_graph,
                                blank_id, blank_penalty,
                                ctc_topk=beam_size if ctc_nbest else None)
        results = {}
        if RNNT_METHOD in methods:
            # first: the search reads the encoder output, which the non-blank filter of
            # attention_rescoring may replace
            B, enc_lens = st['B'], st['enc_lens']
            toks = _search_current(self, B, int(enc_lens.max()) if B > 0 else 0, n_steps)
            results[RNNT_METHOD] = [DecodeResult(t) for t in toks]
        nbest = None
        if RNNT_BEAM_METHOD in methods:      # (before _decode_end, for the same reason)
            B, enc_lens = st['B'], st['enc_lens']
            nbest = _beam_current(self, B, int(enc_lens.max()) if B > 0 else 0, beam_size,
                                  search_ctc_weight, search_transducer_weight)
            results[RNNT_BEAM_METHOD] = _beam_results(nbest)
        if rescoring:                        # (likewise: it reads the encoder output)
            B, enc_lens = st['B'], st['enc_lens']
            max_frames = int(enc_lens.max()) if B > 0 else 0
            if ctc_nbest:
                nbest = _ctc_nbest_current(self, B, st['Tp'], max_frames, beam_size,
                                           st['blank_id'], False)
            elif nbest is None:
                nbest = _beam_current(self, B, max_frames, beam_size, search_ctc_weight,
                                      search_transducer_weight)
            results[RNNT_RESCORE_METHOD] = _rescore_current(
                self, nbest, reverse_weight, ctc_weight, attn_weight, transducer_weight)
        results.update(self._decode_end(st, ctc_weight, reverse_weight, length_penalty, infos))
        return results
