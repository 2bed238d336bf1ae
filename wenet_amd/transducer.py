"""The hybrid transducer (`model: transducer`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * Transducer.greedy_search                  wenet/models/transducer/transducer.py:398-442
  * basic_greedy_search                       wenet/models/transducer/search/greedy_search.py:6-54
  * RNNPredictor / TransducerJoint            transducer/predictor.py:60-206, joint.py:62-92
  * how init_model builds the model           wenet/utils/init_model.py:137-154

The reference decodes one utterance and one symbol at a time; here the whole batch runs in
lock-step on the GPU with a frame lookahead (csrc/transducer.hip), for any batch size, with the
same token lists.  The encoder, the CTC head and the attention decoder are the ones of
`ASRModel`, so its decode modes and `align` work on a `Transducer` unchanged.
"""
import copy
import ctypes
from typing import Dict, List

import numpy as np
import torch

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml
from wenet_amd.search import DecodeResult, _stream_ptr

RNNT_METHOD = 'rnnt_greedy_search'   # wenet/bin/recognize.py:86


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


class Transducer(ASRModel):
    """Hybrid transducer + CTC + attention model with the reference's inference API."""

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        super().__init__(configs, state_dict, device)
        self.blank = self._tcfg.blank
        self.last_rnnt_steps = 0     # lock-step steps of the last transducer search

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

    def decode(self, methods: List[str], speech: torch.Tensor, speech_lengths: torch.Tensor,
               beam_size: int = 1, decoding_chunk_size: int = -1,
               num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
               simulate_streaming: bool = False, reverse_weight: float = 0.0,
               context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
               length_penalty: float = 0.0, infos=None, n_steps: int = 64
               ) -> Dict[str, List[DecodeResult]]:
        """ASRModel.decode, which additionally knows 'rnnt_greedy_search': one encoder pass
        serves every requested mode."""
        others = [m for m in methods if m != RNNT_METHOD]
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
        results.update(self._decode_end(st, ctc_weight, reverse_weight, length_penalty, infos))
        return results
