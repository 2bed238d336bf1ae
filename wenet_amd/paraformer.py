"""Paraformer (`model: paraformer`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * Paraformer._forward_paraformer / decode      wenet/models/paraformer/paraformer.py:329-413
  * LFR, SanmEncoder, SanmDecoder and its layers wenet/models/paraformer/layers.py
  * MultiHeadedAttentionSANM / ...Cross          wenet/models/paraformer/attention.py
  * Cif, cif()                                   wenet/models/paraformer/cif.py:55-142, 250-293
  * paraformer_greedy_search / _beam_search      wenet/models/paraformer/search.py:140-198
  * the recipes                                  examples/aishell/paraformer/conf/*.yaml,
                                                 examples/wenetspeech/paraformer/conf/*.yaml

One encoder pass feeds the CIF predictor, which says how many tokens there are and gives one
acoustic embedding per token; one parallel decoder pass yields every token.  No beam, no step
loop.  The kernels: csrc/attention_d128.hip (heads of 128), csrc/paraformer.hip (LFR front end,
wide LayerNorm, CIF), csrc/cabi_paraformer.hip (the two layer stacks).  The CTC head and its
searches are `ASRModel`'s.

Deviations from the reference:
  * every utterance is encoded as the reference encodes it ALONE -- the reference's batched LFR
    pads a shorter utterance from the batch's zero padding when the longest one needs no right
    padding, so its batched and alone results differ; here they are the same bits;
  * an utterance whose predictor gives zero tokens (the reference raises inside the decoder's
    FSMN conv) returns DecodeResult([], confidence=0.0, tokens_confidence=[]);
  * the timestamp branch (predictor.tp_*) is not computed: DecodeResult.times stays [].
"""
import ctypes
import math
from typing import Dict, List

import numpy as np
import torch

from wenet_amd import _lib
from wenet_amd.model import ASRModel, _stream_ptr
from wenet_amd.search import DecodeResult

PARAFORMER_METHODS = ('paraformer_greedy_search', 'paraformer_beam_search')
CTC_METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search')
METHODS = PARAFORMER_METHODS + CTC_METHODS
MAX_FRAMES = 2048      # encoder frames (60 ms each) the position rows of a handle cover
LFR_M, LFR_N = 7, 6    # layers.py:26: the model builds LFR() with its defaults


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the Paraformer kernels need {want!r})')


def out_len(n: int) -> int:
    """Encoder frames of an utterance of n feature frames decoded alone."""
    return -(-n // LFR_N) if n > 0 else 0


# key -> (required value, the reference's default when the key is missing)
_ENC = dict(input_layer=('paraformer_dummy', 'conv2d'),
            pos_enc_layer_type=('abs_pos_paraformer', 'abs_pos'),
            normalize_before=(True, True), sanm_shfit=(0, 0), static_chunk_size=(0, 0),
            use_dynamic_left_chunk=(False, False))
_DEC = dict(normalize_before=(True, True), sanm_shfit=(0, 0), input_layer=('embed', 'embed'),
            use_output_layer=(True, True), src_attention=(True, True))
_PRED = dict(cnn_groups=(1, 0), l_order=(1, None), r_order=(1, None), residual=(False, True),
             threshold=(1.0, 1.0), smooth_factor=(1.0, 1.0), noise_threshold=(0.0, 0.0))


def paraformer_config_from_yaml(configs: dict):
    """train.yaml dict of a `model: paraformer` recipe -> (wn_config, wn_paraformer_config).
    Exactly the shipped recipes have kernels; every other value is refused by key name.  Dropout
    rates, `gradient_checkpointing`, `use_dynamic_chunk` (a training-time switch: decoding here is
    full context) and the timestamp keys of predictor_conf (`upsample_times`, `smooth_factor2`,
    `noise_threshold2`) do not change what is computed and are ignored."""
    if configs.get('model') != 'paraformer':
        _refuse('model', configs.get('model', 'asr_model'), 'paraformer')
    if configs.get('encoder') != 'sanm_encoder':
        _refuse('encoder', configs.get('encoder', 'conformer'), 'sanm_encoder')
    if configs.get('decoder') != 'sanm_decoder':
        _refuse('decoder', configs.get('decoder', 'bitransformer'), 'sanm_decoder')
    if configs.get('predictor') != 'paraformer_predictor':
        _refuse('predictor', configs.get('predictor'), 'paraformer_predictor')
    ec = configs['encoder_conf']
    dc = configs.get('decoder_conf') or {}
    pc = configs.get('predictor_conf') or {}
    for conf, name, table in ((ec, 'encoder_conf', _ENC), (dc, 'decoder_conf', _DEC),
                              (pc, 'predictor_conf', _PRED)):
        for k, (want, default) in table.items():
            got = conf.get(k, default)
            if got != want:
                _refuse(f'{name}.{k}', got, want)
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    if d % heads != 0 or d // heads not in (64, 128):
        _refuse('encoder_conf.output_size / attention_heads', d / heads, '64 or 128')
    if dc.get('attention_heads', 4) != heads:
        _refuse('decoder_conf.attention_heads', dc.get('attention_heads', 4), heads)
    if pc.get('idim', d) != d:
        _refuse('predictor_conf.idim', pc.get('idim'), d)
    K = ec.get('kernel_size', 11)
    if K % 2 != 1 or not 1 <= K <= 63:
        _refuse('encoder_conf.kernel_size', K, 'an odd size up to 63')
    if dc.get('kernel_size', 11) != K:
        _refuse('decoder_conf.kernel_size', dc.get('kernel_size', 11), K)
    nb = dc.get('num_blocks', 6)
    if dc.get('att_layer_num', 16) != nb:       # layers.py:436: asserted there
        _refuse('decoder_conf.att_layer_num', dc.get('att_layer_num', 16), nb)
    tail = pc.get('tail_threshold', 0.45)
    if not 0.0 < tail < 1.0:
        _refuse('predictor_conf.tail_threshold', tail, 'a value in (0, 1)')
    if configs['input_dim'] % LFR_M != 0:
        _refuse('input_dim', configs['input_dim'], f'a multiple of {LFR_M} (LFR stacks 7 frames)')
    if dc.get('linear_units', 2048) > 2048:
        _refuse('decoder_conf.linear_units', dc['linear_units'], 'at most 2048')
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    if '<sos>' not in st or '<eos>' not in st:      # paraformer.py:139-141
        _refuse('tokenizer_conf.special_tokens', st, "{'<sos>': ..., '<eos>': ...}")
    c = _lib.WnConfig()
    c.feat_dim = configs['input_dim'] // LFR_M
    c.d_model, c.n_heads = d, heads
    c.ffn_dim = ec.get('linear_units', 2048)
    c.n_layers = ec.get('num_blocks', 6)
    c.cnn_kernel = K
    c.causal = c.use_dynamic_chunk = c.static_chunk_size = 0
    c.vocab = configs['output_dim']
    c.has_cmvn = int(configs.get('cmvn', None) == 'global_cmvn')
    c.dec_heads = heads
    c.dec_ffn_dim = dc.get('linear_units', 2048)
    c.dec_layers = 0                      # (no autoregressive decoder: ASRModel's modes are off)
    c.dec_r_layers = c.bidirectional = 0
    c.sos, c.eos = st['<sos>'], st['<eos>']
    c.max_pos = 5000
    c.norm_eps = 1e-5
    c.encoder_type = c.input_layer = c.activation = 0
    p = _lib.WnParaformerConfig()
    p.lfr_m, p.lfr_n = LFR_M, LFR_N
    p.kernel_size = K
    p.dec_blocks = nb
    p.max_frames = MAX_FRAMES
    p.threshold = 1.0
    p.tail_threshold = tail
    p.smooth_factor = 1.0
    p.noise_threshold = 0.0
    return c, p


class Paraformer(ASRModel):
    """Paraformer with the reference's inference API; `paraformer_greedy_search` is its decode
    method."""

    default_decode_method = 'paraformer_greedy_search'   # paraformer.py:112

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        # `encoder.embed.pos_enc.pe` is a buffer: the library rebuilds the rows it keeps in fp64
        sd = {k: v for k, v in state_dict.items() if k != 'encoder.embed.pos_enc.pe'}
        super().__init__(configs, sd, device)
        self.default_decode_method = 'paraformer_greedy_search'

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._pcfg = paraformer_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_paraformer(ctypes.byref(self._cfg), ctypes.byref(self._pcfg),
                                            tensors, n, self.device.index, ctypes.byref(h))

    def clone(self):
        raise NotImplementedError('clone() is outside the accelerated path of a Paraformer model')

    def set_compute_dtype(self, dtype) -> 'Paraformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: a Paraformer model '
                "stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def subsampling_rate(self) -> int:
        return LFR_N

    def right_context(self) -> int:
        return LFR_M - 1 - (LFR_M - 1) // 2

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError('simulate_streaming is outside the accelerated path: the '
                                  'Paraformer encoder attends over the full utterance')

    def forward_encoder_chunk(self, *args, **kwargs):
        raise NotImplementedError('forward_encoder_chunk is outside the accelerated path: the '
                                  'Paraformer encoder attends over the full utterance')

    forward_encoder_chunk_batch = forward_encoder_chunk
    forward_encoder_chunk_by_chunk = forward_encoder_chunk

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        if chunk > 0 or left > 0:
            raise NotImplementedError(
                'decoding_chunk_size / num_decoding_left_chunks are outside the accelerated '
                'path: the Paraformer encoder attends over the full utterance')
        B, T, F = speech.shape
        assert F == self._cfg.feat_dim, 'feature dimension mismatch (fbank frames, before LFR)'
        Tp = out_len(T)
        enc_lens = np.zeros((B, ), dtype=np.int32)
        out = None
        if want_out:
            out = torch.empty((B, Tp, self._cfg.d_model), dtype=torch.float32, device=self.device)
        _lib.check(
            self._L.wn_encode(self._h, speech.data_ptr(), _lib.i32p(lens), B, T, -1, -1,
                              out.data_ptr() if out is not None else None, _lib.i32p(enc_lens),
                              _stream_ptr(self.device)), 'wn_encode')
        return out, enc_lens, Tp

    def _predict_decode(self, B: int, enc_lens):
        """Predictor + decoder on the handle's current batch, whose encoder lengths are
        `enc_lens` -> (tokens (B, L + 1), token numbers (B,), log-probs of the tokens (B, L + 1),
        fire frames (B, L + 1), fires (B,)) with L the longest encoder length: an utterance of L
        frames fires at most L + 1 times (the tail frame).  The padded width of the batch plays no
        part."""
        max_tok = (int(np.max(enc_lens)) if B > 0 else 0) + 1
        tokens = np.zeros((B, max_tok), dtype=np.int32)
        logp = np.zeros((B, max_tok), dtype=np.float32)
        fire_t = np.full((B, max_tok), -1, dtype=np.int32)
        tok_lens = np.zeros((B, ), dtype=np.int32)
        n_fire = np.zeros((B, ), dtype=np.int32)
        _lib.check(
            self._L.wn_paraformer_decode(self._h, _lib.i32p(tokens), _lib.i32p(tok_lens),
                                         _lib.f32p(logp), _lib.i32p(fire_t), _lib.i32p(n_fire),
                                         max_tok, _stream_ptr(self.device)),
            'wn_paraformer_decode')
        return tokens, tok_lens, logp, fire_t, n_fire

    def _forward_paraformer(self, speech, speech_lengths, decoding_chunk_size: int = -1,
                            num_decoding_left_chunks: int = -1) -> Dict[str, object]:
        """paraformer.py:329-360 without the (B, L, V) tensor: `decoder_out` holds the log-prob
        of every chosen token (B, max_tok), `decoder_out_lens` the token numbers; also the token
        ids, the frames the embeddings fired on and the fire counts."""
        speech, lens = self._prep(speech, speech_lengths)
        B = speech.shape[0]
        _, enc_lens, Tp = self._encode(speech, lens, decoding_chunk_size,
                                       num_decoding_left_chunks, False)
        tokens, tok_lens, logp, fire_t, n_fire = self._predict_decode(B, enc_lens)
        return dict(decoder_out=logp, decoder_out_lens=tok_lens, tokens=tokens,
                    fire_frames=fire_t, n_fire=n_fire, encoder_lens=enc_lens, Tp=Tp,
                    speech=speech)

    def decode(self, methods: List[str], speech, speech_lengths, beam_size: int = 1,
               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
               ctc_weight: float = 0.0, simulate_streaming: bool = False,
               reverse_weight: float = 0.0, context_graph=None, blank_id: int = 0,
               blank_penalty: float = 0.0, length_penalty: float = 0.0,
               infos=None) -> Dict[str, List[DecodeResult]]:
        """paraformer.py:362-413.  The positions of a Paraformer output are independent and the
        reference's batch beam search never reorders its history, so the first hypothesis of
        `paraformer_beam_search` is the arg-max of every position: the greedy token list."""
        for m in methods:
            if m not in METHODS:
                raise NotImplementedError(
                    f'decode method {m!r} is outside the accelerated path of a Paraformer model '
                    f'(has: {", ".join(METHODS)})')
        if simulate_streaming:
            self._check_simulate_streaming(speech)
        assert decoding_chunk_size != 0
        speech, lens = self._prep(speech, speech_lengths)
        B = speech.shape[0]
        _, enc_lens, Tp = self._encode(speech, lens, decoding_chunk_size,
                                       num_decoding_left_chunks, False)
        res = dict(encoder_lens=enc_lens, speech=speech)
        results = {}
        if any(m in PARAFORMER_METHODS for m in methods):
            toks, n_tok, logp, _, _ = self._predict_decode(B, enc_lens)
            if 'paraformer_greedy_search' in methods:
                out = []
                for b in range(B):
                    n = int(n_tok[b])
                    if n == 0:
                        out.append(DecodeResult([], confidence=0.0, tokens_confidence=[],
                                                times=[]))
                        continue
                    lp = [float(v) for v in logp[b, :n]]
                    out.append(DecodeResult(toks[b, :n].tolist(),
                                            confidence=math.exp(sum(lp) / n),
                                            tokens_confidence=[math.exp(v) for v in lp],
                                            times=[]))
                results['paraformer_greedy_search'] = out
            if 'paraformer_beam_search' in methods:
                results['paraformer_beam_search'] = [
                    DecodeResult(toks[b, :int(n_tok[b])].tolist(), times=[]) for b in range(B)]
        ctc = [m for m in methods if m in CTC_METHODS]
        if ctc:
            self._use_context_graph(context_graph)
            need_beam = 'ctc_prefix_beam_search' in ctc
            _lib.check(
                self._L.wn_ctc_logprobs(self._h, beam_size if need_beam else 1, blank_id,
                                        blank_penalty, None, Tp, _stream_ptr(self.device)),
                'wn_ctc_logprobs')
            st = dict(methods=ctc, B=B, enc_lens=res['encoder_lens'], need_beam=need_beam,
                      beam_size=beam_size, blank_id=blank_id, speech=res['speech'], Tp=Tp)
            results.update(super()._decode_end(st, 0.0, 0.0, length_penalty, infos))
        return {m: results[m] for m in methods}
