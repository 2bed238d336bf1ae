"""FireRedASR-AED (`model: firered`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * FireRedModel                               wenet/models/firered/model.py:26-63
  * FireRedConformerEncoder / ...EncoderLayer  wenet/models/firered/encoder.py, encoder_layer.py
  * FiredRelPositionMultiHeadedAttention       wenet/models/firered/attention.py:59-183
  * FireRedConv2dSubsampling4                  wenet/models/firered/subsampling.py:23-75
  * the recipe                                 firered/convert_FireRed_AED_L_to_wenet_config_and_ckpt.py:32-105

The encoder is a kernel path of its own (csrc/firered.hip, csrc/cabi_firered.hip): the rel-shift
attention, the 32-channel front end, a plain fp32 layer stack.  The CTC head, the left-to-right
decoder (gelu, tied output layer, no linear_k biases) and the searches are `ASRModel`'s.

Every utterance is decoded as the reference decodes it ALONE: in a batch the
reference lets a shorter utterance's last frames read the batch's padding and gives it one frame
more.  Here the six zero frames stand behind each utterance's own last frame, T' =
((len + 6 - 3) // 2 + 1 - 3) // 2 + 1, and the `attention` search of an utterance runs to its own
T' (the reference's `maxlen`), so alone and batched results are the same.
"""
import ctypes
from typing import Dict, List

import numpy as np
import torch

from wenet_amd import _lib
from wenet_amd.model import ASRModel
from wenet_amd.search import DecodeResult

METHODS = ('attention', 'ctc_greedy_search', 'ctc_prefix_beam_search', 'attention_rescoring')
MAX_FRAMES = 1024      # encoder frames (40 ms each) the position rows of a handle cover


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the FireRed kernels need {want!r})')


def out_len(n: int) -> int:
    """Encoder frames of an utterance of n feature frames decoded alone."""
    return ((n + 6 - 3) // 2 + 1 - 3) // 2 + 1 if n > 0 else 0


# the recipe: key -> (required value, the reference's default when the key is missing)
_ENC = dict(input_layer=('firered_conv2d4', 'conv2d'),
            pos_enc_layer_type=('rel_pos_firered', 'rel_pos'),
            selfattention_layer_type=('firered_rel_selfattn', 'rel_selfattn'),
            final_norm=(False, True), query_bias=(False, True), key_bias=(False, True),
            value_bias=(False, True), conv_bias=(False, True), conv_inner_factor=(4, 2),
            cnn_module_norm=('layer_norm', 'batch_norm'), activation_type=('swish', 'swish'),
            macaron_style=(True, True), use_cnn_module=(True, True),
            normalize_before=(True, True), causal=(False, False),
            use_dynamic_chunk=(False, False), layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            mlp_bias=(True, True), n_kv_head=(None, None), head_dim=(None, None),
            positionwise_conv_kernel_size=(1, 1))
_DEC = dict(activation_type=('gelu', 'relu'), tie_word_embedding=(True, False),
            key_bias=(False, True), src_key_bias=(False, True), input_layer=('embed', 'embed'),
            normalize_before=(True, True), src_attention=(True, True), query_bias=(True, True),
            value_bias=(True, True), mlp_bias=(True, True), n_kv_head=(None, None),
            head_dim=(None, None), layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            use_output_layer=(True, True))


def firered_config_from_yaml(configs: dict):
    """train.yaml dict of a `model: firered` recipe -> (wn_config, wn_firered_config).  Exactly
    the recipe the converter writes has kernels; every other value is refused by name.
    `use_sdpa` and `gradient_checkpointing` do not change what is computed and are ignored."""
    if configs.get('model') != 'firered':
        _refuse('model', configs.get('model', 'asr_model'), 'firered')
    if configs.get('encoder') != 'firered_conformer':
        _refuse('encoder', configs.get('encoder', 'conformer'), 'firered_conformer')
    if configs.get('decoder', 'bitransformer') != 'transformer':
        _refuse('decoder', configs.get('decoder', 'bitransformer'), 'transformer')
    ec = configs['encoder_conf']
    dc = configs.get('decoder_conf') or {}
    for conf, name, table in ((ec, 'encoder_conf', _ENC), (dc, 'decoder_conf', _DEC)):
        for k, (want, default) in table.items():
            got = conf.get(k, default)
            if got != want:
                _refuse(f'{name}.{k}', got, want)
    if ec.get('static_chunk_size', 0) > 0:
        _refuse('encoder_conf.static_chunk_size', ec['static_chunk_size'], -1)
    if ec.get('conv_norm_eps', 1e-5) != 1e-5:
        _refuse('encoder_conf.conv_norm_eps', ec['conv_norm_eps'], 1e-5)
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    if d != heads * 64:
        _refuse('encoder_conf.output_size / attention_heads', d / heads, 64)
    if dc.get('attention_heads', 4) * 64 != d:
        _refuse('decoder_conf.attention_heads', dc.get('attention_heads', 4), d // 64)
    K = ec.get('cnn_module_kernel', 15)
    if K % 2 != 1:
        _refuse('encoder_conf.cnn_module_kernel', K, 'an odd size')
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    if 'sos' not in st or 'eos' not in st:      # model.py:48-50: asserted there
        _refuse('tokenizer_conf.special_tokens', st, "{'sos': ..., 'eos': ...}")
    if (configs.get('model_conf') or {}).get('reverse_weight', 0.0) != 0.0:
        _refuse('model_conf.reverse_weight', configs['model_conf']['reverse_weight'], 0.0)
    c = _lib.WnConfig()
    c.feat_dim = configs['input_dim']
    c.d_model, c.n_heads = d, heads
    c.ffn_dim = ec.get('linear_units', 2048)
    c.n_layers = ec.get('num_blocks', 6)
    c.cnn_kernel = K
    c.causal = c.use_dynamic_chunk = c.static_chunk_size = 0
    c.vocab = configs['output_dim']
    c.has_cmvn = int(configs.get('cmvn', None) == 'global_cmvn')
    c.dec_heads = dc.get('attention_heads', 4)
    c.dec_ffn_dim = dc.get('linear_units', 2048)
    c.dec_layers = dc.get('num_blocks', 6)
    c.dec_r_layers = c.bidirectional = 0
    c.sos, c.eos = st['sos'], st['eos']
    c.max_pos = 5000                      # the decoder's sinusoid table (embedding.py:47-56)
    c.norm_eps = ec.get('norm_eps', 1e-5)
    c.encoder_type = c.input_layer = c.activation = 0
    c.key_bias = 0
    c.cnn_norm = 0
    c.dec_activation, c.dec_key_bias, c.dec_src_key_bias = 1, 1, 1
    c.dec_learned_pos = c.dec_max_pos = 0
    f = _lib.WnFireRedConfig()
    f.sub_channels = 32                   # FireRedConv2dSubsampling4's odim default
    f.conv_inner_factor = 4
    f.max_frames = MAX_FRAMES
    f.attn_norm_eps = 1e-5                # torch.nn.LayerNorm's default, not norm_eps
    return c, f


class FireRed(ASRModel):
    """FireRedModel with the reference's inference API; `attention` is its decode method."""

    default_decode_method = 'attention'   # firered/model.py:29

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        # `encoder.embed.pos_enc.pe` is the (2 * 5000 - 1)-row RELATIVE table here (a buffer the
        # library rebuilds for the distances it keeps), not the decoder's sinusoids
        sd = {k: v for k, v in state_dict.items() if k != 'encoder.embed.pos_enc.pe'}
        super().__init__(configs, sd, device)
        self.default_decode_method = 'attention'
        st = configs['tokenizer_conf']['special_tokens']
        self.sos, self.eos = st['sos'], st['eos']
        self._last_enc = None

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._fcfg = firered_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_firered(ctypes.byref(self._cfg), ctypes.byref(self._fcfg),
                                         tensors, n, self.device.index, ctypes.byref(h))

    def set_compute_dtype(self, dtype) -> 'FireRed':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: the FireRed encoder '
                "stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError("FiredASR don't support streaming")   # firered/model.py:62

    def forward_encoder_chunk(self, *args, **kwargs):
        raise NotImplementedError("FiredASR don't support streaming")

    forward_encoder_chunk_batch = forward_encoder_chunk
    forward_encoder_chunk_by_chunk = forward_encoder_chunk

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        if chunk > 0 or left > 0:
            raise NotImplementedError(
                'decoding_chunk_size / num_decoding_left_chunks are outside the accelerated '
                'path: the FireRed encoder attends over the full utterance')
        B, T, F = speech.shape
        assert F == self._cfg.feat_dim, 'feature dimension mismatch'
        Tp = out_len(T)
        enc_lens = np.zeros((B, ), dtype=np.int32)
        # (always kept: the `attention` search of an utterance runs on its own rows)
        out = torch.empty((B, Tp, self._cfg.d_model), dtype=torch.float32, device=self.device)
        _lib.check(
            self._L.wn_encode(self._h, speech.data_ptr(), _lib.i32p(lens), B, T, -1, -1,
                              out.data_ptr(), _lib.i32p(enc_lens),
                              torch.cuda.current_stream(self.device).cuda_stream),
            'wn_encode')
        self._last_enc = (out, enc_lens)
        return (out if want_out else None), enc_lens, Tp

    def decode(self, methods: List[str], speech, speech_lengths, beam_size: int = 1,
               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
               ctc_weight: float = 0.0, simulate_streaming: bool = False,
               reverse_weight: float = 0.0, **kw) -> Dict[str, List[DecodeResult]]:
        """asr_model.py:267-343 for the four modes a FireRedModel has here.  Every call keeps the
        padded encoder output of its batch (`_last_enc`) until the next encode, CTC-only calls
        included, and an `attention` call leaves the handle's CURRENT batch set to the last
        group of equal-length utterances it searched, not to the whole batch: call `decode` /
        `_forward_encoder` again before anything that reads the handle's current batch
        (`ctc_logprobs` on it, `align`, `_rescore`).  `DecodePipeline` is refused for that
        reason."""
        for m in methods:
            if m not in METHODS:
                raise NotImplementedError(
                    f'decode method {m!r} is outside the accelerated path of a FireRed model '
                    f'(has: {", ".join(METHODS)})')
        if reverse_weight != 0.0:
            raise NotImplementedError('reverse_weight must be 0: a FireRed model has no '
                                      'right-to-left decoder (firered/model.py:47)')
        if simulate_streaming:
            self._check_simulate_streaming(speech)
        return super().decode(methods, speech, speech_lengths, beam_size, decoding_chunk_size,
                              num_decoding_left_chunks, ctc_weight, False, 0.0, **kw)

    def _decode_end(self, st, ctc_weight=0.0, reverse_weight=0.0, length_penalty=0.0, infos=None):
        methods = st['methods']
        rest = dict(st, methods=[m for m in methods if m != 'attention'])
        results = super()._decode_end(rest, ctc_weight, reverse_weight, length_penalty, infos)
        if 'attention' in methods:
            results['attention'] = self._attention_alone(st['B'], st['beam_size'], length_penalty)
        return {m: results[m] for m in methods}

    def _attention_alone(self, B: int, beam_size: int, length_penalty: float):
        """attention_beam_search with every utterance's own T' as `maxlen`, as the reference runs
        it on that utterance alone: the utterances of one length share a call (the handle's
        current batch becomes that group's rows of the encoder output)."""
        from wenet_amd.search import attention_beam_search
        enc, enc_lens = self._last_enc
        if int(enc_lens.min()) <= 0:
            raise RuntimeError("'attention' mode: an utterance has no encoder frames")
        out = [None] * B
        self.last_attention_truncated = False
        for n in sorted(set(int(v) for v in enc_lens)):
            idx = [b for b in range(B) if int(enc_lens[b]) == n]
            rows = enc[torch.as_tensor(idx, device=enc.device), :n].contiguous()
            self._set_encoder_out(rows, np.full((len(idx), ), n, dtype=np.int32))
            for b, r in zip(idx, attention_beam_search(self, len(idx), n, beam_size,
                                                       length_penalty, None)):
                out[b] = r
        return out
