"""Rotary Conformer encoders (`encoder: conformer` with `selfattention_layer_type:
rope_abs_selfattn`, `pos_enc_layer_type: rope_pos`, optionally `n_kv_head` / `head_dim`) on
libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * RopeMultiHeadedAttention                 wenet/models/transformer/attention.py:599-686
  * the MQA / GQA head sharing               wenet/models/transformer/attention.py:47-77, 216-243
  * RopePositionalEncoding                   wenet/models/transformer/embedding.py:201-260
  * google_apply_rotary_emb                  wenet/utils/rope_utils.py:18-26

The encoder is a kernel path of its own (csrc/attention_rope.hip, csrc/cabi_rope.hip): the classic
conv2d front end, x * sqrt(d) with nothing added, a plain fp32 layer stack whose attention rotates
its queries and keys inside the kernel and lets a group of query heads read one K / V head.  The
rotation table is the checkpoint's own `encoder.embed.pos_enc.pe` buffer.  The CTC head, the
decoders, the searches, the alignment, clone() and DecodePipeline are `ASRModel`'s.
"""
import ctypes

from wenet_amd import _lib
from wenet_amd.model import ASRModel

HEAD_DIM, MAX_POS = 64, 3000      # attention_rope; embedding.py:212 (max_len 1500 * 2)


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the rotary kernels need {want!r})')


# key -> (required value, the reference's default when the key is missing)
_ENC = dict(input_layer=('conv2d', 'conv2d'),
            pos_enc_layer_type=('rope_pos', 'rel_pos'),
            selfattention_layer_type=('rope_abs_selfattn', 'rel_selfattn'),
            activation_type=('swish', 'swish'), macaron_style=(True, True),
            use_cnn_module=(True, True), normalize_before=(True, True),
            final_norm=(True, True), conv_bias=(True, True),
            query_bias=(True, True), key_bias=(True, True), value_bias=(True, True),
            mlp_bias=(True, True), conv_inner_factor=(2, 2), conv_norm_eps=(1e-5, 1e-5),
            layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            positionwise_conv_kernel_size=(1, 1))
_DEC = dict(activation_type=('relu', 'relu'), input_layer=('embed', 'embed'),
            normalize_before=(True, True), src_attention=(True, True), query_bias=(True, True),
            key_bias=(True, True), src_key_bias=(True, True), value_bias=(True, True),
            mlp_bias=(True, True), n_kv_head=(None, None), head_dim=(None, None),
            layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            tie_word_embedding=(False, False), use_output_layer=(True, True))


def rope_config_from_yaml(configs: dict):
    """train.yaml dict -> (wn_config, wn_rope_config).  `n_kv_head` (absent: the head count, else
    any divisor of it), `head_dim` (absent or 64), `causal`, `cnn_module_norm` (layer_norm /
    batch_norm), `cnn_module_kernel`, the chunk keys, `gradient_checkpointing` and `use_sdpa` are
    free; every other value is refused by key."""
    if configs.get('model', 'asr_model') != 'asr_model':
        _refuse('model', configs.get('model'), 'asr_model')
    if configs.get('encoder', 'conformer') != 'conformer':
        _refuse('encoder', configs.get('encoder'), 'conformer')
    dec_type = configs.get('decoder', 'bitransformer')
    if dec_type not in ('transformer', 'bitransformer'):
        _refuse('decoder', dec_type, 'transformer')
    ec = configs['encoder_conf']
    dc = configs.get('decoder_conf') or {}
    for conf, name, table in ((ec, 'encoder_conf', _ENC), (dc, 'decoder_conf', _DEC)):
        for k, (want, default) in table.items():
            got = conf.get(k, default)
            if got != want:
                _refuse(f'{name}.{k}', got, want)
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    # (encoder.py:98-104 builds the table with output_size // attention_heads)
    if ec.get('head_dim', None) not in (None, HEAD_DIM):
        _refuse('encoder_conf.head_dim', ec['head_dim'], HEAD_DIM)
    if d != heads * HEAD_DIM or d > 1024:
        _refuse('encoder_conf.output_size / attention_heads', d / heads,
                '64, output_size <= 1024')
    n_kv = ec.get('n_kv_head', None)
    if n_kv is not None and (ec.get('head_dim', None) is None or not isinstance(n_kv, int)
                             or n_kv < 1 or heads % n_kv != 0):
        _refuse('encoder_conf.n_kv_head', n_kv,
                'a divisor of attention_heads, with head_dim: 64 beside it')
    cnn_norm = ec.get('cnn_module_norm', 'batch_norm')
    if cnn_norm not in ('layer_norm', 'batch_norm'):
        _refuse('encoder_conf.cnn_module_norm', cnn_norm, 'layer_norm or batch_norm')
    causal = bool(ec.get('causal', False))
    K = ec.get('cnn_module_kernel', 15)
    if not 1 <= K <= 63 or (not causal and K % 2 != 1):
        _refuse('encoder_conf.cnn_module_kernel', K, 'a size in [1, 63], odd unless causal')
    if configs.get('cmvn', None) not in (None, 'global_cmvn'):
        _refuse('cmvn', configs['cmvn'], 'global_cmvn')
    vocab = configs['output_dim']
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    bidir = dec_type == 'bitransformer'
    c = _lib.WnConfig()
    c.feat_dim = configs['input_dim']
    c.d_model, c.n_heads = d, heads
    c.ffn_dim = ec.get('linear_units', 2048)
    c.n_layers = ec.get('num_blocks', 6)
    c.cnn_kernel = K
    c.causal = int(causal)
    c.use_dynamic_chunk = int(bool(ec.get('use_dynamic_chunk', False)))
    c.static_chunk_size = ec.get('static_chunk_size', 0)
    c.vocab = vocab
    c.has_cmvn = int(configs.get('cmvn', None) == 'global_cmvn')
    c.dec_heads = dc.get('attention_heads', 4)
    c.dec_ffn_dim = dc.get('linear_units', 2048)
    c.dec_layers = dc.get('num_blocks', 6)
    c.dec_r_layers = dc.get('r_num_blocks', 0) if bidir else 0
    c.bidirectional = int(bidir)
    if d % c.dec_heads != 0 or d // c.dec_heads not in (64, 32):
        _refuse('decoder_conf.attention_heads', c.dec_heads, 'heads of 64 or 32')
    c.sos = st.get('<sos>', vocab - 1)
    c.eos = st.get('<eos>', vocab - 1)
    c.max_pos = 5000                      # the decoder's sinusoid table (embedding.py:47-56)
    c.norm_eps = ec.get('norm_eps', 1e-5)
    c.encoder_type = c.input_layer = c.activation = 0
    c.key_bias = 1
    c.cnn_norm = int(cnn_norm == 'batch_norm')
    c.dec_activation = c.dec_key_bias = c.dec_src_key_bias = 0
    c.dec_learned_pos = c.dec_max_pos = 0
    r = _lib.WnRopeConfig()
    r.n_kv_heads, r.head_dim, r.max_pos = n_kv or heads, HEAD_DIM, MAX_POS
    return c, r


class RopeConformer(ASRModel):
    """An asr_model on a rotary Conformer encoder with the reference's inference API: full
    context or chunk masks, fp32."""

    def __init__(self, configs: dict, state_dict, device='cuda'):
        # the checkpoint's `pe` is the rotation table here, not the sinusoid table whose rows
        # ASRModel takes for the decoder's position count: it travels under a name of its own
        sd = dict(state_dict)
        sd['encoder.embed.pos_enc.rope_pe'] = sd.pop('encoder.embed.pos_enc.pe')
        super().__init__(configs, sd, device)

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._rcfg = rope_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_rope(ctypes.byref(self._cfg), ctypes.byref(self._rcfg),
                                      tensors, n, self.device.index, ctypes.byref(h))

    def set_compute_dtype(self, dtype) -> 'RopeConformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: the rotary Conformer '
                "encoder stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError(
            'simulate_streaming is outside the accelerated path: the rotary Conformer encoder '
            'has no chunk-by-chunk path (the table at an offset, the key / value cache)')

    def forward_encoder_chunk(self, *args, **kwargs):
        self._check_simulate_streaming(None)

    forward_encoder_chunk_batch = forward_encoder_chunk
    forward_encoder_chunk_by_chunk = forward_encoder_chunk

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        # (RopePositionalEncoding.position_encoding asserts offset + size <= max_len)
        if self._sub_frames(int(max(lens))) > MAX_POS:
            raise ValueError(
                f'speech_lengths: an utterance of {int(max(lens))} frames gives more than '
                f'{MAX_POS} encoder frames, the rows of the rotation table')
        return super()._encode(speech, lens, chunk, left, want_out)
