"""W2v-BERT 2.0 / conformer_shaw encoders (`encoder: conformer` with Shaw relative-position
attention over stacked frames) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * the recipe                               wenet/models/ssl/w2vbert/convert_w2vbert_to_wenet_config_and_ckpt.py:8-115
  * StackNFramesSubsampling                  wenet/models/transformer/subsampling.py:339-394
  * NoPositionalEncoding                     wenet/models/transformer/embedding.py:178-198
  * ShawRelPositionMultiHeadedAttention      wenet/models/transformer/attention.py:523-596

The encoder is a kernel path of its own (csrc/attention_shaw.hip, csrc/cabi_shaw.hip): the
stacked-frame front end, the Shaw attention, a plain fp32 layer stack.  The CTC head, the
searches, the alignment and (with heads of 64 or 32) the decoder are `ASRModel`'s.

An utterance of L frames gives L // 2 encoder frames, each from its own frames 2t and 2t + 1; the
attention masks the padding and the causal conv module has no right context, so every utterance is
encoded as the reference encodes it ALONE, whatever the batch.
"""
import ctypes
from typing import List

from wenet_amd import _lib
from wenet_amd.model import ASRModel

MAX_LEFT, MAX_RIGHT, STACK = 64, 8, 2     # attention.py:541-542, subsampling.py:346


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the Shaw kernels need {want!r})')


# key -> (required value, the reference's default when the key is missing)
_ENC = dict(input_layer=('stack_n_frames', 'conv2d'),
            pos_enc_layer_type=('no_pos', 'rel_pos'),
            selfattention_layer_type=('shaw_rel_selfattn', 'rel_selfattn'),
            cnn_module_norm=('layer_norm', 'batch_norm'), conv_bias=(False, True),
            activation_type=('swish', 'swish'), macaron_style=(True, True),
            use_cnn_module=(True, True), normalize_before=(True, True),
            use_dynamic_chunk=(False, False), final_norm=(True, True),
            query_bias=(True, True), key_bias=(True, True), value_bias=(True, True),
            mlp_bias=(True, True), conv_inner_factor=(2, 2),
            layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            n_kv_head=(None, None), head_dim=(None, None),
            positionwise_conv_kernel_size=(1, 1))
_DEC = dict(activation_type=('relu', 'relu'), input_layer=('embed', 'embed'),
            normalize_before=(True, True), src_attention=(True, True), query_bias=(True, True),
            key_bias=(True, True), src_key_bias=(True, True), value_bias=(True, True),
            mlp_bias=(True, True), n_kv_head=(None, None), head_dim=(None, None),
            layer_norm_type=('layer_norm', 'layer_norm'),
            mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
            tie_word_embedding=(False, False), use_output_layer=(True, True))


def shaw_config_from_yaml(configs: dict):
    """train.yaml dict of the converter's recipe -> (wn_config, wn_shaw_config).  `causal`, any
    `cnn_module_kernel` in [1, 63] (odd unless causal), `gradient_checkpointing` and `use_sdpa`
    are free; every other value is refused by key.  A decoder whose heads are neither 64 nor 32
    wide (the converter's `attention_head` spelling leaves the default 4 heads, 256 wide at
    d 1024) gives dec_layers = 0: the encoder and the CTC head run, the decoder does not."""
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
    if ec.get('static_chunk_size', 0) > 0:
        _refuse('encoder_conf.static_chunk_size', ec['static_chunk_size'], -1)
    if ec.get('conv_norm_eps', 1e-5) != 1e-5:
        _refuse('encoder_conf.conv_norm_eps', ec['conv_norm_eps'], 1e-5)
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    if d != heads * 64 or d > 1024:
        _refuse('encoder_conf.output_size / attention_heads', d / heads,
                '64, output_size <= 1024')
    causal = bool(ec.get('causal', False))
    K = ec.get('cnn_module_kernel', 15)
    if not 1 <= K <= 63 or (not causal and K % 2 != 1):
        _refuse('encoder_conf.cnn_module_kernel', K, 'a size in [1, 63], odd unless causal')
    if configs.get('cmvn', None) not in (None, 'global_cmvn'):
        _refuse('cmvn', configs['cmvn'], 'global_cmvn')
    if not 1 <= configs['input_dim'] <= 128:
        _refuse('input_dim', configs['input_dim'], 'at most 128')
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
    c.use_dynamic_chunk = c.static_chunk_size = 0
    c.vocab = vocab
    c.has_cmvn = int(configs.get('cmvn', None) == 'global_cmvn')
    c.dec_heads = dc.get('attention_heads', 4)
    c.dec_ffn_dim = dc.get('linear_units', 2048)
    c.dec_layers = dc.get('num_blocks', 6)
    c.dec_r_layers = dc.get('r_num_blocks', 0) if bidir else 0
    c.bidirectional = int(bidir)
    if d % c.dec_heads != 0 or d // c.dec_heads not in (64, 32):
        c.dec_layers = c.dec_r_layers = c.bidirectional = 0
    c.sos = st.get('<sos>', vocab - 1)
    c.eos = st.get('<eos>', vocab - 1)
    c.max_pos = 5000                      # the decoder's sinusoid table (embedding.py:47-56)
    c.norm_eps = ec.get('norm_eps', 1e-5)
    c.encoder_type = c.input_layer = c.activation = 0
    c.key_bias = 1
    c.cnn_norm = 0
    c.dec_activation = c.dec_key_bias = c.dec_src_key_bias = 0
    c.dec_learned_pos = c.dec_max_pos = 0
    h = _lib.WnShawConfig()
    h.max_left, h.max_right, h.stack = MAX_LEFT, MAX_RIGHT, STACK
    return c, h


class ShawConformer(ASRModel):
    """An asr_model on a W2v-BERT 2.0 / conformer_shaw encoder with the reference's inference
    API: 20 ms encoder frames, full context, fp32."""

    def __init__(self, configs: dict, state_dict, device='cuda'):
        cfg, _ = shaw_config_from_yaml(configs)
        sd = dict(state_dict)
        # (the converter's checkpoint carries no decoder: "dummy decoder")
        self._no_decoder = cfg.dec_layers == 0 or not any(k.startswith('decoder.') for k in sd)
        if self._no_decoder:
            sd = {k: v for k, v in sd.items() if not k.startswith('decoder.')}
        super().__init__(configs, sd, device)

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._hcfg = shaw_config_from_yaml(configs)
        if self._no_decoder:
            cfg.dec_layers = cfg.dec_r_layers = cfg.bidirectional = 0
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_shaw(ctypes.byref(self._cfg), ctypes.byref(self._hcfg),
                                      tensors, n, self.device.index, ctypes.byref(h))

    def set_compute_dtype(self, dtype) -> 'ShawConformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: the W2v-BERT (shaw) '
                "encoder stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def set_raw_fbank_input(self, on: bool = True) -> 'ShawConformer':
        """on: every entry that takes features (decode, align, _forward_encoder) takes RAW Kaldi
        fbank (`compute_fbank`), and the encoder normalises it per utterance as
        processor.compute_w2vbert_fbank does -- statistics in a pass of their own, the division
        inside the stacked-frame front end, no normalised tensor in HBM
        (wn_model_set_utt_norm_input).  Off (the default): features as the reference's model
        takes them, e.g. from `compute_w2vbert_fbank` / `compute_feature`."""
        _lib.check(self._L.wn_model_set_utt_norm_input(self._h, int(bool(on))),
                   'wn_model_set_utt_norm_input')
        return self

    def subsampling_rate(self) -> int:    # StackNFramesSubsampling: stride 2
        return STACK

    def right_context(self) -> int:
        return 0

    def _sub_frames(self, T: int) -> int:
        return T // STACK

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError(
            'simulate_streaming is outside the accelerated path: the W2v-BERT (shaw) encoder '
            'has no chunk-by-chunk path (the Shaw attention key / value cache)')

    def forward_encoder_chunk(self, *args, **kwargs):
        self._check_simulate_streaming(None)

    forward_encoder_chunk_batch = forward_encoder_chunk
    forward_encoder_chunk_by_chunk = forward_encoder_chunk

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        if chunk > 0:
            raise NotImplementedError(
                f'decoding_chunk_size={chunk} is outside the accelerated path: the W2v-BERT '
                '(shaw) encoder attends over the full utterance')
        return super()._encode(speech, lens, -1, -1, want_out)

    def decode(self, methods: List[str], *args, **kwargs):
        if self._cfg.dec_layers <= 0:
            for m in methods:
                if m in ('attention', 'attention_rescoring'):
                    raise NotImplementedError(
                        f'decode method {m!r} is outside the accelerated path of this model: '
                        'it has no attention decoder with heads of 64 or 32 '
                        '(decoder_conf.attention_heads; the checkpoint may carry no decoder)')
        return super().decode(methods, *args, **kwargs)
