"""Squeezeformer encoders (`encoder: squeezeformer`) under the asr_model head, on libwenet_amd's
HIP kernels.

Mirrors (reference file:line):
  * SqueezeformerEncoder                      wenet/models/squeezeformer/encoder.py:38-244
  * SqueezeformerEncoderLayer                 squeezeformer/encoder_layer.py:21-121
  * RelPositionMultiHeadedAttention.rel_shift squeezeformer/attention.py:75-99, 148-234
  * TimeReductionLayer1D / ...Stream          squeezeformer/subsampling.py:97-179, 243-323
  * DepthwiseConv2dSubsampling4               squeezeformer/subsampling.py:29-94

The front end, the rel-pos attention without the shift, the feed-forward and conv modules, the
CTC head, both decoders and every search are `ASRModel`'s; the wrapped shift, the time reduction
and the time recovery are csrc/squeezeformer.hip, the layer stack csrc/cabi_squeezeformer.hip: a
plain fp32 path.

Every utterance is encoded as the reference encodes it ALONE: the
reference's front-end mask counts one frame too many for every utterance shorter than the batch's
longest and its shift wraps at the padded length, so its batched output depends on the batch.
Here alone and batched results are the same bits.
"""
import ctypes

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml

WIDTHS = (64, 128, 256, 512)      # encoder_dim: the widths dwconv_ln_silu has kernels for


def _refuse(key, got, want):
    raise NotImplementedError(
        f'encoder_conf.{key}={got!r} is outside the accelerated path (the Squeezeformer kernels '
        f'need {want})')


# key -> (accepted values, the reference's default when the key is missing)
_TABLE = dict(time_reduction_layer_type=(('conv1d', 'stream'), 'conv1d'),
              dw_stride=((False, ), False),
              normalize_before=((False, ), False),
              concat_after=((False, ), False),
              pos_enc_layer_type=(('rel_pos', ), 'rel_pos'),
              activation_type=(('swish', ), 'swish'),
              cnn_norm_type=(('layer_norm', 'batch_norm'), 'batch_norm'),
              do_rel_shift=((True, False), True),
              causal=((True, False), False),
              adaptive_scale=((True, False), True),
              use_dynamic_chunk=((True, False), False),
              use_dynamic_left_chunk=((True, False), False))
# read below, or without effect on inference
_OTHER = ('input_size', 'encoder_dim', 'output_size', 'attention_heads', 'num_blocks', 'reduce_idx',
          'recover_idx', 'feed_forward_expansion_factor', 'input_dropout_rate',
          'feed_forward_dropout_rate', 'attention_dropout_rate', 'cnn_module_kernel', 'dropout',
          'init_weights', 'static_chunk_size')


def _one_index(key, v):
    """reduce_idx / recover_idx: None, an int or a one-element list -> int or None."""
    if isinstance(v, (list, tuple)):
        if len(v) != 1:
            _refuse(key, v, 'one reduction and one recovery (an int or a one-element list)')
        v = v[0]
    if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
        _refuse(key, v, 'an int')
    return v


def squeezeformer_config_from_yaml(configs: dict):
    """train.yaml dict of an `encoder: squeezeformer` recipe -> (wn_config,
    wn_squeezeformer_config).  The decoder, tokenizer and model keys are read as for a Conformer
    model; every encoder value without a kernel is refused, naming its key."""
    enc = configs.get('encoder')
    if enc != 'squeezeformer':
        raise NotImplementedError(f'encoder {enc!r} is outside the accelerated path')
    ec = configs.get('encoder_conf') or {}
    for k in ec:
        if k not in _TABLE and k not in _OTHER:
            _refuse(k, ec[k], 'a key SqueezeformerEncoder takes')
    for k, (accepted, default) in _TABLE.items():
        got = ec.get(k, default)
        if got not in accepted:
            _refuse(k, got, ' or '.join(repr(a) for a in accepted))
    d = ec.get('encoder_dim', 256)
    if ec.get('output_size', 256) != d:
        _refuse('output_size', ec.get('output_size', 256),
                f'encoder_dim ({d}): no final_proj')
    if d not in WIDTHS:
        _refuse('encoder_dim', d, f'one of {WIDTHS}')
    heads = ec.get('attention_heads', 4)
    if not isinstance(heads, int) or heads <= 0 or d != heads * 64:
        _refuse('attention_heads', heads, f'a head width of 64 (encoder_dim {d} / 64 heads)')
    factor = ec.get('feed_forward_expansion_factor', 4)
    if not isinstance(factor, int) or factor <= 0 or (d * factor) % 32 != 0:
        _refuse('feed_forward_expansion_factor', factor,
                'encoder_dim * factor a positive multiple of 32')
    blocks = ec.get('num_blocks', 12)
    causal = bool(ec.get('causal', False))
    K = ec.get('cnn_module_kernel', 31)
    if not isinstance(K, int) or not 1 <= K <= 63 or (not causal and K % 2 != 1):
        _refuse('cnn_module_kernel', K, '1..63, odd unless causal')
    reduce_idx = _one_index('reduce_idx', ec.get('reduce_idx', 5))
    recover_idx = _one_index('recover_idx', ec.get('recover_idx', 11))
    if reduce_idx is None and recover_idx is not None:
        _refuse('recover_idx', recover_idx, 'None when reduce_idx is None')
    if reduce_idx is not None:
        if recover_idx is None:
            _refuse('recover_idx', None,
                    'a recovery for the reduction (no 80-ms CTC frame rate)')
        if not 0 <= reduce_idx < recover_idx < blocks:
            _refuse('reduce_idx', reduce_idx, '0 <= reduce_idx < recover_idx < num_blocks')
    # everything that is not the encoder's own: the Conformer reading of the same file
    base = dict(configs, encoder='conformer')
    base['encoder_conf'] = dict(
        output_size=d, attention_heads=heads, num_blocks=blocks, linear_units=d * factor,
        causal=causal, use_dynamic_chunk=bool(ec.get('use_dynamic_chunk', False)),
        static_chunk_size=ec.get('static_chunk_size', 0), norm_eps=1e-5,
        cnn_module_norm=ec.get('cnn_norm_type', 'batch_norm'), cnn_module_kernel=K)
    c = config_from_yaml(base)
    q = _lib.WnSqueezeformerConfig()
    q.reduce_idx = -1 if reduce_idx is None else reduce_idx
    q.recover_idx = -1 if recover_idx is None else recover_idx
    q.reduce_kernel = 5 if ec.get('time_reduction_layer_type', 'conv1d') == 'conv1d' else 1
    q.do_rel_shift = int(bool(ec.get('do_rel_shift', True)))
    return c, q


class Squeezeformer(ASRModel):
    """An ASRModel whose encoder is a Squeezeformer.  decode() with every mode of an ASRModel with
    the same decoder, transcribe, align, context biasing, clone() and DecodePipeline work
    unchanged; decoding_chunk_size / num_decoding_left_chunks change the attention mask only, as
    in the reference."""

    def _config(self, configs: dict) -> _lib.WnConfig:
        if configs.get('model', 'asr_model') == 'transducer':
            raise NotImplementedError(
                "model 'transducer' with encoder 'squeezeformer' is outside the accelerated path")
        cfg, self._qcfg = squeezeformer_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_squeezeformer(ctypes.byref(self._cfg), ctypes.byref(self._qcfg),
                                               tensors, n, self.device.index, ctypes.byref(h))

    def _chunk_mask_size(self, decoding_chunk_size: int) -> int:
        """The chunk size of the attention mask a call gets (0: full context), mask.py:126-198."""
        if self._cfg.use_dynamic_chunk:
            return decoding_chunk_size if decoding_chunk_size > 0 else 0
        return max(self._cfg.static_chunk_size, 0)

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        cs = self._chunk_mask_size(chunk)
        if cs > 0 and self._qcfg.do_rel_shift:
            raise NotImplementedError(
                f'decoding_chunk_size={chunk} (a chunk mask of size {cs}) on a model with '
                'do_rel_shift: true is outside the accelerated path: the wrapped-shift attention '
                'kernel is full context only')
        if cs > 0 and cs % 2 != 0 and self._qcfg.reduce_idx >= 0:
            raise NotImplementedError(
                f'decoding_chunk_size={chunk} (a chunk mask of odd size {cs}) on a model with a '
                'time reduction is outside the accelerated path: mask[:, ::2, ::2] of an odd '
                'chunk mask is no chunk window at the half rate')
        return super()._encode(speech, lens, chunk, left, want_out)

    def set_compute_dtype(self, dtype) -> 'Squeezeformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: a Squeezeformer '
                "encoder stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def _no_chunks(self, *args, **kwargs):
        raise NotImplementedError(
            'forward_encoder_chunk: Conformer encoders only (a Squeezeformer encoder is outside '
            "the accelerated path of chunk-by-chunk encoding: the time reduction's caches)")

    def _check_simulate_streaming(self, speech):
        self._no_chunks()

    forward_encoder_chunk = _no_chunks
    forward_encoder_chunk_batch = _no_chunks
    forward_encoder_chunk_by_chunk = _no_chunks
