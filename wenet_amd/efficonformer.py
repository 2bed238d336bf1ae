"""Efficient Conformer encoders (`encoder: efficientConformer`) under the asr_model head, on
libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * EfficientConformerEncoder                 wenet/models/efficient_conformer/encoder.py:38-295
  * StrideConformerEncoderLayer               efficient_conformer/encoder_layer.py:76-165
  * GroupedRelPositionMultiHeadedAttention    efficient_conformer/attention.py:83-126, 180-258
  * ConvolutionModule with a stride           efficient_conformer/convolution.py:93-154
  * Conv2dSubsampling2                        efficient_conformer/subsampling.py:25-75

The conv2d front end, the rel-pos attention of the plain layers, the feed-forward and conv modules,
after_norm, the CTC head, both decoders and every search are `ASRModel`'s; the grouped attention,
the strided depthwise conv and the average-pool residual are csrc/efficonformer.hip, the layer
stack csrc/cabi_efficonformer.hip: a plain fp32 path.

Every utterance is encoded as the reference encodes it ALONE: in a padded
reference batch the last key group of a shorter utterance mixes in padding frames and the average
pool folds one into an odd length's last frame, so its batched output depends on the batch.  Here
alone and batched results are the same bits.
"""
import ctypes

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml

WIDTHS = (64, 128, 256, 512)      # output_size: the widths the depthwise conv kernels have
GROUPED_WIDTHS = (96, 192)        # group_size * d_k: the instantiations of attention_grouped
MAX_STRIDE_LAYERS = 4


def _refuse(key, got, want):
    raise NotImplementedError(
        f'encoder_conf.{key}={got!r} is outside the accelerated path (the Efficient Conformer '
        f'kernels need {want})')


# key -> (accepted values, the reference's default when the key is missing)
_TABLE = dict(input_layer=(('conv2d', 'conv2d2'), 'conv2d'),
              pos_enc_layer_type=(('rel_pos', ), 'rel_pos'),
              normalize_before=((True, ), True),
              macaron_style=((True, ), True),
              use_cnn_module=((True, ), True),
              activation_type=(('swish', ), 'swish'),
              cnn_module_norm=(('layer_norm', 'batch_norm'), 'batch_norm'),
              causal=((True, False), False),
              use_dynamic_chunk=((True, False), False),
              use_dynamic_left_chunk=((True, False), False),
              stride_kernel=((True, False), True))
# the keys of efficient_conf, which init_model flattens into the encoder's arguments
_EFFICIENT = ('stride_layer_idx', 'stride', 'group_layer_idx', 'group_size', 'stride_kernel')
# read below, or without effect on inference
_OTHER = ('input_size', 'output_size', 'attention_heads', 'linear_units', 'num_blocks',
          'dropout_rate', 'positional_dropout_rate', 'attention_dropout_rate',
          'cnn_module_kernel', 'static_chunk_size', 'efficient_conf') + _EFFICIENT


def _index_list(key, v):
    """stride_layer_idx / stride / group_layer_idx: an int or a list / tuple of ints -> list."""
    if isinstance(v, int) and not isinstance(v, bool):
        return [v]
    if isinstance(v, (list, tuple)) and all(
            isinstance(x, int) and not isinstance(x, bool) for x in v):
        return list(v)
    _refuse(key, v, 'an int or a list of ints')


def efficonformer_plan(configs: dict) -> dict:
    """The layer plan of an `encoder: efficientConformer` recipe: `stride_layers`,
    `group_layers`, per layer its conv `kernels` and the `rates` it runs at (the product of the
    strides in front of it), `front_rate` and `total_rate`.  Every value without a kernel is
    refused, naming its key."""
    enc = configs.get('encoder')
    if enc != 'efficientConformer':
        raise NotImplementedError(f'encoder {enc!r} is outside the accelerated path')
    ec = dict(configs.get('encoder_conf') or {})
    nested = ec.get('efficient_conf')
    if nested is not None:
        if not isinstance(nested, dict):
            _refuse('efficient_conf', nested, 'a mapping')
        for k in nested:
            if k not in _EFFICIENT:
                _refuse(f'efficient_conf.{k}', nested[k], 'a key EfficientConformerEncoder takes')
            if k in ec:    # (init_model passes both: a duplicate keyword argument)
                _refuse(k, ec[k], 'the key either in efficient_conf or flattened, not both')
        ec.update(nested)
    for k in ec:
        if k not in _TABLE and k not in _OTHER:
            _refuse(k, ec[k], 'a key EfficientConformerEncoder takes')
    for k, (accepted, default) in _TABLE.items():
        got = ec.get(k, default)
        if got not in accepted or (isinstance(got, bool) != isinstance(accepted[0], bool)):
            _refuse(k, got, ' or '.join(repr(a) for a in accepted))
    d = ec.get('output_size', 256)
    if d not in WIDTHS:
        _refuse('output_size', d, f'one of {WIDTHS}')
    heads = ec.get('attention_heads', 4)
    if not isinstance(heads, int) or heads <= 0 or d % heads or d // heads not in (32, 64):
        _refuse('attention_heads', heads, f'a head width of 32 or 64 (output_size {d})')
    blocks = ec.get('num_blocks', 6)
    if not isinstance(blocks, int) or not 1 <= blocks <= 31:
        _refuse('num_blocks', blocks, '1..31')
    stride_layers = _index_list('stride_layer_idx', ec.get('stride_layer_idx', 3))
    strides = _index_list('stride', ec.get('stride', 2))
    group_layers = _index_list('group_layer_idx', ec.get('group_layer_idx', (0, 1, 2, 3)))
    if any(s != 2 for s in strides):
        _refuse('stride', ec.get('stride', 2), 'a stride of 2 in every stride layer')
    if len(strides) != len(stride_layers):
        _refuse('stride', ec.get('stride', 2), 'one stride per stride_layer_idx entry')
    if len(stride_layers) > MAX_STRIDE_LAYERS or sorted(set(stride_layers)) != stride_layers or \
            any(not 0 <= i < blocks for i in stride_layers):
        _refuse('stride_layer_idx', ec.get('stride_layer_idx', 3),
                f'at most {MAX_STRIDE_LAYERS} ascending layer indices below num_blocks')
    group_layers = sorted(set(group_layers))
    if any(not 0 <= i < blocks for i in group_layers):
        _refuse('group_layer_idx', ec.get('group_layer_idx'), 'layer indices below num_blocks')
    g = ec.get('group_size', 3)
    if group_layers and (not isinstance(g, int) or isinstance(g, bool) or g < 1
                         or g * (d // heads) not in GROUPED_WIDTHS):
        _refuse('group_size', g,
                f'group_size * (output_size / attention_heads) in {GROUPED_WIDTHS}: other head '
                'widths have no instantiation of attention_grouped')
    causal = bool(ec.get('causal', False))
    K = ec.get('cnn_module_kernel', 15)
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= 63:
        _refuse('cnn_module_kernel', K, '1..63')
    stride_kernel = bool(ec.get('stride_kernel', True))
    kernels, rates, rate = [], [], 1
    for i in range(blocks):
        if K < 1 or (not causal and K % 2 != 1):
            _refuse('cnn_module_kernel', ec.get('cnn_module_kernel', 15),
                    f'an odd kernel in every layer of a non-causal model (layer {i} gets {K}'
                    + (' with stride_kernel: true)' if stride_kernel else ')'))
        kernels.append(K)
        rates.append(rate)
        if i in stride_layers:
            rate *= 2
            if stride_kernel:
                K = K // 2
    static = ec.get('static_chunk_size', 0)
    if static and static > 0 and static % rate:
        _refuse('static_chunk_size', static, f'a multiple of the product of the strides, {rate}')
    front = 2 if ec.get('input_layer', 'conv2d') == 'conv2d2' else 4
    return dict(ec=ec, d=d, heads=heads, head_dim=d // heads, blocks=blocks,
                stride_layers=stride_layers, group_layers=group_layers, group_size=g,
                stride_kernel=stride_kernel, kernels=kernels, rates=rates, front_rate=front,
                total_rate=rate, causal=causal)


def efficonformer_config_from_yaml(configs: dict):
    """train.yaml dict of an `encoder: efficientConformer` recipe -> (wn_config,
    wn_efficonformer_config).  The decoder, tokenizer and model keys are read as for a Conformer
    model; every encoder value without a kernel is refused, naming its key."""
    plan = efficonformer_plan(configs)
    ec = plan['ec']
    # everything that is not the encoder's own: the Conformer reading of the same file
    base = dict(configs, encoder='conformer')
    base['encoder_conf'] = dict(
        output_size=plan['d'], attention_heads=plan['heads'],
        num_blocks=plan['blocks'], linear_units=ec.get('linear_units', 2048),
        causal=plan['causal'], use_dynamic_chunk=bool(ec.get('use_dynamic_chunk', False)),
        static_chunk_size=ec.get('static_chunk_size', 0), norm_eps=1e-5,
        cnn_module_norm=ec.get('cnn_module_norm', 'batch_norm'),
        cnn_module_kernel=plan['kernels'][0])
    c = config_from_yaml(base)
    e = _lib.WnEfficonformerConfig()
    e.group_size = plan['group_size'] if plan['group_layers'] else 1
    e.group_mask = sum(1 << i for i in plan['group_layers'])
    e.n_stride = len(plan['stride_layers'])
    for j, i in enumerate(plan['stride_layers']):
        e.stride_layers[j] = i
    e.stride_kernel = int(plan['stride_kernel'])
    e.front_rate = plan['front_rate']
    e.head_dim = plan['head_dim']
    return c, e


class EfficientConformer(ASRModel):
    """An ASRModel whose encoder is an Efficient Conformer.  decode() with every mode of an
    ASRModel with the same decoder, transcribe, align, context biasing, clone() and
    DecodePipeline work unchanged; decoding_chunk_size / num_decoding_left_chunks change the
    attention mask only, as in the reference.  `plan` is the parsed layer plan."""

    def _config(self, configs: dict) -> _lib.WnConfig:
        if configs.get('model', 'asr_model') == 'transducer':
            raise NotImplementedError(
                "model 'transducer' with encoder 'efficientConformer' is outside the accelerated "
                'path')
        cfg, self._ecfg = efficonformer_config_from_yaml(configs)
        self.plan = {k: v for k, v in efficonformer_plan(configs).items() if k != 'ec'}
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_efficonformer(ctypes.byref(self._cfg), ctypes.byref(self._ecfg),
                                               tensors, n, self.device.index, ctypes.byref(h))

    def subsampling_rate(self) -> int:
        """The TRUE frame rate of the encoder output: the front end's rate times the product of
        the strides.  (The reference's subsampling_rate() reports the front end's alone, which
        puts its own alignment times off by that product: DESIGN.md section 1.)"""
        return self.plan['front_rate'] * self.plan['total_rate']

    def right_context(self) -> int:
        return 6 if self.plan['front_rate'] == 4 else 2   # subsampling.py right_context

    def _chunk_mask_size(self, decoding_chunk_size: int) -> int:
        """The chunk size of the attention mask a call gets (0: full context), mask.py:126-198."""
        if self._cfg.use_dynamic_chunk:
            return decoding_chunk_size if decoding_chunk_size > 0 else 0
        return max(self._cfg.static_chunk_size, 0)

    def _final_frames(self, t0: int) -> int:
        for _ in self.plan['stride_layers']:
            t0 = (t0 + 1) // 2
        return t0

    def _encode(self, speech, lens, chunk, left, want_out: bool):
        import numpy as np
        import torch
        from wenet_amd.model import _stream_ptr
        cs = self._chunk_mask_size(chunk)
        total = self.plan['total_rate']
        if cs % total:
            raise NotImplementedError(
                f'decoding_chunk_size={chunk} (a chunk mask of size {cs}) is outside the '
                f'accelerated path: the mask size must be divisible by the product of the '
                f'strides, {total} (its mask behind a stride layer is no chunk window otherwise)')
        B, T, F = speech.shape
        assert F == self._cfg.feat_dim, 'feature dimension mismatch'
        t0 = ((T - 1) // 2 - 1) // 2 if self.plan['front_rate'] == 4 else (T - 1) // 2
        Tp = self._final_frames(t0)
        enc_lens = np.zeros((B, ), dtype=np.int32)
        out = None
        if want_out:
            out = torch.empty((B, Tp, self._cfg.d_model), dtype=torch.float32, device=self.device)
        _lib.check(
            self._L.wn_encode(self._h, speech.data_ptr(), _lib.i32p(lens), B, T, chunk, left,
                              out.data_ptr() if out is not None else None, _lib.i32p(enc_lens),
                              _stream_ptr(self.device)),
            'wn_encode')
        return out, enc_lens, Tp

    def set_compute_dtype(self, dtype) -> 'EfficientConformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: an Efficient Conformer '
                "encoder stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def set_global_chunk_size(self, global_chunk_size):
        raise NotImplementedError(
            f'global_chunk_size={global_chunk_size!r} is outside the accelerated path: the ONNX '
            'export path of EfficientConformerEncoder (encoder.py:217-229)')

    def _no_chunks(self, *args, **kwargs):
        raise NotImplementedError(
            'forward_encoder_chunk: Conformer encoders only (an Efficient Conformer encoder is '
            'outside the accelerated path of chunk-by-chunk encoding: the rate-mixed attention '
            'cache of efficient_conformer/encoder.py:297-459)')

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError(
            'simulate_streaming is outside the accelerated path of an Efficient Conformer encoder '
            '(the rate-mixed attention cache of efficient_conformer/encoder.py:297-459)')

    forward_encoder_chunk = _no_chunks
    forward_encoder_chunk_batch = _no_chunks
    forward_encoder_chunk_by_chunk = _no_chunks
