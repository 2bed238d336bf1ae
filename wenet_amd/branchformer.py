"""Branchformer and E-Branchformer encoders (`encoder: branchformer` / `e_branchformer`) under
the asr_model head, on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * BranchformerEncoder / ...EncoderLayer     wenet/models/branchformer/encoder.py:28-134,
                                              encoder_layer.py:26-206
  * ConvolutionalGatingMLP                    wenet/models/branchformer/cgmlp.py:30-194
  * EBranchformerEncoder / ...EncoderLayer    wenet/models/e_branchformer/encoder.py:32-180,
                                              encoder_layer.py:27-148

The front end, the rel-pos attention, the feed-forward modules, after_norm, the CTC head, both
decoders and every search are `ASRModel`'s; the cgMLP's gating unit and the E-Branchformer merge
conv are csrc/branchformer.hip, the layer stack csrc/cabi_branchformer.hip: a plain fp32 path.

Every utterance is encoded as the reference encodes it ALONE: the
reference's cgMLP and merge convs ignore the padding mask, so in a reference batch a shorter
utterance of a non-causal model reads the batch's subsampled padding.  Here a conv sees the
utterance's own frames and its own zero padding; alone and batched results are the same bits.
"""
import ctypes

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml

ENCODERS = ('branchformer', 'e_branchformer')
MAX_GATE_CHANNELS = 1024      # csgu_gate: cgmlp_linear_units / 2, a multiple of 64
MAX_CONV_KERNEL = 63


def _refuse(key, got, want):
    raise NotImplementedError(
        f'encoder_conf.{key}={got!r} is outside the accelerated path (the Branchformer kernels '
        f'need {want})')


# key -> (required value, the reference's default when the key is missing)
_COMMON = dict(input_layer=('conv2d', 'conv2d'), pos_enc_layer_type=('rel_pos', 'rel_pos'),
               selfattention_layer_type=('rel_selfattn', 'rel_selfattn'),
               gate_activation=('identity', 'identity'), query_bias=(True, True),
               key_bias=(True, True), value_bias=(True, True),
               layer_norm_type=('layer_norm', 'layer_norm'), n_kv_head=(None, None),
               head_dim=(None, None))
_BRANCHFORMER = dict(merge_method=('concat', 'concat'), use_attn=(True, True),
                     use_cgmlp=(True, True))
_EBRANCHFORMER = dict(use_ffn=(True, True), macaron_style=(True, True),
                      activation_type=('swish', 'swish'), conv_bias=(True, True),
                      mlp_type=('position_wise_feed_forward', 'position_wise_feed_forward'),
                      mlp_bias=(True, True))


def branchformer_config_from_yaml(configs: dict):
    """train.yaml dict of an `encoder: branchformer` / `e_branchformer` recipe ->
    (wn_config, wn_branchformer_config).  The decoder, tokenizer and model keys are read as for a
    Conformer model; every encoder value without a kernel is refused, naming its key."""
    enc = configs.get('encoder')
    if enc not in ENCODERS:
        raise NotImplementedError(f'encoder {enc!r} is outside the accelerated path')
    ec = configs['encoder_conf']
    table = dict(_COMMON)
    table.update(_BRANCHFORMER if enc == 'branchformer' else _EBRANCHFORMER)
    for k, (want, default) in table.items():
        got = ec.get(k, default)
        if got != want:
            _refuse(k, got, repr(want))
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    if heads <= 0 or d % heads != 0 or d // heads not in (32, 64):
        _refuse('output_size / attention_heads', d / max(heads, 1), 'a head width of 32 or 64')
    causal = bool(ec.get('causal', False))
    U = ec.get('cgmlp_linear_units', 2048)
    if U % 128 != 0 or not 128 <= U <= 2 * MAX_GATE_CHANNELS:
        _refuse('cgmlp_linear_units', U,
                f'a multiple of 128 up to {2 * MAX_GATE_CHANNELS} (gate channels in 64s)')
    K = ec.get('cgmlp_conv_kernel', 31)
    if not 1 <= K <= MAX_CONV_KERNEL or (not causal and K % 2 != 1):
        _refuse('cgmlp_conv_kernel', K, f'1..{MAX_CONV_KERNEL}, odd unless causal')
    Km = ec.get('merge_conv_kernel', 3) if enc == 'e_branchformer' else 0
    if enc == 'e_branchformer' and (not 1 <= Km <= MAX_CONV_KERNEL
                                    or (not causal and Km % 2 != 1)):
        _refuse('merge_conv_kernel', Km, f'1..{MAX_CONV_KERNEL}, odd unless causal')
    # everything that is not the encoder's own: the Conformer reading of the same file, with the
    # encoder keys it would refuse or misread taken out
    base = dict(configs, encoder='conformer')
    base['encoder_conf'] = dict(
        output_size=d, attention_heads=heads, num_blocks=ec.get('num_blocks', 12),
        linear_units=ec.get('linear_units', 2048) if enc == 'e_branchformer' else U,
        causal=causal, use_dynamic_chunk=ec.get('use_dynamic_chunk', False),
        static_chunk_size=ec.get('static_chunk_size', 0), norm_eps=ec.get('norm_eps', 1e-5),
        cnn_module_norm='layer_norm', cnn_module_kernel=1)
    c = config_from_yaml(base)
    if c.ffn_dim % 32 != 0:
        _refuse('linear_units', c.ffn_dim, 'a multiple of 32')
    b = _lib.WnBranchformerConfig()
    b.kind = 1 if enc == 'branchformer' else 2
    b.cgmlp_units, b.cgmlp_kernel, b.merge_kernel = U, K, Km
    b.linear_after_conv = int(bool(ec.get('use_linear_after_conv', False)))
    b.head_dim = d // heads
    return c, b


class Branchformer(ASRModel):
    """An ASRModel whose encoder is a Branchformer or an E-Branchformer.  decode() with every
    mode of an ASRModel with the same decoder, transcribe, align, context biasing, clone() and
    DecodePipeline work unchanged; decoding_chunk_size / num_decoding_left_chunks change the
    attention mask only, as in the reference."""

    def _config(self, configs: dict) -> _lib.WnConfig:
        if configs.get('model', 'asr_model') == 'transducer':
            raise NotImplementedError(
                f"model 'transducer' with encoder {configs.get('encoder')!r} is outside the "
                'accelerated path')
        cfg, self._bcfg = branchformer_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_branchformer(ctypes.byref(self._cfg), ctypes.byref(self._bcfg),
                                              tensors, n, self.device.index, ctypes.byref(h))

    def set_compute_dtype(self, dtype) -> 'Branchformer':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: a Branchformer '
                "encoder stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def _no_chunks(self, *args, **kwargs):
        raise NotImplementedError(
            'forward_encoder_chunk: Conformer encoders only (a Branchformer encoder is outside '
            "the accelerated path of chunk-by-chunk encoding: the cgMLP's conv cache)")

    def _check_simulate_streaming(self, speech):
        self._no_chunks()

    forward_encoder_chunk = _no_chunks
    forward_encoder_chunk_batch = _no_chunks
    forward_encoder_chunk_by_chunk = _no_chunks
