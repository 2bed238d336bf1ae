"""ctypes binding of libwenet_amd.so (include/wenet_amd.h).

There is deliberately no fallback: if the HIP library is missing or fails to
load, every use of the model raises.
"""
import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int32,
                    c_int64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libwenet_amd.so')


class WnConfig(Structure):
    _fields_ = [(n, c_int32) for n in (
        'feat_dim', 'd_model', 'n_heads', 'ffn_dim', 'n_layers', 'cnn_kernel',
        'causal', 'use_dynamic_chunk', 'static_chunk_size', 'vocab',
        'has_cmvn', 'dec_heads', 'dec_ffn_dim', 'dec_layers', 'dec_r_layers',
        'bidirectional', 'sos', 'eos', 'max_pos')] + [('norm_eps', c_float)] + [
            (n, c_int32) for n in ('encoder_type', 'input_layer', 'activation',
                                   'key_bias', 'cnn_norm',
                                   # decoder variants (the Whisper decoder); 0 = classic
                                   'dec_activation', 'dec_key_bias', 'dec_src_key_bias',
                                   'dec_learned_pos', 'dec_max_pos')]


class WnTransducerConfig(Structure):
    """wn_transducer_config: predictor / joint widths of a hybrid transducer."""
    _fields_ = [(n, c_int32) for n in ('pred_embed', 'pred_hidden', 'pred_layers', 'pred_out',
                                       'join_dim', 'blank')]


class WnStatelessPredictorConfig(Structure):
    """wn_stateless_predictor_config: an embedding (kind 1) or conv (kind 2) predictor."""
    _fields_ = [(n, c_int32) for n in ('kind', 'context', 'heads', 'activation', 'conv_bias')] + [
        ('norm_eps', c_float)]


class WnFireRedConfig(Structure):
    """wn_firered_config: what a FireRedASR-AED encoder has on top of wn_config."""
    _fields_ = [(n, c_int32) for n in ('sub_channels', 'conv_inner_factor', 'max_frames')] + [
        ('attn_norm_eps', c_float)]


class WnBranchformerConfig(Structure):
    """wn_branchformer_config: what a Branchformer / E-Branchformer encoder has on top of
    wn_config."""
    _fields_ = [(n, c_int32) for n in ('kind', 'cgmlp_units', 'cgmlp_kernel', 'merge_kernel',
                                       'linear_after_conv', 'head_dim')]


class WnParaformerConfig(Structure):
    """wn_paraformer_config: what a Paraformer has on top of wn_config."""
    _fields_ = [(n, c_int32) for n in ('lfr_m', 'lfr_n', 'kernel_size', 'dec_blocks',
                                       'max_frames')] + [
        (n, c_float) for n in ('threshold', 'tail_threshold', 'smooth_factor',
                               'noise_threshold')]


class WnSenseVoiceConfig(Structure):
    """wn_sensevoice_config: what a SenseVoice Small model has on top of wn_config."""
    _fields_ = [(n, c_int32) for n in ('lfr_m', 'lfr_n', 'kernel_size', 'tp_blocks',
                                       'max_frames', 'n_query', 'n_embed')]


class WnSqueezeformerConfig(Structure):
    """wn_squeezeformer_config: what a Squeezeformer encoder has on top of wn_config."""
    _fields_ = [(n, c_int32) for n in ('reduce_idx', 'recover_idx', 'reduce_kernel',
                                       'do_rel_shift')]


class WnEfficonformerConfig(Structure):
    """wn_efficonformer_config: what an Efficient Conformer encoder has on top of wn_config."""
    _fields_ = [('group_size', c_int32), ('group_mask', c_int32), ('n_stride', c_int32),
                ('stride_layers', c_int32 * 4), ('stride_kernel', c_int32),
                ('front_rate', c_int32), ('head_dim', c_int32)]


class WnTensor(Structure):
    _fields_ = [('name', c_char_p), ('data', POINTER(c_float)),
                ('numel', c_int64)]


class WnStreamResult(Structure):
    """wn_stream_result: where wn_stream_advance* put a call's results (host arrays)."""
    _fields_ = [('n_hyps', POINTER(c_int32)), ('hyp_lens', POINTER(c_int32)),
                ('hyp_tlens', POINTER(c_int32)), ('hyp_tokens', POINTER(c_int32)),
                ('hyp_times', POINTER(c_int32)), ('hyp_scores', POINTER(c_double)),
                ('hyp_viterbi', POINTER(c_double)), ('frames_decoded', POINTER(c_int32)),
                ('trailing_blank', POINTER(c_int32)), ('max_len', c_int32)]


class WnRnntStreamResult(Structure):
    """wn_rnnt_stream_result: where wn_rnnt_stream_advance_encoded puts a call's results (host
    arrays)."""
    _fields_ = [('tok_lens', POINTER(c_int32)), ('tokens', POINTER(c_int32)),
                ('times', POINTER(c_int32)), ('frames_decoded', POINTER(c_int32)),
                ('trailing_blank', POINTER(c_int32)), ('max_len', c_int32),
                ('steps', POINTER(c_int32))]


class WnRnntBeamStreamResult(Structure):
    """wn_rnnt_beam_stream_result: where wn_rnnt_beam_stream_advance_encoded puts a call's
    results (host arrays)."""
    _fields_ = [('n_hyps', POINTER(c_int32)), ('hyp_lens', POINTER(c_int32)),
                ('hyp_tokens', POINTER(c_int32)), ('hyp_scores', POINTER(c_double)),
                ('frames_decoded', POINTER(c_int32)), ('trailing_blank', POINTER(c_int32)),
                ('max_len', c_int32)]


class WnAttentionOp(Structure):
    """wn_attention_op: the arguments of wn_op_attention."""
    _fields_ = [('Q', c_void_p), ('K', c_void_p), ('V', c_void_p),
                ('ldq', c_int32), ('ldk', c_int32), ('ldv', c_int32),
                ('q_rows', c_int32), ('kv_rows', c_int32),
                ('P', c_void_p), ('ldp', c_int32), ('p_rows', c_int32),
                ('p_off', POINTER(c_int32)), ('bias_u', c_void_p), ('bias_v', c_void_p),
                ('O', c_void_p), ('ldo', c_int32),
                ('q_off', POINTER(c_int32)), ('q_len', POINTER(c_int32)),
                ('kv_off', POINTER(c_int32)), ('kv_len', POINTER(c_int32)),
                ('n_seq', c_int32), ('n_heads', c_int32), ('mask_mode', c_int32),
                ('chunk_size', c_int32), ('left_chunks', c_int32), ('scale', c_float),
                ('flags', c_int32), ('precision', c_int32), ('x6_galign', c_int32)]


class WnGemmOp(Structure):
    """wn_gemm_op: the arguments of wn_op_gemm_ex."""
    _fields_ = [('A', c_void_p), ('W', c_void_p), ('bias', c_void_p), ('resid', c_void_p),
                ('C', c_void_p), ('M', c_int32), ('N', c_int32), ('K', c_int32),
                ('lda', c_int32), ('ldc', c_int32), ('ldr', c_int32), ('alpha', c_float),
                ('act', c_int32), ('glu', c_int32), ('precision', c_int32),
                ('a_row_off', POINTER(c_int64)), ('a_elems', c_int64), ('conv_C', c_int32),
                ('conv_sy', c_int64), ('conv_sx', c_int64)]


class WnGemmLowpOp(Structure):
    """wn_gemm_lowp_op: the arguments of wn_op_gemm_lowp_ex."""
    _fields_ = [('A', c_void_p), ('W', c_void_p), ('bias', c_void_p), ('resid', c_void_p),
                ('C', c_void_p), ('a_scale', c_void_p), ('w_scale', c_void_p),
                ('c_scale', c_void_p), ('M', c_int32), ('N', c_int32), ('K', c_int32),
                ('lda', c_int32), ('ldc', c_int32), ('ldr', c_int32),
                ('a_scale_pitch', c_int32), ('w_scale_pitch', c_int32),
                ('c_scale_pitch', c_int32), ('alpha', c_float), ('act', c_int32),
                ('glu', c_int32), ('dtype', c_int32), ('c_mode', c_int32),
                ('a_bytes', c_int64), ('w_bytes', c_int64), ('a_scale_bytes', c_int64),
                ('w_scale_bytes', c_int64), ('c_scale_bytes', c_int64)]


# every symbol include/wenet_amd.h declares
EXPORTS = [
    'wn_last_error', 'wn_version', 'wn_model_create', 'wn_model_destroy', 'wn_model_clone',
    'wn_model_set_precision', 'wn_model_get_precision', 'wn_batch_size', 'wn_model_set_encode_gate', 'wn_op_gemm_bf16',
    'wn_op_gemm_bf16_stored', 'wn_op_gemm_ex', 'wn_op_gemm_lowp_ex', 'wn_op_mx_quantize_ex',
    'wn_attention_beam_search', 'wn_attention_beam_search_prompt', 'wn_attention_truncated',
    'wn_op_gemm_skinny', 'wn_encode_chunk_batch', 'wn_op_gemm_lowp', 'wn_op_mx_quantize', 'wn_op_ffn_fused', 'wn_op_gemm_x6', 'wn_op_ffn_x6', 'wn_op_gemm_x6r', 'wn_op_gemm_x6r512', 'wn_profile_kernel_name', 'wn_profile_ffn_split', 'wn_profile_ffn_clocks', 'wn_profile_gemm_clocks', 'wn_filter_blank_embedding',
    'wn_workspace_create', 'wn_resample_length', 'wn_resample', 'wn_fbank', 'wn_log_mel', 'wn_encode', 'wn_encode_chunk', 'wn_set_encoder_out',
    'wn_ctc_logprobs', 'wn_set_ctc_probs', 'wn_ctc_greedy_search', 'wn_ctc_force_align',
    'wn_set_context_graph', 'wn_ctc_prefix_beam_search', 'wn_attention_rescoring', 'wn_rescore', 'wn_rescore_prefetch', 'wn_decoder_forward', 'wn_decoder_next_topk', 'wn_op_gemm',
    'wn_op_layernorm', 'wn_op_log_add', 'wn_op_attention', 'wn_op_dwconv', 'wn_op_conv1',
    'wn_op_conv2d4',
    'wn_op_ctc_rows', 'wn_debug_set', 'wn_profile_enable',
    'wn_profile_collect', 'wn_tune_set', 'wn_model_tune_set', 'wn_tune_get',
    'wn_stream_create', 'wn_stream_destroy', 'wn_stream_set_endpoint', 'wn_stream_reset',
    'wn_stream_advance', 'wn_stream_advance_encoded',
    'wn_model_create_transducer', 'wn_transducer_greedy_search', 'wn_op_lstm_step',
    'wn_op_joint_argmax', 'wn_transducer_beam_search', 'wn_op_joint_fuse_topk',
    'wn_op_rnnt_beam_step', 'wn_transducer_beam_stats',
    'wn_rnnt_stream_create', 'wn_rnnt_stream_destroy', 'wn_rnnt_stream_reset',
    'wn_rnnt_stream_advance_encoded', 'wn_rnnt_stream_state',
    'wn_rnnt_beam_stream_create', 'wn_rnnt_beam_stream_destroy', 'wn_rnnt_beam_stream_reset',
    'wn_rnnt_beam_stream_advance_encoded', 'wn_rnnt_beam_stream_state',
    'wn_op_rnnt_beam_step_carry',
    'wn_transducer_score', 'wn_transducer_score_stats', 'wn_transducer_score_times',
    'wn_op_rnnt_trie',
    'wn_op_joint_logp_gather', 'wn_op_rnnt_lattice',
    'wn_op_attn_self_step', 'wn_op_attn_step_embed', 'wn_op_attn_prompt_cache', 'wn_op_beam_init',
    'wn_op_beam_update', 'wn_op_beam_finish',
    'wn_op_layernorm_ex', 'wn_op_layernorm2', 'wn_op_layernorm_mx', 'wn_op_ffn_reduce_ln',
    'wn_op_gemm_rowln',
    'wn_model_create_transducer_stateless', 'wn_op_stateless_step',
    'wn_op_attention_relshift', 'wn_op_firered_frontend', 'wn_model_create_firered',
    'wn_model_create_branchformer', 'wn_op_csgu_gate', 'wn_op_merge_dwconv', 'wn_csgu_time_tile',
    'wn_model_create_squeezeformer', 'wn_op_attention_sqshift', 'wn_op_time_reduce',
    'wn_op_time_recover',
    'wn_model_create_efficonformer', 'wn_op_attention_grouped', 'wn_op_stride_dwconv_ln_silu',
    'wn_op_avgpool_residual_add',
    'wn_op_attention_d128', 'wn_op_lfr_front', 'wn_op_layernorm_wide', 'wn_op_cif_alpha',
    'wn_op_cif_fire', 'wn_model_create_paraformer', 'wn_paraformer_decode',
    'wn_op_attention_d32',
    'wn_model_create_sensevoice', 'wn_sensevoice_set_queries', 'wn_op_sv_front',
]

_lib = None


def lib():
    """Load (once) and return the library; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -m wenet_amd.build` '
            '(hipcc --offload-arch=gfx950). wenet_amd has no CPU fallback.')
    # torch first: its bundled libamdhip64.so.7 must be the one HIP runtime in
    # the process so that torch device pointers and ours share a context.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    i32, i64, f32, vp = c_int32, c_int64, c_float, c_void_p
    pi32, pf64 = POINTER(c_int32), POINTER(c_double)
    L.wn_last_error.restype = c_char_p
    L.wn_profile_kernel_name.restype = c_char_p
    L.wn_profile_kernel_name.argtypes = [vp]
    L.wn_profile_ffn_split.restype = c_int32
    L.wn_profile_ffn_split.argtypes = [vp]
    L.wn_profile_ffn_clocks.argtypes = [POINTER(ctypes.c_uint64)]
    L.wn_profile_gemm_clocks.argtypes = [POINTER(ctypes.c_uint64)]
    L.wn_version.restype = c_char_p
    L.wn_model_create.argtypes = [POINTER(WnConfig), POINTER(WnTensor), i32,
                                  i32, POINTER(vp)]
    L.wn_model_destroy.argtypes = [vp]
    L.wn_model_clone.argtypes = [vp, POINTER(vp)]
    L.wn_model_destroy.restype = None
    L.wn_workspace_create.argtypes = [i32, POINTER(vp)]
    L.wn_fbank.argtypes = [vp, vp, POINTER(i64), i32, vp, i32, pi32, vp]
    L.wn_log_mel.argtypes = [vp, vp, POINTER(i64), i32, i32, vp, i32, pi32, vp]
    L.wn_encode.argtypes = [vp, vp, pi32, i32, i32, i32, i32, vp, pi32, vp]
    L.wn_set_encoder_out.argtypes = [vp, vp, pi32, i32, i32, vp]
    L.wn_ctc_logprobs.argtypes = [vp, i32, i32, f32, vp, i32, vp]
    L.wn_encode_chunk.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, pi32,
                                  pi32, vp]
    L.wn_encode_chunk_batch.argtypes = [vp, i32, vp, i32, pi32, i32, POINTER(vp), pi32,
                                        POINTER(vp), vp, POINTER(vp), POINTER(vp), pi32, pi32,
                                        vp]
    L.wn_resample_length.argtypes = [ctypes.c_int64, i32, i32]
    L.wn_resample_length.restype = ctypes.c_int64
    L.wn_resample.argtypes = [vp, vp, ctypes.c_int64, i32, i32, vp, ctypes.c_int64, vp]
    L.wn_set_ctc_probs.argtypes = [vp, vp, pi32, i32, i32, i32, i32, vp]
    L.wn_ctc_greedy_search.argtypes = [vp, i32, pi32, pi32, i32, vp]
    L.wn_ctc_force_align.argtypes = [vp, i32, f32, pi32, pi32, i32, vp, pi32, i32, i32, i32,
                                     pi32, POINTER(f32), pi32, POINTER(f32), POINTER(f32), vp]
    L.wn_set_context_graph.argtypes = [vp, i32, pi32, pf64, pf64, pf64, i32, pi32, pi32,
                                       pi32, vp]
    L.wn_ctc_prefix_beam_search.argtypes = [vp, i32, i32, pi32, pi32, pi32,
                                            pi32, pi32, pf64, i32, vp]
    L.wn_stream_create.argtypes = [vp, i32, i32, i32, i32, POINTER(vp), vp]
    L.wn_stream_destroy.argtypes = [vp]
    L.wn_stream_set_endpoint.argtypes = [vp, f32, f32]
    L.wn_stream_reset.argtypes = [vp, i32, pi32, vp]
    L.wn_stream_advance.argtypes = [vp, i32, pi32, vp, pi32, i32, i32, i32,
                                    POINTER(WnStreamResult), vp]
    L.wn_stream_advance_encoded.argtypes = [vp, i32, pi32, vp, pi32, i32, i32,
                                            POINTER(WnStreamResult), vp]
    L.wn_attention_rescoring.argtypes = [vp, i32, pi32, pi32, pi32, i32, f32,
                                         POINTER(f32), POINTER(f32), vp]
    L.wn_rescore.argtypes = [vp, i32, pi32, pi32, pi32, pf64, i32, c_double, c_double, pi32,
                             POINTER(f32), pf64, pf64, POINTER(f32), vp]
    L.wn_rescore_prefetch.argtypes = [vp, i32, vp]
    L.wn_decoder_forward.argtypes = [vp, i32, i32, i32, pi32, pi32, i32, vp, vp]
    L.wn_decoder_next_topk.argtypes = [vp, i32, pi32, pi32, pi32, i32, i32,
                                       POINTER(f32), pi32, vp]
    L.wn_attention_beam_search.argtypes = [vp, i32, i32, f32, pi32, pi32, vp]
    L.wn_attention_beam_search_prompt.argtypes = [vp, i32, i32, f32, pi32, i32, pi32, pi32, vp]
    L.wn_attention_truncated.argtypes = [vp]
    L.wn_op_gemm.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp]
    L.wn_op_gemm_skinny.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.wn_op_gemm_bf16.argtypes = L.wn_op_gemm.argtypes
    L.wn_op_gemm_ex.argtypes = [POINTER(WnGemmOp), pi32, vp]
    L.wn_op_gemm_bf16_stored.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, vp]
    L.wn_op_gemm_lowp.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32,
                                  i32, vp]
    L.wn_op_mx_quantize.argtypes = [vp, i32, i32, vp, vp, vp]
    L.wn_op_gemm_lowp_ex.argtypes = [POINTER(WnGemmLowpOp), pi32, vp]
    L.wn_op_mx_quantize_ex.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp]
    L.wn_op_ffn_fused.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32,
                                  f32, vp]
    L.wn_op_gemm_x6.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, i32, vp]
    L.wn_op_ffn_x6.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32,
                               f32, i32, vp]
    L.wn_filter_blank_embedding.argtypes = [vp, vp, pi32, pi32, vp]
    L.wn_op_gemm_x6r.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp]
    L.wn_op_gemm_x6r512.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32,
                                    i32, vp]
    L.wn_model_set_precision.argtypes = [vp, i32]
    L.wn_model_get_precision.argtypes = [vp]
    L.wn_batch_size.argtypes = [vp]
    L.wn_batch_size.restype = i32
    L.wn_model_set_encode_gate.argtypes = [vp, vp]
    L.wn_op_layernorm.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp]
    L.wn_op_log_add.argtypes = [vp, vp, vp, i32, vp]
    L.wn_op_attention.argtypes = [POINTER(WnAttentionOp), pi32, vp]
    L.wn_op_dwconv.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, pi32, pi32, i32, i32,
                               i32, i32, i32, i32, f32, vp]
    L.wn_op_conv1.argtypes = [vp, vp, vp, vp, vp, vp, pi32, pi32, i32, i32, i32, i32, i32, i32,
                              vp]
    L.wn_op_conv2d4.argtypes = [vp, vp, pi32, i32, i32, vp, vp, vp, pi32, pi32, vp]
    L.wn_op_ctc_rows.argtypes = [vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, i32, vp]
    L.wn_debug_set.argtypes = [vp, c_char_p, i32]
    L.wn_tune_set.argtypes = [c_char_p, i32]
    L.wn_model_tune_set.argtypes = [vp, c_char_p, i32]
    L.wn_tune_get.argtypes = [vp, c_char_p, pi32]
    L.wn_profile_enable.argtypes = [vp, i32]
    L.wn_profile_collect.argtypes = [vp, pi32, pf64, pf64]
    L.wn_model_create_transducer.argtypes = [POINTER(WnConfig), POINTER(WnTransducerConfig),
                                             POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_model_create_transducer_stateless.argtypes = [
        POINTER(WnConfig), POINTER(WnTransducerConfig), POINTER(WnStatelessPredictorConfig),
        POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_op_stateless_step.argtypes = [POINTER(WnStatelessPredictorConfig), pi32, POINTER(vp),
                                       pi32, vp, i32, i32, i32, i32, vp]
    L.wn_transducer_greedy_search.argtypes = [vp, i32, pi32, pi32, i32, pi32, vp]
    L.wn_rnnt_stream_create.argtypes = [vp, i32, i32, i32, i32, POINTER(vp), vp]
    L.wn_rnnt_stream_destroy.argtypes = [vp]
    L.wn_rnnt_stream_reset.argtypes = [vp, i32, pi32, vp]
    L.wn_rnnt_stream_advance_encoded.argtypes = [vp, i32, pi32, vp, pi32, i32,
                                                 POINTER(WnRnntStreamResult), vp]
    L.wn_rnnt_stream_state.argtypes = [vp, i32, POINTER(f32), POINTER(f32), POINTER(f32), pi32,
                                       vp]
    L.wn_rnnt_beam_stream_create.argtypes = [vp, i32, i32, i32, f32, f32, POINTER(vp), vp]
    L.wn_rnnt_beam_stream_destroy.argtypes = [vp]
    L.wn_rnnt_beam_stream_reset.argtypes = [vp, i32, pi32, vp]
    L.wn_rnnt_beam_stream_advance_encoded.argtypes = [vp, i32, pi32, vp, pi32, i32,
                                                      POINTER(WnRnntBeamStreamResult), vp]
    L.wn_rnnt_beam_stream_state.argtypes = [vp, i32, pi32, pf64, pi32, pi32, POINTER(f32),
                                            POINTER(f32), POINTER(f32), vp]
    L.wn_op_rnnt_beam_step_carry.argtypes = [i32, i32, i32, i32, i32, pi32, i32, pi32, pf64, pi32,
                                             pi32, POINTER(f32), pi32, pi32, pi32, pi32, pi32,
                                             pi32, pf64, pi32, pi32, pi32, pi32, pi32, pi32, pi32,
                                             pi32, vp]
    L.wn_op_lstm_step.argtypes = [vp, POINTER(vp), i32, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                  i32, vp]
    L.wn_op_joint_argmax.argtypes = [vp, i32, vp, i32, pi32, pi32, vp, vp, i32, i32, i32, pi32,
                                     POINTER(f32), vp]
    L.wn_transducer_beam_search.argtypes = [vp, i32, f32, f32, pi32, pi32, pi32, pf64, i32, vp]
    L.wn_transducer_beam_stats.argtypes = [vp, pi32, POINTER(i64)]
    L.wn_op_joint_fuse_topk.argtypes = [vp, i32, vp, i32, pi32, pi32, vp, vp, i32, i32, i32, vp,
                                        i32, pi32, f32, f32, i32, POINTER(f32), pi32,
                                        POINTER(f32), vp]
    L.wn_op_rnnt_beam_step.argtypes = [i32, i32, i32, i32, i32, pi32, i32, pi32, pf64, pi32, pi32,
                                       POINTER(f32), pi32, pi32, pf64, pi32, pi32, pi32, pi32,
                                       pi32, pi32, vp]
    L.wn_transducer_score.argtypes = [vp, i32, pi32, pi32, pi32, i32, pf64, vp]
    L.wn_transducer_score_stats.argtypes = [vp, POINTER(i64), POINTER(i64), pi32]
    L.wn_transducer_score_times.argtypes = [vp, POINTER(f32)]
    L.wn_op_rnnt_trie.argtypes = [i32, pi32, pi32, i32, i32, pi32, pi32, pi32, pi32, pi32, pi32,
                                  pi32]
    L.wn_op_joint_logp_gather.argtypes = [vp, i32, vp, i32, pi32, pi32, vp, vp, i32, i32, i32,
                                          pi32, pi32, POINTER(f32), vp]
    L.wn_op_rnnt_lattice.argtypes = [i32, pi32, pi32, POINTER(f32), POINTER(f32), pf64, vp]
    L.wn_op_attn_self_step.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, vp, vp]
    L.wn_op_attn_step_embed.argtypes = [vp, i32, vp, i32, vp, i32, f32, i32, i32, vp, vp]
    L.wn_op_attn_prompt_cache.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    L.wn_op_beam_init.argtypes = [i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.wn_op_beam_update.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, i32, pi32, vp]
    L.wn_op_beam_finish.argtypes = [i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp]
    L.wn_op_layernorm_ex.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, f32, i32, vp]
    L.wn_op_layernorm2.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp]
    L.wn_op_layernorm_mx.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, f32, vp]
    L.wn_op_ffn_reduce_ln.argtypes = [vp, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, i64, i32, i32,
                                      f32, i32, vp]
    L.wn_op_gemm_rowln.argtypes = [vp, i32, vp, vp, vp, i32, f32, vp, i32, vp, vp, f32, vp, i32,
                                   i32, i32, vp]
    L.wn_model_create_firered.argtypes = [POINTER(WnConfig), POINTER(WnFireRedConfig),
                                          POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_op_attention_relshift.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp,
                                           vp, vp, i32, pi32, pi32, i32, i32, f32, vp]
    L.wn_op_firered_frontend.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, pi32, pi32,
                                         pi32, i32, i32, i32, i32, vp]
    L.wn_model_create_branchformer.argtypes = [POINTER(WnConfig), POINTER(WnBranchformerConfig),
                                               POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_op_csgu_gate.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, i32, pi32,
                                  pi32, i32, vp]
    L.wn_op_merge_dwconv.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, pi32, pi32,
                                     i32, vp]
    L.wn_csgu_time_tile.argtypes = []
    L.wn_model_create_squeezeformer.argtypes = [POINTER(WnConfig), POINTER(WnSqueezeformerConfig),
                                                POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_op_attention_sqshift.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp,
                                          vp, i32, pi32, pi32, i32, i32, f32, vp]
    L.wn_op_time_reduce.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, i32, pi32, pi32,
                                    pi32, i32, vp]
    L.wn_op_time_recover.argtypes = [vp, i32, vp, i32, i32, vp, i32, i32, i32, pi32, pi32, pi32,
                                     i32, vp]
    L.wn_model_create_efficonformer.argtypes = [POINTER(WnConfig), POINTER(WnEfficonformerConfig),
                                                POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_op_attention_grouped.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, pi32, vp,
                                          vp, vp, i32, pi32, pi32, i32, i32, i32, i32, i32, i32,
                                          i32, f32, vp]
    L.wn_op_stride_dwconv_ln_silu.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, f32,
                                              i32, i32, i32, vp, i32, i32, pi32, pi32, pi32, i32,
                                              vp]
    L.wn_op_avgpool_residual_add.argtypes = [vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, pi32,
                                             pi32, pi32, i32, vp]
    L.wn_model_create_paraformer.argtypes = [POINTER(WnConfig), POINTER(WnParaformerConfig),
                                             POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_paraformer_decode.argtypes = [vp, pi32, pi32, POINTER(f32), pi32, pi32, i32, vp]
    L.wn_op_attention_d128.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, pi32, pi32,
                                       pi32, pi32, i32, i32, f32, vp]
    L.wn_op_attention_d32.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, pi32, pi32,
                                      pi32, pi32, i32, i32, f32, i32, vp]
    L.wn_op_lfr_front.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, pi32, pi32, pi32,
                                  i32, i32, i32, i32, i32, f32, f32, vp]
    L.wn_op_layernorm_wide.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, f32, vp]
    L.wn_op_cif_alpha.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, f32, f32, vp, pi32, pi32,
                                  i32, vp]
    L.wn_op_cif_fire.argtypes = [vp, i32, i32, i32, vp, pi32, pi32, i32, f32, f32, vp, i32, i32,
                                 pi32, pi32, pi32, pi32, pi32, vp]
    L.wn_model_create_sensevoice.argtypes = [POINTER(WnConfig), POINTER(WnSenseVoiceConfig),
                                             POINTER(WnTensor), i32, i32, POINTER(vp)]
    L.wn_sensevoice_set_queries.argtypes = [vp, pi32, i32]
    # feats mean istd embed pe | pe_rows | ln_w ln_b out | ldo out_rows | lens out_off qid out_len
    L.wn_op_sv_front.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, pi32, pi32, pi32,
                                 pi32, i32, i32, i32, i32, i32, f32, f32, vp]
    for n in EXPORTS:
        if n not in ('wn_last_error', 'wn_version', 'wn_model_destroy',
                     'wn_resample_length', 'wn_profile_kernel_name',
                     'wn_profile_ffn_split'):
            getattr(L, n).restype = i32
    _lib = L
    return L


def check(status: int, what: str = ''):
    if status != 0:
        msg = lib().wn_last_error().decode('utf8', 'replace')
        if status == -4:  # handle busy (one host thread per handle)
            raise RuntimeError(f'{what}: {msg}')
        if status == -1 and ('must not be 0' in msg or 'null' in msg):
            raise AssertionError(f'{what}: {msg}')
        raise RuntimeError(f'{what} failed ({status}): {msg}')


def i32p(a):
    return a.ctypes.data_as(POINTER(c_int32))


def f32p(a):
    return a.ctypes.data_as(POINTER(c_float))


def f64p(a):
    return a.ctypes.data_as(POINTER(c_double))


def i64p(a):
    return a.ctypes.data_as(POINTER(c_int64))
