"""Synthetic model directories, weights and inputs for tests and bench.py.

There is no network for checkpoints or datasets, so the named reference
configurations are rebuilt here from their yaml (the dicts below restate
/root/reference/examples/*/s0/conf/*.yaml, cited per entry) and filled with
deterministic random weights whose names and shapes are exactly the reference
``state_dict`` (tests/test_oracle_vs_reference.py checks that against the real
``init_model`` when the reference tree is present).

Weights are drawn per tensor from ``numpy.random.Generator(PCG64)`` keyed by
(seed, tensor name) so any process -- this container, the GPU box, a different
rank -- regenerates bit-identical tensors without shipping a 200 MB file.

The CTC head is "sharpened": a Xavier-random CTC projection gives near-uniform
posteriors whose per-frame argmax margin (~1e-5) is below fp32 reordering noise
(hard part 1) and whose greedy output is ~T' tokens long,
which no real model produces.  We scale the projection and bias blank so that
about 3/4 of frames are blank and the top-1 margin is O(1), like a trained CTC
model.
"""
import copy
import math
import os
import zlib
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np
import torch

_SPECIAL = {'<blank>': 0, '<unk>': 1, '<sos>': 2, '<eos>': 2}

# decoder_conf of examples/aishell/whisper/conf/finetune_whisper_largev3.yaml:20-37
_WHISPER_DEC = dict(activation_type='gelu', dropout_rate=0.0, input_layer='embed_learnable_pe',
                    key_bias=False, src_key_bias=False, normalize_before=True,
                    positional_dropout_rate=0.0, self_attention_dropout_rate=0.0,
                    src_attention=True, src_attention_dropout_rate=0.0,
                    tie_word_embedding=True, use_output_layer=True)
_WHISPER_TOK = dict(bpe_path=None, is_multilingual=True, non_lang_syms_path=None,
                    num_languages=100, split_with_space=False, symbol_table_path=None)
WHISPER_DEC_MAX_POS = 448    # LearnablePositionalEncoding max_len (embedding.py:171)

CONFIGS = {
    # examples/aishell/s0/conf/train_u2++_conformer.yaml:4-62
    'aishell_u2pp': {
        'input_dim': 80, 'output_dim': 4233,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=256, attention_heads=4,
                             linear_units=2048, num_blocks=12,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=8,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             causal=True, use_dynamic_chunk=True,
                             cnn_module_norm='layer_norm',
                             use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=4, linear_units=2048,
                             num_blocks=3, r_num_blocks=3, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3),
    },
    # examples/aishell/s0/conf/train_u2++_lite_conformer.yaml:1-68 at its own widths
    'aishell_u2pp_lite': {
        'input_dim': 80, 'output_dim': 4233,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=256, attention_heads=4,
                             linear_units=2048, num_blocks=12,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=8,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             causal=True, use_dynamic_chunk=True,
                             cnn_module_norm='layer_norm',
                             use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=4, linear_units=1024,
                             num_blocks=3, r_num_blocks=3, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3,
                           apply_non_blank_embedding=True),
    },
    # the same recipe at tiny widths for tests
    'tiny_lite': {
        'input_dim': 80, 'output_dim': 53,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=64, attention_heads=1,
                             linear_units=128, num_blocks=2,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=8,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             causal=True, use_dynamic_chunk=True,
                             cnn_module_norm='layer_norm',
                             use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=1, linear_units=96,
                             num_blocks=2, r_num_blocks=1, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3,
                           apply_non_blank_embedding=True),
    },
    # examples/librispeech/s0/conf/train_conformer_bidecoder_large.yaml:3-62
    'librispeech_bidecoder_large': {
        'input_dim': 80, 'output_dim': 5002,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=512, attention_heads=8,
                             linear_units=2048, num_blocks=12,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=31,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             cnn_module_norm='layer_norm'),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=8, linear_units=2048,
                             num_blocks=3, r_num_blocks=3, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3),
    },
    # examples/wenetspeech/s0/conf/train_u2++_conformer.yaml:1-60
    'wenetspeech_u2pp': {
        'input_dim': 80, 'output_dim': 5538,
        'encoder': 'conformer',
        'encoder_conf': dict(activation_type='swish',
                             attention_dropout_rate=0.1, attention_heads=8,
                             causal=True, cnn_module_kernel=15,
                             cnn_module_norm='layer_norm', dropout_rate=0.1,
                             input_layer='conv2d', linear_units=2048,
                             normalize_before=True, num_blocks=12,
                             output_size=512, pos_enc_layer_type='rel_pos',
                             positional_dropout_rate=0.1,
                             selfattention_layer_type='rel_selfattn',
                             use_cnn_module=True, use_dynamic_chunk=True,
                             use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=8, dropout_rate=0.1,
                             linear_units=2048, num_blocks=3,
                             positional_dropout_rate=0.1, r_num_blocks=3,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3),
    },
    # miniature of the u2++ recipe (causal conv, dynamic chunk, bi-decoder)
    'tiny_causal': {
        'input_dim': 80, 'output_dim': 67,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=128, attention_heads=2,
                             linear_units=192, num_blocks=2, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=8,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             causal=True, use_dynamic_chunk=True,
                             cnn_module_norm='layer_norm',
                             use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=2, linear_units=160,
                             num_blocks=2, r_num_blocks=1, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False, reverse_weight=0.3),
    },
    # examples/aishell/whisper/conf/finetune_whisper_largev3.yaml:1-17 (encoder)
    # at 2 of its 32 blocks: the Whisper-large-v3 widths (1280 / 20 heads /
    # 5120, 128 mel bins) at a size a CPU reference run can afford.  Encoder +
    # CTC head only; the Whisper decoder is outside the accelerated path.
    'whisper_largev3_2blocks': {
        'input_dim': 128, 'output_dim': 307,
        'encoder': 'transformer',
        'encoder_conf': dict(activation_type='gelu', attention_dropout_rate=0.0,
                             attention_heads=20, dropout_rate=0.0,
                             input_layer='conv1d2', key_bias=False,
                             linear_units=5120, normalize_before=True,
                             num_blocks=2, output_size=1280,
                             pos_enc_layer_type='abs_pos_whisper',
                             positional_dropout_rate=0.0, static_chunk_size=-1,
                             use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False),
        'decoder': None, 'decoder_conf': {},
        'cmvn': None,
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # the full Whisper-large-v3 encoder (32 blocks; 0.63 G parameters) for
    # bench.py --workload config5
    'whisper_largev3': {
        'input_dim': 128, 'output_dim': 307,
        'encoder': 'transformer',
        'encoder_conf': dict(activation_type='gelu', attention_dropout_rate=0.0,
                             attention_heads=20, dropout_rate=0.0,
                             input_layer='conv1d2', key_bias=False,
                             linear_units=5120, normalize_before=True,
                             num_blocks=32, output_size=1280,
                             pos_enc_layer_type='abs_pos_whisper',
                             positional_dropout_rate=0.0, static_chunk_size=-1,
                             use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False),
        'decoder': None, 'decoder_conf': {},
        'cmvn': None,
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # miniature of the same encoder family (whisper-tiny widths: 384 / 6 heads)
    'whisper_tiny_like': {
        'input_dim': 80, 'output_dim': 211,
        'encoder': 'transformer',
        'encoder_conf': dict(activation_type='gelu', attention_dropout_rate=0.0,
                             attention_heads=6, dropout_rate=0.0,
                             input_layer='conv1d2', key_bias=False,
                             linear_units=1536, normalize_before=True,
                             num_blocks=4, output_size=384,
                             pos_enc_layer_type='abs_pos_whisper',
                             positional_dropout_rate=0.0, static_chunk_size=-1,
                             use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False),
        'decoder': None, 'decoder_conf': {},
        'cmvn': None,
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # examples/aishell/whisper/conf/finetune_whisper_largev3.yaml:1-56 in miniature WITH its
    # decoder (gelu, learnable positions, no key biases, tied-then-cloned output layer) and the
    # Whisper special tokens inside the vocabulary: languages sot + 1 .. (en = 152, zh = 153)
    'whisper_tiny_dec': {
        'input_dim': 80, 'output_dim': 160,
        'encoder': 'transformer',
        'encoder_conf': dict(activation_type='gelu', attention_dropout_rate=0.0,
                             attention_heads=2, dropout_rate=0.0,
                             input_layer='conv1d2', key_bias=False,
                             linear_units=256, normalize_before=True,
                             num_blocks=2, output_size=128,
                             pos_enc_layer_type='abs_pos_whisper',
                             positional_dropout_rate=0.0, static_chunk_size=-1,
                             use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False),
        'decoder': 'transformer',
        'decoder_conf': dict(_WHISPER_DEC, attention_heads=2, linear_units=256,
                             num_blocks=2),
        'cmvn': None,
        'model': 'whisper',
        'tokenizer': 'whisper',
        'tokenizer_conf': dict(_WHISPER_TOK, special_tokens=dict(
            eot=150, sot=151, translate=154, transcribe=155, sot_prev=156, no_speech=157,
            no_timestamps=158, timestamp_begin=159)),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # the whole Whisper-large-v3 (32 + 32 blocks, 51866 tokens) for tools/bench_whisper_decode.py
    'whisper_largev3_dec': {
        'input_dim': 128, 'output_dim': 51866,
        'encoder': 'transformer',
        'encoder_conf': dict(activation_type='gelu', attention_dropout_rate=0.0,
                             attention_heads=20, dropout_rate=0.0,
                             input_layer='conv1d2', key_bias=False,
                             linear_units=5120, normalize_before=True,
                             num_blocks=32, output_size=1280,
                             pos_enc_layer_type='abs_pos_whisper',
                             positional_dropout_rate=0.0, static_chunk_size=-1,
                             use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False),
        'decoder': 'transformer',
        'decoder_conf': dict(_WHISPER_DEC, attention_heads=20, linear_units=5120,
                             num_blocks=32),
        'cmvn': None,
        'model': 'whisper',
        'tokenizer': 'whisper',
        'tokenizer_conf': dict(_WHISPER_TOK, special_tokens=dict(
            eot=50257, no_speech=50363, no_timestamps=50364, sot=50258, sot_prev=50362,
            timestamp_begin=50365, transcribe=50360, translate=50359)),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # examples/aishell/s0/conf/train_conformer.yaml:1-35: the offline recipe --
    # symmetric conv (kernel 15), cnn_module_norm left at its default
    # 'batch_norm', left-to-right decoder
    'aishell_conformer': {
        'input_dim': 80, 'output_dim': 4233,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=256, attention_heads=4,
                             linear_units=2048, num_blocks=12, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             attention_dropout_rate=0.0, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=15,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn'),
        'decoder': 'transformer',
        'decoder_conf': dict(attention_heads=4, linear_units=2048, num_blocks=6,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.0,
                             src_attention_dropout_rate=0.0),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # miniature of it (batch_norm in the conv module)
    'tiny_bn': {
        'input_dim': 80, 'output_dim': 89,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=128, attention_heads=2,
                             linear_units=160, num_blocks=2, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             attention_dropout_rate=0.0, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=15,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn'),
        'decoder': 'transformer',
        'decoder_conf': dict(attention_heads=2, linear_units=128, num_blocks=2,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.0,
                             src_attention_dropout_rate=0.0),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
    # miniature of the offline recipe (symmetric conv, full attention,
    # left-to-right decoder only)
    'tiny_sym': {
        'input_dim': 80, 'output_dim': 101,
        'encoder': 'conformer',
        'encoder_conf': dict(output_size=64, attention_heads=1,
                             linear_units=128, num_blocks=3, dropout_rate=0.1,
                             positional_dropout_rate=0.1,
                             attention_dropout_rate=0.1, input_layer='conv2d',
                             normalize_before=True, cnn_module_kernel=15,
                             use_cnn_module=True, activation_type='swish',
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn',
                             cnn_module_norm='layer_norm'),
        'decoder': 'transformer',
        'decoder_conf': dict(attention_heads=1, linear_units=96, num_blocks=2,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1,
                           length_normalized_loss=False),
    },
}

# joint_conf / predictor_conf of examples/aishell/rnnt/conf/conformer_u2pp_rnnt.yaml:24-43 and
# its model_conf (:80-87) at the given widths
def _rnnt(base: str, enc_out: int, embed: int, hidden: int, out: int, join: int) -> dict:
    c = copy.deepcopy(CONFIGS[base])
    c['joint'] = 'transducer_joint'
    c['joint_conf'] = dict(enc_output_size=enc_out, pred_output_size=out, join_dim=join,
                           prejoin_linear=True, postjoin_linear=False, joint_mode='add',
                           activation='tanh')
    c['predictor'] = 'rnn'
    c['predictor_conf'] = dict(embed_size=embed, output_size=out, embed_dropout=0.1,
                               hidden_size=hidden, num_layers=2, bias=True, rnn_type='lstm',
                               dropout=0.1)
    c['model'] = 'transducer'
    c['model_conf'] = dict(transducer_weight=0.75, ctc_weight=0.1, attention_weight=0.15,
                           lsm_weight=0.1, length_normalized_loss=False, reverse_weight=0.3)
    return c


# hybrid transducers: the encoder / CTC head / bi-decoder of the base recipe + predictor + joint
# tiny_causal with widths that are deliberately no multiples of 64 (join_dim: of 32 only)
CONFIGS['tiny_rnnt'] = _rnnt('tiny_causal', 128, 64, 80, 96, 160)
# the same with a vocabulary of 65 x 128 + 9: the joint kernel leaves 66 column-block partials
# per row, more than the wave that reduces them has lanes
CONFIGS['tiny_rnnt_wide'] = dict(CONFIGS['tiny_rnnt'], output_dim=8329)
# examples/aishell/rnnt/conf/conformer_u2pp_rnnt.yaml:1-87 at full width (tools/bench_transducer.py)
CONFIGS['aishell_u2pp_rnnt'] = _rnnt('aishell_u2pp', 256, 256, 256, 256, 512)


# the reference's stateless predictors (predictor.py:209-495) in place of the LSTM: `kind`
# 'embedding' (examples/aishell/rnnt/conf/example_embedding_predictor.yaml:24-43) or 'conv';
# embed_size == output_size == joint_conf.pred_output_size
def _rnnt_stateless(base: str, kind: str, embed: int, join: int, **conf) -> dict:
    c = copy.deepcopy(CONFIGS[base])
    c['predictor'] = kind
    c['predictor_conf'] = dict(embed_size=embed, output_size=embed, embed_dropout=0.1, **conf)
    c['joint_conf'] = dict(c['joint_conf'], pred_output_size=embed, join_dim=join)
    return c


CONFIGS['tiny_rnnt_embed'] = _rnnt_stateless('tiny_rnnt', 'embedding', 80, 160, n_head=4,
                                             history_size=3, bias=False)
CONFIGS['tiny_rnnt_conv'] = _rnnt_stateless('tiny_rnnt', 'conv', 96, 160, history_size=2,
                                            activation='relu', bias=True)
# example_embedding_predictor.yaml at full width (tools/bench_transducer.py --predictor embedding)
CONFIGS['aishell_u2pp_rnnt_embed'] = _rnnt_stateless('aishell_u2pp_rnnt', 'embedding', 320, 320,
                                                     n_head=4, history_size=5, bias=False)

RNNT_BLANK_BIAS = 6.0    # make_state_dict's default bias of the joint's blank logit


# FireRedASR-AED (wenet/models/firered/convert_FireRed_AED_L_to_wenet_config_and_ckpt.py:32-105)
# at the given widths
def _firered(d: int, heads: int, ffn: int, enc_blocks: int, dec_blocks: int, vocab: int) -> dict:
    return {
        'input_dim': 80, 'output_dim': vocab,
        'encoder': 'firered_conformer',
        'encoder_conf': dict(gradient_checkpointing=True, input_layer='firered_conv2d4',
                             final_norm=False, output_size=d, attention_heads=heads,
                             linear_units=ffn, num_blocks=enc_blocks, dropout_rate=0.1,
                             positional_dropout_rate=0.1, attention_dropout_rate=0.0,
                             normalize_before=True, use_dynamic_chunk=False,
                             use_dynamic_left_chunk=False, pos_enc_layer_type='rel_pos_firered',
                             static_chunk_size=-1, key_bias=False, value_bias=False,
                             query_bias=False, activation_type='swish', conv_bias=False,
                             conv_inner_factor=4, cnn_module_kernel=33,
                             cnn_module_norm='layer_norm',
                             selfattention_layer_type='firered_rel_selfattn'),
        'decoder': 'transformer',
        'decoder_conf': dict(tie_word_embedding=True, gradient_checkpointing=True,
                             attention_heads=heads, linear_units=ffn, num_blocks=dec_blocks,
                             dropout_rate=0.1, positional_dropout_rate=0.1,
                             self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0,
                             use_output_layer=True, normalize_before=True, src_attention=True,
                             activation_type='gelu', src_key_bias=False, key_bias=False),
        'tokenizer': 'bpe',
        'tokenizer_conf': dict(split_with_space=True, bpe_path='train_bpe1000.model',
                               symbol_table_path='units.txt', non_lang_syms_path=None,
                               special_tokens=dict(sos=3, eos=4)),
        'model': 'firered',
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
    }


FIRERED_EOS_BIAS = 0.75   # _make_firered_state_dict's logit bias of <eos>
CONFIGS['tiny_firered'] = _firered(128, 2, 256, 2, 2, 41)
# FireRedASR-AED-L: d 1280, 20 heads, ffn 5120, 16 + 16 blocks, vocabulary 7832
CONFIGS['firered_aed_l'] = _firered(1280, 20, 5120, 16, 16, 7832)
# its widths with one block each and a small vocabulary (the tests: 90 M weights, not 1.1 G)
CONFIGS['firered_aed_l_1blk'] = _firered(1280, 20, 5120, 1, 1, 41)


# Branchformer / E-Branchformer under the asr_model head
# (examples/aishell/s0/conf/train_ebranchformer.yaml, train_u2++_branchformer.yaml)
def _ebranchformer(d, heads, ffn, units, k, merge_k, blocks, dec_heads, dec_ffn, dec_blocks,
                   vocab) -> dict:
    return {
        'input_dim': 80, 'output_dim': vocab,
        'encoder': 'e_branchformer',
        'encoder_conf': dict(output_size=d, attention_heads=heads, linear_units=ffn,
                             num_blocks=blocks, cgmlp_linear_units=units, cgmlp_conv_kernel=k,
                             use_linear_after_conv=False, gate_activation='identity',
                             merge_conv_kernel=merge_k, dropout_rate=0.1,
                             positional_dropout_rate=0.1, attention_dropout_rate=0.1,
                             input_layer='conv2d', activation_type='swish', causal=False,
                             pos_enc_layer_type='rel_pos',
                             selfattention_layer_type='rel_selfattn'),
        'decoder': 'transformer',
        'decoder_conf': dict(attention_heads=dec_heads, linear_units=dec_ffn,
                             num_blocks=dec_blocks, dropout_rate=0.1,
                             positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False),
    }


def _branchformer(d, heads, units, k, blocks, dec_heads, dec_ffn, dec_blocks, vocab) -> dict:
    return {
        'input_dim': 80, 'output_dim': vocab,
        'encoder': 'branchformer',
        'encoder_conf': dict(output_size=d, use_attn=True, attention_heads=heads,
                             selfattention_layer_type='rel_selfattn',
                             pos_enc_layer_type='rel_pos', use_cgmlp=True,
                             cgmlp_linear_units=units, cgmlp_conv_kernel=k,
                             use_linear_after_conv=False, gate_activation='identity',
                             merge_method='concat', cgmlp_weight=0.5,
                             attn_branch_drop_rate=0.0, num_blocks=blocks, dropout_rate=0.1,
                             positional_dropout_rate=0.1, attention_dropout_rate=0.1,
                             input_layer='conv2d', stochastic_depth_rate=0.0, causal=True,
                             use_dynamic_chunk=True, use_dynamic_left_chunk=False),
        'decoder': 'bitransformer',
        'decoder_conf': dict(attention_heads=dec_heads, linear_units=dec_ffn,
                             num_blocks=dec_blocks, r_num_blocks=dec_blocks, dropout_rate=0.1,
                             positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
                             src_attention_dropout_rate=0.1),
        'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False,
                           reverse_weight=0.3),
    }


# d 64 with 2 heads: d_k = 32, the zero-padded head layout; non-causal, both convs 31 taps
CONFIGS['tiny_ebranchformer'] = _ebranchformer(64, 2, 128, 256, 31, 31, 2, 1, 96, 1, 41)
# d_k = 64, causal cgMLP (the pad frame is csgu.norm.bias), chunk masks
CONFIGS['tiny_branchformer'] = _branchformer(128, 2, 256, 15, 2, 2, 96, 1, 41)
# the shipped recipes' widths: tools/bench_branchformer.py only
CONFIGS['aishell_ebranchformer'] = _ebranchformer(256, 8, 1024, 1024, 31, 31, 17, 4, 2048, 6,
                                                  4233)
CONFIGS['aishell_u2pp_branchformer'] = _branchformer(256, 4, 2048, 63, 24, 4, 2048, 3, 4233)


# Paraformer (examples/aishell/paraformer/conf/train_paraformer.yaml) at the given widths
def _paraformer(d, heads, ffn, enc_blocks, dec_blocks, vocab) -> dict:
    return {
        'input_dim': 560, 'output_dim': vocab,
        'encoder': 'sanm_encoder',
        'encoder_conf': dict(attention_dropout_rate=0.0, attention_heads=heads, dropout_rate=0.0,
                             input_layer='paraformer_dummy', kernel_size=11, linear_units=ffn,
                             normalize_before=True, num_blocks=enc_blocks, output_size=d,
                             pos_enc_layer_type='abs_pos_paraformer',
                             positional_dropout_rate=0.0, sanm_shfit=0,
                             gradient_checkpointing=True),
        'decoder': 'sanm_decoder',
        'decoder_conf': dict(att_layer_num=dec_blocks, attention_heads=heads, dropout_rate=0.0,
                             kernel_size=11, linear_units=ffn, num_blocks=dec_blocks,
                             positional_dropout_rate=0.0, sanm_shfit=0,
                             self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0,
                             gradient_checkpointing=True),
        'tokenizer': 'paraformer',
        'tokenizer_conf': {'seg_dict_path': 'seg_dict', 'symbol_table_path': 'units.txt',
                           'special_tokens': {'<blank>': 0, '<eos>': 2, '<sos>': 1,
                                              '<unk>': vocab - 1}},
        'model': 'paraformer',
        'model_conf': dict(ctc_weight=0.3, length_normalized_loss=False, lsm_weight=0.1,
                           sampling_ratio=0.75),
        'predictor': 'paraformer_predictor',
        'predictor_conf': dict(cnn_groups=1, idim=d, l_order=1, noise_threshold2=0.01, r_order=1,
                               residual=False, smooth_factor2=0.25, tail_threshold=0.45,
                               threshold=1.0, upsample_times=3),
    }


# d 256 with 2 heads: d_k = 128, the released model's head width; 1 + 2 encoder blocks
CONFIGS['tiny_paraformer'] = _paraformer(256, 2, 256, 3, 2, 50)
# the aishell recipe: 50 encoder blocks at d 512 with 4 heads, 16 decoder blocks
CONFIGS['paraformer_large'] = _paraformer(512, 4, 2048, 50, 16, 8404)
# its widths with one encoder block behind encoders0 and one decoder block (the tests)
CONFIGS['paraformer_large_1blk'] = _paraformer(512, 4, 2048, 2, 1, 50)


# SenseVoice Small as wenet/models/sensevoice/convert_sensevoice_small_to_wenet_config_and_ckpt.py
# writes its train.yaml (the encoder_conf of the released config.yaml without the two keys the
# converter deletes), at the given widths
def _sensevoice(d, heads, ffn, blocks, tp_blocks, kernel, vocab) -> dict:
    return {
        'input_dim': 560, 'output_dim': vocab,
        'encoder': 'sanm_encoder_with_tp',
        'encoder_conf': dict(output_size=d, attention_heads=heads, linear_units=ffn,
                             num_blocks=blocks, tp_blocks=tp_blocks, dropout_rate=0.1,
                             positional_dropout_rate=0.1, attention_dropout_rate=0.1,
                             input_layer='paraformer_dummy', normalize_before=True,
                             kernel_size=kernel, sanm_shfit=0,
                             pos_enc_layer_type='abs_pos_paraformer'),
        'lfr_conf': {'lfr_m': 7, 'lfr_n': 6},
        'decoder': None,
        'ctc_conf': {'ctc_blank_id': 0},
        'tokenizer': 'sentencepiece',
        'tokenizer_conf': {'model_path': 'chn_jpn_yue_eng_ko_spectok.bpe.model',
                           'special_tokens': {'</s>': 2, '<s>': 1, '<blank>': 0, '<unk>': 0}},
        'model': 'sensevoice_small',
        'model_conf': dict(length_normalized_loss=False, ctc_weight=1.0, lsm_weight=0.1),
    }


# d 256 with 2 heads: d_k = 128, the released model's head width; 1 + 1 blocks and 2 tp blocks
CONFIGS['tiny_sensevoice'] = _sensevoice(256, 2, 256, 2, 2, 11, 50)
# d_k = 64 (the existing attention kernel), 3 taps, one tp block
CONFIGS['tiny_sensevoice_h64'] = _sensevoice(128, 2, 64, 2, 1, 3, 50)
# the released widths with one block behind encoders0 and one tp block (the tests)
CONFIGS['sensevoice_small_1blk'] = _sensevoice(512, 4, 2048, 2, 1, 11, 50)
# the released model: 50 + 20 blocks at d 512 with 4 heads (tools/bench_sensevoice.py only)
CONFIGS['sensevoice_small'] = _sensevoice(512, 4, 2048, 50, 20, 11, 25055)


# Squeezeformer under the asr_model head (examples/librispeech/s0/conf/train_squeezeformer.yaml,
# train_u2++_squeezeformer.yaml, train_squeezeformer_bidecoder_large.yaml)
def _squeezeformer(d, heads, factor, blocks, reduce_idx, recover_idx, k, reduction, shift, cnn_norm,
                   causal, dynamic_chunk, decoder, dec_heads, dec_ffn, dec_blocks, vocab) -> dict:
    ec = dict(encoder_dim=d, output_size=d, attention_heads=heads, num_blocks=blocks,
              reduce_idx=reduce_idx, recover_idx=recover_idx, pos_enc_layer_type='rel_pos',
              time_reduction_layer_type=reduction, feed_forward_expansion_factor=factor,
              input_dropout_rate=0.1, feed_forward_dropout_rate=0.1, attention_dropout_rate=0.1,
              cnn_module_kernel=k, do_rel_shift=shift, cnn_norm_type=cnn_norm,
              adaptive_scale=True, normalize_before=False, causal=causal)
    if dynamic_chunk:
        ec.update(use_dynamic_chunk=True, use_dynamic_left_chunk=False)
    dc = dict(attention_heads=dec_heads, linear_units=dec_ffn, num_blocks=dec_blocks,
              dropout_rate=0.1, positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
              src_attention_dropout_rate=0.1)
    mc = dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False)
    if decoder == 'bitransformer':
        dc['r_num_blocks'] = dec_blocks
        mc['reverse_weight'] = 0.3
    return {'input_dim': 80, 'output_dim': vocab, 'encoder': 'squeezeformer', 'encoder_conf': ec,
            'decoder': decoder, 'decoder_conf': dc, 'model_conf': mc}


# conv1d reduction, the wrapped shift, an eval-mode BatchNorm, non-causal K 31, FFN x 4
CONFIGS['tiny_squeezeformer'] = _squeezeformer(128, 2, 4, 4, 1, 3, 31, 'conv1d', True,
                                               'batch_norm', False, False, 'transformer', 2, 96,
                                               1, 41)
# stream reduction, no shift, LayerNorm, causal K 15, chunk masks, FFN x 8, two decoders
CONFIGS['tiny_squeezeformer_u2pp'] = _squeezeformer(128, 2, 8, 4, 1, 3, 15, 'stream', False,
                                                    'layer_norm', True, True, 'bitransformer', 2,
                                                    96, 1, 41)
# train_squeezeformer.yaml at its real widths: tools/bench_squeezeformer.py only
CONFIGS['librispeech_squeezeformer'] = _squeezeformer(256, 4, 4, 12, 5, 11, 31, 'conv1d', True,
                                                      'layer_norm', False, False, 'transformer',
                                                      4, 2048, 6, 5002)


# Efficient Conformer under the asr_model head (examples/aishell/s0/conf/
# train_u2++_efficonformer_v1.yaml, ..._v1_stream.yaml, ..._v2.yaml and the two librispeech ones)
def _efficonformer(d, heads, ffn, blocks, input_layer, stride_idx, group_idx, stride_kernel, k,
                   cnn_norm, causal, decoder, dec_heads, dec_ffn, dec_blocks, vocab) -> dict:
    ec = dict(output_size=d, attention_heads=heads, linear_units=ffn, num_blocks=blocks,
              dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.1,
              input_layer=input_layer, pos_enc_layer_type='rel_pos', normalize_before=True,
              activation_type='swish', use_cnn_module=True, cnn_module_kernel=k,
              cnn_module_norm=cnn_norm, causal=causal, use_dynamic_chunk=True,
              use_dynamic_left_chunk=False,
              efficient_conf=dict(stride_layer_idx=list(stride_idx), stride=[2] * len(stride_idx),
                                  group_layer_idx=list(group_idx), group_size=3,
                                  stride_kernel=stride_kernel))
    dc = dict(attention_heads=dec_heads, linear_units=dec_ffn, num_blocks=dec_blocks,
              dropout_rate=0.1, positional_dropout_rate=0.1, self_attention_dropout_rate=0.1,
              src_attention_dropout_rate=0.1)
    mc = dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False)
    if decoder == 'bitransformer':
        dc['r_num_blocks'] = dec_blocks
        mc['reverse_weight'] = 0.3
    return {'input_dim': 80, 'output_dim': vocab, 'encoder': 'efficientConformer',
            'encoder_conf': ec, 'decoder': decoder, 'decoder_conf': dc, 'model_conf': mc}


# conv2d, heads of 32 (W = 96), grouped layers 0 and 1 of which 1 strides, the kernel halved
# behind it (15 -> 7), non-causal, LayerNorm, two decoders
CONFIGS['tiny_efficonformer_v1'] = _efficonformer(128, 4, 256, 4, 'conv2d', [1], [0, 1], True, 15,
                                                  'layer_norm', False, 'bitransformer', 2, 96, 1,
                                                  41)
# conv2d2, heads of 64 (W = 192), two grouped stride layers (one at the half rate), the kernel
# kept, causal, an eval-mode BatchNorm
CONFIGS['tiny_efficonformer_v2'] = _efficonformer(128, 2, 256, 5, 'conv2d2', [1, 3], [1, 3], False,
                                                  15, 'batch_norm', True, 'transformer', 2, 96, 1,
                                                  41)
# train_u2++_efficonformer_v1.yaml (aishell) at its encoder's widths, a decoder of 4 heads (it
# predates the d_k = 32 decoder kernels and profiles/efficonformer_aishell.json was measured on
# it; the recipe's own 8 heads: aishell_efficonformer_v1_dec8): tools/bench_efficonformer.py only
CONFIGS['aishell_efficonformer_v1'] = _efficonformer(256, 8, 2048, 12, 'conv2d', [3], [0, 1, 2, 3],
                                                     True, 15, 'layer_norm', False,
                                                     'bitransformer', 4, 2048, 3, 4233)
# decoders with heads of 32 (csrc/attention_d32.hip, self_attn_step_d32_kernel): tiny_efficonformer_v1
# with 4 decoder heads at 128
CONFIGS['tiny_efficonformer_v1_dec32'] = _efficonformer(128, 4, 256, 4, 'conv2d', [1], [0, 1], True,
                                                        15, 'layer_norm', False, 'bitransformer', 4,
                                                        96, 1, 41)
# train_u2++_efficonformer_v1.yaml (aishell) as shipped: the decoders' 8 heads of 32 ...
CONFIGS['aishell_efficonformer_v1_dec8'] = _efficonformer(256, 8, 2048, 12, 'conv2d', [3],
                                                          [0, 1, 2, 3], True, 15, 'layer_norm',
                                                          False, 'bitransformer', 8, 2048, 3, 4233)
# ... and one encoder block (grouped), one block per decoder, a small vocabulary at the same
# widths: the width test
CONFIGS['aishell_efficonformer_v1_dec8_1blk'] = _efficonformer(256, 8, 2048, 1, 'conv2d', [], [0],
                                                               True, 15, 'layer_norm', False,
                                                               'bitransformer', 8, 2048, 1, 41)
# the tiny_bn Conformer (LayerNorm in the conv module) under two decoders of 4 heads at 128
CONFIGS['tiny_dec32'] = {
    'input_dim': 80, 'output_dim': 41,
    'encoder': 'conformer',
    'encoder_conf': dict(CONFIGS['tiny_bn']['encoder_conf'], cnn_module_norm='layer_norm'),
    'decoder': 'bitransformer',
    'decoder_conf': dict(attention_heads=4, linear_units=96, num_blocks=2, r_num_blocks=2,
                         dropout_rate=0.1, positional_dropout_rate=0.1,
                         self_attention_dropout_rate=0.0, src_attention_dropout_rate=0.0),
    'model_conf': dict(ctc_weight=0.3, lsm_weight=0.1, length_normalized_loss=False,
                       reverse_weight=0.3),
}


def _to_efficonformer(sd, configs, seed):
    """The Conformer-shaped dict of make_state_dict under an EfficientConformerEncoder's shapes
    (wenet/models/efficient_conformer/encoder.py:140-215): pos_bias_u / v of a grouped layer are
    (h, group * d_k), the depthwise kernel behind a stride layer is K // 2 with stride_kernel,
    a stride layer carries the concat_linear its forward never uses, and conv2d2 has one conv
    and a projection over d * ((idim - 1) // 2) pixels."""
    ec = configs['encoder_conf']
    ef = ec['efficient_conf']
    d, h = ec['output_size'], ec['attention_heads']
    g = ef['group_size']
    out = OrderedDict(sd)
    if ec['input_layer'] == 'conv2d2':
        del out['encoder.embed.conv.2.weight'], out['encoder.embed.conv.2.bias']
        n_in = d * ((configs['input_dim'] - 1) // 2)
        b = 1.0 / math.sqrt(n_in)
        out['encoder.embed.out.0.weight'] = _uniform(seed, 'out2.weight', (d, n_in), b)
        out['encoder.embed.out.0.bias'] = _uniform(seed, 'out2.bias', (d, ), b)
    K = ec['cnn_module_kernel']
    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        if i in ef['group_layer_idx']:
            b = math.sqrt(6.0 / (h + g * d // h))
            for n in ('pos_bias_u', 'pos_bias_v'):
                out[f'{p}.self_attn.{n}'] = _uniform(seed, f'{p}.grouped.{n}', (h, g * d // h), b)
        if K != ec['cnn_module_kernel']:
            b = 1.0 / math.sqrt(K)
            out[p + '.conv_module.depthwise_conv.weight'] = _uniform(seed, p + '.dwk.w',
                                                                     (d, 1, K), b)
        if i in ef['stride_layer_idx']:
            b = 1.0 / math.sqrt(2 * d)
            out[p + '.concat_linear.weight'] = _uniform(seed, p + '.cat.w', (d, 2 * d), b)
            out[p + '.concat_linear.bias'] = _uniform(seed, p + '.cat.b', (d, ), b)
            if ef['stride_kernel']:
                K = K // 2
    return out


def make_configs(name: str) -> dict:
    """Parsed-``train.yaml`` equivalent for a named configuration."""
    c = copy.deepcopy(CONFIGS[name])
    c.setdefault('ctc', 'ctc')
    c.setdefault('ctc_conf', {'ctc_blank_id': 0})
    c.setdefault('model', 'asr_model')
    c.setdefault('cmvn', 'global_cmvn')
    c.setdefault('cmvn_conf', {'cmvn_file': 'global_cmvn',
                               'is_json_cmvn': True})
    c.setdefault('tokenizer', 'char')
    c.setdefault('tokenizer_conf', {'symbol_table_path': 'units.txt',
                                    'split_with_space': False,
                                    'bpe_path': None,
                                    'non_lang_syms_path': None,
                                    'is_multilingual': False,
                                    'num_languages': 1,
                                    'special_tokens': dict(_SPECIAL)})
    c.setdefault('dataset', 'asr')
    c.setdefault('dataset_conf', {
        'resample_conf': {'resample_rate': 16000},
        'fbank_conf': {'num_mel_bins': 80, 'frame_shift': 10,
                       'frame_length': 25, 'dither': 0.0},
    })
    return c


def _rng(seed: int, name: str) -> np.random.Generator:
    return np.random.Generator(
        np.random.PCG64([seed, zlib.crc32(name.encode('utf-8'))]))


def _uniform(seed, name, shape, bound):
    return _rng(seed, name).uniform(-bound, bound, size=shape).astype(
        np.float32)


def _normal(seed, name, shape, std=1.0, mean=0.0):
    return (_rng(seed, name).standard_normal(size=shape) * std + mean).astype(
        np.float32)


def positional_table(d_model: int, max_len: int = 5000) -> torch.Tensor:
    """The `pe` buffer of wenet/models/transformer/embedding.py:47-56."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(
        torch.arange(0, d_model, 2, dtype=torch.float32) *
        -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0)


def _add_transducer(sd, configs: dict, seed: int, blank_bias: float):
    """predictor.* / joint.* of a `model: transducer` configuration (RNNPredictor,
    predictor.py:60-88; TransducerJoint, joint.py:34-49).  Matrices ~ N(0, 3 / sqrt(fan_in)) and
    biases ~ N(0, 0.1) -- with the default inits a random joint's arg-max hardly depends on the
    predictor state -- and `blank_bias` on the blank logit: about 6 leaves a few symbols per
    frame group, 9 and more empties whole utterances."""
    pc, jc = configs['predictor_conf'], configs['joint_conf']
    V = configs['output_dim']
    kind = configs.get('predictor', 'rnn')
    E, P = pc['embed_size'], pc['output_size']
    H, L = (pc['hidden_size'], pc['num_layers']) if kind == 'rnn' else (0, 0)
    J = jc['join_dim']

    def mat(name, out_f, in_f):
        sd[name] = _normal(seed, name, (out_f, in_f), 3.0 / math.sqrt(in_f))

    def vec(name, n):
        sd[name] = _normal(seed, name, (n, ), 0.1)

    sd['predictor.embed.weight'] = _normal(seed, 'predictor.embed.weight', (V, E), 1.0)
    for l in range(L):
        mat(f'predictor.rnn.weight_ih_l{l}', 4 * H, E if l == 0 else H)
        mat(f'predictor.rnn.weight_hh_l{l}', 4 * H, H)
        vec(f'predictor.rnn.bias_ih_l{l}', 4 * H)
        vec(f'predictor.rnn.bias_hh_l{l}', 4 * H)
    linears = [('joint.enc_ffn', J, jc['enc_output_size']), ('joint.pred_ffn', J, P),
               ('joint.ffn_out', V, J)]
    if kind == 'rnn':
        linears.insert(0, ('predictor.projection', P, H))
    else:
        # EmbeddingPredictor / ConvPredictor (predictor.py:218-242, :381-405)
        C = pc.get('history_size', 2) + 1
        if kind == 'embedding':
            mat('predictor.pos_embed.weight', pc['n_head'], E * C)
            if pc.get('bias', False):
                vec('predictor.pos_embed.bias', pc['n_head'])   # (the reference never reads it)
            linears.insert(0, ('predictor.ffn', E, E))
        else:
            sd['predictor.conv.weight'] = _normal(seed, 'predictor.conv.weight', (E, 1, C),
                                                  3.0 / math.sqrt(C))
            if pc.get('bias', False):
                vec('predictor.conv.bias', E)
        sd['predictor.norm.weight'] = _normal(seed, 'predictor.norm.weight', (E, ), 0.1, 1.0)
        vec('predictor.norm.bias', E)
    for name, o, i in linears:
        mat(name + '.weight', o, i)
        vec(name + '.bias', o)
    blank = ((configs.get('tokenizer_conf') or {}).get('special_tokens') or {}).get('<blank>', 0)
    sd['joint.ffn_out.bias'][blank] += np.float32(blank_bias)


def _add_branch_layer(sd, p, configs, seed, lin, norm):
    """What a BranchformerEncoderLayer / EBranchformerEncoderLayer holds beside its attention
    (wenet/models/branchformer/encoder_layer.py:66-110, e_branchformer/encoder_layer.py:58-91).
    Not the ESPnet initialisation of the reference (conv weight 1e-6, bias 1), under which a
    dropped tap or a wrong pad value is invisible: conv taps of order 1 / sqrt(K), the gate
    norm's bias of order 0.3."""
    ec = configs['encoder_conf']
    d, U = ec['output_size'], ec['cgmlp_linear_units']
    C, K = U // 2, ec['cgmlp_conv_kernel']
    ebf = configs['encoder'] == 'e_branchformer'
    lin(p + '.cgmlp.channel_proj1.0', U, d)
    sd[p + '.cgmlp.csgu.norm.weight'] = _normal(seed, p + '.csgu.norm.w', (C, ), 0.1, 1.0)
    sd[p + '.cgmlp.csgu.norm.bias'] = _normal(seed, p + '.csgu.norm.b', (C, ), 0.3)
    b = 1.0 / math.sqrt(K)
    sd[p + '.cgmlp.csgu.conv.weight'] = _uniform(seed, p + '.csgu.conv.w', (C, 1, K), b)
    sd[p + '.cgmlp.csgu.conv.bias'] = _uniform(seed, p + '.csgu.conv.b', (C, ), b)
    if ec.get('use_linear_after_conv', False):
        lin(p + '.cgmlp.csgu.linear', C, C)
    lin(p + '.cgmlp.channel_proj2', d, C)
    for n in ('norm_mha', 'norm_mlp', 'norm_final'):
        norm(f'{p}.{n}', d)
    lin(p + '.merge_proj', d, 2 * d)
    if ebf:
        Km = ec.get('merge_conv_kernel', 3)
        b = 1.0 / math.sqrt(Km)
        sd[p + '.depthwise_conv_fusion.weight'] = _uniform(seed, p + '.fusion.w',
                                                           (2 * d, 1, Km), b)
        sd[p + '.depthwise_conv_fusion.bias'] = _uniform(seed, p + '.fusion.b', (2 * d, ), b)
        ffn = ec['linear_units']
        for ff in ('feed_forward', 'feed_forward_macaron'):
            lin(f'{p}.{ff}.w_1', ffn, d)
            lin(f'{p}.{ff}.w_2', d, ffn)
        norm(p + '.norm_ff', d)
        norm(p + '.norm_ff_macaron', d)
    else:
        # (read by merge_method learned_ave only)
        for n in ('pooling_proj1', 'pooling_proj2', 'weight_proj1', 'weight_proj2'):
            lin(f'{p}.{n}', 1, d)


def _to_squeezeformer(sd, configs, seed):
    """The Conformer-shaped dict of make_state_dict under a SqueezeformerEncoder's names
    (wenet/models/squeezeformer/encoder.py:149-185): the front end's convs and projection, preln
    instead of after_norm, post-LN blocks with an adaptive scale and bias in front of every module
    (not the ones and zeros of the reference's initialisation, under which a dropped fold is
    invisible), the time reduction and time_recover_layer."""
    ec = configs['encoder_conf']
    d = ec['encoder_dim']
    rename = {'encoder.embed.conv.0.': 'encoder.embed.pw_conv.',
              'encoder.embed.conv.2.': 'encoder.embed.dw_conv.',
              'encoder.embed.out.0.': 'encoder.embed.input_proj.0.',
              'encoder.after_norm.': 'encoder.preln.'}
    layer = {'.feed_forward_macaron.': '.ffn1.', '.feed_forward.': '.ffn2.',
             '.norm_mha.': '.layer_norm1.', '.norm_ff_macaron.': '.layer_norm2.',
             '.norm_conv.': '.layer_norm3.', '.norm_ff.': '.layer_norm4.'}
    out = OrderedDict()
    for k, v in sd.items():
        if k.startswith('encoder.encoders.'):
            if '.norm_final.' in k:
                continue
            for a, b in layer.items():
                k = k.replace(a, b)
        else:
            for a, b in rename.items():
                if k.startswith(a):
                    k = b + k[len(a):]
        out[k] = v
    for i in range(ec['num_blocks']):
        for mod in ('self_attn', 'ffn1', 'ffn2', 'conv_module'):
            p = f'encoder.encoders.{i}.{mod}'
            out[p + '.ada_scale'] = _normal(seed, p + '.ada_scale', (1, 1, d), 0.2, 1.0)
            out[p + '.ada_bias'] = _normal(seed, p + '.ada_bias', (1, 1, d), 0.3)
    Kr = 5 if ec.get('time_reduction_layer_type', 'conv1d') == 'conv1d' else 1
    p = 'encoder.time_reduction_layer'
    b = 1.0 / math.sqrt(Kr)
    out[p + '.dw_conv.weight'] = _uniform(seed, p + '.dw.w', (d, 1, Kr), b)
    out[p + '.dw_conv.bias'] = _uniform(seed, p + '.dw.b', (d, ), b)
    b = 1.0 / math.sqrt(d)
    out[p + '.pw_conv.weight'] = _uniform(seed, p + '.pw.w', (d, d, 1), b)
    out[p + '.pw_conv.bias'] = _uniform(seed, p + '.pw.b', (d, ), b)
    out['encoder.time_recover_layer.weight'] = _uniform(seed, 'recover.w', (d, d), b)
    out['encoder.time_recover_layer.bias'] = _uniform(seed, 'recover.b', (d, ), b)
    return out


def make_state_dict(configs: dict, seed: int = 0, sharpen_ctc: bool = True,
                    rnnt_blank_bias: float = RNNT_BLANK_BIAS
                    ) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic random weights with the reference's names and shapes.
    `rnnt_blank_bias`: `model: transducer` configurations only (_add_transducer)."""
    ec, dc = configs['encoder_conf'], configs.get('decoder_conf') or {}
    d = ec['output_size']
    h = ec['attention_heads']
    ffn = ec.get('linear_units', 2048)
    K = ec.get('cnn_module_kernel', 15)
    branch = configs.get('encoder') in ('branchformer', 'e_branchformer')
    squeeze = configs.get('encoder') == 'squeezeformer'
    if squeeze:
        ffn = d * ec.get('feed_forward_expansion_factor', 4)
    if configs.get('encoder', 'conformer') == 'transformer':
        return _make_transformer_state_dict(configs, seed, sharpen_ctc)
    if configs.get('encoder') == 'firered_conformer':
        return _make_firered_state_dict(configs, seed, sharpen_ctc)
    if configs.get('encoder') == 'sanm_encoder':
        return _make_paraformer_state_dict(configs, seed, sharpen_ctc)
    if configs.get('encoder') == 'sanm_encoder_with_tp':
        return _make_sensevoice_state_dict(configs, seed, sharpen_ctc)
    idim, V = configs['input_dim'], configs['output_dim']
    sd: Dict[str, np.ndarray] = OrderedDict()

    def lin(name, out_f, in_f, bias=True):
        b = 1.0 / math.sqrt(in_f)
        sd[name + '.weight'] = _uniform(seed, name + '.weight', (out_f, in_f), b)
        if bias:
            sd[name + '.bias'] = _uniform(seed, name + '.bias', (out_f, ), b)

    def norm(name, n):
        sd[name + '.weight'] = _normal(seed, name + '.weight', (n, ), 0.1, 1.0)
        sd[name + '.bias'] = _normal(seed, name + '.bias', (n, ), 0.1)

    def attn(name, n, rel=False):
        if rel:
            b = math.sqrt(6.0 / (h + n // h))
            sd[name + '.pos_bias_u'] = _uniform(seed, name + '.pos_bias_u',
                                                (h, n // h), b)
            sd[name + '.pos_bias_v'] = _uniform(seed, name + '.pos_bias_v',
                                                (h, n // h), b)
        for p in ('linear_q', 'linear_k', 'linear_v', 'linear_out'):
            lin(f'{name}.{p}', n, n)
        if rel:
            lin(f'{name}.linear_pos', n, n, bias=False)

    if configs.get('cmvn') == 'global_cmvn':
        sd['encoder.global_cmvn.mean'] = _normal(seed, 'cmvn.mean', (idim, ),
                                                 1.5, 11.0)
        sd['encoder.global_cmvn.istd'] = (
            1.0 / (2.5 + np.abs(_normal(seed, 'cmvn.std', (idim, ), 0.5)))
        ).astype(np.float32)
    b = 1.0 / 3.0
    sd['encoder.embed.conv.0.weight'] = _uniform(seed, 'conv0.w', (d, 1, 3, 3), b)
    sd['encoder.embed.conv.0.bias'] = _uniform(seed, 'conv0.b', (d, ), b)
    b = 1.0 / math.sqrt(9 * d)
    sd['encoder.embed.conv.2.weight'] = _uniform(seed, 'conv2.w', (d, d, 3, 3), b)
    sd['encoder.embed.conv.2.bias'] = _uniform(seed, 'conv2.b', (d, ), b)
    fdim = ((idim - 1) // 2 - 1) // 2
    lin('encoder.embed.out.0', d, d * fdim)
    sd['encoder.embed.pos_enc.pe'] = positional_table(d).numpy()
    norm('encoder.after_norm', d)
    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        if branch:   # (the layer classes call their attention `attn`)
            attn(p + '.attn', d, rel=True)
            _add_branch_layer(sd, p, configs, seed, lin, norm)
            continue
        attn(p + '.self_attn', d, rel=True)
        for ff in ('feed_forward', 'feed_forward_macaron'):
            lin(f'{p}.{ff}.w_1', ffn, d)
            lin(f'{p}.{ff}.w_2', d, ffn)
        b = 1.0 / math.sqrt(d)
        sd[p + '.conv_module.pointwise_conv1.weight'] = _uniform(
            seed, p + '.pw1.w', (2 * d, d, 1), b)
        sd[p + '.conv_module.pointwise_conv1.bias'] = _uniform(
            seed, p + '.pw1.b', (2 * d, ), b)
        b = 1.0 / math.sqrt(K)
        sd[p + '.conv_module.depthwise_conv.weight'] = _uniform(
            seed, p + '.dw.w', (d, 1, K), b)
        sd[p + '.conv_module.depthwise_conv.bias'] = _uniform(
            seed, p + '.dw.b', (d, ), b)
        norm(p + '.conv_module.norm', d)
        if ec.get('cnn_norm_type' if squeeze else 'cnn_module_norm',
                  'batch_norm') == 'batch_norm':
            # BatchNorm1d buffers (eval mode uses the running statistics)
            sd[p + '.conv_module.norm.running_mean'] = _normal(
                seed, p + '.bn.mean', (d, ), 0.3)
            sd[p + '.conv_module.norm.running_var'] = (
                0.5 + np.abs(_normal(seed, p + '.bn.var', (d, ), 0.5))).astype(np.float32)
            sd[p + '.conv_module.norm.num_batches_tracked'] = np.asarray(1000, np.int64)
        b = 1.0 / math.sqrt(d)
        sd[p + '.conv_module.pointwise_conv2.weight'] = _uniform(
            seed, p + '.pw2.w', (d, d, 1), b)
        sd[p + '.conv_module.pointwise_conv2.bias'] = _uniform(
            seed, p + '.pw2.b', (d, ), b)
        for n in ('norm_ff', 'norm_mha', 'norm_ff_macaron', 'norm_conv',
                  'norm_final'):
            norm(f'{p}.{n}', d)

    def decoder(prefix, nblocks):
        sd[prefix + '.embed.0.weight'] = _normal(seed, prefix + '.embed',
                                                 (V, d), 1.0)
        sd[prefix + '.embed.1.pe'] = positional_table(d).numpy()
        norm(prefix + '.after_norm', d)
        lin(prefix + '.output_layer', V, d)
        for j in range(nblocks):
            p = f'{prefix}.decoders.{j}'
            attn(p + '.self_attn', d)
            attn(p + '.src_attn', d)
            lin(p + '.feed_forward.w_1', dc['linear_units'], d)
            lin(p + '.feed_forward.w_2', d, dc['linear_units'])
            for n in ('norm1', 'norm2', 'norm3'):
                norm(f'{p}.{n}', d)

    if configs.get('decoder', 'bitransformer') == 'bitransformer':
        decoder('decoder.left_decoder', dc['num_blocks'])
        decoder('decoder.right_decoder', dc.get('r_num_blocks', 0))
    else:
        decoder('decoder', dc['num_blocks'])
    lin('ctc.ctc_lo', V, d)
    if sharpen_ctc:
        sd['ctc.ctc_lo.weight'] = sd['ctc.ctc_lo.weight'] * np.float32(12.0)
        sd['ctc.ctc_lo.bias'] = sd['ctc.ctc_lo.bias'] * np.float32(12.0)
        # Non-blank logits are ~N(0, sigma^2) with sigma = 12/sqrt(3); the
        # expected max of V-1 of them follows the Gumbel asymptotics below.
        # Blank gets a constant logit slightly above it (zero weight row), so
        # roughly 2/3..4/5 of the frames come out blank.
        n = max(V - 1, 2)
        a = math.sqrt(2.0 * math.log(n))
        emax = a - (math.log(math.log(n)) + math.log(4 * math.pi)) / (2 * a) \
            + 0.5772 / a
        sd['ctc.ctc_lo.weight'][0, :] = 0.0
        sd['ctc.ctc_lo.bias'][0] = np.float32(12.0 / math.sqrt(3.0) * emax *
                                              1.10)
    # decoders: sharpen the output layers the same way so rescoring scores
    # separate hypotheses by O(1) rather than by rounding noise.
    for k in list(sd.keys()):
        if k.endswith('output_layer.weight') or k.endswith('output_layer.bias'):
            sd[k] = sd[k] * np.float32(4.0)
    if configs.get('model') == 'transducer':
        _add_transducer(sd, configs, seed, rnnt_blank_bias)
    if squeeze:
        sd = _to_squeezeformer(sd, configs, seed)
    if configs.get('encoder') == 'efficientConformer':
        sd = _to_efficonformer(sd, configs, seed)
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v)))
                       for k, v in sd.items())


def firered_rel_positional_table(d_model: int, max_len: int = 5000) -> torch.Tensor:
    """The `pe` buffer of FireRedRelPositionalEncoding (wenet/models/firered/attention.py:27-44):
    (1, 2 max_len - 1, d), row c = the sinusoid of the relative position max_len - 1 - c."""
    rel = torch.arange(max_len - 1, -max_len, -1, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) *
                         -(math.log(10000.0) / d_model))
    pe = torch.zeros(2 * max_len - 1, d_model)
    pe[:, 0::2] = torch.sin(rel * div_term)
    pe[:, 1::2] = torch.cos(rel * div_term)
    return pe.unsqueeze(0)


def _make_firered_state_dict(configs, seed, sharpen_ctc):
    """FireRedModel (wenet/models/firered/): names and shapes as init_model gives them.  No
    biases on linear_q / k / v / out of the encoder's attention and on its convolutions, three
    LayerNorms inside the attention, a conv module over 2 d channels, no norm_mha / after_norm;
    a left-to-right decoder without linear_k biases whose output layer is tied to the
    embedding."""
    ec, dc = configs['encoder_conf'], configs['decoder_conf']
    d, h, ffn = ec['output_size'], ec['attention_heads'], ec['linear_units']
    K, inner = ec['cnn_module_kernel'], ec['conv_inner_factor']
    idim, V = configs['input_dim'], configs['output_dim']
    C = 32                                    # FireRedConv2dSubsampling4's odim default
    sd: Dict[str, np.ndarray] = OrderedDict()

    def lin(name, out_f, in_f, bias=True):
        b = 1.0 / math.sqrt(in_f)
        sd[name + '.weight'] = _uniform(seed, name + '.weight', (out_f, in_f), b)
        if bias:
            sd[name + '.bias'] = _uniform(seed, name + '.bias', (out_f, ), b)

    def norm(name, n):
        sd[name + '.weight'] = _normal(seed, name + '.weight', (n, ), 0.1, 1.0)
        sd[name + '.bias'] = _normal(seed, name + '.bias', (n, ), 0.1)

    if configs.get('cmvn') == 'global_cmvn':
        sd['encoder.global_cmvn.mean'] = _normal(seed, 'cmvn.mean', (idim, ), 1.5, 11.0)
        sd['encoder.global_cmvn.istd'] = (
            1.0 / (2.5 + np.abs(_normal(seed, 'cmvn.std', (idim, ), 0.5)))).astype(np.float32)
    sd['encoder.embed.conv.0.weight'] = _uniform(seed, 'conv0.w', (C, 1, 3, 3), 1.0 / 3.0)
    sd['encoder.embed.conv.0.bias'] = _uniform(seed, 'conv0.b', (C, ), 1.0 / 3.0)
    b = 1.0 / math.sqrt(9 * C)
    sd['encoder.embed.conv.2.weight'] = _uniform(seed, 'conv2.w', (C, C, 3, 3), b)
    sd['encoder.embed.conv.2.bias'] = _uniform(seed, 'conv2.b', (C, ), b)
    lin('encoder.embed.out.0', d, C * (((idim - 1) // 2 - 1) // 2))
    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        a = p + '.self_attn'
        b = math.sqrt(6.0 / (h + d // h))
        sd[a + '.pos_bias_u'] = _uniform(seed, a + '.pos_bias_u', (h, d // h), b)
        sd[a + '.pos_bias_v'] = _uniform(seed, a + '.pos_bias_v', (h, d // h), b)
        for n in ('linear_q', 'linear_k', 'linear_v', 'linear_out', 'linear_pos'):
            lin(f'{a}.{n}', d, d, bias=False)
        for n in ('layer_norm_q', 'layer_norm_k', 'layer_norm_v'):
            norm(f'{a}.{n}', d)
        for ff in ('feed_forward', 'feed_forward_macaron'):
            lin(f'{p}.{ff}.w_1', ffn, d)
            lin(f'{p}.{ff}.w_2', d, ffn)
        di = d * inner // 2                   # channels behind the GLU
        sd[p + '.conv_module.pointwise_conv1.weight'] = _uniform(
            seed, p + '.pw1.w', (2 * di, d, 1), 1.0 / math.sqrt(d))
        sd[p + '.conv_module.depthwise_conv.weight'] = _uniform(
            seed, p + '.dw.w', (di, 1, K), 1.0 / math.sqrt(K))
        norm(p + '.conv_module.norm', di)
        sd[p + '.conv_module.pointwise_conv2.weight'] = _uniform(
            seed, p + '.pw2.w', (d, di, 1), 1.0 / math.sqrt(di))
        for n in ('norm_ff', 'norm_ff_macaron', 'norm_conv', 'norm_final'):
            norm(f'{p}.{n}', d)
    sd['encoder.embed.pos_enc.pe'] = firered_rel_positional_table(d).numpy()
    sd['decoder.embed.0.weight'] = _normal(seed, 'decoder.embed', (V, d), 1.0)
    sd['decoder.embed.1.pe'] = positional_table(d).numpy()
    norm('decoder.after_norm', d)
    for j in range(dc['num_blocks']):
        p = f'decoder.decoders.{j}'
        for a in ('self_attn', 'src_attn'):
            for n in ('linear_q', 'linear_k', 'linear_v', 'linear_out'):
                lin(f'{p}.{a}.{n}', d, d, bias=n != 'linear_k')
        lin(p + '.feed_forward.w_1', dc['linear_units'], d)
        lin(p + '.feed_forward.w_2', d, dc['linear_units'])
        for n in ('norm1', 'norm2', 'norm3'):
            norm(f'{p}.{n}', d)
    # tie_word_embedding: the output layer IS the embedding; its bias is a parameter of its
    # own.  A tied random decoder repeats one token when the token's own embedding (logit =
    # E . LN(E[last] + ...): the last token wins) or the nearly constant layer outputs dominate
    # the residual stream: at this scale the positional rows (amplitude 1) weigh as much as the
    # scaled embedding (sqrt(d) E, std 0.7), so the arg-max moves with the step
    sd['decoder.embed.0.weight'] = sd['decoder.embed.0.weight'] * np.float32(0.7 / math.sqrt(d))
    sd['decoder.output_layer.weight'] = sd['decoder.embed.0.weight']
    sd['decoder.output_layer.bias'] = _uniform(seed, 'decoder.output_layer.bias', (V, ), 0.1)
    # layer matrices x 3 (as for the Whisper decoder below: with smaller ones the next token
    # barely depends on the input or the position), <eos> a logit bias so that some hypotheses
    # end before the cap
    for k in list(sd):
        if k.startswith('decoder.decoders.') and k.endswith('.weight') and sd[k].ndim == 2:
            sd[k] = sd[k] * np.float32(3.0)
    eos = configs['tokenizer_conf']['special_tokens']['eos']
    sd['decoder.output_layer.bias'][eos] += np.float32(FIRERED_EOS_BIAS)
    lin('ctc.ctc_lo', V, d)
    if sharpen_ctc:      # as make_state_dict: roughly 2/3 .. 4/5 of the frames come out blank
        sd['ctc.ctc_lo.weight'] = sd['ctc.ctc_lo.weight'] * np.float32(12.0)
        sd['ctc.ctc_lo.bias'] = sd['ctc.ctc_lo.bias'] * np.float32(12.0)
        n = max(V - 1, 2)
        a = math.sqrt(2.0 * math.log(n))
        emax = a - (math.log(math.log(n)) + math.log(4 * math.pi)) / (2 * a) + 0.5772 / a
        sd['ctc.ctc_lo.weight'][0, :] = 0.0
        sd['ctc.ctc_lo.bias'][0] = np.float32(12.0 / math.sqrt(3.0) * emax * 1.10)
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())


def _make_paraformer_state_dict(configs, seed, sharpen_ctc):
    """Paraformer (wenet/models/paraformer/): names and shapes as init_model gives them --
    encoders0 over the 560 LFR columns + num_blocks - 1 encoders, FSMN convs without bias, the CIF
    predictor with its timestamp branch (tp_*: carried, not read by the library), SANM decoder
    layers without embedding, decoders3, the sampler's embedding, a CTC head."""
    ec, dc, pc = configs['encoder_conf'], configs['decoder_conf'], configs['predictor_conf']
    d, ffn, K = ec['output_size'], ec['linear_units'], ec['kernel_size']
    idim, V = configs['input_dim'], configs['output_dim']
    sd: Dict[str, np.ndarray] = OrderedDict()

    def lin(name, out_f, in_f, bias=True):
        b = 1.0 / math.sqrt(in_f)
        sd[name + '.weight'] = _uniform(seed, name + '.weight', (out_f, in_f), b)
        if bias:
            sd[name + '.bias'] = _uniform(seed, name + '.bias', (out_f, ), b)

    def norm(name, n):
        sd[name + '.weight'] = _normal(seed, name + '.weight', (n, ), 0.1, 1.0)
        sd[name + '.bias'] = _normal(seed, name + '.bias', (n, ), 0.1)

    def fsmn(name, k):
        sd[name + '.fsmn_block.weight'] = _uniform(seed, name + '.fsmn', (d, 1, k),
                                                   1.0 / math.sqrt(k))

    if configs.get('cmvn') == 'global_cmvn':
        sd['encoder.global_cmvn.mean'] = _normal(seed, 'cmvn.mean', (idim, ), 1.5, 11.0)
        sd['encoder.global_cmvn.istd'] = (
            1.0 / (2.5 + np.abs(_normal(seed, 'cmvn.std', (idim, ), 0.5)))).astype(np.float32)
    sd['encoder.embed.pos_enc.pe'] = whisper_positional_table(idim, 5000).numpy()
    for i in range(ec['num_blocks']):
        p = 'encoder.encoders0.0' if i == 0 else f'encoder.encoders.{i - 1}'
        a = p + '.self_attn'
        lin(a + '.linear_out', d, d)
        lin(a + '.linear_q_k_v', 3 * d, idim if i == 0 else d)
        fsmn(a, K)
        lin(p + '.feed_forward.w_1', ffn, d)
        lin(p + '.feed_forward.w_2', d, ffn)
        norm(p + '.norm1', idim if i == 0 else d)
        norm(p + '.norm2', d)
    norm('encoder.after_norm', d)
    # Cif: Conv1d(d, d, l_order + r_order + 1) dense, Linear(d, 1).  The output weight x 4: the
    # alphas then spread over (0, 1) instead of sitting at 0.5, so the fires fall irregularly
    taps = pc['l_order'] + pc['r_order'] + 1
    b = 1.0 / math.sqrt(d * taps)
    sd['predictor.predictor.cif_conv1d.weight'] = _uniform(seed, 'cif.conv.w', (d, d, taps), b)
    sd['predictor.predictor.cif_conv1d.bias'] = _uniform(seed, 'cif.conv.b', (d, ), b)
    lin('predictor.predictor.cif_output', 1, d)
    sd['predictor.predictor.cif_output.weight'] = \
        sd['predictor.predictor.cif_output.weight'] * np.float32(4.0)
    up = pc['upsample_times']
    sd['predictor.tp_upsample_cnn.weight'] = _uniform(seed, 'tp.up.w', (d, d, up),
                                                      1.0 / math.sqrt(d * up))
    sd['predictor.tp_upsample_cnn.bias'] = _uniform(seed, 'tp.up.b', (d, ), 1.0 / math.sqrt(d * up))
    for sfx in ('', '_reverse'):
        b = 1.0 / math.sqrt(d)
        sd['predictor.tp_blstm.weight_ih_l0' + sfx] = _uniform(seed, 'tp.ih' + sfx, (4 * d, d), b)
        sd['predictor.tp_blstm.weight_hh_l0' + sfx] = _uniform(seed, 'tp.hh' + sfx, (4 * d, d), b)
        sd['predictor.tp_blstm.bias_ih_l0' + sfx] = _uniform(seed, 'tp.bih' + sfx, (4 * d, ), b)
        sd['predictor.tp_blstm.bias_hh_l0' + sfx] = _uniform(seed, 'tp.bhh' + sfx, (4 * d, ), b)
    lin('predictor.tp_output', 1, 2 * d)
    dffn = dc['linear_units']
    for j in range(dc['num_blocks'] + 1):
        last = j == dc['num_blocks']
        p = 'decoder.decoders3.0' if last else f'decoder.decoders.{j}'
        lin(p + '.feed_forward.w_1', dffn, d)
        lin(p + '.feed_forward.w_2', d, dffn, bias=False)
        norm(p + '.feed_forward.norm', dffn)
        norm(p + '.norm1', d)
        if last:
            break
        norm(p + '.norm2', d)
        norm(p + '.norm3', d)
        fsmn(p + '.self_attn', dc['kernel_size'])
        lin(p + '.src_attn.linear_q', d, d)
        lin(p + '.src_attn.linear_k_v', 2 * d, d)
        lin(p + '.src_attn.linear_out', d, d)
    norm('decoder.after_norm', d)
    lin('decoder.output_layer', V, d)
    # x 6: the arg-max of a row then leads its runner-up by a margin a rounding does not close
    sd['decoder.output_layer.weight'] = sd['decoder.output_layer.weight'] * np.float32(6.0)
    sd['embed.weight'] = _normal(seed, 'embed', (V, d), 1.0)
    lin('ctc.ctc_lo', V, d)
    if sharpen_ctc:      # as make_state_dict: roughly 2/3 .. 4/5 of the frames come out blank
        sd['ctc.ctc_lo.weight'] = sd['ctc.ctc_lo.weight'] * np.float32(12.0)
        sd['ctc.ctc_lo.bias'] = sd['ctc.ctc_lo.bias'] * np.float32(12.0)
        n = max(V - 1, 2)
        a = math.sqrt(2.0 * math.log(n))
        emax = a - (math.log(math.log(n)) + math.log(4 * math.pi)) / (2 * a) + 0.5772 / a
        sd['ctc.ctc_lo.weight'][0, :] = 0.0
        sd['ctc.ctc_lo.bias'][0] = np.float32(12.0 / math.sqrt(3.0) * emax * 1.10)
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())


def _make_sensevoice_state_dict(configs, seed, sharpen_ctc):
    """SenseVoice Small (wenet/models/sensevoice/): names and shapes as init_model gives them --
    the CMVN on the model (`global_cmvn.*`, not on its encoder), the 16 x 560 query table,
    encoders0 over the 560 columns + num_blocks - 1 encoders, after_norm, tp_encoders, tp_norm,
    a CTC head."""
    ec = configs['encoder_conf']
    d, ffn, K = ec['output_size'], ec['linear_units'], ec['kernel_size']
    idim, V = configs['input_dim'], configs['output_dim']
    sd: Dict[str, np.ndarray] = OrderedDict()

    def lin(name, out_f, in_f):
        b = 1.0 / math.sqrt(in_f)
        sd[name + '.weight'] = _uniform(seed, name + '.weight', (out_f, in_f), b)
        sd[name + '.bias'] = _uniform(seed, name + '.bias', (out_f, ), b)

    def norm(name, n):
        sd[name + '.weight'] = _normal(seed, name + '.weight', (n, ), 0.1, 1.0)
        sd[name + '.bias'] = _normal(seed, name + '.bias', (n, ), 0.1)

    def layer(p, in_f):
        a = p + '.self_attn'
        lin(a + '.linear_out', d, d)
        lin(a + '.linear_q_k_v', 3 * d, in_f)
        sd[a + '.fsmn_block.weight'] = _uniform(seed, a + '.fsmn', (d, 1, K), 1.0 / math.sqrt(K))
        lin(p + '.feed_forward.w_1', ffn, d)
        lin(p + '.feed_forward.w_2', d, ffn)
        norm(p + '.norm1', in_f)
        norm(p + '.norm2', d)

    sd['encoder.embed.pos_enc.pe'] = whisper_positional_table(idim, 5000).numpy()
    for i in range(ec['num_blocks']):
        layer('encoder.encoders0.0' if i == 0 else f'encoder.encoders.{i - 1}',
              idim if i == 0 else d)
    norm('encoder.after_norm', d)
    for i in range(ec['tp_blocks']):
        layer(f'encoder.tp_encoders.{i}', d)
    norm('encoder.tp_norm', d)
    lin('ctc.ctc_lo', V, d)
    if sharpen_ctc:      # as make_state_dict: roughly 2/3 .. 4/5 of the frames come out blank
        sd['ctc.ctc_lo.weight'] = sd['ctc.ctc_lo.weight'] * np.float32(12.0)
        sd['ctc.ctc_lo.bias'] = sd['ctc.ctc_lo.bias'] * np.float32(12.0)
        n = max(V - 1, 2)
        a = math.sqrt(2.0 * math.log(n))
        emax = a - (math.log(math.log(n)) + math.log(4 * math.pi)) / (2 * a) + 0.5772 / a
        sd['ctc.ctc_lo.weight'][0, :] = 0.0
        sd['ctc.ctc_lo.bias'][0] = np.float32(12.0 / math.sqrt(3.0) * emax * 1.10)
    # query rows of the size of a CMVN-normalised LFR row (~ unit variance)
    sd['embed.weight'] = _normal(seed, 'sv.embed', (16, idim), 1.0)
    sd['global_cmvn.mean'] = _normal(seed, 'cmvn.mean', (idim, ), 1.5, 11.0)
    sd['global_cmvn.istd'] = (
        1.0 / (2.5 + np.abs(_normal(seed, 'cmvn.std', (idim, ), 0.5)))).astype(np.float32)
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())


def whisper_positional_table(d_model: int, max_len: int = 1500) -> torch.Tensor:
    """The `pe` buffer of WhisperPositionalEncoding
    (wenet/models/transformer/embedding.py:154-163)."""
    inc = np.log(10000) / (d_model // 2 - 1)
    inv = torch.exp(-inc * torch.arange(d_model // 2))
    st = torch.arange(max_len)[:, np.newaxis] * inv[np.newaxis, :]
    return torch.cat([torch.sin(st), torch.cos(st)], dim=1).unsqueeze(0)


def _make_transformer_state_dict(configs, seed, sharpen_ctc):
    """TransformerEncoder (Whisper recipe) + CTC head; names as the reference's
    state_dict (encoder.embed.conv.{0,2}, encoder.encoders.i.{self_attn,
    feed_forward,norm1,norm2}, encoder.after_norm, ctc.ctc_lo)."""
    ec = configs['encoder_conf']
    d, ffn = ec['output_size'], ec['linear_units']
    idim, V = configs['input_dim'], configs['output_dim']
    sd: Dict[str, np.ndarray] = OrderedDict()

    def lin(name, out_f, in_f, bias=True):
        b = 1.0 / math.sqrt(in_f)
        sd[name + '.weight'] = _uniform(seed, name + '.weight', (out_f, in_f), b)
        if bias:
            sd[name + '.bias'] = _uniform(seed, name + '.bias', (out_f, ), b)

    def norm(name, n):
        sd[name + '.weight'] = _normal(seed, name + '.weight', (n, ), 0.1, 1.0)
        sd[name + '.bias'] = _normal(seed, name + '.bias', (n, ), 0.1)

    b = 1.0 / math.sqrt(3 * idim)
    sd['encoder.embed.conv.0.weight'] = _uniform(seed, 'tconv0.w', (d, idim, 3), b)
    sd['encoder.embed.conv.0.bias'] = _uniform(seed, 'tconv0.b', (d, ), b)
    b = 1.0 / math.sqrt(3 * d)
    sd['encoder.embed.conv.2.weight'] = _uniform(seed, 'tconv2.w', (d, d, 3), b)
    sd['encoder.embed.conv.2.bias'] = _uniform(seed, 'tconv2.b', (d, ), b)
    sd['encoder.embed.pos_enc.pe'] = whisper_positional_table(d).numpy().astype(
        np.float32)
    norm('encoder.after_norm', d)
    for i in range(ec['num_blocks']):
        p = f'encoder.encoders.{i}'
        lin(p + '.self_attn.linear_q', d, d)
        lin(p + '.self_attn.linear_k', d, d, bias=bool(ec.get('key_bias', True)))
        lin(p + '.self_attn.linear_v', d, d)
        lin(p + '.self_attn.linear_out', d, d)
        lin(p + '.feed_forward.w_1', ffn, d)
        lin(p + '.feed_forward.w_2', d, ffn)
        norm(p + '.norm1', d)
        norm(p + '.norm2', d)
    if configs.get('decoder') is not None:
        # the Whisper decoder (decoder.py:59-135 as the recipe configures it): learnable `pe`,
        # linear_k without bias, an output layer of its own (init_model clones the embedding
        # into it and fine-tuning moves both, so checkpoints carry two different tensors).
        # Scales: embedding ~ N(0, 0.3), pe ~ N(0, 0.9), layer matrices x 3 -- with smaller ones
        # a random decoder's next token barely depends on its input or its position and every
        # hypothesis is one token repeated; <eot> gets a logit bias of 1.25 so that some
        # hypotheses end before the cap (with 3 everything ends at once)
        dc = configs['decoder_conf']
        dffn = dc['linear_units']
        sd['decoder.embed.0.weight'] = _normal(seed, 'decoder.embed', (V, d), 0.3)
        sd['decoder.embed.1.pe'] = _normal(
            seed, 'decoder.pe', (1, WHISPER_DEC_MAX_POS, d), 0.9)
        norm('decoder.after_norm', d)
        lin('decoder.output_layer', V, d)
        eot = ((configs.get('tokenizer_conf') or {}).get('special_tokens') or {}).get('eot')
        if eot is not None:
            sd['decoder.output_layer.bias'][eot] += np.float32(1.25)
        first = len(sd)
        for j in range(dc['num_blocks']):
            p = f'decoder.decoders.{j}'
            for a, kb in (('self_attn', dc.get('key_bias', True)),
                          ('src_attn', dc.get('src_key_bias', True))):
                lin(f'{p}.{a}.linear_q', d, d)
                lin(f'{p}.{a}.linear_k', d, d, bias=bool(kb))
                lin(f'{p}.{a}.linear_v', d, d)
                lin(f'{p}.{a}.linear_out', d, d)
            lin(p + '.feed_forward.w_1', dffn, d)
            lin(p + '.feed_forward.w_2', d, dffn)
            for n in ('norm1', 'norm2', 'norm3'):
                norm(f'{p}.{n}', d)
        for k in list(sd.keys())[first:]:
            if k.endswith('.weight') and sd[k].ndim == 2:
                sd[k] = sd[k] * np.float32(3.0)
    lin('ctc.ctc_lo', V, d)
    if sharpen_ctc:
        sd['ctc.ctc_lo.weight'] = sd['ctc.ctc_lo.weight'] * np.float32(12.0)
        sd['ctc.ctc_lo.bias'] = sd['ctc.ctc_lo.bias'] * np.float32(12.0)
        n = max(V - 1, 2)
        a = math.sqrt(2.0 * math.log(n))
        emax = a - (math.log(math.log(n)) + math.log(4 * math.pi)) / (2 * a) \
            + 0.5772 / a
        sd['ctc.ctc_lo.weight'][0, :] = 0.0
        sd['ctc.ctc_lo.bias'][0] = np.float32(12.0 / math.sqrt(3.0) * emax * 1.10)
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v)))
                       for k, v in sd.items())


def make_features(batch: int, num_frames, seed: int = 1234,
                  feat_dim: int = 80) -> Tuple[torch.Tensor, torch.Tensor]:
    """Padded (B, Tmax, F) fbank-like features + int32 lengths, sorted by
    length descending like `padding` (wenet/dataset/processor.py:539).
    `num_frames` is an int (fixed length) or a (lo, hi) range."""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    if isinstance(num_frames, (tuple, list)):
        lens = rng.integers(num_frames[0], num_frames[1] + 1, size=batch)
    else:
        lens = np.full((batch, ), int(num_frames))
    lens = np.sort(lens)[::-1].copy()
    tmax = int(lens.max())
    feats = np.zeros((batch, tmax, feat_dim), dtype=np.float32)
    for b in range(batch):
        # log-mel-like: smooth in time, mean ~11, std ~3
        x = rng.standard_normal((int(lens[b]), feat_dim)).astype(np.float32)
        x[1:] = 0.6 * x[:-1] + 0.8 * x[1:]
        feats[b, :lens[b]] = 11.0 + 3.0 * x
    return torch.from_numpy(feats), torch.from_numpy(lens.astype(np.int32))


def make_audio(num_samples: int, seed: int = 1234,
               sample_rate: int = 16000) -> np.ndarray:
    """16 kHz mono fp32 in [-1, 1]: three chirps + coloured noise, peak 0.3
    (SURVEY.md section 8d synthetic-input recipe)."""
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    t = np.arange(num_samples, dtype=np.float64) / sample_rate
    x = np.zeros(num_samples, dtype=np.float64)
    for _ in range(3):
        f0, f1 = rng.uniform(100, 3000, size=2)
        dur = max(t[-1], 1e-3)
        phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / dur)
        x += rng.uniform(0.3, 1.0) * np.sin(phase + rng.uniform(0, 2 * np.pi))
    noise = rng.standard_normal(num_samples)
    noise = np.convolve(noise, np.ones(8) / 8.0, mode='same')
    x += 0.5 * noise
    x *= 0.3 / max(np.abs(x).max(), 1e-9)
    return x.astype(np.float32)


def write_model_dir(path: str, name: str, seed: int = 0) -> str:
    """Write a directory `wenet.load_model` / `wenet_amd.load_model` accepts
    (wenet/cli/model.py:71-92): train.yaml, final.pt, units.txt, global_cmvn."""
    import json
    import yaml
    os.makedirs(path, exist_ok=True)
    configs = make_configs(name)
    sd = make_state_dict(configs, seed)
    # JSON CMVN stats that reproduce the synthetic mean / istd through
    # wenet/utils/cmvn.py:21-43
    mean = sd['encoder.global_cmvn.mean'].double().numpy()
    istd = sd['encoder.global_cmvn.istd'].double().numpy()
    n = 1000
    var = 1.0 / (istd * istd)
    with open(os.path.join(path, 'global_cmvn'), 'w') as f:
        json.dump({'mean_stat': (mean * n).tolist(),
                   'var_stat': ((var + mean * mean) * n).tolist(),
                   'frame_num': n}, f)
    V = configs['output_dim']
    with open(os.path.join(path, 'units.txt'), 'w', encoding='utf8') as f:
        f.write('<blank> 0\n<unk> 1\n<sos/eos> 2\n')
        for i in range(3, V):
            f.write(f'u{i} {i}\n')
    configs['cmvn_conf']['cmvn_file'] = os.path.join(path, 'global_cmvn')
    configs['tokenizer_conf']['symbol_table_path'] = os.path.join(
        path, 'units.txt')
    with open(os.path.join(path, 'train.yaml'), 'w') as f:
        yaml.safe_dump(configs, f)
    torch.save(sd, os.path.join(path, 'final.pt'))
    return path


def peaky_logprobs(batch: int, frames, vocab: int, peak: float, seed: int):
    """Seeded (B, T, V) float32 log-softmax rows with two boosted tokens per frame
    and frequent blanks (token 0), plus int32 lengths in `frames`: inputs for the
    search-only fixtures (prefixes re-merge, biasing phrases match often)."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(frames[0], frames[1] + 1, (batch, ), generator=g)
    lens[0] = frames[1]
    T = int(lens.max())
    x = torch.randn(batch, T, vocab, generator=g)
    hot = torch.randint(0, vocab, (batch, T, 2), generator=g)
    x.scatter_add_(2, hot, torch.full(hot.shape, float(peak)))
    x[..., 0] += 1.0
    return torch.log_softmax(x, dim=-1), lens.to(torch.int32)


# ---------------------------------------------------------------------------
# BASELINE.json `configs` as bench.py workloads.  bench.py, the `-m gpu` parity
# tests at these sizes and oracle/gen_golden_bench.py (which runs the REAL
# reference on them) all take the batch from here, so the committed goldens
# (tests/golden/bench_*.npz) are the reference's answer to exactly the batch the
# benchmark times.
BENCH_BEAM = 10
BENCH_FRAMES = (800, 1200)   # 8..12 s of 10 ms frames, mean ~10 s
BENCH_WORKLOADS = {
    'config2': dict(config='aishell_u2pp', batch=32, method='ctc_prefix_beam_search',
                    kw={}, text='BASELINE.json configs[1]: AIShell u2++ conformer '
                    '12L/4head/256d fbank80, batch 32 x ~10 s per GPU (8-12 s '
                    'ragged), ctc_prefix_beam_search beam 10'),
    'config3': dict(config='librispeech_bidecoder_large', batch=64,
                    method='attention_rescoring',
                    kw=dict(ctc_weight=0.5, reverse_weight=0.3),
                    text='BASELINE.json configs[2]: LibriSpeech conformer '
                    'bidecoder-large 12L/8head/512d fbank80, batch 64 x ~10 s per GPU, '
                    'attention_rescoring beam 10, ctc_weight 0.5, reverse_weight 0.3'),
    'config4': dict(config='wenetspeech_u2pp', batch=32,
                    method='ctc_prefix_beam_search',
                    kw=dict(decoding_chunk_size=16, num_decoding_left_chunks=-1),
                    text='BASELINE.json configs[3]: WenetSpeech u2++ conformer '
                    '12L/8head/512d, decoding_chunk_size 16 (chunk-mask streaming), '
                    'batch 32 x ~10 s per GPU, ctc_prefix_beam_search beam 10'),
    'config5': dict(config='whisper_largev3', batch=16, method='ctc_greedy_search',
                    kw={}, frames=(3000, 3000), feat_dim=128,
                    text='BASELINE.json configs[4]: Whisper-large-v3 encoder '
                    '32L/20head/1280d, 128 mel bins, 30 s windows, batch 16 per GPU, '
                    '+ a 307-way CTC head and greedy search'),
}


def make_bench_group(workload: str, group: int = 0):
    """Utterance group `group` of a bench workload: `batch` utterances, seed
    1234 + group.  Group 0 is the whole batch of a 1-GPU run."""
    wl = BENCH_WORKLOADS[workload]
    return make_features(wl['batch'], wl.get('frames', BENCH_FRAMES),
                         seed=1234 + group, feat_dim=wl.get('feat_dim', 80))


def make_bench_batch(workload: str, world: int = 1):
    """Global batch of `bench.py --workload W --gpus world`: groups 0..world-1
    back to back (global index = group * batch + index in group), zero-padded to
    the longest utterance.  Weak scaling: `batch` utterances per GPU."""
    groups = [make_bench_group(workload, g) for g in range(world)]
    if world == 1:
        return groups[0]
    tmax = max(int(f.size(1)) for f, _ in groups)
    feats = torch.zeros((sum(f.size(0) for f, _ in groups), tmax, groups[0][0].size(2)),
                        dtype=torch.float32)
    r = 0
    for f, _ in groups:
        feats[r:r + f.size(0), :f.size(1)] = f
        r += f.size(0)
    return feats, torch.cat([l for _, l in groups])
