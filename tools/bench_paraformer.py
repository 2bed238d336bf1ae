#!/usr/bin/env python3
"""Timing record of the Paraformer path: `paraformer_large` (the aishell recipe: 50 encoder blocks
at d 512 with 4 heads of 128, 16 decoder blocks, vocabulary 8404; synthetic weights), B = 32
utterances of 8-12 s, fp32, after warm-up.

    python tools/bench_paraformer.py [--steps 5 --warmup 2 --batch 32 --out-dir DIR]

Records: the encoder (LFR front end + 50 blocks), predictor + decoder (wn_paraformer_decode on
the encoded batch), the predictor alone through its two operator hooks on the same encoder rows
(wn_op_cif_alpha + wn_op_cif_fire: the library's launches plus the hooks' descriptor uploads and
result copies, so an upper bound) and the decoder as the difference (a lower bound), `decode(['paraformer_greedy_search'])` and `decode(['ctc_greedy_search'])` on the same
batch in audio-s/s, and per launch `attention_d128` (4 heads x 128) beside `attention_kernel` on
the equal-FLOP problem of the same rows as 8 heads x 64, in the same process.  One run, untuned.
Writes profiles/paraformer_large.json and docs/LOG_round23.md (or both into --out-dir).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def attention_pair(enc_lens, steps, warmup):
    """One layer's self attention on the batch's packed rows: 4 heads x 128 on attention_d128
    against 8 heads x 64 on attention_kernel (the same Q K^T and P V FLOPs)."""
    from wenet_amd import _lib
    L = _lib.lib()
    d = 512
    lens = np.asarray(enc_lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = int(lens.sum())
    g = torch.Generator(device='cuda').manual_seed(0)
    qkv = torch.randn(M, 3 * d, device='cuda', generator=g)
    O = torch.empty(M, d, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * d, qkv.data_ptr() + 8 * d

    def d128():
        _lib.check(L.wn_op_attention_d128(q, k, v, 3 * d, 3 * d, 3 * d, M, M, O.data_ptr(), d,
                                          _lib.i32p(off), _lib.i32p(lens), _lib.i32p(off),
                                          _lib.i32p(lens), len(lens), 4, 128 ** -0.5, st),
                   'attention_d128')

    op = _lib.WnAttentionOp()
    op.Q, op.K, op.V = q, k, v
    op.ldq = op.ldk = op.ldv = 3 * d
    op.q_rows = op.kv_rows = M
    op.O, op.ldo = O.data_ptr(), d
    op.q_off = op.kv_off = _lib.i32p(off)
    op.q_len = op.kv_len = _lib.i32p(lens)
    op.n_seq, op.n_heads, op.mask_mode, op.left_chunks, op.scale = len(lens), 8, 0, -1, 0.125
    form = ctypes.c_int32(0)

    def d64():
        _lib.check(L.wn_op_attention(ctypes.byref(op), ctypes.byref(form), st), 'attention')

    return timed(d128, steps * 4, warmup), timed(d64, steps * 4, warmup), hex(form.value)


def predictor_hooks(sd, enc, enc_lens, steps, warmup):
    """The CIF predictor on the batch's packed encoder rows through the operator hooks."""
    from wenet_amd import _lib
    L = _lib.lib()
    B, d = len(enc_lens), enc.shape[2]
    lens = np.asarray(enc_lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    M = int(lens.sum())
    rows = torch.cat([enc[b, :int(lens[b])] for b in range(B)]).contiguous()
    cw = sd['predictor.predictor.cif_conv1d.weight'].permute(0, 2, 1).reshape(d, 3 * d)
    cw = cw.contiguous().cuda()
    cb = sd['predictor.predictor.cif_conv1d.bias'].cuda()
    ow = sd['predictor.predictor.cif_output.weight'].reshape(-1).contiguous().cuda()
    ob = sd['predictor.predictor.cif_output.bias'].cuda()
    alpha = torch.empty(M, device='cuda')
    caps = (lens + 1).astype(np.int32)
    emb_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int32)
    E = int(caps.sum())
    emb = torch.empty(E, d, device='cuda')
    fire_t = np.zeros(E, dtype=np.int32)
    n_fire, tok = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        _lib.check(L.wn_op_cif_alpha(rows.data_ptr(), d, M, d, cw.data_ptr(), cb.data_ptr(),
                                     ow.data_ptr(), ob.data_ptr(), 1.0, 0.0, alpha.data_ptr(),
                                     _lib.i32p(off), _lib.i32p(lens), B, st), 'cif_alpha')
        _lib.check(L.wn_op_cif_fire(rows.data_ptr(), d, M, d, alpha.data_ptr(), _lib.i32p(off),
                                    _lib.i32p(lens), B, 1.0, 0.45, emb.data_ptr(), d, E,
                                    _lib.i32p(emb_off), _lib.i32p(caps), _lib.i32p(fire_t),
                                    _lib.i32p(n_fire), _lib.i32p(tok), st), 'cif_fire')

    return timed(run, steps, warmup), int(tok.sum())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out-dir', default=None)
    args = ap.parse_args(argv)
    from wenet_amd import Paraformer
    from wenet_amd import synthetic as S
    t0 = time.time()
    configs = S.make_configs('paraformer_large')
    sd = S.make_state_dict(configs, 0)
    model = Paraformer(configs, sd, device='cuda:0')
    print(f'model built in {time.time() - t0:.1f} s', flush=True)
    feats, lens = S.make_features(args.batch, (800, 1200), seed=7)
    feats = feats.cuda()
    B = feats.shape[0]
    audio_s = float(lens.sum()) * 0.01
    enc_ms = timed(lambda: model._forward_encoder(feats, lens), args.steps, args.warmup)
    enc, mask = model._forward_encoder(feats, lens)
    enc_lens = mask.squeeze(1).sum(1).tolist()
    pd_ms = timed(lambda: model._predict_decode(B, enc_lens), args.steps, args.warmup)
    tok_lens = model._predict_decode(B, enc_lens)[1]
    pred_ms, pred_tokens = predictor_hooks(sd, enc, enc_lens, args.steps, args.warmup)
    assert pred_tokens == int(tok_lens.sum())
    model._forward_encoder(feats, lens)
    greedy_ms = timed(lambda: model.decode(['paraformer_greedy_search'], feats, lens), args.steps,
                      args.warmup)
    ctc_ms = timed(lambda: model.decode(['ctc_greedy_search'], feats, lens), args.steps,
                   args.warmup)
    a128, a64, form = attention_pair(enc_lens, args.steps, args.warmup)
    res = dict(status='measured, one run, untuned', config='paraformer_large', batch=B,
               audio_s=audio_s, steps=args.steps, warmup=args.warmup, dtype='fp32',
               enc_frames=int(sum(enc_lens)), tokens=int(tok_lens.sum()), encoder_ms=enc_ms,
               predictor_decoder_ms=pd_ms, predictor_hooks_ms=pred_ms,
               decoder_ms=pd_ms - pred_ms, greedy_ms=greedy_ms, ctc_greedy_ms=ctc_ms,
               greedy_audio_s_per_s=audio_s / (greedy_ms * 1e-3),
               ctc_greedy_audio_s_per_s=audio_s / (ctc_ms * 1e-3),
               attention_d128_ms=a128, attention_8x64_ms=a64, attention_8x64_form=form,
               ffn='linear() pairs with ReLU / residual epilogues; ffn_fused was not tried',
               kernel_split='not collected')
    pdir = args.out_dir or os.path.join(ROOT, 'profiles')
    ldir = args.out_dir or os.path.join(ROOT, 'docs')
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, 'paraformer_large.json'), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    with open(os.path.join(ldir, 'LOG_round23.md'), 'w') as f:
        f.write(LOG.format(**res))
    print(json.dumps(res))
    return 0


LOG = """# Round 23: Paraformer models

`tools/bench_paraformer.py`: `paraformer_large` (synthetic weights), B = {batch} x 8-12 s
({audio_s:.1f} s of audio, {enc_frames} encoder frames, {tokens} tokens), fp32, {steps} steps
after {warmup}.  One run, untuned.

| what | ms |
| --- | --- |
| encoder (LFR front end + 50 blocks) | {encoder_ms:.2f} |
| predictor + decoder (`wn_paraformer_decode`, 16 blocks) | {predictor_decoder_ms:.2f} |
| predictor alone (`wn_op_cif_alpha` + `wn_op_cif_fire`, with the hooks' host copies: an upper bound) | {predictor_hooks_ms:.2f} |
| decoder (the difference: a lower bound) | {decoder_ms:.2f} |
| `decode(['paraformer_greedy_search'])`, encoder included | {greedy_ms:.2f} |
| `decode(['ctc_greedy_search'])` on the same handle | {ctc_greedy_ms:.2f} |
| `attention_d128`, one layer, 4 heads x 128 | {attention_d128_ms:.3f} |
| `attention_kernel`, the same rows as 8 heads x 64 (form {attention_8x64_form}) | {attention_8x64_ms:.3f} |

{greedy_audio_s_per_s:.0f} audio-s/s through `paraformer_greedy_search`,
{ctc_greedy_audio_s_per_s:.0f} through `ctc_greedy_search`.  Feed-forward modules: {ffn}.  Kernel split: {kernel_split}.
"""

if __name__ == '__main__':
    sys.exit(main())
