"""References, cases and fixtures of the rotary Conformer encoders (csrc/attention_rope.hip,
csrc/cabi_rope.hip): tests/test_rope_host.py on the CPU, tests/test_gpu_attention_rope.py and
tests/test_gpu_rope_model.py on the GPU.

`attention` is the plain formula -- rotate, expand the kv heads, scores, window mask, softmax,
P.V -- in fp64, and in fp32 as the yardstick e_plain of the tolerance.  The packed cases reuse the
data regimes of attention_d32_refs at a head width of 64 (K and V are the first n_kv_heads heads
of a draw for n_heads) between rows of +-1e18.  No GPU in here.
"""
import math

import torch

import attention_d32_refs as D
import kernel_refs as KR
import paraformer_refs as PR

DK = 64
SCALE = 1.0 / math.sqrt(DK)


def table(n):
    """(n, 64) fp32, cos[32] | sin[32] per position: what the host stages from the checkpoint."""
    from wenet_amd.synthetic import rope_table
    pe = rope_table(DK, n)[0]
    return torch.cat([pe[..., 0], pe[..., 1]], 1).contiguous()


def rotate(x, tab):
    """x (n, heads, 64), tab (n, 64): [x1 c - x2 s | x1 s + x2 c] (google_apply_rotary_emb)."""
    c, s = tab[:, None, :32].to(x.dtype), tab[:, None, 32:].to(x.dtype)
    x1, x2 = x[..., :32], x[..., 32:]
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], -1)


def attention(q, k, v, tab, H, Hkv, scale=SCALE, mode=0, chunk=0, left=-1, dt=torch.float64):
    """One sequence: q (n, H 64), k / v (n, Hkv 64), tab (>= n, 64) -> (n, H 64) in dt.  Query head
    h reads K / V head h // (H // Hkv)."""
    n = q.shape[0]
    q3 = rotate(q.to(dt).view(n, H, DK), tab[:n]).transpose(0, 1)
    k3 = rotate(k.to(dt).view(n, Hkv, DK), tab[:n]).transpose(0, 1)
    v3 = v.to(dt).view(n, Hkv, DK).transpose(0, 1)
    k3, v3 = (t.repeat_interleave(H // Hkv, 0) for t in (k3, v3))
    hidden = ~KR.chunk_window(n, n, mode, chunk, left)
    s = (torch.matmul(q3, k3.transpose(1, 2)) * scale).masked_fill(hidden, -float('inf'))
    return torch.matmul(torch.softmax(s, -1), v3).transpose(0, 1).reshape(n, H * DK)


def make_case(H, Hkv, lens, regime='unit', param=None, seed=0, order=None, mode=0, chunk=0,
              left=-1):
    """Q | K | V of every sequence as the three column ranges of one packed buffer of (H + 2 Hkv)
    * 64 columns; the table with three rows more than the longest sequence."""
    qs, ks, vs = D.raw_rows(regime, param, H, lens, lens, lens, seed, DK)
    w = Hkv * DK
    buf, offs, total = PR.pack_rows([torch.cat([q, k[:, :w], v[:, :w]], 1)
                                     for q, k, v in zip(qs, ks, vs)], order, gap=3, lead=2)
    return dict(H=H, Hkv=Hkv, d=H * DK, w=w, lens=list(lens), buf=buf, offs=offs, rows=total,
                tab=table(max(lens) + 3), mode=mode, chunk=chunk, left=left, scale=SCALE)


def case_refs(c):
    """(fp64 reference (rows, d), zero where no sequence owns; e_plain; the largest |v|)."""
    d, w = c['d'], c['w']
    out = {dt: torch.zeros(c['rows'], d, dtype=torch.float64)
           for dt in (torch.float64, torch.float32)}
    vmax = 0.0
    for o, n in zip(c['offs'], c['lens']):
        if n == 0:
            continue
        q, k, v = c['buf'][o:o + n, :d], c['buf'][o:o + n, d:d + w], c['buf'][o:o + n, d + w:]
        for dt in out:
            out[dt][o:o + n] = attention(q, k, v, c['tab'], c['H'], c['Hkv'], c['scale'],
                                         c['mode'], c['chunk'], c['left'], dt).double()
        vmax = max(vmax, v.abs().max().item())
    ref = out[torch.float64]
    return ref, (out[torch.float32] - ref).abs().max().item(), vmax


# the recorded models (tools/gen_golden_rope.py -> tests/golden/rope/<config>.npz).  T' = 36, 33, 16, 5,
# 1; `chunks` = (decoding_chunk_size, num_decoding_left_chunks) recorded beside full context
MODELS = {
    'tiny_rope': dict(frames=[147, 135, 67, 23, 7], fseed=950, beam=5, ctc_weight=0.5,
                      reverse_weight=0.3, chunks=[(4, 2), (16, -1)]),
    'tiny_rope_mqa': dict(frames=[147, 135, 67, 23, 7], fseed=960, beam=5, ctc_weight=0.5,
                          reverse_weight=0.0, chunks=[]),
}


def model_features(name):
    """The utterances of a model fixture, one (n, 80) fp32 matrix each."""
    from wenet_amd import synthetic as S
    t = MODELS[name]
    return [S.make_features(1, n, seed=t['fseed'] + i)[0][0] for i, n in enumerate(t['frames'])]
