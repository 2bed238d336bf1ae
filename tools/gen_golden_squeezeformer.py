#!/usr/bin/env python3
"""Record what the REAL reference's Squeezeformer modules compute, for
tests/test_squeezeformer_host.py and tests/test_gpu_squeezeformer.py.

    python tools/gen_golden_squeezeformer.py        # CPU only; needs the reference tree

tests/golden/squeezeformer/modules*.npz -- every module in fp64 (.double()) on the inputs
tests/squeezeformer_refs.py rebuilds from their seeds:
  attn_<T>           squeezeformer RelPositionMultiHeadedAttention(2 heads, d 128, do_rel_shift,
                     adaptive_scale) at T = 1, 2, 33
  reduce1d_<T>, reducestream_<T>   TimeReductionLayer1D / TimeReductionLayerStream (d 64) at
                     T = 1, 2, 5, 33, 64
  layer_<model>      SqueezeformerEncoderLayer, block 0 of each tiny model, on 40 frames

tests/golden/squeezeformer/<model>*.npz -- the reference model of the two tiny configurations
(init_model + the synthetic state dict, loaded strictly) on utterances of 291, 135, 131, 127, 15,
11 and 7 frames (T' = 72, 33, 32, 31, 3, 2, 1), every utterance decoded ALONE with
decoding_chunk_size -1 (0 on a dynamic-chunk model draws a random chunk), in fp32 and as
.double():
  enc64_<n>          the fp64 encoder output (tiny_squeezeformer_u2pp: also
                     enc64_<n>_c<chunk>_l<left> at decoding_chunk_size 4, left chunks -1 and 2,
                     of the 135- and the 15-frame utterance)
  meta.e_enc / e_enc_chunk   per utterance, the fp32 reference's own max abs error against fp64
  meta.tokens        ctc_greedy_search, ctc_prefix_beam_search (beam 5), attention_rescoring
                     (beam 5, ctc_weight 0.5, reverse_weight 0.3 on the bidecoder model)
  meta.scores / e_score   the fp64 scores of the two beam modes and |fp32 - fp64| of them
A weight seed is REJECTED unless the fp64 and the fp32 reference decode the same tokens in every
mode and at least three utterances have non-empty CTC results.

No file is larger than the largest FireRed fixture: arrays are cut into row blocks
(`<name>__part<i>`) and dealt into files of at most 64 KB of array data.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

OUT = os.path.join(ROOT, 'tests', 'golden', 'squeezeformer')
FILE_BYTES = 64 * 1024
MAX_FILE = 72309          # tests/golden/firered/firered_tiny_enc3.npz
RESCORE_CTC_WEIGHT = 0.5


def save_split(stem, meta, arrays):
    """<stem>.npz (meta + arrays) and <stem>_<i>.npz, each with at most FILE_BYTES of arrays."""
    parts = []
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        rows = max(1, (FILE_BYTES // 2) // max(a[0].nbytes, 1)) if a.ndim > 1 else len(a)
        if a.nbytes <= FILE_BYTES // 2:
            parts.append((k, a))
        else:
            for i, r0 in enumerate(range(0, a.shape[0], rows)):
                parts.append((f'{k}__part{i}', a[r0:r0 + rows]))
    files, cur, size = [], {}, 0
    for k, a in parts:
        if cur and size + a.nbytes > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    files.append(cur)
    for f in os.listdir(OUT):
        if f == stem + '.npz' or (f.startswith(stem + '_') and f.endswith('.npz')
                                  and f[len(stem) + 1:-4].isdigit()):
            os.remove(os.path.join(OUT, f))
    for i, d in enumerate(files):
        path = os.path.join(OUT, f'{stem}.npz' if i == 0 else f'{stem}_{i}.npz')
        extra = dict(meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)) if i == 0 \
            else {}
        np.savez_compressed(path, **extra, **d)
        assert os.path.getsize(path) <= MAX_FILE, (path, os.path.getsize(path))
        print(f'{path}: {os.path.getsize(path)} bytes')


def _decode_alone(model, feats, dtype, reverse_weight):
    toks = {m: [] for m in SQ.METHODS}
    scores = {'ctc_prefix_beam_search': [], 'attention_rescoring': []}
    with torch.no_grad():
        for f in feats:
            r = model.decode(list(SQ.METHODS), f.unsqueeze(0).to(dtype),
                             torch.tensor([f.shape[0]]), beam_size=SQ.CTC_BEAM,
                             decoding_chunk_size=-1,
                             ctc_weight=RESCORE_CTC_WEIGHT, reverse_weight=reverse_weight)
            for m in SQ.METHODS:
                toks[m].append(list(map(int, r[m][0].tokens)))
            for m in scores:
                scores[m].append(float(r[m][0].score))
    return toks, scores


def try_seed(name, wseed):
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, wseed)
    feats = SQ.tiny_features(name)
    rw = SQ.TINY[name]['reverse_weight']
    m32 = build_reference_model(configs, sd)
    t32, s32 = _decode_alone(m32, feats, torch.float32, rw)
    if sum(len(u) > 0 for u in t32['ctc_prefix_beam_search']) < 3 or \
            sum(len(u) > 0 for u in t32['ctc_greedy_search']) < 3:
        return 'fewer than three utterances with a non-empty CTC result', None
    m64 = build_reference_model(configs, sd).double()
    t64, s64 = _decode_alone(m64, feats, torch.float64, rw)
    if t64 != t32:
        return 'fp64 and fp32 decode different tokens (near-tie)', None
    arrays, e_enc, enc_lens, e_chunk = {}, [], [], {}
    chunked = bool(configs['encoder_conf'].get('use_dynamic_chunk', False))
    with torch.no_grad():
        for f in feats:
            n = f.shape[0]
            ln = torch.tensor([n])
            e64, mk = m64._forward_encoder(f.unsqueeze(0).double(), ln)
            e32, _ = m32._forward_encoder(f.unsqueeze(0), ln)
            assert int(mk.sum()) == e64.shape[1]
            arrays[f'enc64_{n}'] = e64[0].numpy()
            e_enc.append(float((e32[0].double() - e64[0]).abs().max()))
            enc_lens.append(int(e64.shape[1]))
            if chunked and n in SQ.CHUNK_FRAMES:
                for (cs, lc) in SQ.CHUNK_CASES:
                    c64, _ = m64._forward_encoder(f.unsqueeze(0).double(), ln, cs, lc)
                    c32, _ = m32._forward_encoder(f.unsqueeze(0), ln, cs, lc)
                    key = f'{n}_c{cs}_l{lc}'
                    arrays['enc64_' + key] = c64[0].numpy()
                    e_chunk[key] = float((c32[0].double() - c64[0]).abs().max())
    e_score = {k: [abs(a - b) for a, b in zip(s32[k], s64[k])] for k in s64}
    meta = dict(SQ.TINY[name], config=name, wseed=wseed, ctc_beam=SQ.CTC_BEAM, tokens=t64,
                e_enc=e_enc, enc_lens=enc_lens, e_enc_chunk=e_chunk, scores=s64, e_score=e_score,
                rescore_ctc_weight=RESCORE_CTC_WEIGHT)
    return None, (meta, arrays)


def write_model_fixture(name):
    for wseed in range(200):
        why, got = try_seed(name, wseed)
        if got is None:
            print(f'{name} seed {wseed}: rejected: {why}')
            continue
        meta, arrays = got
        print(f'{name} seed {wseed}: accepted; lengths',
              {k: [len(u) for u in v] for k, v in meta['tokens'].items()}, 'of',
              meta['enc_lens'], 'e_enc', meta['e_enc'], meta['e_enc_chunk'])
        save_split(name, meta, arrays)
        return 0
    print(f'{name}: no seed met the conditions')
    return 1


def write_module_fixture():
    from wenet.models.squeezeformer.attention import RelPositionMultiHeadedAttention
    from wenet.models.squeezeformer.convolution import ConvolutionModule
    from wenet.models.squeezeformer.encoder_layer import SqueezeformerEncoderLayer
    from wenet.models.squeezeformer.positionwise_feed_forward import PositionwiseFeedForward
    from wenet.models.squeezeformer.subsampling import (TimeReductionLayer1D,
                                                        TimeReductionLayerStream)
    arrays = {}
    with torch.no_grad():
        m = SQ.ATTN_MODULE
        x, sd, pos = SQ.attn_module_inputs()
        att = RelPositionMultiHeadedAttention(m['H'], m['d'], 0.0, True, True, False)
        att = att.double().eval()
        att.load_state_dict(sd, strict=True)
        for T in m['frames']:
            xx = x[:T].unsqueeze(0)
            y, _ = att(xx, xx, xx, torch.ones(1, T, T, dtype=torch.bool), pos[:T].unsqueeze(0))
            arrays[f'attn_{T}'] = y[0].numpy()
        m = SQ.REDUCE_MODULE
        for K, cls, key in ((5, TimeReductionLayer1D, 'reduce1d'),
                            (1, TimeReductionLayerStream, 'reducestream')):
            x, sd = SQ.reduce_module_inputs(K)
            red = cls(m['d'], m['d']).double().eval()
            red.load_state_dict(sd, strict=True)
            for T in m['frames']:
                y, ln, _, _ = red(x[:T].unsqueeze(0), torch.tensor([T]),
                                  torch.ones(1, T, T, dtype=torch.bool),
                                  torch.ones(1, 1, T, dtype=torch.bool))
                assert int(ln[0]) == (T + 1) // 2 == y.shape[1]
                arrays[f'{key}_{T}'] = y[0].numpy()
        for name in SQ.TINY:
            x, configs, sd = SQ.layer_module_inputs(name)
            ec = configs['encoder_conf']
            d, H = ec['encoder_dim'], ec['attention_heads']
            act = torch.nn.SiLU()
            ff = lambda: PositionwiseFeedForward(d, d * ec['feed_forward_expansion_factor'], 0.0,
                                                 act, True, False)
            layer = SqueezeformerEncoderLayer(
                d, RelPositionMultiHeadedAttention(H, d, 0.0, ec['do_rel_shift'], True, False),
                ff(), ConvolutionModule(d, ec['cnn_module_kernel'], act, ec['cnn_norm_type'],
                                        ec['causal'], True, True, False), ff(), False, 0.0, False)
            layer = layer.double().eval()
            p = 'encoder.encoders.0.'
            layer.load_state_dict({k[len(p):]: (v.double() if v.is_floating_point() else v)
                                   for k, v in sd.items() if k.startswith(p)}, strict=True)
            T = x.shape[0]
            pe = sd['encoder.embed.pos_enc.pe'].double().reshape(1, -1, d)
            y = layer(x.unsqueeze(0), torch.ones(1, T, T, dtype=torch.bool), pe[:, :T],
                      torch.ones(1, 1, T, dtype=torch.bool))[0]
            arrays[f'layer_{name}'] = y[0].numpy()
    save_split('modules', dict(attn=SQ.ATTN_MODULE, reduce=SQ.REDUCE_MODULE,
                               layer_frames=SQ.LAYER_T), arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    global SQ
    import squeezeformer_refs as SQ
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    os.makedirs(OUT, exist_ok=True)
    write_module_fixture()
    return max(write_model_fixture(n) for n in SQ.TINY)


if __name__ == '__main__':
    sys.exit(main())
