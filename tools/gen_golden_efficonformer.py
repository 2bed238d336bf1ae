#!/usr/bin/env python3
"""Record what the REAL reference's Efficient Conformer modules compute, for
tests/test_efficonformer_host.py and tests/test_gpu_efficonformer.py.

    python tools/gen_golden_efficonformer.py        # CPU only; needs the reference tree

tests/golden/efficonformer/modules*.npz -- every module in fp64 (.double()) on the inputs
tests/efficonformer_refs.py rebuilds from their seeds:
  attn_<name>_<T>    GroupedRelPositionMultiHeadedAttention (d 128; 4 heads: W = 96, 2 heads:
                     W = 192; group_size 3) at T = 1, 2, 3, 4, 33, full context
  attn_<name>_21_c<chunk>_l<left>_m<m>   the same at T = 21 under
                     subsequent_chunk_mask(21 m / 3, chunk, left)[::m / 3, ::m / 3] (the mask a
                     grouped layer behind m / 3-fold striding is handed; it takes [::3, ::3] itself)
  conv_<name>_<T>    ConvolutionModule with stride 2 (d 64; K 15 LayerNorm, K 7 causal BatchNorm in
                     eval mode) at T = 1, 2, 3, 16, 33
  layer_<model>      the first StrideConformerEncoderLayer of each tiny model on 40 frames
  mask_m<m>_c<chunk>_l<left>   subsequent_chunk_mask(50, chunk, left)[::m, ::m] as uint8
  pool_<T>           AvgPool1d(2, 2, ceil_mode=True, count_include_pad=False) of arange rows

tests/golden/efficonformer/<model>*.npz -- the reference model of the two tiny configurations
(init_model + the synthetic state dict, loaded strictly) on the utterances of
efficonformer_refs.TINY, every utterance decoded ALONE with decoding_chunk_size -1 (0 on a
dynamic-chunk model draws a random chunk), in fp32 and as .double():
  enc64_<n>          the fp64 encoder output (also enc64_<n>_c<chunk>_l<left> for the model's two
                     chunk-mask cases on two utterances)
  meta.e_enc / e_enc_chunk   per utterance, the fp32 reference's own max abs error against fp64
  meta.tokens        ctc_greedy_search, ctc_prefix_beam_search (beam 5), attention_rescoring
                     (beam 5, ctc_weight 0.5, reverse_weight 0.3 on the bidecoder model)
  meta.scores / e_score   the fp64 scores of the two beam modes and |fp32 - fp64| of them
A weight seed is REJECTED unless the fp64 and the fp32 reference decode the same tokens in every
mode and at least three utterances have non-empty CTC results.

tests/golden/efficonformer/recipes/*.yaml -- the network sections of the five shipped recipes
(settings only).

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

OUT = os.path.join(ROOT, 'tests', 'golden', 'efficonformer')
FILE_BYTES = 64 * 1024
MAX_FILE = 72309          # tests/golden/firered/firered_tiny_enc3.npz
RESCORE_CTC_WEIGHT = 0.5
RECIPE_FILES = {
    'aishell_v1': 'examples/aishell/s0/conf/train_u2++_efficonformer_v1.yaml',
    'aishell_v1_stream': 'examples/aishell/s0/conf/train_u2++_efficonformer_v1_stream.yaml',
    'aishell_v2': 'examples/aishell/s0/conf/train_u2++_efficonformer_v2.yaml',
    'librispeech_v1': 'examples/librispeech/s0/conf/train_u2++_efficonformer_v1.yaml',
    'librispeech_v2': 'examples/librispeech/s0/conf/train_u2++_efficonformer_v2.yaml',
}
RECIPE_KEYS = ('encoder', 'encoder_conf', 'decoder', 'decoder_conf', 'model', 'model_conf', 'ctc',
               'ctc_conf', 'cmvn', 'tokenizer')


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
    toks = {m: [] for m in EF.METHODS}
    scores = {'ctc_prefix_beam_search': [], 'attention_rescoring': []}
    with torch.no_grad():
        for f in feats:
            r = model.decode(list(EF.METHODS), f.unsqueeze(0).to(dtype),
                             torch.tensor([f.shape[0]]), beam_size=EF.CTC_BEAM,
                             decoding_chunk_size=-1,
                             ctc_weight=RESCORE_CTC_WEIGHT, reverse_weight=reverse_weight)
            for m in EF.METHODS:
                toks[m].append(list(map(int, r[m][0].tokens)))
            for m in scores:
                scores[m].append(float(r[m][0].score))
    return toks, scores


def try_seed(name, wseed):
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs(name)
    sd = S.make_state_dict(configs, wseed)
    feats = EF.tiny_features(name)
    tiny = EF.TINY[name]
    rw = tiny['reverse_weight']
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
    with torch.no_grad():
        for f in feats:
            n = f.shape[0]
            ln = torch.tensor([n])
            e64, _ = m64._forward_encoder(f.unsqueeze(0).double(), ln)
            e32, _ = m32._forward_encoder(f.unsqueeze(0), ln)
            arrays[f'enc64_{n}'] = e64[0].numpy()
            e_enc.append(float((e32[0].double() - e64[0]).abs().max()))
            enc_lens.append(int(e64.shape[1]))
            if n in tiny['chunk_frames']:
                for (cs, lc) in tiny['chunk_cases']:
                    c64, _ = m64._forward_encoder(f.unsqueeze(0).double(), ln, cs, lc)
                    c32, _ = m32._forward_encoder(f.unsqueeze(0), ln, cs, lc)
                    key = f'{n}_c{cs}_l{lc}'
                    arrays['enc64_' + key] = c64[0].numpy()
                    e_chunk[key] = float((c32[0].double() - c64[0]).abs().max())
    e_score = {k: [abs(a - b) for a, b in zip(s32[k], s64[k])] for k in s64}
    meta = dict(frames=tiny['frames'], fseed=tiny['fseed'], reverse_weight=rw, config=name,
                wseed=wseed, ctc_beam=EF.CTC_BEAM, tokens=t64, e_enc=e_enc, enc_lens=enc_lens,
                e_enc_chunk=e_chunk, scores=s64, e_score=e_score,
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
    from wenet.models.efficient_conformer.attention import GroupedRelPositionMultiHeadedAttention
    from wenet.models.efficient_conformer.convolution import ConvolutionModule
    from wenet.models.efficient_conformer.encoder_layer import StrideConformerEncoderLayer
    from wenet.models.transformer.positionwise_feed_forward import PositionwiseFeedForward
    from wenet.utils.mask import subsequent_chunk_mask
    from wenet_amd.efficonformer import efficonformer_plan
    arrays = {}
    act = torch.nn.SiLU()
    with torch.no_grad():
        for name, m in EF.ATTN_MODULE.items():
            x, sd, pos = EF.attn_module_inputs(name)
            att = GroupedRelPositionMultiHeadedAttention(m['H'], m['d'], 0.0, m['g'])
            att = att.double().eval()
            att.load_state_dict(sd, strict=True)
            for T in m['frames']:
                xx = x[:T].unsqueeze(0)
                y, _ = att(xx, xx, xx, torch.ones(1, 1, T, dtype=torch.bool), pos[:T].unsqueeze(0))
                arrays[f'attn_{name}_{T}'] = y[0].numpy()
            T = EF.ATTN_MASK_T
            xx = x[:T].unsqueeze(0)
            for (mm, c, left) in EF.ATTN_MASK_CASES:
                f = mm // m['g']
                mask = subsequent_chunk_mask(T * f, c, left)[::f, ::f].unsqueeze(0)
                y, _ = att(xx, xx, xx, mask, pos[:T].unsqueeze(0))
                arrays[f'attn_{name}_{T}_c{c}_l{left}_m{mm}'] = y[0].numpy()
        for name, m in EF.CONV_MODULE.items():
            x, sd = EF.conv_module_inputs(name)
            conv = ConvolutionModule(m['d'], m['K'], act, m['norm'], m['causal'], True, 2)
            conv = conv.double().eval()
            conv.load_state_dict(sd, strict=True)
            for T in EF.CONV_FRAMES:
                y, _ = conv(x[:T].clone().unsqueeze(0), torch.ones(1, 1, T, dtype=torch.bool))
                assert y.shape[1] == (T + 1) // 2
                arrays[f'conv_{name}_{T}'] = y[0].numpy()
        for name in EF.TINY:
            x, configs, sd = EF.layer_module_inputs(name)
            plan = efficonformer_plan(configs)
            ec = plan['ec']
            d, H, i = plan['d'], plan['heads'], plan['stride_layers'][0]
            assert i in plan['group_layers']
            ff = lambda: PositionwiseFeedForward(d, ec['linear_units'], 0.0, act)
            layer = StrideConformerEncoderLayer(
                d, GroupedRelPositionMultiHeadedAttention(H, d, 0.0, plan['group_size']), ff(), ff(),
                ConvolutionModule(d, plan['kernels'][i], act, ec['cnn_module_norm'], plan['causal'],
                                  True, 2),
                torch.nn.AvgPool1d(kernel_size=2, stride=2, padding=0, ceil_mode=True,
                                   count_include_pad=False), 0.0, True)
            layer = layer.double().eval()
            p = f'encoder.encoders.{i}.'
            layer.load_state_dict({k[len(p):]: (v.double() if v.is_floating_point() else v)
                                   for k, v in sd.items() if k.startswith(p)}, strict=True)
            T = x.shape[0]
            pe = sd['encoder.embed.pos_enc.pe'].double().reshape(1, -1, d)
            y = layer(x.unsqueeze(0), torch.ones(1, 1, T, dtype=torch.bool), pe[:, :T],
                      torch.ones(1, 1, T, dtype=torch.bool))[0]
            arrays[f'layer_{name}'] = y[0].numpy()
        for (mm, c, left) in EF.MASK_CASES:
            arrays[f'mask_m{mm}_c{c}_l{left}'] = subsequent_chunk_mask(
                EF.MASK_T, c, left)[::mm, ::mm].numpy().astype(np.uint8)
        pool = torch.nn.AvgPool1d(2, 2, ceil_mode=True, count_include_pad=False)
        for T in (1, 2, 3, 4):
            arrays[f'pool_{T}'] = pool(torch.arange(1.0, T + 1.0).double().view(1, 1, T))[0, 0].numpy()
    save_split('modules', dict(attn=EF.ATTN_MODULE, conv=EF.CONV_MODULE, layer_frames=EF.LAYER_T),
               arrays)


def write_recipes():
    import yaml
    from oracle._ref_harness import REFERENCE_ROOT as ref
    os.makedirs(os.path.join(OUT, 'recipes'), exist_ok=True)
    for name, rel in RECIPE_FILES.items():
        with open(os.path.join(ref, rel)) as f:
            full = yaml.safe_load(f)
        keep = {k: full[k] for k in RECIPE_KEYS if k in full}
        with open(os.path.join(OUT, 'recipes', name + '.yaml'), 'w') as f:
            yaml.safe_dump(keep, f, sort_keys=False)


def accept_tuple_cache():
    """The reference's plain ConformerEncoderLayer hands its attention the (k, v) cache TUPLE of
    wenet/models/transformer/attention.py, and GroupedRelPositionMultiHeadedAttention.forward
    calls `.size` on it (efficient_conformer/attention.py:218): a grouped layer that is no stride
    layer -- layers 0 to 2 of the v1 recipes -- raises in the reference as it stands.  The empty
    tuple is replaced by the empty tensor the grouped attention was written for; what it computes
    is untouched."""
    from wenet.models.efficient_conformer.attention import \
        GroupedRelPositionMultiHeadedAttention as G
    inner = G.forward

    def forward(self, query, key, value, mask=torch.ones((0, 0, 0), dtype=torch.bool),
                pos_emb=torch.empty(0), cache=torch.zeros((0, 0, 0, 0))):
        if isinstance(cache, tuple):
            assert all(c.numel() == 0 for c in cache)
            cache = torch.zeros((0, 0, 0, 0))
        return inner(self, query, key, value, mask, pos_emb, cache)

    G.forward = forward


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    accept_tuple_cache()
    global EF
    import efficonformer_refs as EF
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    os.makedirs(OUT, exist_ok=True)
    write_recipes()
    write_module_fixture()
    return max(write_model_fixture(n) for n in EF.TINY)


if __name__ == '__main__':
    sys.exit(main())
