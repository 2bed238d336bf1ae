#!/usr/bin/env python3
"""Record what the REAL reference's Paraformer computes, for tests/test_paraformer_host.py and
tests/test_gpu_paraformer.py.

    python tools/gen_golden_paraformer.py [--modules-only]   # CPU only; needs the reference tree

tests/golden/paraformer/modules*.npz -- modules as .double() on inputs tests/paraformer_refs.py
rebuilds from their seeds:
  lfr_<n>            LFR() alone on n = 1, 5, 6, 7, 24, 97 frames (a gather: stored as fp32)
  cif_*              Cif(64, 1, 1, residual False, cnn_groups 1) with the weights of
                     paraformer_refs.cif_module_inputs on its 40-frame input: alphas (with the
                     tail), fires, embeddings, token_num
  sanm_attention     MultiHeadedAttentionSANM(2 heads x 128, 11 taps) on a 40-frame input
  sanm_decoder_layer SanmDecoderLayer (d 256, 512 units) on 9 token rows against 40 frames; the
                     weights and inputs of both: paraformer_refs.sanm_*_inputs
  chain_<name>_*     cif() in fp32 on the three alpha rows of paraformer_refs.CIF_ALPHA_ROWS (+ the
                     tail frame): the fires tensor and the embeddings
  meta.beautify      paraformer_beautify_result on paraformer_refs.BEAUTIFY_CASES

tests/golden/paraformer/tiny*.npz -- the reference model of `tiny_paraformer` (init_model + the
synthetic state dict, loaded strictly) on utterances of 418, 196, 190, 24, 7 and 1 frames, every
utterance ALONE, in fp32 and as .double():
  enc64_<n>          the fp64 encoder output of two of them
  meta.e_enc / e_logp   the fp32 reference's own error against fp64 on the encoder output and
                     on the chosen tokens' log-probs
  meta.token_num, fire_frames, tokens (all four methods), raised (the 1-frame utterance)
A weight seed is REJECTED unless the fp64 reference gives: every fire decision at least 1e-3 from
the threshold, every alpha sum at least 1e-2 from an integer, the fire count equal to token_num,
every chosen token at least 1e-3 above the runner-up, at least 3 distinct tokens per utterance
of T' >= 32, and the same lists from the fp32 and the fp64 reference.

Arrays are cut into row blocks (`<name>__part<i>`) and dealt into files of at most 64 KB.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

OUT = os.path.join(ROOT, 'tests', 'golden', 'paraformer')
FILE_BYTES = 64 * 1024
PF_METHODS = ('paraformer_greedy_search', 'paraformer_beam_search')


def save_split(stem, meta, arrays):
    """<stem>.npz (meta + arrays) and <stem>_<i>.npz, each with at most FILE_BYTES of arrays."""
    parts = []
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.nbytes <= FILE_BYTES // 2 or a.ndim < 2:
            parts.append((k, a))
            continue
        rows = max(1, (FILE_BYTES // 2) // max(a[0].nbytes, 1))
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
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        if f == stem + '.npz' or (f.startswith(stem + '_') and f.endswith('.npz')
                                  and f[len(stem) + 1:-4].isdigit()):
            os.remove(os.path.join(OUT, f))
    for i, d in enumerate(files):
        path = os.path.join(OUT, f'{stem}.npz' if i == 0 else f'{stem}_{i}.npz')
        extra = dict(meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)) if i == 0 \
            else {}
        np.savez_compressed(path, **extra, **d)
        assert os.path.getsize(path) <= 80 * 1024, (path, os.path.getsize(path))
        print(f'{path}: {os.path.getsize(path)} bytes')


def write_module_fixture():
    from wenet.models.paraformer.cif import Cif, cif
    from wenet.models.paraformer.layers import LFR
    from wenet.models.paraformer.search import paraformer_beautify_result
    arrays = {}
    lfr = LFR()
    for n in PR.GOLDEN_LFR_N:
        x = PR.features(n, PR.MODULE_SEED).double()
        y, ln = lfr(x.unsqueeze(0), torch.tensor([n]))
        assert int(ln[0]) == y.shape[1]
        assert torch.equal(y[0].float().double(), y[0])     # a gather of fp32 frames
        arrays[f'lfr_{n}'] = y[0].float().numpy()
    ci = PR.cif_module_inputs()
    d, T = ci['h'].shape[1], ci['h'].shape[0]
    g = torch.Generator().manual_seed(PR.MODULE_SEED + 1)
    mod = Cif(d, 1, 1, threshold=1.0, dropout=0.0, smooth_factor=1.0, noise_threshold=0.0,
              tail_threshold=0.45, residual=False, cnn_groups=1).double().eval()
    mod.load_state_dict({'cif_conv1d.weight': ci['conv_w'], 'cif_conv1d.bias': ci['conv_b'],
                         'cif_output.weight': ci['out_w'], 'cif_output.bias': ci['out_b']},
                        strict=True)
    with torch.no_grad():
        emb, token_num, alphas, fires = mod(ci['h'].unsqueeze(0),
                                            mask=torch.ones(1, 1, T, dtype=torch.bool))
    arrays.update(cif_alphas=alphas[0].numpy(), cif_fires=fires[0].numpy(),
                  cif_emb=emb[0].numpy(), cif_token_num=token_num.numpy())
    for name, row in PR.CIF_ALPHA_ROWS.items():
        a = torch.tensor(row + [0.45], dtype=torch.float32).unsqueeze(0)
        hh = torch.randn(1, a.shape[1], 64, generator=g)
        hh[:, -1] = 0.0
        e, f = cif(hh, a, 1.0)
        arrays[f'chain_{name}_h'] = hh[0].numpy()
        arrays[f'chain_{name}_fires'] = f[0].numpy()
        arrays[f'chain_{name}_emb'] = e[0].numpy()
    # one MultiHeadedAttentionSANM and one SanmDecoderLayer as .double(), all-ones masks
    from wenet.models.paraformer.attention import (DummyMultiHeadSANM, MultiHeadAttentionCross,
                                                   MultiHeadedAttentionSANM)
    from wenet.models.paraformer.layers import (PositionwiseFeedForwardDecoderSANM,
                                                SanmDecoderLayer)
    H, dm, K = PR.SANM_H, PR.SANM_D, PR.SANM_K
    x, sd = PR.sanm_attention_inputs()
    att = MultiHeadedAttentionSANM(H, dm, dm, 0.0, K).double().eval()
    att.load_state_dict(sd, strict=True)
    ones = torch.ones(1, 1, x.shape[0], dtype=torch.bool)
    with torch.no_grad():
        y, _ = att(x.unsqueeze(0), x.unsqueeze(0), x.unsqueeze(0), ones, ones)
    arrays['sanm_attention'] = y[0].numpy()
    tgt, mem, sd = PR.sanm_decoder_layer_inputs()
    layer = SanmDecoderLayer(dm, DummyMultiHeadSANM(H, dm, dm, 0.0, K),
                             MultiHeadAttentionCross(H, dm, dm, 0.0, K, 0, dm),
                             PositionwiseFeedForwardDecoderSANM(dm, PR.DECL_UNITS, 0.0),
                             0.0).double().eval()
    layer.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y, _, _, _ = layer(tgt.unsqueeze(0), torch.ones(1, 1, tgt.shape[0], dtype=torch.bool),
                           mem.unsqueeze(0), torch.ones(1, 1, mem.shape[0], dtype=torch.bool))
    arrays['sanm_decoder_layer'] = y[0].numpy()
    meta = dict(beautify=[paraformer_beautify_result(list(t)) for t in PR.BEAUTIFY_CASES])
    save_split('modules', meta, arrays)


def _run_alone(model, feats, dtype):
    """Per utterance: dict(raised) or dict(enc, alphas, fires, token_num, logp rows, tokens)."""
    from wenet.models.paraformer.search import (paraformer_beam_search,
                                                paraformer_greedy_search)
    from wenet.models.transformer.search import ctc_greedy_search, ctc_prefix_beam_search
    out = []
    with torch.no_grad():
        for f in feats:
            x, ln = f.unsqueeze(0).to(dtype), torch.tensor([f.shape[0]])
            enc, mask = model._forward_encoder(x, ln)
            r = dict(enc=enc[0].double())
            ctc = model.ctc_logprobs(enc, 0.0, 0)
            el = mask.squeeze(1).sum(1)
            r['tokens'] = {
                'ctc_greedy_search': list(map(int, ctc_greedy_search(ctc, el, 0)[0].tokens)),
                'ctc_prefix_beam_search': list(map(int, ctc_prefix_beam_search(
                    ctc, el, PR.CTC_BEAM, None, 0)[0].tokens))}
            _, _, alphas, fires = model.predictor.predictor(enc, mask=mask)
            r['alphas'], r['fires'] = alphas[0].double(), fires[0].double()
            try:
                res = model._forward_paraformer(x, ln)
                r['raised'] = False
            except Exception as e:      # noqa: BLE001 -- recorded: the zero-token utterance
                r['raised'] = True
                r['error'] = type(e).__name__
                out.append(r)
                continue
            dec, n = res['decoder_out'], res['decoder_out_lens']
            r['token_num'] = int(n[0])
            g = paraformer_greedy_search(dec, n, None)[0]
            b = paraformer_beam_search(dec, n, beam_size=PR.CTC_BEAM, eos=model.eos)[0]
            r['tokens']['paraformer_greedy_search'] = list(map(int, g.tokens))
            r['tokens']['paraformer_beam_search'] = list(map(int, b.tokens))
            rows = dec[0, :int(n[0])].double()
            top2 = rows.topk(2, dim=-1).values
            r['logp'] = top2[:, 0]
            r['gap'] = float((top2[:, 0] - top2[:, 1]).min()) if rows.shape[0] else 1.0
            out.append(r)
    return out


def try_seed(wseed):
    from oracle.gen_golden import build_reference_model
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_paraformer')
    sd = S.make_state_dict(configs, wseed)
    feats = PR.tiny_features()
    r64 = _run_alone(build_reference_model(configs, sd).double(), feats, torch.float64)
    token_num, fire_frames, raised, margins = [], [], [], dict(fire=1.0, sum=1.0, gap=1.0)
    for f, r in zip(feats, r64):
        tp = PR.lfr_rows(f.shape[0])
        a = r['alphas'].numpy()
        margins['fire'] = min(margins['fire'], float(np.abs(r['fires'].numpy() - 1.0).min()))
        margins['sum'] = min(margins['sum'], float(abs(a.sum() - round(a.sum()))))
        fr = [int(t) for t in np.nonzero(r['fires'].numpy() >= 1.0)[0]]
        n_tok = int(np.floor(a.sum()))
        if len(fr) != n_tok:
            return 'fire count != token_num', None
        raised.append(bool(r['raised']))
        if r['raised'] != (n_tok == 0):
            return 'the reference raised on an utterance with tokens (or not on one without)', None
        if not r['raised']:
            if r['token_num'] != n_tok:
                return 'token_num of the model != floor(sum alpha)', None
            margins['gap'] = min(margins['gap'], r['gap'])
            if tp >= 32 and len(set(r['tokens']['paraformer_greedy_search'])) < 3:
                return 'fewer than 3 distinct tokens on a long utterance', None
        token_num.append(n_tok)
        fire_frames.append(fr)
    if margins['fire'] < 1e-3 or margins['sum'] < 1e-2 or margins['gap'] < 1e-3:
        return f'margins {margins}', None
    if raised != [n == 1 for n in PR.TINY_LENS]:
        return f'raised {raised}', None
    r32 = _run_alone(build_reference_model(configs, sd), feats, torch.float32)
    e_enc, e_logp = [], []
    for a, b in zip(r32, r64):
        if a['tokens'] != b['tokens'] or a['raised'] != b['raised']:
            return 'fp64 and fp32 decode different tokens (near-tie)', None
        e_enc.append(float((a['enc'] - b['enc']).abs().max()))
        e_logp.append(0.0 if b['raised'] or b['token_num'] == 0
                      else float((a['logp'] - b['logp']).abs().max()))
    arrays = {}
    for f, r in zip(feats, r64):
        if f.shape[0] in PR.TINY_ENC_SAVED:
            arrays[f'enc64_{f.shape[0]}'] = r['enc'].numpy()
        if not r['raised']:
            arrays[f'logp64_{f.shape[0]}'] = r['logp'].numpy()
    methods = ('ctc_greedy_search', 'ctc_prefix_beam_search') + PF_METHODS
    tokens = {m: [r['tokens'].get(m, []) for r in r64] for m in methods}
    meta = dict(config='tiny_paraformer', wseed=wseed, lens=PR.TINY_LENS, fseed=PR.TINY_FSEED,
                ctc_beam=PR.CTC_BEAM, tokens=tokens, token_num=token_num, fire_frames=fire_frames,
                raised=raised, errors=[r.get('error') for r in r64], e_enc=e_enc, e_logp=e_logp,
                margins=margins, enc_lens=[PR.lfr_rows(n) for n in PR.TINY_LENS])
    return None, (meta, arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    global PR
    import paraformer_refs as PR
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    write_module_fixture()
    if '--modules-only' in sys.argv:
        return 0
    for wseed in range(60):
        why, got = try_seed(wseed)
        if got is None:
            print(f'seed {wseed}: rejected: {why}')
            continue
        meta, arrays = got
        print(f'seed {wseed}: accepted; token_num {meta["token_num"]} margins {meta["margins"]} '
              f'e_enc {meta["e_enc"]} e_logp {meta["e_logp"]}')
        save_split('tiny', meta, arrays)
        return 0
    print('no seed met the conditions')
    return 1


if __name__ == '__main__':
    sys.exit(main())
