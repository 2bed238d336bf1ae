#!/usr/bin/env python3
"""Record what the REAL reference's SenseVoice Small computes, for tests/test_sensevoice_host.py
and tests/test_gpu_sensevoice.py.

    python tools/gen_golden_sensevoice.py        # CPU only; needs the reference tree

tests/golden/sensevoice/<config>*.npz for `tiny_sensevoice` and `tiny_sensevoice_h64` -- the
reference model (init_model + the synthetic state dict, loaded strictly) through
SenseVoiceSmall.decode on utterances of 1, 6, 7, 167, 169, 360 and 431 frames, every utterance
ALONE, in fp32 and as .double(), under three query settings (sensevoice_refs.SETTINGS: default,
en / withitn, an unknown lid with an unknown itn):
  enc64_<setting>_<n>   the fp64 encoder output (what model.encoder returns inside decode) of the
                        utterances in sensevoice_refs.TINY_ENC_SAVED
  meta.settings.<name>  tokens of both CTC methods at beam 5, the prefix-beam scores, and the fp32
                        reference's own error against fp64: e_enc (encoder output), e_logp (CTC
                        log-probs), e_score (first prefix-beam score)
  meta.enc_lens, meta.zero_raised / zero_error (decode on an utterance without frames)
A weight seed is REJECTED unless, for every utterance and setting: the fp32 and the fp64 token
lists agree, the fp64 gap between the best and the second-best class exceeds 64 e_logp at every
frame, and the gap between the first and the second beam score exceeds 64 e_score.  The third
setting must equal the first bit for bit.

Arrays are cut into row blocks (`<name>__part<i>`) and dealt into files of at most 64 KB.
"""
import argparse
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

OUT = os.path.join(ROOT, 'tests', 'golden', 'sensevoice')
FILE_BYTES = 64 * 1024
MARGIN = 64.0


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


def build_reference_model(configs, sd, workdir):
    """init_model on the configuration, with the synthetic CMVN as the json file the reference
    reads (wenet/utils/cmvn.py), then the state dict loaded strictly."""
    from wenet.utils.init_model import init_model
    mean = sd['global_cmvn.mean'].double().numpy()
    istd = sd['global_cmvn.istd'].double().numpy()
    n = 1000
    var = 1.0 / (istd * istd)
    path = os.path.join(workdir, 'global_cmvn')
    with open(path, 'w') as f:
        json.dump({'mean_stat': (mean * n).tolist(),
                   'var_stat': ((var + mean * mean) * n).tolist(), 'frame_num': n}, f)
    rc = copy.deepcopy(configs)
    rc['cmvn_conf'] = {'cmvn_file': path, 'is_json_cmvn': True}
    model, _ = init_model(argparse.Namespace(), rc)
    # the model takes the CMVN off its encoder: its state dict says global_cmvn.*
    assert set(model.state_dict()) == set(sd), \
        (sorted(set(model.state_dict()) - set(sd)), sorted(set(sd) - set(model.state_dict())))
    model.load_state_dict(sd, strict=True)
    model.eval()
    return model


def _run_alone(model, feats, dtype, infos):
    """Per utterance through SenseVoiceSmall.decode: dict(enc, logp, tokens, scores)."""
    got = {}
    hook = model.encoder.register_forward_hook(lambda mod, args, out: got.update(enc=out[0]))
    out = []
    try:
        with torch.no_grad():
            for f in feats:
                x, ln = f.unsqueeze(0).to(dtype), torch.tensor([f.shape[0]])
                before = ln.clone()
                res = model.decode(list(SR.METHODS), x, ln, beam_size=SR.CTC_BEAM,
                                   infos=dict(infos))
                assert torch.equal(ln, before) or torch.equal(ln, before + 4)
                enc = got['enc']
                logp = model.ctc_logprobs(enc, 0.0, 0)[0].double()
                pb = res['ctc_prefix_beam_search'][0]
                out.append(dict(enc=enc[0].double(), logp=logp,
                                tokens={m: [int(t) for t in res[m][0].tokens]
                                        for m in SR.METHODS},
                                scores=[float(s) for s in pb.nbest_scores]))
    finally:
        hook.remove()
    return out


def try_seed(config, wseed, workdir):
    from wenet_amd import synthetic as S
    configs = S.make_configs(config)
    sd = S.make_state_dict(configs, wseed)
    feats = SR.tiny_features()
    m64 = build_reference_model(configs, sd, workdir).double()
    m32 = build_reference_model(configs, sd, workdir)
    settings, arrays = {}, {}
    for name, infos in SR.SETTINGS.items():
        r64 = _run_alone(m64, feats, torch.float64, infos)
        r32 = _run_alone(m32, feats, torch.float32, infos)
        e_enc, e_logp, e_score = [], [], []
        for f, a, b in zip(feats, r32, r64):
            if a['tokens'] != b['tokens']:
                return f'{name}: fp64 and fp32 decode different tokens (near-tie)', None
            e_enc.append(float((a['enc'] - b['enc']).abs().max()))
            e_logp.append(float((a['logp'] - b['logp']).abs().max()))
            e_score.append(abs(a['scores'][0] - b['scores'][0]))
            top2 = b['logp'].topk(2, dim=-1).values
            gap = float((top2[:, 0] - top2[:, 1]).min())
            if not gap > MARGIN * e_logp[-1]:
                return (f'{name}: class gap {gap:.3e} <= 64 e_logp ({e_logp[-1]:.3e}) on '
                        f'{f.shape[0]} frames'), None
            if len(b['scores']) > 1:
                sgap = b['scores'][0] - b['scores'][1]
                if not sgap > MARGIN * e_score[-1]:
                    return (f'{name}: beam gap {sgap:.3e} <= 64 e_score ({e_score[-1]:.3e}) on '
                            f'{f.shape[0]} frames'), None
        saved = SR.TINY_ENC_SAVED if name != 'unknown' else SR.TINY_ENC_SAVED[:1]
        for f, r in zip(feats, r64):
            if f.shape[0] in saved:
                arrays[f'enc64_{name}_{f.shape[0]}'] = r['enc'].numpy()
        settings[name] = dict(
            infos=infos, tokens={m: [r['tokens'][m] for r in r64] for m in SR.METHODS},
            scores=[r['scores'][0] for r in r64], nbest_scores=[r['scores'] for r in r64],
            e_enc=e_enc, e_logp=e_logp, e_score=e_score)
        if name == 'unknown':
            # unknown values fall back to auto / woitn: the same bits as the default
            d64 = _run_alone(m64, feats, torch.float64, SR.SETTINGS['default'])
            for a, b in zip(r64, d64):
                assert torch.equal(a['enc'], b['enc']) and a['tokens'] == b['tokens'] \
                    and a['scores'] == b['scores']
    zero = dict(zero_raised=False, zero_error=None)
    try:
        with torch.no_grad():
            m32.decode(['ctc_greedy_search'], torch.zeros(1, 0, 80), torch.tensor([0]))
    except Exception as e:      # noqa: BLE001 -- recorded: the utterance without frames
        zero = dict(zero_raised=True, zero_error=type(e).__name__)
    meta = dict(config=config, wseed=wseed, lens=SR.TINY_LENS, fseed=SR.TINY_FSEED,
                ctc_beam=SR.CTC_BEAM, enc_lens=[SR.enc_rows(n) for n in SR.TINY_LENS],
                settings=settings, **zero)
    return None, (meta, arrays)


def main():
    from oracle import _ref_harness
    _ref_harness.install()
    global SR
    import sensevoice_refs as SR
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with tempfile.TemporaryDirectory() as workdir:
        for config in SR.TINY_CONFIGS:
            for wseed in range(60):
                why, got = try_seed(config, wseed, workdir)
                if got is None:
                    print(f'{config} seed {wseed}: rejected: {why}')
                    continue
                meta, arrays = got
                print(f'{config} seed {wseed}: accepted; ' + '; '.join(
                    f'{k}: e_enc {max(v["e_enc"]):.2e} e_logp {max(v["e_logp"]):.2e} '
                    f'e_score {max(v["e_score"]):.2e}' for k, v in meta['settings'].items()))
                save_split(config, meta, arrays)
                break
            else:
                print(f'{config}: no seed met the conditions')
                return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
