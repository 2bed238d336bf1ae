#!/usr/bin/env python3
"""CTC forced alignment on MI355X: the command line of `wenet/bin/alignment.py`.

    python -m wenet_amd.bin.alignment --config train.yaml --checkpoint final.pt \\
        --dict units.txt --input_file data.list --result_file out/align.txt \\
        [--batch_size 32] [--gen_praat] [--blank_thres 0.999999] [--thres 0.000001]

`input_file` is a raw data list (one JSON object per line with `key`, `wav`, `txt`, read like
bin/recognize.py reads it).  Every utterance's transcript is tokenised with the config's
tokenizer and aligned to its audio; the result file gets one line per key: the key and the
space-separated label id of every encoder frame.  (The reference writes the `repr` of a
tensor there, which elides the middle of long alignments.)  With `--gen_praat` a `<key>.lab`
(`begin end token` per line) and a `<key>.TextGrid` land next to the result file.

Unlike the reference (alignment.py:179-181) any batch size works: consecutive groups of
`batch_size` utterances, longest first inside a batch.  An utterance whose transcript does
not fit into its frames is logged and skipped; the exit status stays 0.
"""
import argparse
import json
import logging
import os
import sys
from typing import List, Sequence


def get_args(argv=None):
    p = argparse.ArgumentParser(description='use ctc to generate alignment')
    p.add_argument('--config', required=True, help='config file')
    p.add_argument('--input_file', required=True, help='format data file')
    p.add_argument('--data_type', default='raw', choices=['raw'],
                   help='raw lists only (the transcript is the list\'s "txt")')
    p.add_argument('--gpu', type=int, default=-1, help='device index (default 0)')
    p.add_argument('--device', default='cuda', choices=['cuda'],
                   help='only the MI355X path exists; there is no CPU fallback')
    p.add_argument('--blank_thres', default=0.999999, type=float, help='ctc blank thes')
    p.add_argument('--thres', default=0.000001, type=float, help='ctc non blank thes')
    p.add_argument('--checkpoint', required=True, help='checkpoint model')
    p.add_argument('--dict', required=True, help='dict file')
    p.add_argument('--non_lang_syms',
                   help='non-linguistic symbol file (accepted; not used on this path)')
    p.add_argument('--result_file', required=True, help='alignment result file')
    p.add_argument('--batch_size', type=int, default=1, help='batch size (any)')
    p.add_argument('--gen_praat', action='store_true',
                   help='convert alignment to a praat format')
    p.add_argument('--bpe_model', default=None, type=str, help='bpe model for english part')
    args = p.parse_args(argv)
    if args.batch_size < 1:
        p.error('--batch_size must be positive')
    return args


def read_char_dict(path: str):
    """alignment.py:186-192: id -> symbol."""
    char_dict = {}
    with open(path, 'r', encoding='utf8') as fin:
        for line in fin:
            arr = line.strip().split()
            assert len(arr) == 2
            char_dict[int(arr[1])] = arr[0]
    return char_dict


def read_align_list(path: str):
    """(key, wav source, txt) per utterance of a raw list, in list order."""
    from wenet_amd.bin.recognize import read_data_list
    entries = read_data_list(path, 'raw')
    txts = []
    with open(path, 'r', encoding='utf8') as f:
        for line in f:
            if line.strip():
                txts.append(json.loads(line).get('txt', ''))
    return [(k, src, t) for (k, src), t in zip(entries, txts)]


def format_result_line(key: str, alignment: Sequence[int]) -> str:
    return '{} {}'.format(key, ' '.join(str(int(a)) for a in alignment))


def write_praat(result_file: str, key: str, result, subsample: int, char_dict,
                blank_id: int = 0) -> List[str]:
    """`<key>.lab` and `<key>.TextGrid` next to the result file (alignment.py:252-268)."""
    from wenet_amd.align import get_labformat, write_textgrid
    lab = get_labformat(result.frames, subsample, char_dict, blank_id)
    d = os.path.dirname(result_file)
    with open(os.path.join(d, key + '.lab'), 'w', encoding='utf-8') as f:
        f.writelines(lab)
    write_textgrid(os.path.join(d, key + '.TextGrid'),
                   (len(result.alignment) + 1) * 0.01 * subsample, lab)
    return lab


def align_batches(model, entries, labels_of, args, blank_id, char_dict, fout):
    """Align `entries` batch by batch; returns (aligned, skipped)."""
    import torch
    from wenet_amd.bin.recognize import padding_order, static_batches
    from wenet_amd.model import read_wav
    n_ok = n_skip = 0
    sub = model.subsampling_rate()
    for batch in static_batches(entries, args.batch_size):
        waves = []
        for _, src, _ in batch:
            w, sr = (read_wav(src[0], return_rate=True, start=src[1], end=src[2])
                     if isinstance(src, tuple) else read_wav(src, return_rate=True))
            waves.append(w if sr == 16000 else model.resample(w, sr, 16000))
        feats, lens = model.compute_fbank(waves)
        perm = padding_order(torch.as_tensor(lens).tolist())
        idx = torch.as_tensor(perm, dtype=torch.long)
        feats = feats.index_select(0, idx.to(feats.device))
        lens = torch.as_tensor(lens).cpu().index_select(0, idx)
        batch = [batch[i] for i in perm]
        labels = [labels_of(txt) for _, _, txt in batch]
        results = model.align(feats, lens, labels, blank_id=blank_id,
                              blank_thres=args.blank_thres, thres=args.thres)
        for (key, _, _), r in zip(batch, results):
            if not r.ok:
                logging.warning('%s: %d labels do not fit into the encoder frames; skipped',
                                key, len(r.tokens))
                n_skip += 1
                continue
            fout.write(format_result_line(key, r.alignment) + '\n')
            if args.gen_praat and r.frames:
                write_praat(args.result_file, key, r, sub, char_dict, blank_id)
            n_ok += 1
    return n_ok, n_skip


def main(argv=None):
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(levelname)s %(message)s')
    import torch
    import yaml
    from wenet_amd.align import tokenize_text
    from wenet_amd.bin.recognize import check_feature_conf, load_state
    from wenet_amd.model import ASRModel
    from wenet_amd.tokenizer import get_blank_id, init_tokenizer, read_symbol_table

    device = torch.device('cuda', args.gpu if args.gpu >= 0 else 0)
    torch.cuda.set_device(device)
    with open(args.config, 'r') as fin:
        configs = yaml.load(fin, Loader=yaml.FullLoader)
    check_feature_conf(configs)
    char_dict = read_char_dict(args.dict)
    symbol_table = read_symbol_table(args.dict)
    kind, bpe = 'char', args.bpe_model
    if 'tokenizer_conf' in configs:
        tok = init_tokenizer(configs)
        kind, bpe = tok.kind, args.bpe_model or tok.bpe_path
    elif bpe is not None:
        kind = 'bpe'
    blank_id = get_blank_id(configs, symbol_table)
    model = ASRModel(configs, load_state(configs, args.checkpoint), device)
    entries = read_align_list(args.input_file)
    os.makedirs(os.path.dirname(os.path.abspath(args.result_file)), exist_ok=True)
    with open(args.result_file, 'w', encoding='utf-8') as fout:
        n_ok, n_skip = align_batches(
            model, entries, lambda txt: tokenize_text(txt, symbol_table, bpe, kind), args,
            blank_id, char_dict, fout)
    logging.info('aligned %d utterances, skipped %d', n_ok, n_skip)
    return 0


if __name__ == '__main__':
    sys.exit(main())
