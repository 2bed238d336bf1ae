#!/usr/bin/env python3
"""Single-file transcription: the `wenet` command of the reference
(wenet/cli/transcribe.py:20-73) on the MI355X path.

    python -m wenet_amd.bin.transcribe audio.wav -m /path/to/model_dir

`model_dir` holds train.yaml, final.pt, units.txt (+ global_cmvn), like
`wenet.load_model` expects (cli/model.py:71-110); there is no model download
(no network) and no CPU device.  Like the reference's `main`, the text of
`model.transcribe(audio_file)` is printed; `--beam`, `--context_path` /
`--context_score` are honoured here (the reference parses and ignores them).

    python -m wenet_amd.bin.transcribe audio.wav -m /path/to/model_dir --stream [--chunk 16]

feeds the file's features through one streaming session (wenet_amd.streaming) in chunk-sized
pieces, prints every partial result that differs from the one before, then the final text.

    python -m wenet_amd.bin.transcribe audio.wav -m /path/to/model_dir --align --label "TEXT"

force-aligns the file with the given transcript (wenet/cli/transcribe.py:39-42 declares the two
options) and prints the `.lab` lines of wenet/bin/alignment.py: `begin end token` per token.
"""
import argparse
import sys


def get_args(argv=None):
    p = argparse.ArgumentParser(description='transcribe one wav file on MI355X')
    p.add_argument('audio_file', help='audio file to transcribe (PCM16 wav)')
    p.add_argument('-m', '--model', required=True, help='local model dir')
    p.add_argument('--device', default='cuda', choices=['cuda'],
                   help='only the MI355X path exists')
    p.add_argument('-t', '--show_tokens_info', action='store_true',
                   help='also print tokens, time stamps and confidences')
    p.add_argument('--beam', type=int, default=None,
                   help='beam size (default: the decode() default of transcribe)')
    p.add_argument('--context_path', type=str, default=None, help='context list file')
    p.add_argument('--context_score', type=float, default=6.0, help='context score')
    p.add_argument('--task', default=None, choices=['transcribe', 'translate', 'vad'],
                   help='Whisper models: the task token of the prompt (default transcribe)')
    p.add_argument('--lang', default=None,
                   help='Whisper models: language code of the prompt, e.g. en, zh (default en)')
    p.add_argument('--lid', default=None,
                   help='SenseVoice models: language of the query row (auto, zh, en, yue, ja, ko, '
                        'nospeech; default auto)')
    p.add_argument('--itn', default=None, choices=['withitn', 'woitn'],
                   help='SenseVoice models: text normalisation of the query row (default woitn)')
    p.add_argument('--stream', action='store_true',
                   help='decode through a streaming session, printing partial results')
    p.add_argument('--chunk', type=int, default=16,
                   help='decoding_chunk_size of --stream (encoder frames per step)')
    p.add_argument('--search', default='ctc_prefix_beam_search',
                   choices=['ctc_prefix_beam_search', 'rnnt_greedy_search',
                            'rnnt_prefix_beam_search'],
                   help='the search of --stream; rnnt_greedy_search needs a transducer model '
                        'and does no attention rescoring; rnnt_prefix_beam_search needs one '
                        'too and keeps an n-best per chunk (--beam_size, --search_ctc_weight, '
                        '--search_transducer_weight)')
    p.add_argument('--beam_size', type=int, default=5,
                   help='beam of --search rnnt_prefix_beam_search')
    p.add_argument('--search_ctc_weight', type=float, default=0.3,
                   help='CTC weight of the shallow fusion in --search rnnt_prefix_beam_search')
    p.add_argument('--search_transducer_weight', type=float, default=0.7,
                   help='transducer weight of that fusion')
    p.add_argument('--align', action='store_true',
                   help='force align the input audio and transcript')
    p.add_argument('--label', type=str, default=None, help='the input label to align')
    args = p.parse_args(argv)
    if args.align and args.label is None:
        p.error('--align needs --label TEXT')
    if args.label is not None and not args.align:
        p.error('--label is only read with --align')
    return args


def align_file(model, audio_file, label, out=print):
    """Force-align the file with `label`; `out` gets the .lab lines.  Returns the AlignResult."""
    from wenet_amd.align import get_labformat
    r = model.align_wav(audio_file, label)
    if not r.ok:
        raise SystemExit(f'--align: the {len(r.tokens)} tokens of the label do not fit into '
                         f'the audio')
    tok = model.tokenizer
    char_dict = getattr(tok, 'char_dict', None) or getattr(tok, 'id2sym', None)
    for line in get_labformat(r.frames, model.subsampling_rate(), char_dict):
        out(line.rstrip('\n'))
    return r


def stream_file(model, audio_file, chunk, beam_size=10, out=print,
                search='ctc_prefix_beam_search', search_ctc_weight=0.3,
                search_transducer_weight=0.7):
    """One streaming session over the file; `out` gets each changed partial, then the final
    result's text.  Returns the final DecodeResult."""
    from wenet_amd.streaming import RnntBeamStreamingRecognizer, StreamingRecognizer
    speech = model.compute_feature(audio_file).to(model.device)
    if search == RnntBeamStreamingRecognizer.SEARCH:
        rec = RnntBeamStreamingRecognizer(model, 1, chunk, beam_size=beam_size,
                                          search_ctc_weight=search_ctc_weight,
                                          search_transducer_weight=search_transducer_weight,
                                          max_seconds=speech.size(0) / 100.0 + 1.0)
    else:
        rec = StreamingRecognizer(model, 1, chunk, beam_size=beam_size,
                                  max_seconds=speech.size(0) / 100.0 + 1.0, search=search)
    sid = rec.open()
    piece = chunk * model.subsampling_rate()
    shown = None
    for i in range(0, speech.size(0), piece):
        rec.accept(sid, speech[i:i + piece])
        for r in rec.step().values():
            text = model.tokenizer.detokenize(list(r.tokens))[0]
            if text != shown:
                out(f'[partial] {text}')
                shown = text
    result = rec.finish(sid)
    rec.close(sid)
    result.text = model.tokenizer.detokenize(list(result.tokens))[0]
    return result


def main(argv=None):
    args = get_args(argv)
    import torch
    import wenet_amd
    model = wenet_amd.load_model(args.model, device=args.device)
    if args.align:
        align_file(model, args.audio_file, args.label)
        return 0
    if args.stream:
        if args.context_path is not None:
            raise SystemExit('--stream does not support --context_path')
        if args.search == 'rnnt_prefix_beam_search':
            result = stream_file(model, args.audio_file, args.chunk, args.beam or args.beam_size,
                                 search=args.search, search_ctc_weight=args.search_ctc_weight,
                                 search_transducer_weight=args.search_transducer_weight)
        else:
            result = stream_file(model, args.audio_file, args.chunk, args.beam or 10,
                                 search=args.search)
    elif args.beam is None and args.context_path is None and args.task is None \
            and args.lang is None and args.lid is None and args.itn is None:
        result = model.transcribe(args.audio_file)      # asr_model.py:345-358
    else:
        graph = None
        if args.context_path is not None:
            from wenet_amd.context_graph import ContextGraph
            bpe = getattr(model.tokenizer, 'bpe_path', None)
            graph = ContextGraph(args.context_path, model.tokenizer.symbol_table, bpe,
                                 args.context_score)
        infos = None
        if args.task is not None or args.lang is not None:
            from wenet_amd import whisper
            if not whisper.is_whisper(model.special_tokens):
                raise SystemExit('--task / --lang are read by Whisper models only')
            infos = dict(tasks=[args.task or 'transcribe'], langs=[args.lang or 'en'])
        if args.lid is not None or args.itn is not None:
            if not isinstance(model, wenet_amd.SenseVoiceSmall):
                raise SystemExit('--lid / --itn are read by SenseVoice models only')
            infos = dict(lid=args.lid or 'auto', itn=args.itn or 'woitn')
        speech = model.compute_feature(args.audio_file)
        method = model.default_decode_method
        result = model.decode([method], speech.unsqueeze(0),
                              torch.tensor([speech.size(0)]),
                              beam_size=args.beam or 10, context_graph=graph,
                              infos=infos)[method][0]
        result.text = model.tokenizer.detokenize(result.tokens)[0]
    print(result.text)
    if args.show_tokens_info:
        print('tokens', list(result.tokens))
        print('times', result.times)
        print('tokens_confidence', result.tokens_confidence)
    return 0


if __name__ == '__main__':
    sys.exit(main())
