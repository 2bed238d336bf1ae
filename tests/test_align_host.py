"""Host side of the forced alignment, no GPU: the restated `get_frames_timestamp` /
`get_labformat` against the recorded outputs of the real reference functions
(tests/golden/align/frames_labformat.json, tools/gen_golden_align.py), the command lines, the
result-file and .lab formats, the C ABI declaration and its device-free argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(G.GOLDEN_DIR, 'align', 'frames_labformat.json')


def _records():
    with open(GOLD) as f:
        return json.load(f)


def test_frames_and_labformat_equal_the_reference_functions():
    from wenet_amd import align as A
    gold = _records()
    sub = gold['subsample']
    logp = {}
    n = n_blank_kept = 0
    pairs_seen = set()
    for rec in gold['records']:
        if rec['case'] not in logp:
            logp[rec['case']] = G.load_case(rec['case'])[1]
        arr = logp[rec['case']]
        lp = arr['ctc_logp'][rec['utt'], :arr['enc_lens'][rec['utt']]]
        char_dict = {i: f't{i}' for i in range(lp.shape[-1])}
        alignment = list(rec['alignment'])
        for p in rec['pairs']:
            ts = A.get_frames_timestamp(alignment, lp, p['blank_thres'], p['thres'])
            assert ts == p['timestamp'], (rec['case'], rec['utt'], rec['what'], p['thres'])
            assert A.get_labformat(ts, sub, char_dict) == p['labformat']
            assert alignment == rec['alignment']        # the caller's list is not changed
            iv = A.get_intervals(ts, sub)
            assert ['{:.2f} {:.2f} t{}\n'.format(*x) for x in iv] == p['labformat']
            n += 1
            n_blank_kept += any(0 in g for g in ts)
            pairs_seen.add((p['blank_thres'], p['thres']))
    assert n == 3 * len(gold['records']) and len(gold['records']) >= 60
    assert pairs_seen == {(0.999999, 1e-6), (0.999, 1e-10), (0.6, 0.05)}
    assert n_blank_kept > 0     # both branches of the border rule are exercised
    assert {r['case'] for r in gold['records']} == {'tiny_sym_full', 'tiny_causal_full',
                                                    'tiny_bn_full'}


def test_two_column_frame_logprobs_are_all_the_time_stamp_rule_reads():
    """align() hands get_frames_timestamp the (T', 2) array of wn_ctc_force_align (blank, label
    of the frame's token group): same groups as with the full matrix."""
    from wenet_amd import align as A
    gold = _records()
    arr = G.load_case('tiny_causal_full')[1]
    done = 0
    for rec in gold['records']:
        if rec['case'] != 'tiny_causal_full':
            continue
        lp = arr['ctc_logp'][rec['utt'], :arr['enc_lens'][rec['utt']]]
        path = rec['alignment']
        grp, fl = 0, np.zeros((len(path), 2), np.float32)
        for t in range(len(path) - 1, -1, -1):      # what the kernel's backtrace records
            if path[t] != 0:
                grp = path[t]
            fl[t] = (lp[t, 0], lp[t, grp])
        for p in rec['pairs']:
            ts = A.get_frames_timestamp(path, A._TwoColumns(fl, 0), p['blank_thres'], p['thres'])
            assert ts == p['timestamp']
            done += 1
    assert done >= 30


def test_frames_with_a_nonzero_blank_and_the_all_blank_alignment():
    from wenet_amd import align as A
    lp = np.log(np.full((6, 4), 0.25, np.float32))
    assert A.get_frames_timestamp([3, 3, 3], lp, blank_id=3) == []
    ts = A.get_frames_timestamp([3, 1, 1, 3, 2, 3], lp, 0.999, 0.9, blank_id=3)
    # blank prob 0.25 < 0.999: every frame in front of a token joins it
    assert ts == [[1, 1, 1], [2, 2, 3]]
    assert A.get_intervals(ts, 4, blank_id=3) == [(0.0, 0.12, 1), (0.12, 0.12 + 0.08, 2)]


def test_textgrid_text():
    from wenet_amd import align as A
    txt = A.format_textgrid(1.0, ['0.00 0.12 a\n', '0.20 0.40 b\n'])
    assert txt.startswith('File type = "ooTextFile"\nObject class = "TextGrid"\n')
    assert 'name = "line"' in txt and 'intervals: size = 5' in txt
    assert 'text = "a"' in txt and 'text = "b"' in txt and 'xmin = 0.2001' in txt


def test_alignment_cli_arguments_and_result_format(tmp_path):
    from wenet_amd.bin import alignment as cli
    a = cli.get_args(['--config', 'c.yaml', '--checkpoint', 'f.pt', '--dict', 'u.txt',
                      '--input_file', 'd.list', '--result_file', 'o/r.txt', '--batch_size', '24',
                      '--gen_praat', '--blank_thres', '0.9', '--thres', '0.01', '--gpu', '0',
                      '--bpe_model', 'b.model'])
    assert (a.batch_size, a.gen_praat, a.blank_thres, a.thres) == (24, True, 0.9, 0.01)
    assert (a.config, a.checkpoint, a.dict, a.input_file, a.result_file) == \
        ('c.yaml', 'f.pt', 'u.txt', 'd.list', 'o/r.txt')
    assert a.device == 'cuda' and a.bpe_model == 'b.model'
    d = cli.get_args(['--config', 'c', '--checkpoint', 'f', '--dict', 'u', '--input_file', 'd',
                      '--result_file', 'r'])
    assert (d.batch_size, d.blank_thres, d.thres, d.gen_praat) == (1, 0.999999, 0.000001, False)
    with pytest.raises(SystemExit):
        cli.get_args(['--config', 'c'])
    assert cli.format_result_line('utt1', np.array([0, 0, 7, 7, 0, 12])) == 'utt1 0 0 7 7 0 12'

    lst = tmp_path / 'data.list'
    lst.write_text('{"key": "a", "wav": "/x/a.wav", "txt": "hello"}\n\n'
                   '{"key": "b", "wav": "/x/b.wav", "txt": "wo rld", "start": 1.0, "end": 2.5}\n')
    assert cli.read_align_list(str(lst)) == [('a', '/x/a.wav', 'hello'),
                                             ('b', ('/x/b.wav', 1.0, 2.5), 'wo rld')]
    units = tmp_path / 'units.txt'
    units.write_text('<blank> 0\na 1\nb 2\n')
    assert cli.read_char_dict(str(units)) == {0: '<blank>', 1: 'a', 2: 'b'}

    # .lab / .TextGrid next to the result file
    from wenet_amd.align import AlignResult
    r = AlignResult(tokens=[1, 2], alignment=[0, 1, 1, 0, 2, 0], score=-1.0, ok=True,
                    frames=[[0, 1, 1], [0, 2, 0]])
    lab = cli.write_praat(str(tmp_path / 'res.txt'), 'utt', r, 4, {1: 'a', 2: 'b'})
    assert lab == ['0.04 0.12 a\n', '0.16 0.20 b\n']
    assert (tmp_path / 'utt.lab').read_text() == '0.04 0.12 a\n0.16 0.20 b\n'
    assert 'text = "b"' in (tmp_path / 'utt.TextGrid').read_text()


def test_transcribe_cli_align_options():
    from wenet_amd.bin import transcribe as cli
    a = cli.get_args(['x.wav', '-m', 'dir', '--align', '--label', 'some text'])
    assert a.align and a.label == 'some text'
    assert not cli.get_args(['x.wav', '-m', 'dir']).align
    with pytest.raises(SystemExit):
        cli.get_args(['x.wav', '-m', 'dir', '--align'])
    with pytest.raises(SystemExit):
        cli.get_args(['x.wav', '-m', 'dir', '--label', 'text'])


def test_tokenize_text_char_units():
    from wenet_amd.align import tokenize_text
    table = {'<blank>': 0, '<unk>': 1, 'a': 2, 'b': 3, '▁': 4}
    assert tokenize_text(' ab a?\n', table) == [2, 3, 4, 2, 1]
    assert tokenize_text('a?', {'a': 2}) == [2]


def test_force_align_is_declared_exported_and_public():
    import wenet_amd
    from wenet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    assert 'int wn_ctc_force_align(wn_model* m' in header
    assert 'wn_ctc_force_align' in _lib.EXPORTS
    assert hasattr(_lib.lib(), 'wn_ctc_force_align')
    assert callable(wenet_amd.force_align) and callable(wenet_amd.force_align_batch)
    assert wenet_amd.AlignResult(tokens=[]).ok is False
    from wenet_amd.model import ASRModel
    assert callable(ASRModel.align) and callable(ASRModel.align_wav)
    # refuses CPU tensors like the other free functions
    import torch
    with pytest.raises(RuntimeError):
        wenet_amd.force_align(torch.zeros(4, 3), torch.tensor([1]))


def test_force_align_argument_validation_without_a_device():
    """Label ids, label lengths and the blank are checked before the handle or the device is
    touched: the checks answer even with no handle at all."""
    from wenet_amd import _lib
    L = _lib.lib()
    B, Tp, V, ML = 2, 8, 10, 3
    lens = np.array([8, 6], np.int32)
    status = np.zeros(B, np.int32)
    fake_logp = ctypes.c_void_p(4096)        # never dereferenced: the checks fail first

    def call(labels, label_lens, blank=0, m=None, logp=fake_logp, lens_=lens, st=status):
        lab = np.ascontiguousarray(labels, np.int32)
        ll = np.ascontiguousarray(label_lens, np.int32)
        return L.wn_ctc_force_align(m, blank, 0.0, _lib.i32p(lab), _lib.i32p(ll), ML, logp,
                                    _lib.i32p(lens_) if lens_ is not None else None, B, Tp, V,
                                    None, None, _lib.i32p(st) if st is not None else None,
                                    None, None, None)

    ok = [[1, 2, 3], [4, 5, 0]]
    assert call([[1, 2, 10], [4, 5, 6]], [3, 3]) == -1
    assert b'outside the vocabulary' in L.wn_last_error()
    assert call([[1, -1, 3], [4, 5, 6]], [3, 3]) == -1
    assert b'outside the vocabulary' in L.wn_last_error()
    assert call(ok, [3, 4]) == -1
    assert b'label_len' in L.wn_last_error()
    assert call(ok, [3, 3]) == -1                      # the blank (0) among the labels
    assert b'blank_id among the labels' in L.wn_last_error()
    assert call(ok, [3, 2], blank=10) == -1
    assert b'blank_id outside' in L.wn_last_error()
    assert call(ok, [3, 2], lens_=np.array([9, 6], np.int32)) == -1
    assert b'length > Tp' in L.wn_last_error()
    assert call(ok, [3, 2], st=None) == -1
    assert b'null' in L.wn_last_error()
    # everything valid: only now the missing handle is noticed
    assert call(ok, [3, 2]) == -1
    assert b'null handle' in L.wn_last_error()
    # without log-probs the call needs a current batch
    assert call(ok, [3, 2], logp=None, lens_=None) == -1
    assert b'no current batch' in L.wn_last_error()
