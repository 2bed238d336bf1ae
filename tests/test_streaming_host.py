"""Host side of the streaming recognizer (wenet_amd/streaming.py), no GPU: the feature
windows of a session whose frames arrive in pieces, the endpoint rules, the wn_stream_* C ABI
surface and its argument checks, the --stream options of the transcribe tool."""
import ctypes
import os
import random
import re

import pytest

from wenet_amd.streaming import (ChunkWindower, CtcEndpointConfig, CtcEndpointRule,
                                 endpoint_rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_EXPORTS = ('wn_stream_create', 'wn_stream_destroy', 'wn_stream_set_endpoint',
                  'wn_stream_reset', 'wn_stream_advance', 'wn_stream_advance_encoded')


def _reference_windows(n, chunk, subsampling, right_context):
    """BaseEncoder.forward_chunk_by_chunk's loop (encoder.py:337-352)."""
    context = right_context + 1
    stride = subsampling * chunk
    window = (chunk - 1) * subsampling + context
    return [(cur, min(cur + window, n)) for cur in range(0, n - context + 1, stride)]


@pytest.mark.parametrize('chunk', [1, 3, 4, 16])
def test_windows_equal_forward_chunk_by_chunk_however_the_frames_arrive(chunk):
    sub, rc = 4, 6
    context, stride = rc + 1, sub * chunk
    lengths = [0, 1, context - 1, context, context + 1, stride, stride + context - 1]
    lengths += [5 * stride + context + r for r in range(stride)]     # every remainder
    lengths += [7 * stride + r for r in (0, 1, stride - 1)]
    rng = random.Random(1000 + chunk)
    for n in lengths:
        for trial in range(4):
            w = ChunkWindower(chunk, sub, rc)
            got, fed = [], 0
            while fed < n:
                k = rng.choice([0, 1, 2, 5, stride - 1, stride, stride + 3, 3 * stride])
                k = min(k, n - fed)
                w.push(k)
                fed += k
                # steps are taken at arbitrary moments: sometimes several, sometimes none
                for _ in range(rng.choice([0, 1, 1, 4])):
                    if w.ready():
                        got.append(w.pop())
                        assert got[-1][1] <= fed and w.keep_from() <= got[-1][1]
            got += w.flush()
            assert got == _reference_windows(n, chunk, sub, rc), (chunk, n, trial)
            assert not w.ready()


def test_full_windows_have_one_length_and_the_tail_is_at_least_the_context():
    w = ChunkWindower(16, 4, 6)
    assert (w.stride, w.window, w.context) == (64, 67, 7)
    w.push(66)
    assert not w.ready()
    w.push(1)
    assert w.pop() == (0, 67) and not w.ready()
    w.push(10)                     # 77 frames: 13 past the second window's start
    assert w.flush() == [(64, 77)]
    w = ChunkWindower(16, 4, 6)
    w.push(64 + 6)                 # one frame short of a second window's context
    assert w.flush() == [(0, 67)]


def test_endpoint_rules_known_answers():
    c = CtcEndpointConfig()
    assert (c.blank, c.blank_threshold, c.blank_scale) == (0, 0.8, 1.0)
    assert (c.rule1.must_decoded_sth, c.rule1.min_trailing_silence,
            c.rule1.min_utterance_length) == (False, 5000, 0)
    assert (c.rule2.must_decoded_sth, c.rule2.min_trailing_silence,
            c.rule2.min_utterance_length) == (True, 1000, 0)
    assert (c.rule3.must_decoded_sth, c.rule3.min_trailing_silence,
            c.rule3.min_utterance_length) == (False, 0, 20000)
    ms = 40   # 10 ms x subsampling 4
    assert endpoint_rule(c, 124, 124, False, ms) is None        # 4960 ms of silence
    assert endpoint_rule(c, 125, 125, False, ms) == 'rule1'     # 5000 ms
    assert endpoint_rule(c, 100, 25, True, ms) == 'rule2'       # 1000 ms after a result
    assert endpoint_rule(c, 100, 24, True, ms) is None
    assert endpoint_rule(c, 100, 25, False, ms) is None         # nothing decoded: rule1 only
    assert endpoint_rule(c, 499, 0, True, ms) is None
    assert endpoint_rule(c, 500, 0, False, ms) == 'rule3'       # 20000 ms long
    assert endpoint_rule(c, 500, 0, True, ms) == 'rule3'
    assert endpoint_rule(c, 600, 130, True, ms) == 'rule1'      # the first rule that fires
    # a custom rule set: rule2 off, rule3 at 2 s
    c2 = CtcEndpointConfig(rule2=CtcEndpointRule(True, 10 ** 9, 0),
                           rule3=CtcEndpointRule(False, 0, 2000))
    assert endpoint_rule(c2, 49, 30, True, ms) is None
    assert endpoint_rule(c2, 50, 30, True, ms) == 'rule3'


def test_stream_exports_in_header_binding_and_library():
    from wenet_amd import _lib, build
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(wn_[a-z0-9_]+)\s*\(', src))
    build.build(force=False, verbose=False)
    L = _lib.lib()
    for name in STREAM_EXPORTS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    for field in ('n_hyps', 'hyp_lens', 'hyp_tlens', 'hyp_tokens', 'hyp_times', 'hyp_scores',
                  'hyp_viterbi', 'frames_decoded', 'trailing_blank', 'max_len'):
        assert re.search(r'\b%s;' % field, src), field
        assert field in [f[0] for f in _lib.WnStreamResult._fields_]


def test_stream_null_arguments_are_rejected_without_a_device():
    from wenet_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    one = (ctypes.c_int32 * 1)(0)
    res = _lib.WnStreamResult()
    fake = ctypes.c_void_p(16)    # never dereferenced: the null checks come first
    calls = [
        ('wn_stream_create', lambda: L.wn_stream_create(None, 1, 4, 10, 0, ctypes.byref(h), None)),
        ('wn_stream_create', lambda: L.wn_stream_create(fake, 1, 4, 10, 0, None, None)),
        ('wn_stream_set_endpoint', lambda: L.wn_stream_set_endpoint(None, 0.8, 1.0)),
        ('wn_stream_reset', lambda: L.wn_stream_reset(None, 1, one, None)),
        ('wn_stream_advance', lambda: L.wn_stream_advance(None, 1, one, fake, one, 1, 8, 0,
                                                         ctypes.byref(res), None)),
        ('wn_stream_advance', lambda: L.wn_stream_advance(fake, 1, one, None, one, 1, 8, 0,
                                                         ctypes.byref(res), None)),
        ('wn_stream_advance', lambda: L.wn_stream_advance(fake, 1, one, fake, one, 1, 8, 0,
                                                         None, None)),
        ('wn_stream_advance_encoded',
         lambda: L.wn_stream_advance_encoded(None, 1, one, fake, one, 16, 0, ctypes.byref(res),
                                             None)),
        ('wn_stream_advance_encoded',
         lambda: L.wn_stream_advance_encoded(fake, 1, one, None, one, 16, 0, ctypes.byref(res),
                                             None)),
    ]
    for name, call in calls:
        assert call() == -1, name
        msg = L.wn_last_error()
        assert b'null' in msg and name.encode() in msg, (name, msg)
    assert L.wn_stream_destroy(None) == 0


def test_transcribe_stream_options():
    from wenet_amd.bin import transcribe as T
    a = T.get_args(['a.wav', '-m', 'dir'])
    assert a.stream is False and a.chunk == 16 and a.beam is None
    assert a.context_path is None and a.context_score == 6.0 and not a.show_tokens_info
    a = T.get_args(['a.wav', '-m', 'dir', '--stream', '--chunk', '16'])
    assert a.stream is True and a.chunk == 16
    assert T.get_args(['a.wav', '-m', 'dir', '--stream', '--chunk', '8', '--beam', '4']).chunk == 8
