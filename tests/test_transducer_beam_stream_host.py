"""CPU checks of the streaming transducer beam sessions' host side: the new C-ABI symbols, the
ctypes layout of wn_rnnt_beam_stream_result against the header, the refusals that need no device,
the recognizer subclass and the transcribe tool's new choice."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('wn_rnnt_beam_stream_create', 'wn_rnnt_beam_stream_destroy',
           'wn_rnnt_beam_stream_reset', 'wn_rnnt_beam_stream_advance_encoded',
           'wn_rnnt_beam_stream_state', 'wn_op_rnnt_beam_step_carry')


def _header():
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_library_exports_the_beam_stream_symbols():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    src = _header()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(r'\bint %s\(' % name, src), name
        assert getattr(L, name).restype is ctypes.c_int32
    # the one-shot hook stays
    assert hasattr(L, 'wn_op_rnnt_beam_step') and 'wn_op_rnnt_beam_step' in _lib.EXPORTS


def test_result_struct_matches_the_header():
    from wenet_amd import _lib
    body = re.search(r'typedef struct wn_rnnt_beam_stream_result \{([^{}]*?)\} '
                     r'wn_rnnt_beam_stream_result;', _header(), re.S).group(1)
    declared = [(typ.replace(' ', ''), name) for typ, name in
                re.findall(r'\b((?:int32_t|double)\s*\*?)\s*(\w+)\s*;', body)]
    fields = _lib.WnRnntBeamStreamResult._fields_
    assert [n for _, n in declared] == [n for n, _ in fields]
    assert [n for n, _ in fields] == ['n_hyps', 'hyp_lens', 'hyp_tokens', 'hyp_scores',
                                      'frames_decoded', 'trailing_blank', 'max_len']
    want = {'int32_t*': ctypes.POINTER(ctypes.c_int32), 'double*': ctypes.POINTER(ctypes.c_double),
            'int32_t': ctypes.c_int32}
    for (typ, name), (_, ctype) in zip(declared, fields):
        assert ctype is want[typ], name
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.WnRnntBeamStreamResult) == 7 * p
    assert _lib.WnRnntBeamStreamResult.max_len.offset == 6 * p


def test_null_arguments_are_refused_without_a_device():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    out = ctypes.c_void_p()
    assert L.wn_rnnt_beam_stream_create(None, 4, 5, 100, 0.3, 0.7, ctypes.byref(out), None) == -1
    assert b'wn_rnnt_beam_stream_create' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert out.value is None
    assert L.wn_rnnt_beam_stream_reset(None, 1, None, None) == -1
    assert b'wn_rnnt_beam_stream_reset' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert L.wn_rnnt_beam_stream_advance_encoded(None, 1, None, None, None, 4, None, None) == -1
    assert b'wn_rnnt_beam_stream_advance_encoded' in L.wn_last_error()
    assert b'null' in L.wn_last_error()
    assert L.wn_rnnt_beam_stream_state(None, 0, None, None, None, None, None, None, None,
                                       None) == -1
    assert b'wn_rnnt_beam_stream_state' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert L.wn_rnnt_beam_stream_destroy(None) == 0
    z = (ctypes.c_int32 * 4)()
    d = (ctypes.c_double * 4)()
    f = (ctypes.c_float * 4)()
    # the carry hook: its own null check, then the shared body's refusals under its own name
    assert L.wn_op_rnnt_beam_step_carry(1, 2, 0, 4, 0, z, 2, z, d, z, z, f, z, None, None, None,
                                        None, z, d, z, z, z, z, z, z, None, None, None) == -1
    assert b'wn_op_rnnt_beam_step_carry' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert L.wn_op_rnnt_beam_step_carry(1, 17, 0, 4, 0, z, 2, z, d, z, z, f, z, z, z, z, z, z, d,
                                        z, z, z, z, z, z, z, z, None) == -1
    assert b'wn_op_rnnt_beam_step_carry: beam must be in [1, 16]' in L.wn_last_error()


def test_recognizer_subclass_and_tool_choice():
    import inspect
    import wenet_amd
    from wenet_amd.bin import transcribe as T
    from wenet_amd.streaming import (RnntBeamStreamingRecognizer, RnntBeamStreamSearch,
                                     RnntStreamSearch, StreamingRecognizer)
    # what the existing tests pin stays true
    assert StreamingRecognizer.SEARCHES == ('ctc_prefix_beam_search', 'rnnt_greedy_search')
    with pytest.raises(SystemExit):
        T.get_args(['x.wav', '-m', 'dir', '--stream', '--search', 'rnnt_beam_search'])
    assert wenet_amd.RnntBeamStreamingRecognizer is RnntBeamStreamingRecognizer
    assert issubclass(RnntBeamStreamingRecognizer, StreamingRecognizer)
    sig = inspect.signature(RnntBeamStreamingRecognizer.__init__).parameters
    assert list(sig)[1:8] == ['model', 'n_sessions', 'decoding_chunk_size',
                              'num_decoding_left_chunks', 'beam_size', 'search_ctc_weight',
                              'search_transducer_weight']
    assert (sig['num_decoding_left_chunks'].default, sig['beam_size'].default,
            sig['search_ctc_weight'].default, sig['search_transducer_weight'].default) \
        == (-1, 5, 0.3, 0.7)
    for name in ('open', 'accept', 'step', 'finish', 'close', 'encoder_out'):
        assert callable(getattr(RnntBeamStreamingRecognizer, name))
    fin = inspect.signature(RnntBeamStreamingRecognizer.finish).parameters
    assert list(fin)[1:] == ['sid', 'rescoring', 'attn_weight', 'transducer_weight', 'ctc_weight',
                             'reverse_weight']
    assert fin['rescoring'].default is True
    sig = inspect.signature(RnntBeamStreamSearch.__init__).parameters
    assert list(sig)[1:8] == ['handle', 'device', 'n_slots', 'beam_size', 'max_frames',
                              'ctc_weight', 'transducer_weight']
    for name in ('reset', 'advance_encoded', 'state', 'close'):
        assert callable(getattr(RnntBeamStreamSearch, name))
        assert callable(getattr(RnntStreamSearch, name))       # "the same methods"
    a = T.get_args(['x.wav', '-m', 'dir', '--stream', '--search', 'rnnt_prefix_beam_search',
                    '--beam_size', '3', '--search_ctc_weight', '0.25',
                    '--search_transducer_weight', '0.75'])
    assert (a.search, a.beam_size, a.search_ctc_weight, a.search_transducer_weight) \
        == ('rnnt_prefix_beam_search', 3, 0.25, 0.75)
    a = T.get_args(['x.wav', '-m', 'dir', '--stream'])
    assert (a.search, a.beam_size, a.search_ctc_weight, a.search_transducer_weight) \
        == ('ctc_prefix_beam_search', 5, 0.3, 0.7)
    assert RnntBeamStreamingRecognizer.SEARCH == 'rnnt_prefix_beam_search'
