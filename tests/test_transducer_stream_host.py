"""CPU checks of the streaming transducer sessions' host side: the new C-ABI symbols, the ctypes
layout of wn_rnnt_stream_result against the header, the refusals that need no device, the
recognizer's and the transcribe tool's new options."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('wn_rnnt_stream_create', 'wn_rnnt_stream_destroy', 'wn_rnnt_stream_reset',
           'wn_rnnt_stream_advance_encoded', 'wn_rnnt_stream_state')


def _header():
    src = open(os.path.join(ROOT, 'include', 'wenet_amd.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_library_exports_the_stream_symbols():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    src = _header()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(r'\bint %s\(' % name, src), name
        assert getattr(L, name).restype is ctypes.c_int32


def test_result_struct_matches_the_header():
    from wenet_amd import _lib
    body = re.search(r'typedef struct wn_rnnt_stream_result \{([^{}]*?)\} wn_rnnt_stream_result;',
                     _header(), re.S).group(1)
    declared = [(typ.replace(' ', ''), name) for typ, name in
                re.findall(r'\b(int32_t\s*\*?)\s*(\w+)\s*;', body)]
    fields = _lib.WnRnntStreamResult._fields_
    assert [n for _, n in declared] == [n for n, _ in fields]
    assert [n for n, _ in fields] == ['tok_lens', 'tokens', 'times', 'frames_decoded',
                                      'trailing_blank', 'max_len', 'steps']
    for (typ, name), (_, ctype) in zip(declared, fields):
        want = ctypes.POINTER(ctypes.c_int32) if typ.endswith('*') else ctypes.c_int32
        assert ctype is want, name
    # five pointers, an int32 padded to pointer alignment, one pointer
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.WnRnntStreamResult) == 7 * p
    assert _lib.WnRnntStreamResult.max_len.offset == 5 * p
    assert _lib.WnRnntStreamResult.steps.offset == 6 * p


def test_null_arguments_are_refused_without_a_device():
    from wenet_amd import _lib, build
    build.build(force=False, verbose=False)
    L = _lib.lib()
    out = ctypes.c_void_p()
    assert L.wn_rnnt_stream_create(None, 4, 100, 100, 64, ctypes.byref(out), None) == -1
    assert b'wn_rnnt_stream_create' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert out.value is None
    assert L.wn_rnnt_stream_reset(None, 1, None, None) == -1
    assert b'wn_rnnt_stream_reset' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert L.wn_rnnt_stream_advance_encoded(None, 1, None, None, None, 4, None, None) == -1
    assert b'wn_rnnt_stream_advance_encoded' in L.wn_last_error()
    assert b'null' in L.wn_last_error()
    assert L.wn_rnnt_stream_state(None, 0, None, None, None, None, None) == -1
    assert b'wn_rnnt_stream_state' in L.wn_last_error() and b'null' in L.wn_last_error()
    assert L.wn_rnnt_stream_destroy(None) == 0


def test_recognizer_and_tool_options():
    import inspect
    from wenet_amd.bin import transcribe as T
    from wenet_amd.streaming import RnntStreamSearch, StreamingRecognizer
    sig = inspect.signature(StreamingRecognizer.__init__).parameters
    assert sig['search'].default == 'ctc_prefix_beam_search' and sig['n_steps'].default == 64
    assert StreamingRecognizer.SEARCHES == ('ctc_prefix_beam_search', 'rnnt_greedy_search')
    sig = inspect.signature(RnntStreamSearch.__init__).parameters
    assert list(sig)[1:7] == ['handle', 'device', 'n_slots', 'max_frames', 'max_tokens', 'n_steps']
    assert sig['n_steps'].default == 64
    for name in ('reset', 'advance_encoded', 'state', 'close'):
        assert callable(getattr(RnntStreamSearch, name))
    a = T.get_args(['x.wav', '-m', 'dir', '--stream'])
    assert a.search == 'ctc_prefix_beam_search'
    a = T.get_args(['x.wav', '-m', 'dir', '--stream', '--search', 'rnnt_greedy_search'])
    assert a.search == 'rnnt_greedy_search'
    with pytest.raises(SystemExit):
        T.get_args(['x.wav', '-m', 'dir', '--stream', '--search', 'rnnt_beam_search'])
