"""Operator tests of csrc/utt_norm.hip through wn_op_utt_stats, wn_utt_normalize (on a workspace
handle) and wn_op_stack_frames_ln_utt, against the reference's two torch calls in fp64
(tests/utt_norm_refs.py).

Tolerance: the project's rule, err <= kernel_refs.bound(e_plain, scale) = 8 e_plain + 16 fp32 ulps
of the output's scale, e_plain = the same two calls in fp32 on the CPU, with the cap asserted.  One
padded batch holds the lengths of utt_norm_refs.LENS; frames behind an utterance's end hold +-1e18,
the statistics and the stacked rows are pre-filled with a pattern that every element no utterance
owns must keep, and the batch in reversed order gives the same bits per utterance."""
import ctypes
import re

import pytest
import torch

import utt_norm_refs as UR
from test_gpu_attention_d32 import PATTERN, _L, _i32, _pattern, _stream, record

pytestmark = pytest.mark.gpu

LENS, T = UR.LENS, UR.T_PAD
_REFS = {}


@pytest.fixture(scope='module')
def ws():
    _lib, L = _L()
    h = ctypes.c_void_p()
    _lib.check(L.wn_workspace_create(0, ctypes.byref(h)), 'workspace')
    yield h
    L.wn_model_destroy(h)


def run(ws, feats, lens, w, b, F=None, T_arg=T, shift=0):
    """stats hook -> (mean, std); wn_utt_normalize -> out; form (b) fed the hook's statistics ->
    rows.  F / T_arg / shift replace arguments (the refusals)."""
    _lib, L = _L()
    B, F = len(lens), F or feats.shape[-1]
    x, wd, bd = feats.cuda(), w.cuda(), b.cuda()
    mean, std = _pattern(B, feats.shape[-1]), _pattern(B, feats.shape[-1])
    ln = _lib.i32p(_i32(lens))
    _lib.check(L.wn_op_utt_stats(x.data_ptr(), ln, B, T_arg, F, mean.data_ptr(), std.data_ptr(),
                                 _stream()), 'utt_stats')
    out = _pattern(B * T, feats.shape[-1])
    _lib.check(L.wn_utt_normalize(ws, x.data_ptr() + shift, ln, B, T_arg, F, out.data_ptr(),
                                  _stream()), 'utt_normalize')
    offs, at = [], 1                                   # one guard row in front, two between
    for n in lens:
        offs.append(at)
        at += n // 2 + 2
    rows, got_len = _pattern(at, 2 * F + 4), _i32([0] * B)
    _lib.check(L.wn_op_stack_frames_ln_utt(
        x.data_ptr(), mean.data_ptr(), std.data_ptr(), None, None, wd.data_ptr(),
        bd.data_ptr(), rows.data_ptr(), 2 * F + 4, at, ln, _lib.i32p(_i32(offs)),
        _lib.i32p(got_len), B, T_arg, F, _stream()), 'stack_frames_ln_utt')
    torch.cuda.synchronize()
    assert got_len.tolist() == [n // 2 for n in lens]
    own = torch.zeros(at, 2 * F + 4, dtype=torch.bool)
    for of, n in zip(offs, lens):
        own[of:of + n // 2, :2 * F] = True
    rows = rows.cpu()
    assert bool((rows[~own] == PATTERN).all()), 'a store outside the owned rows'
    return (mean.cpu(), std.cpu(), out.cpu().view(B, T, -1),
            [rows[of:of + n // 2, :2 * F] for of, n in zip(offs, lens)])


@pytest.mark.parametrize('regime,F', [(r, 80) for r in UR.REGIMES] + [('fbank', 128)])
def test_utt_norm(ws, regime, F):
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(2 * F, generator=g), torch.randn(2 * F, generator=g)
    if (regime, F) not in _REFS:          # one reference per case, shared and left alone
        refs = []
        for i, n in enumerate(LENS):
            x = UR.utterance(regime, F, i, n)
            r64, r32 = (UR.normalize(x, fp32) if n >= 2 else None for fp32 in (False, True))
            refs.append(r64 and dict(r64=r64 + (UR.stack_ln(r64[2], w, b), ),
                                     r32=r32 + (UR.stack_ln(r32[2], w, b), )))
        _REFS[regime, F] = refs
    refs = _REFS[regime, F]
    feats, lens = UR.make_batch(regime, F)
    mean, std, out, rows = run(ws, feats, lens, w, b)
    f32 = torch.float32
    for i, n in enumerate(LENS):
        assert bool((out[i, n:] == 0).all()), 'padded frames of utt_normalize must be exactly 0'
        if n < 2:
            assert bool((mean[i] == PATTERN).all() and (std[i] == PATTERN).all()), \
                'statistics rows of an utterance of fewer than 2 frames must stay untouched'
            assert bool(out[i, :n].view(f32).isnan().all())      # the reference's std of one frame
            continue
        got = (mean[i].view(f32), std[i].view(f32), out[i, :n].view(f32), rows[i].view(f32))
        for what, y, r64, r32 in zip(('mean', 'std', 'normalize', 'stack_frames_ln_utt'), got,
                                     refs[i]['r64'], refs[i]['r32']):
            record(f'{what}[{regime}, F={F}, len={n}]', (y.double() - r64).abs().max().item(),
                   (r32.double() - r64).abs().max().item(), r64.abs().max().item())
    order = list(range(len(LENS)))[::-1]
    feats_r, lens_r = UR.make_batch(regime, F, order)
    rev = run(ws, feats_r, lens_r, w, b)
    for i, n in enumerate(LENS):
        j = order.index(i)
        for a, c in ((mean[i], rev[0][j]), (std[i], rev[1][j]), (out[i], rev[2][j]),
                     (rows[i], rev[3][j])):
            assert torch.equal(a, c), f'utterance {i} depends on its place in the batch'


REFUSALS = [
    (dict(F=132), 'F > 128'),
    (dict(F=78), 'F % 4 != 0'),
    (dict(shift=4), '16-byte aligned'),
    (dict(T_arg=LENS[-1] - 1), 'len > T'),
]


@pytest.mark.parametrize('over,message', REFUSALS, ids=[m for _, m in REFUSALS])
def test_refusals(ws, over, message):
    feats = torch.zeros(len(LENS), T, 132)
    w = torch.ones(2 * 132)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        run(ws, feats, LENS, w, w, **{'F': 80, **over})
