"""Operator tests of csrc/attention_shaw.hip through wn_op_attention_shaw and
wn_op_stack_frames_ln, against the plain formulas of tests/shaw_refs.py in fp64.

Tolerance: the project's rule for every fp32 attention kernel, err <= kernel_refs.bound(e_plain,
scale) = 8 e_plain + 16 fp32 ulps of the output scale, e_plain = the same plain formula in fp32,
with the cap asserted.  One packed batch holds the smallest lengths that reach each branch of the
kernel: 1; 8 / 9 / 10 (the right clamp starts at j - i = 8); 32 / 33 (the tile edge); 64 / 65 / 66
(the left clamp is first reached at 65); 97 (a tile wholly right of a wave's band); 129 and 200
(tiles wholly left of it); and a sequence of length 0 between two live ones.  Sequences lie
between rows of +-1e18, the output is pre-filled with a pattern that every element no sequence
owns must keep (ldo is padded), and the same batch in reversed packing order gives the same bits.

The `coded` regime makes the table say which row was read (shaw_refs.coded_table);
tests/test_shaw_host.py shows on the CPU that each of the four wrong readings --
off by one, wrap instead of clamp, a zero row instead of the clamp row, head h reading row
73 h + c -- leaves the bound on it.
"""
import re

import pytest
import torch

import attention_d32_refs as D
import kernel_refs as KR
import paraformer_refs as PR
import shaw_refs as SR
from test_gpu_attention_d32 import PATTERN, _L, _i32, _pattern, _stream, record

pytestmark = pytest.mark.gpu

LENS = SR.LENS
REGIMES = D.REGIMES + [('coded', None)]
_REFS = {}


def run(c, q_shift=0, **over):
    """The hook on case c; `over` replaces arguments (the refusals)."""
    _lib, L = _L()
    d = c['d']
    a = dict(ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d + 4, mask_mode=0, kbias=None, p_off=None,
             blk_tab=None, bf16=0)
    a.update(over)
    buf, table = c['buf'].cuda(), c['table'].cuda()
    o = _pattern(c['rows'], d + 4)
    _, off, ln = PR.sorted_layout(c['offs'], c['lens'])
    off, ln = _i32(off), _i32(ln)
    b = buf.data_ptr()
    ptr = {k: (buf.data_ptr() if a[k] else None) for k in ('kbias', 'p_off', 'blk_tab')}
    _lib.check(L.wn_op_attention_shaw(
        b + q_shift, b + 4 * d, b + 8 * d, a['ldq'], a['ldk'], a['ldv'], c['rows'],
        table.data_ptr(), o.data_ptr(), a['ldo'], _lib.i32p(off), _lib.i32p(ln), len(ln), c['H'],
        SR.SCALE, a['mask_mode'], ptr['kbias'], ptr['p_off'], ptr['blk_tab'], a['bf16'],
        _stream()), 'attention_shaw')
    torch.cuda.synchronize()
    oc = o.cpu()
    own = torch.zeros(c['rows'], d + 4, dtype=torch.bool)
    for of, n in zip(c['offs'], c['lens']):
        own[of:of + n, :d] = True
    assert bool((oc[~own] == PATTERN).all()), 'a store outside the owned elements'
    return oc.view(torch.float32)[:, :d], own[:, 0]


@pytest.mark.parametrize('H', [1, 2])
@pytest.mark.parametrize('regime,param', REGIMES)
def test_attention_shaw(regime, param, H):
    name = f'{regime}_{param}_h{H}'
    c = SR.make_case(H, regime, param)
    if name not in _REFS:          # one reference per case, shared and left alone
        _REFS[name] = SR.case_refs(c)
    ref, e_plain, scale = _REFS[name]
    out, own = run(c)
    assert torch.isfinite(out[own]).all(), name
    record(f'attention_shaw[{name}]', (out[own].double() - ref[own]).abs().max().item(), e_plain,
           scale)
    r = SR.make_case(H, regime, param, order=list(range(len(LENS)))[::-1])
    out_r, _ = run(r)
    for i, t in enumerate(c['lens']):
        o0, o1 = c['offs'][i], r['offs'][i]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: sequence {i} depends on where it is packed'


REFUSALS = [
    (dict(mask_mode=1), 'mask_mode must be 0'),
    (dict(mask_mode=2), 'mask_mode must be 0'),
    (dict(kbias=True), 'no kbias'),
    (dict(p_off=True), 'no p_off'),
    (dict(blk_tab=True), 'no block list'),
    (dict(bf16=1), 'no bf16 flags'),
    (dict(bf16=2), 'no bf16 flags'),
    (dict(ldq=3 * 128 + 2), 'strides % 4'),
    (dict(ldo=124), 'a stride is smaller than n_heads * 64'),
    (dict(q_shift=4), '16-byte aligned'),
]


@pytest.mark.parametrize('over,message', REFUSALS, ids=[m for _, m in REFUSALS])
def test_attention_shaw_refusals(over, message):
    c = SR.make_case(2, 'unit', None, lens=[9])
    with pytest.raises(RuntimeError, match=re.escape(message)):
        run(c, **over)


# ---------------------------------------------------------------------------------------------
# stack_frames_ln

FRAME_LENS = [0, 1, 2, 3, 7, 8]
T_PAD, F_DIM = 9, 80


@pytest.mark.parametrize('cmvn', [False, True])
def test_stack_frames_ln(cmvn):
    """Lengths 0 .. 8 at padded T = 9: odd lengths drop their last frame, 0 and 1 give no row; the
    frames behind an utterance's end hold +-1e18 and must not be read."""
    _lib, L = _L()
    g = torch.Generator().manual_seed(17)
    B, n = len(FRAME_LENS), 2 * F_DIM
    feats = torch.full((B, T_PAD, F_DIM), KR.POISON)
    for b, t in enumerate(FRAME_LENS):
        feats[b, :t] = torch.randn(t, F_DIM, generator=g) * 3.0 + 1.0
    mean = torch.randn(F_DIM, generator=g) if cmvn else None
    istd = (torch.rand(F_DIM, generator=g) + 0.5) if cmvn else None
    w, bb = torch.randn(n, generator=g), torch.randn(n, generator=g)
    refs = SR.ref_stack_frames_ln(feats, FRAME_LENS, mean, istd, w, bb)
    plain = SR.ref_stack_frames_ln(feats, FRAME_LENS, mean, istd, w, bb, fp32=True)
    lens_out = [t // 2 for t in FRAME_LENS]
    offs, at = [], 1                                   # one guard row in front, two between
    for t in lens_out:
        offs.append(at)
        at += t + 2
    o = _pattern(at, n + 4)
    got_len = _i32([0] * B)
    dev = [t.cuda() if t is not None else None for t in (feats, mean, istd, w, bb)]
    _lib.check(L.wn_op_stack_frames_ln(
        dev[0].data_ptr(), dev[1].data_ptr() if cmvn else None,
        dev[2].data_ptr() if cmvn else None, dev[3].data_ptr(), dev[4].data_ptr(), o.data_ptr(),
        n + 4, at, _lib.i32p(_i32(FRAME_LENS)), _lib.i32p(_i32(offs)), _lib.i32p(got_len), B,
        T_PAD, F_DIM, _stream()), 'stack_frames_ln')
    torch.cuda.synchronize()
    assert got_len.tolist() == lens_out
    oc = o.cpu()
    own = torch.zeros(at, n + 4, dtype=torch.bool)
    for of, t in zip(offs, lens_out):
        own[of:of + t, :n] = True
    assert bool((oc[~own] == PATTERN).all()), 'a store outside the owned rows'
    out = oc.view(torch.float32)
    for b, t in enumerate(lens_out):
        if t:
            e_plain = (plain[b] - refs[b]).abs().max().item()
            err = (out[offs[b]:offs[b] + t, :n].double() - refs[b]).abs().max().item()
            record(f'stack_frames_ln[cmvn={cmvn}, len={FRAME_LENS[b]}]', err, e_plain,
                   refs[b].abs().max().item())
