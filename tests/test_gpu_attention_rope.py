"""Operator tests of attention_rope_kernel (csrc/attention_rope.hip) through wn_op_attention_rope:
rotary self attention with grouped key / value heads against the plain formula of
tests/rope_refs.py  softmax(mask(rot(q) rot(k)^T * scale)) v  in fp64.

Tolerance: the project's rule, err <= kernel_refs.bound(e_plain, scale) = 8 e_plain + 16 fp32 ulps
of the output scale, e_plain = the same plain formula in fp32, with the cap asserted.  Exactness as
in test_gpu_attention_d32.py: sequences packed between rows of +-1e18, the output pre-filled with
a pattern that every element no sequence owns keeps (ldo is padded), and the same batch in reversed
packing order gives the same bits per sequence -- which also shows that a row's position counts
from its own sequence's start, not from its row offset.
"""
import pytest
import torch

import attention_d32_refs as D
import paraformer_refs as PR
import rope_refs as RR
from test_gpu_attention_d32 import PATTERN, _L, _i32, _pattern, _stream, record

pytestmark = pytest.mark.gpu

# a key tile's edge, a wave's, the 128-row block edge of G_b = 1, a dead sequence between live ones
LENS = [1, 31, 32, 0, 33, 64, 65, 128, 129, 200]
PAIRS = [(1, 1), (2, 2), (4, 2), (4, 1), (8, 1)]     # G_b 1, 1, 2, 4, and G = 8 as two blocks
_REFS = {}


def run(c, **over):
    _lib, L = _L()
    a = dict(c, ldq=c['d'] + 2 * c['w'], ldk=c['d'] + 2 * c['w'], ldo=c['d'] + 4,
             max_pos=c['tab'].shape[0], q_shift=0, kbias=0, p_off=0, blk_tab=0, flags=0)
    a.update(over)
    d, w, ldo = c['d'], c['w'], a['ldo']
    buf, tab = c['buf'].cuda(), c['tab'].cuda()
    o = _pattern(c['rows'], ldo)
    _, off, ln = PR.sorted_layout(c['offs'], c['lens'])
    b = buf.data_ptr()
    ptr = {k: (b if a[k] else None) for k in ('kbias', 'p_off', 'blk_tab')}
    _lib.check(L.wn_op_attention_rope(
        b + a['q_shift'], b + 4 * d, b + 4 * (d + w), a['ldq'], a['ldk'], a['ldk'], c['rows'],
        tab.data_ptr(), a['max_pos'], o.data_ptr(), ldo, _lib.i32p(_i32(off)), _lib.i32p(_i32(ln)),
        len(ln), a['H'], a['Hkv'], c['scale'], a['mode'], a['chunk'], a['left'], ptr['kbias'],
        ptr['p_off'], ptr['blk_tab'], a['flags'], _stream()), 'attention_rope')
    torch.cuda.synchronize()
    oc = o.cpu()
    own = torch.zeros(c['rows'], ldo, dtype=torch.bool)
    for of, n in zip(c['offs'], c['lens']):
        own[of:of + n, :d] = True
    assert bool((oc[~own] == PATTERN).all()), 'a store outside the owned elements'
    return oc.view(torch.float32)[:, :d], own[:, 0]


def check(name, **kw):
    c = RR.make_case(**kw)
    if name not in _REFS:          # one reference per case, shared and left alone
        _REFS[name] = RR.case_refs(c)
    ref, e_plain, scale = _REFS[name]
    out, own = run(c)
    assert torch.isfinite(out[own]).all(), name
    record(f'attention_rope[{name}]', (out[own].double() - ref[own]).abs().max().item(), e_plain,
           scale)
    n = len(c['lens'])
    r = RR.make_case(order=list(range(n))[::-1], **kw)
    out_r, _ = run(r)
    for i, t in enumerate(c['lens']):
        o0, o1 = c['offs'][i], r['offs'][i]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: sequence {i} depends on where it is packed'


@pytest.mark.parametrize('H,Hkv', PAIRS)
def test_head_pairs(H, Hkv):
    check(f'full_{H}_{Hkv}', H=H, Hkv=Hkv, lens=LENS, seed=40 + H + Hkv)


@pytest.mark.parametrize('regime', D.REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_regimes(regime):
    """4 query heads on 2 K / V heads, 65 rows, full context."""
    check(f'regime_{regime}', H=4, Hkv=2, lens=[65], regime=regime[0], param=regime[1], seed=34)


@pytest.mark.parametrize('Hkv', [2, 1])
@pytest.mark.parametrize('chunk,left,lens', [(4, -1, [7, 33, 65]), (3, 0, [7, 33, 65]),
                                             (16, 1, [97, 130]), (16, 0, [33])])
def test_chunk_windows(chunk, left, lens, Hkv):
    """The windows of tests/test_gpu_attention_d32_relpos.py: a chunk that does not divide the
    tile, blocks that start past key tile 0, a last block of one row."""
    check(f'chunk_{chunk}_{left}_{Hkv}', H=4, Hkv=Hkv, lens=lens, seed=80 + chunk, mode=2,
          chunk=chunk, left=left)


REFUSALS = [('mask_mode must be 0 .* or 2 .*not 1 \\(causal\\)', dict(mode=1)),
            ('chunk_size must be positive under mask_mode 2', dict(mode=2, chunk=0)),
            ('no kbias', dict(kbias=1)), ('no p_off', dict(p_off=1)),
            ('no block list', dict(blk_tab=1)),
            ('fp32 only, no bf16 flags', dict(flags=1)), ('fp32 only, no bf16 flags', dict(flags=2)),
            ('n_heads % n_kv_heads != 0', dict(Hkv=3)),
            ('the Q / O stride is smaller than n_heads \\* 64', dict(ldq=252)),
            ('the Q / O stride is smaller than n_heads \\* 64', dict(ldo=252)),
            ('the K / V stride is smaller than n_kv_heads \\* 64', dict(ldk=124)),
            ('strides % 4', dict(ldq=514)),
            ('16-byte aligned', dict(q_shift=4)),
            ('a sequence is longer than the table', dict(max_pos=4))]


@pytest.mark.parametrize('match,over', REFUSALS, ids=[str(o) for _, o in REFUSALS])
def test_refusals(match, over):
    c = RR.make_case(4, 2, [5], seed=1)
    with pytest.raises(RuntimeError, match='attention_rope: .*' + match):
        run(c, **over)
