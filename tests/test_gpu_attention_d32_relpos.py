"""Operator tests of attention_d32_relpos_kernel (csrc/attention_d32_relpos.hip) through
wn_op_attention_d32_relpos: the rel-pos, chunk-masked attention of encoder heads of 32 against
the plain formula  softmax(mask(((q + u) k^T + (q + v) p^T) * scale)) v  in fp64.

Tolerance: the project's rule, err <= kernel_refs.bound(e_plain, scale) = 8 e_plain + 16 fp32 ulps
of the output scale, e_plain = the same plain formula in fp32, with the cap asserted.  Exactness as
in test_gpu_attention_d32.py: sequences packed between rows of +-1e18, the output pre-filled with
a pattern that every element no sequence owns keeps (ldo is padded), and the same batch in reversed
packing order gives the same bits per sequence.  u, v and P are drawn in the regime of q and k:
P = the key rows and u, v = two query rows of a second draw of attention_d32_refs.raw_rows.
"""
import numpy as np
import pytest
import torch

import attention_d32_refs as D
import kernel_refs as KR
import paraformer_refs as PR
from test_gpu_attention_d32 import PATTERN, _L, _i32, _pattern, _stream, record

pytestmark = pytest.mark.gpu

FULL_LENS = [1, 31, 32, 33, 64, 65, 129]
_REFS = {}


def make_case(H, lens, regime='unit', param=None, seed=0, order=None, mode=0, chunk=0, left=-1):
    """Q | K | V of every sequence as the three column blocks of one packed buffer (ld = 3 d); P
    with three rows more than the longest sequence and ldp = d + 4."""
    d, n_p = H * 32, max(lens) + 3
    qs, ks, vs = D.raw_rows(regime, param, H, lens, lens, lens, seed)
    q2, k2, _ = D.raw_rows(regime, param, H, [2], [n_p], [n_p], seed + 500)
    buf, offs, total = PR.pack_rows([torch.cat(r, 1) for r in zip(qs, ks, vs)], order, gap=3,
                                    lead=2)
    pos = torch.full((n_p, d + 4), KR.POISON)
    pos[:, :d] = k2[0]
    return dict(H=H, d=d, lens=list(lens), buf=buf, offs=offs, rows=total, pos=pos,
                u=q2[0][0].clone(), v=q2[0][1].clone(), mode=mode, chunk=chunk, left=left,
                scale=D.SCALE)


def reference(c, dt):
    """The plain formula in dtype dt; (rows, d) fp64, zero in rows no sequence owns."""
    H, d = c['H'], c['d']
    out = torch.zeros(c['rows'], d, dtype=torch.float64)
    u, v = c['u'].to(dt).view(H, 1, 32), c['v'].to(dt).view(H, 1, 32)
    for o, n in zip(c['offs'], c['lens']):
        q, k, val = (c['buf'][o:o + n, i * d:(i + 1) * d].to(dt).view(n, H, 32).transpose(0, 1)
                     for i in range(3))
        p = c['pos'][:n, :d].to(dt).view(n, H, 32).transpose(0, 1)
        s = (torch.matmul(q + u, k.transpose(1, 2)) + torch.matmul(q + v, p.transpose(1, 2)))
        hidden = ~KR.chunk_window(n, n, c['mode'], c['chunk'], c['left'])
        w = torch.softmax((s * c['scale']).masked_fill(hidden, -float('inf')), dim=-1)
        out[o:o + n] = torch.matmul(w, val).transpose(0, 1).reshape(n, d).double()
    return out


def case_refs(c):
    ref = reference(c, torch.float64)
    vmax = max(c['buf'][o:o + n, 2 * c['d']:].abs().max().item()
               for o, n in zip(c['offs'], c['lens']))
    return ref, (reference(c, torch.float32) - ref).abs().max().item(), vmax


def run(c, **over):
    _lib, L = _L()
    a = dict(c, **over)
    d, ldo = c['d'], c['d'] + 4
    buf, pos, u, v = (c[k].cuda() for k in ('buf', 'pos', 'u', 'v'))
    o = _pattern(c['rows'], ldo)
    _, off, ln = PR.sorted_layout(c['offs'], c['lens'])
    off, ln = _i32(off), _i32(ln)
    kl = _i32(a.get('kv_lens', ln))
    b = buf.data_ptr()
    _lib.check(L.wn_op_attention_d32_relpos(
        b, b + 4 * d, b + 8 * d, 3 * d, 3 * d, 3 * d, c['rows'], c['rows'], o.data_ptr(), ldo,
        _lib.i32p(off), _lib.i32p(ln), _lib.i32p(off), _lib.i32p(kl), len(ln), c['H'],
        c['scale'], a['mode'], pos.data_ptr(), d + 4, a.get('p_rows', pos.shape[0]),
        u.data_ptr(), v.data_ptr(), a['chunk'], a['left'], _stream()), 'attention_d32_relpos')
    torch.cuda.synchronize()
    oc = o.cpu()
    own = torch.zeros(c['rows'], ldo, dtype=torch.bool)
    for of, n in zip(c['offs'], c['lens']):
        own[of:of + n, :d] = True
    assert bool((oc[~own] == PATTERN).all()), 'a store outside the owned elements'
    return oc.view(torch.float32)[:, :d], own[:, 0]


def check(name, **kw):
    c = make_case(**kw)
    if name not in _REFS:          # one reference per case, shared and left alone
        _REFS[name] = case_refs(c)
    ref, e_plain, scale = _REFS[name]
    out, own = run(c)
    assert torch.isfinite(out[own]).all(), name
    record(f'attention_d32_relpos[{name}]', (out[own].double() - ref[own]).abs().max().item(),
           e_plain, scale)
    n = len(c['lens'])
    r = make_case(order=list(range(n))[::-1], **kw)
    out_r, _ = run(r)
    for i, t in enumerate(c['lens']):
        o0, o1 = c['offs'][i], r['offs'][i]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: sequence {i} depends on where it is packed'


@pytest.mark.parametrize('H', [1, 8])
def test_full_context(H):
    """1 .. 129 rows in one batch: both sides of a key tile, of a block of 64 and of 128 rows, a
    dead wave (129 = one live wave of four in the second block)."""
    check(f'full_h{H}', H=H, lens=FULL_LENS, seed=70 + H)


@pytest.mark.parametrize('chunk,left,lens', [(4, -1, [7, 33, 65]), (3, 0, [7, 33, 65]),
                                             (16, 1, [97, 130]), (16, 0, [33])])
def test_chunk_windows(chunk, left, lens):
    """(3, 0): a chunk that does not divide the tile; (16, 1) at 97 and 130 rows: blocks that start
    past key tile 0; (16, 0) at 33: a last block of one row."""
    check(f'chunk_{chunk}_{left}', H=2, lens=lens, seed=80 + chunk, mode=2, chunk=chunk, left=left)


@pytest.mark.parametrize('regime', D.REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_regimes(regime):
    """4 heads, 65 rows, full context; u, v and P in the regime of q and k."""
    check(f'regime_{regime}', H=4, lens=[65], regime=regime[0], param=regime[1], seed=33)


@pytest.mark.parametrize('side', [-1, 0])
@pytest.mark.parametrize('mode', [0, 2])
def test_both_block_shapes(side, mode):
    """The longest sequence one row short of the launcher's threshold (blocks of 2 waves) and at it
    (4 waves), full context and (16, 1)."""
    thr = _L()[1].wn_attention_d32_relpos_nw4_len()
    check(f'nw_{side}_{mode}', H=2, lens=[thr + side, 40], seed=90, mode=mode, chunk=16, left=1)


def test_refusals():
    c = make_case(2, [5], seed=1)
    for match, over in [('mask_mode must be 0 .* or 2 .*not 1 \\(causal\\)', dict(mode=1)),
                        ('chunk_size must be positive under mask_mode 2', dict(mode=2, chunk=0)),
                        ('p_rows is smaller than the longest sequence', dict(p_rows=4)),
                        ('self attention only, q_len != kv_len', dict(kv_lens=[4]))]:
        with pytest.raises(RuntimeError, match='attention_d32_relpos: ' + match):
            run(c, **over)
