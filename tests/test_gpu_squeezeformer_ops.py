"""Operator tests of the Squeezeformer kernels (csrc/squeezeformer.hip) through the hooks
wn_op_attention_sqshift / wn_op_time_reduce / wn_op_time_recover, against the plain fp64
references of tests/squeezeformer_refs.py (pinned to the reference's modules on the CPU,
tests/test_squeezeformer_host.py, where the yardsticks' caps and the sensitivity of the sign cases
are checked too).

Tolerance, the rule of tests/test_gpu_kernels.py: err <= 8 * e_plain + 16 fp32 ulps of the output
scale (kernel_refs.bound), e_plain = the error of the plain fp32 evaluation of the same formula on
the same inputs.  time_recover_add is one add per element: bit-exact against the fp32 statement.
Sequences are packed between rows of +-1e18; output buffers start as a bit pattern that every
element no sequence owns must still hold.
"""
import numpy as np
import pytest
import torch

import kernel_refs as KR
import squeezeformer_refs as SQ

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def record(name, err, e_plain, scale):
    b = KR.bound(e_plain, scale)
    line = (f'{name} err={err:.3e} e_plain={e_plain:.3e} scale={scale:.3e} '
            f'ratio={err / b if b > 0 else 0.0:.3f}')
    print(line)
    assert KR.cap_ok(e_plain, scale), line
    assert err <= b, line


def _owned(rows, seqs, ld, C):
    own = torch.zeros(rows, ld, dtype=torch.bool)
    for (o, n) in seqs:
        own[o:o + n, :C] = True
    return own


def run_sqshift(c, pad=8):
    _lib, L = _L()
    d = c['H'] * 64
    ldo = d + pad
    q, k, v, P = c['q'].cuda(), c['k'].cuda(), c['v'].cuda(), c['P'].cuda()
    bu, bv = c['bias_u'].cuda().contiguous(), c['bias_v'].cuda().contiguous()
    o = torch.full((c['rows'], ldo), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    _lib.check(L.wn_op_attention_sqshift(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d, d, c['rows'], P.data_ptr(), d, P.shape[0],
        bu.data_ptr(), bv.data_ptr(), o.data_ptr(), ldo, _lib.i32p(off), _lib.i32p(ln), len(off),
        c['H'], c['scale'], torch.cuda.current_stream().cuda_stream), 'attention_sqshift')
    torch.cuda.synchronize()
    oc = o.cpu()
    assert bool((oc[~_owned(c['rows'], c['seqs'], ldo, d)] == PATTERN).all()), \
        'a store outside the owned rows / columns'
    return oc.view(torch.float32)[:, :d]


@pytest.mark.parametrize('name', sorted(SQ.SQSHIFT_CASES))
def test_attention_sqshift(name):
    """Ragged lengths 1, 2, 31, 32, 33, 65, 100 (the single frame, the one- and two-row wraps,
    the tile edges on both sides), a peaked regime, the sign cases, a table with rows >= len.
    Unowned rows hold +-1e18: a read of query row i0 + 32 behind a sequence, of a neighbour's
    key or of a padded key would leave the output non-finite or off by far more than the bound."""
    c = SQ.make_sqshift_case(**SQ.SQSHIFT_CASES[name])
    ref, e_plain, scale = SQ.sqshift_refs(c)
    out = run_sqshift(c)
    own = c['own']
    assert torch.isfinite(out[own]).all(), name
    record(f'attention_sqshift {name}', (out[own].double() - ref[own]).abs().max().item(), e_plain,
           scale)


def test_attention_sqshift_does_not_depend_on_the_packing():
    """The same sequences packed in another order and behind other gaps: the same bits."""
    lens = [33, 1, 65, 32]
    a = SQ.make_sqshift_case(2, lens, seed=9, sign=True)
    out_a = run_sqshift(a)
    b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.items()}
    offs, rows = KR.pack_layout(lens[::-1], 1, 0)
    sgn = torch.where(torch.arange(128) % 2 == 0, 1.0, -1.0) * KR.POISON
    for key, s in (('q', -sgn), ('k', sgn), ('v', -sgn)):
        t = s.expand(rows, 128).clone()
        for pos, u in enumerate(range(len(lens))[::-1]):
            o, n = a['seqs'][u]
            t[offs[pos]:offs[pos] + n] = a[key][o:o + n]
        b[key] = t
    b['seqs'] = [(offs[pos], lens[u]) for pos, u in enumerate(range(len(lens))[::-1])]
    b['rows'] = rows
    out_b = run_sqshift(b)
    for pos, u in enumerate(range(len(lens))[::-1]):
        (oa, n), (ob, _) = a['seqs'][u], b['seqs'][pos]
        assert torch.equal(out_a[oa:oa + n].view(torch.int32),
                           out_b[ob:ob + n].view(torch.int32)), u


def _tap_major(wt):
    return wt[:, 0, :].t().contiguous().cuda()          # (C, 1, K) -> [K][C]


@pytest.mark.parametrize('K', [5, 1])
@pytest.mark.parametrize('C', [128, 512])
def test_time_reduce_dwconv(K, C):
    """Lengths 1, 2, 5, 31, 32, 33, 64, 65 packed with poisoned gaps: exactly ceil(len / 2) rows
    per utterance, everything else untouched."""
    _lib, L = _L()
    c = SQ.make_time_case(C, K, seed=K + C)
    ref, e_plain, scale = SQ.time_reduce_refs(c)
    ldy = C + 4
    x, wt, bias = c['x'].cuda(), _tap_major(c['wt']), c['bias'].cuda()
    y = torch.full((c['rows2'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    off2 = _i32(c['offs2'])
    _lib.check(L.wn_op_time_reduce(x.data_ptr(), C, c['rows'], C, wt.data_ptr(), bias.data_ptr(),
                                   K, c['pad'], y.data_ptr(), ldy, c['rows2'], _lib.i32p(off),
                                   _lib.i32p(ln), _lib.i32p(off2), len(off),
                                   torch.cuda.current_stream().cuda_stream), 'time_reduce')
    torch.cuda.synchronize()
    yc = y.cpu()
    own = _owned(c['rows2'], list(zip(c['offs2'], c['lens2'])), ldy, C)
    assert bool((yc[~own] == PATTERN).all()), 'a store outside the ceil(len / 2) owned rows'
    out = yc.view(torch.float32)[:, :C]
    rows = own[:, 0]
    assert torch.isfinite(out[rows]).all()
    record(f'time_reduce K={K} C={C}', (out[rows].double() - ref[rows]).abs().max().item(),
           e_plain, scale)


@pytest.mark.parametrize('in_place', [False, True])
def test_time_recover_add_is_exact(in_place):
    _lib, L = _L()
    C = 128
    c = SQ.make_time_case(C, 1, seed=77)
    want = SQ.ref_time_recover(c['x'], c['z'], c['seqs'], c['offs2'], dtype=torch.float32).float()
    skip, z = c['x'].cuda(), c['z'].cuda()
    ldy = C if in_place else C + 4
    y = skip if in_place else torch.full((c['rows'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    off2 = _i32(c['offs2'])
    _lib.check(L.wn_op_time_recover(skip.data_ptr(), C, z.data_ptr(), C, c['rows2'], y.data_ptr(),
                                    ldy, c['rows'], C, _lib.i32p(off), _lib.i32p(ln),
                                    _lib.i32p(off2), len(off),
                                    torch.cuda.current_stream().cuda_stream), 'time_recover')
    torch.cuda.synchronize()
    yc = y.cpu()
    own = _owned(c['rows'], c['seqs'], ldy, C)
    if in_place:
        assert torch.equal(yc[~own[:, 0]], c['x'][~own[:, 0]]), 'an unowned row was written'
        out = yc
    else:
        assert bool((yc[~own] == PATTERN).all()), 'a store outside the owned rows / columns'
        out = yc.view(torch.float32)[:, :C]
    rows = own[:, 0]
    assert torch.equal(out[rows].view(torch.int32), want[rows].view(torch.int32))
