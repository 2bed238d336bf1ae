"""Operator tests of the Efficient Conformer kernels (csrc/efficonformer.hip) through the hooks
wn_op_attention_grouped / wn_op_stride_dwconv_ln_silu / wn_op_avgpool_residual_add, against the
plain fp64 references of tests/efficonformer_refs.py (pinned to the reference's modules on the
CPU, tests/test_efficonformer_host.py).

Tolerance, the rule of tests/test_gpu_kernels.py: err <= 8 * e_plain + 16 fp32 ulps of the output
scale (kernel_refs.bound), e_plain = the error of the plain fp32 evaluation of the same formula on
the same inputs, itself capped (kernel_refs.cap_ok).  avgpool_residual_add is two roundings per
element: bit-exact against the fp32 statement.  Sequences are packed between rows of +-1e18, the
position rows behind every length and the pad columns of every stride hold them too; output
buffers start as a bit pattern that every element no sequence owns must still hold.
"""
import numpy as np
import pytest
import torch

import efficonformer_refs as EF
import kernel_refs as KR

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


_CASES = {}


def _grouped_case(W):
    """One case per width, its reference inputs computed once and left unchanged."""
    if W not in _CASES:
        _CASES[W] = EF.make_grouped_case(W, seed=W)
    return _CASES[W]


def run_grouped(c, chunk, left, mask_step, pad=8):
    _lib, L = _L()
    D = c['D']
    ldo = D + pad
    q, k, v, P = c['q'].cuda(), c['k'].cuda(), c['v'].cuda(), c['P'].cuda()
    bu, bv = c['bias_u'].cuda().contiguous(), c['bias_v'].cuda().contiguous()
    o = torch.full((c['rows'], ldo), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    poff = _i32(c['p_offs'])
    _lib.check(L.wn_op_attention_grouped(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), q.shape[1], k.shape[1], v.shape[1], c['rows'],
        P.data_ptr(), P.shape[1], c['p_rows'], _lib.i32p(poff), bu.data_ptr(), bv.data_ptr(),
        o.data_ptr(), ldo, _lib.i32p(off), _lib.i32p(ln), len(off), c['H'], c['g'], c['W'],
        mask_step, chunk, left, c['scale'], torch.cuda.current_stream().cuda_stream),
        'attention_grouped')
    torch.cuda.synchronize()
    oc = o.cpu()
    assert bool((oc[~_owned(c['rows'], c['seqs'], ldo, D)] == PATTERN).all()), \
        'a store outside the owned frames / columns'
    return oc.view(torch.float32)[:, :D]


@pytest.mark.parametrize('chunk,left,mask_step', EF.GROUPED_MASKS)
@pytest.mark.parametrize('W', [96, 192])
def test_attention_grouped(W, chunk, left, mask_step):
    """Lengths 1, 2, 3, 4, 31, 95, 97, 200 (T mod 3 = 0, 1, 2, a lone partial group, exactly one
    key tile, more than one key tile and query block), row strides larger than D, full context
    and chunk masks evaluated on frame indices.  Everything a sequence does not own holds
    +-1e18, the position rows behind its length included: a frame >= len read from memory
    instead of as zeros leaves the output non-finite or off by far more than the bound."""
    c = _grouped_case(W)
    ref, e_plain, scale = EF.grouped_refs(c, chunk, left, mask_step)
    out = run_grouped(c, chunk, left, mask_step)
    own = c['own']
    assert torch.isfinite(out[own]).all()
    record(f'attention_grouped W={W} c={chunk} l={left} m={mask_step}',
           (out[own].double() - ref[own]).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('W', [96, 192])
def test_attention_grouped_does_not_depend_on_the_packing(W):
    """The same sequences alone in a buffer of their own: the same bits as inside the batch."""
    c = _grouped_case(W)
    out = run_grouped(c, 16, 2, 3)
    for i in (2, 4, 7):       # lengths 3, 31, 200
        (o, n), po = c['seqs'][i], c['p_offs'][i]
        one = dict(c, q=c['q'][o:o + n].clone(), k=c['k'][o:o + n].clone(),
                   v=c['v'][o:o + n].clone(), P=c['P'][po:po + n].clone(), seqs=[(0, n)],
                   p_offs=[0], rows=n, p_rows=n)
        alone = run_grouped(one, 16, 2, 3)
        assert torch.equal(alone.view(torch.int32), out[o:o + n].view(torch.int32)), n


def _tap_major(wt):
    return wt[:, 0, :].t().contiguous().cuda()          # (C, 1, K) -> [K][C]


@pytest.mark.parametrize('norm_mode', [0, 1])
@pytest.mark.parametrize('causal', [0, 1, 2])           # 2: causal with a pad frame
@pytest.mark.parametrize('K', [15, 7])
@pytest.mark.parametrize('D', [128, 256])
def test_stride_dwconv_ln_silu(D, K, causal, norm_mode):
    """Lengths 1, 2, 3, 16, 33, 64 packed with poisoned gaps: exactly ceil(len / 2) rows per
    utterance, everything else untouched."""
    _lib, L = _L()
    c = EF.make_stride_case(D, K, seed=K + D + causal)
    cpad = c['cpad'] if causal == 2 else None
    ref, e_plain, scale = EF.stride_dwconv_refs(c, norm_mode, causal > 0, cpad)
    ldy = D + 4
    x, wt, bias = c['x'].cuda(), _tap_major(c['wt']), c['bias'].cuda()
    lw, lb = c['ln_w'].cuda(), c['ln_b'].cuda()
    cp = cpad.cuda() if cpad is not None else None
    y = torch.full((c['rows2'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    off2 = _i32(c['offs2'])
    _lib.check(L.wn_op_stride_dwconv_ln_silu(
        x.data_ptr(), D, c['rows'], D, wt.data_ptr(), bias.data_ptr(),
        cp.data_ptr() if cp is not None else None, lw.data_ptr(), lb.data_ptr(), norm_mode, 1e-5,
        K, int(causal > 0), 2, y.data_ptr(), ldy, c['rows2'], _lib.i32p(off), _lib.i32p(ln),
        _lib.i32p(off2), len(off), torch.cuda.current_stream().cuda_stream),
        'stride_dwconv_ln_silu')
    torch.cuda.synchronize()
    yc = y.cpu()
    own = _owned(c['rows2'], list(zip(c['offs2'], c['lens2'])), ldy, D)
    assert bool((yc[~own] == PATTERN).all()), 'a store outside the ceil(len / 2) owned rows'
    out = yc.view(torch.float32)[:, :D]
    rows = own[:, 0]
    assert torch.isfinite(out[rows]).all()
    record(f'stride_dwconv D={D} K={K} causal={causal} norm={norm_mode}',
           (out[rows].double() - ref[rows]).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('in_place', [False, True])
def test_avgpool_residual_add_is_exact(in_place):
    """(a + b) * 0.5 for a full window, a itself for the last window of an odd length, then one
    add: the same bits as the fp32 statement."""
    _lib, L = _L()
    C = 128
    c = EF.make_stride_case(C, 7, seed=77)
    want = EF.ref_avgpool_residual(c['x'], c['z'], c['seqs'], c['offs2'],
                                   dtype=torch.float32).float()
    x, z = c['x'].cuda(), c['z'].cuda()
    ldy = C if in_place else C + 4
    y = z if in_place else torch.full((c['rows2'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    off2 = _i32(c['offs2'])
    _lib.check(L.wn_op_avgpool_residual_add(
        x.data_ptr(), C, c['rows'], z.data_ptr(), C, y.data_ptr(), ldy, c['rows2'], C, 2,
        _lib.i32p(off), _lib.i32p(ln), _lib.i32p(off2), len(off),
        torch.cuda.current_stream().cuda_stream), 'avgpool_residual_add')
    torch.cuda.synchronize()
    yc = y.cpu()
    own = _owned(c['rows2'], list(zip(c['offs2'], c['lens2'])), ldy, C)
    if in_place:
        assert torch.equal(yc[~own[:, 0]], c['z'][~own[:, 0]]), 'an unowned row was written'
        out = yc
    else:
        assert bool((yc[~own] == PATTERN).all()), 'a store outside the owned rows / columns'
        out = yc.view(torch.float32)[:, :C]
    rows = own[:, 0]
    assert torch.equal(out[rows].view(torch.int32), want[rows].view(torch.int32))
    # the odd tails: lengths 1, 3, 33 end in the last frame itself
    for (o, n), o2 in zip(c['seqs'], c['offs2']):
        if n % 2:
            t = (n - 1) // 2
            assert torch.equal(out[o2 + t], (c['z'][o2 + t] + c['x'][o + n - 1]))
