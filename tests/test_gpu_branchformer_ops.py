"""Operator tests of the Branchformer kernels (csrc/branchformer.hip) through the hooks
wn_op_csgu_gate / wn_op_merge_dwconv, against the plain fp64 references of
tests/branchformer_refs.py (pinned to the reference's modules on the CPU,
tests/test_branchformer_host.py).

Tolerance of every case, the rule of tests/test_gpu_kernels.py: err <= 8 * e_plain + 16 fp32 ulps
of the output scale (kernel_refs.bound), e_plain = the error of the plain fp32 evaluation of the
same formula on the same inputs.  Every launch packs four utterances of 1, 5, tile - 1 and
tile + 1 frames (tile = wn_csgu_time_tile(): nothing but padding, shorter than the conv's history,
one tile less a frame, two tiles) between rows of +-1e18, and runs a second time with the
utterances packed in reversed order: per utterance the two results are the same bits, so no row
of a neighbour is ever read.  Output buffers start as a bit pattern that every element no
utterance owns must still hold.
"""
import numpy as np
import pytest
import torch

import branchformer_refs as BR
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


def _tap_major(wt):
    return wt[:, 0, :].t().contiguous().cuda()          # (C, 1, K) -> [K][C]


def _owned(c, ld):
    own = torch.zeros(c['rows'], ld, dtype=torch.bool)
    for (o, n) in c['seqs']:
        own[o:o + n, :c['C']] = True
    return own


def run_csgu(c, gate=True, pad=8):
    _lib, L = _L()
    C = c['C']
    ldy = C + pad
    h = c['h'].cuda()
    y = torch.full((c['rows'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    wt = _tap_major(c['wt'])
    lw, lb, bias = c['ln_w'].cuda(), c['ln_b'].cuda(), c['bias'].cuda()
    _lib.check(L.wn_op_csgu_gate(h.data_ptr(), 2 * C, c['rows'], C, lw.data_ptr(), lb.data_ptr(),
                                 wt.data_ptr(), bias.data_ptr(), c['K'], int(c['causal']),
                                 int(gate), y.data_ptr(), ldy, _lib.i32p(off), _lib.i32p(ln),
                                 len(off), torch.cuda.current_stream().cuda_stream), 'csgu_gate')
    torch.cuda.synchronize()
    yc = y.cpu()
    assert bool((yc[~_owned(c, ldy)] == PATTERN).all()), 'a store outside the owned rows / columns'
    return yc.view(torch.float32)[:, :C]


def run_merge(c, pad=4):
    _lib, L = _L()
    C = c['C']
    ldc, ldy = 2 * C, C + pad                 # x = the first C columns of h
    x = c['h'].cuda()
    y = torch.full((c['rows'], ldy), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in c['seqs']]), _i32([s[1] for s in c['seqs']])
    wt, bias = _tap_major(c['wt']), c['bias'].cuda()
    _lib.check(L.wn_op_merge_dwconv(x.data_ptr(), ldc, c['rows'], C, wt.data_ptr(),
                                    bias.data_ptr(), c['K'], int(c['causal']), y.data_ptr(), ldy,
                                    _lib.i32p(off), _lib.i32p(ln), len(off),
                                    torch.cuda.current_stream().cuda_stream), 'merge_dwconv')
    torch.cuda.synchronize()
    yc = y.cpu()
    assert bool((yc[~_owned(c, ldy)] == PATTERN).all()), 'a store outside the owned rows / columns'
    return yc.view(torch.float32)[:, :C]


def _both_orders(make, run, refs, name):
    """The case in packing order 0..3 against the reference, then reversed: the same bits per
    utterance."""
    c = make(None)
    ref, e_plain, scale = refs(c)
    out = run(c)
    own = _owned(c, c['C'])[:, 0]
    assert torch.isfinite(out[own]).all(), name
    record(name, (out[own].double() - ref[own]).abs().max().item(), e_plain, scale)
    n = len(c['seqs'])
    r = make(list(range(n))[::-1])
    out_r = run(r)
    for u in range(n):
        (o0, t), (o1, _) = c['seq_of'][u], r['seq_of'][u]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: utterance {u} depends on where it is packed'


def test_time_tile_hook():
    _, L = _L()
    assert L.wn_csgu_time_tile() >= 8


CSGU_CASES = [(C, K, causal) for C in (128, 1024) for K in (3, 31) for causal in (False, True)] \
    + [(C, 63, True) for C in (128, 1024)]


@pytest.mark.parametrize('C,K,causal', CSGU_CASES)
def test_csgu_gate(C, K, causal):
    _, L = _L()
    lens = BR.op_lens(L.wn_csgu_time_tile())
    make = lambda order: BR.make_csgu_case(C, K, causal, lens, seed=C + K + int(causal),
                                           order=order)
    _both_orders(make, run_csgu, BR.csgu_refs, f'csgu_gate[C={C},K={K},causal={causal}]')


@pytest.mark.parametrize('causal', [False, True])
def test_csgu_conv_alone(causal):
    """gate = 0 (use_linear_after_conv: the kernel stops behind the conv)."""
    _, L = _L()
    c = BR.make_csgu_case(128, 15, causal, BR.op_lens(L.wn_csgu_time_tile()), seed=77)
    ref, e_plain, scale = BR.csgu_refs(c, gate=False)
    out = run_csgu(c, gate=False)
    own = _owned(c, c['C'])[:, 0]
    record(f'csgu_conv[causal={causal}]', (out[own].double() - ref[own]).abs().max().item(),
           e_plain, scale)


@pytest.mark.parametrize('C,K,causal', [(C, K, causal) for C in (128, 512) for K in (3, 31)
                                        for causal in (False, True)])
def test_merge_dwconv(C, K, causal):
    _, L = _L()
    lens = BR.op_lens(L.wn_csgu_time_tile())

    def make(order):
        c = BR.make_csgu_case(C, K, causal, lens, seed=500 + C + K + int(causal), order=order)
        return c

    _both_orders(make, run_merge, BR.merge_refs, f'merge_dwconv[C={C},K={K},causal={causal}]')


def test_refused_shapes():
    _lib, L = _L()
    c = BR.make_csgu_case(128, 4, False, [5], seed=1)      # an even K without causal
    with pytest.raises(RuntimeError, match='odd unless causal'):
        run_csgu(c)
    c = BR.make_csgu_case(128, 3, False, [5], seed=1)
    c['C'] = 96                                             # not a multiple of 64
    with pytest.raises(RuntimeError, match='multiple of 64'):
        run_merge(c)
