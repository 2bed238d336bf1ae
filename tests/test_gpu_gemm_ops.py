"""Operator tests of the fp32 and the bf16-on-the-fly matrix-core GEMMs (csrc/gemm.hip,
csrc/gemm_bf16.hip, csrc/gemm_epilogue.h) through wn_op_gemm_ex, which hands gemm_f32 the whole
GemmArgs -- strides, the GLU epilogue, gathered rows, the implicit 3x3 / stride-2 operand --
against the plain fp64 reference of tests/kernel_refs.py (`ref_gemm`, checked against second
statements on the CPU in tests/test_kernel_refs.py).  The cases are kernel_refs.GEMM_CASES.

Every case
  * asserts the route (block shape, waves, K tile, prefetch depth, GLU / CONV, precision, epilogue)
    the dispatch reports,
  * gives C as (M + 3, ldc) words of PATTERN, ldc = N + 5 (GLU: N / 2 + 4): every word outside
    [0, M) x [0, N) (N / 2) must still hold it,
  * has POISON in the pad columns of A (lda = K + 4) and of the residual (ldr = N + 3) and in every
    float of a gathered buffer that no (row, k) reads,
  * runs twice and compares the bits,
  * meets kernel_refs.bound(e_plain, scale) in its fp32 form -- 8 e_plain + 16 ulps of max |ref|
    -- in BOTH precisions: the accumulators are fp32 and the reference of precision 1 already
    carries the operand rounding.
Regimes: `unit` standard normal; `coded` one-hot operand rows (gathered kinds: one-hot frames /
pixels) against W[n][k] = (37 n + 11 k) mod 251 - 125, integer bias and residual, GLU gates
that are exactly open or shut: the reference is exact in fp32 and the comparison is rtol = atol = 0;
`wide` biases that put the SiLU / GELU arguments and the GLU gates at 0, +-20, +-88, +-90, +-104.
resid rC: C == resid in place with ldr == ldc, as the encoder's residual stream runs it.

Kernel instantiation -> cases (ids of test_gemm_case; `every` = act 0..3 x r0 / r1):
  gemm_f32_kernel<128,128,2,4,act,resid>            f32-plain-128x128w2x4k32pf1-200x24571x32-*
                                                    (every, rC, coded, wide), 12285x500x32 (tall)
  gemm_f32_kernel<128,128,2,4,NONE|RELU,resid,PF 2> f32-plain-128x128w2x4k32pf2-200x24571x{1024,
                                                    1056,1088}: all four
  gemm_f32_kernel<64,128,2,4,act,resid>             f32-plain-64x128w2x4k32pf1-100x24570x32 (every)
  gemm_f32_kernel<64,128,2,4,...,PF 2>              ...pf2-100x24570x1024 (RELU, r0), x1056 (NONE, r1)
  gemm_f32_kernel<64,64,2,2,act,resid>              f32-plain-64x64w2x2k32pf1-{1x1,65x67,333x200}x32
  gemm_f32_kernel<64,64,2,2,NONE|RELU,resid,PF 2>   ...pf2-65x67x{1024,1056,1088}: all four
  gemm_f32_kernel<64,128,2,2,GLU>                   f32-plain-glu-64x128w2x2*: N 64 / 128 / 192 x M 1 /
                                                    63 / 130
  gemm_f32_kernel<128,128,4,2,GLU>                  f32-plain-glu-128x128w4x2*-129x14272x32
  gemm_f32_kernel<64,128,2,2,NONE|RELU|GELU,resid,CONV>    f32-rows-64x128w2x2*-66x200x96 (all six),
                                                    f32-conv3-64x128w2x2*-69x70x{288,576}
  gemm_f32_kernel<128,128,2,2,NONE|RELU|GELU,resid,CONV>   f32-rows-128x128w2x2*-129x24571x96 (all
                                                    six), f32-conv3-128x128w2x2*-138x24571x{288,576}
  gemm_bf16_kernel<128,128,2,4,act,resid,BK 64|32>  bf16-plain-128x128w2x4k{64,32}*-200x14331x{64,96}
                                                    (every); the 256-row shapes under gemm_tile_bf16 = 1
  gemm_bf16_kernel<64,64,2,2,act,resid,BK 64|32>    bf16-plain-64x64w2x2k{64,32}* (every at 333x200)
  gemm_bf16_kernel<64,128,2,2,GLU,BK 64|32>         bf16-plain-glu-64x128w2x2k{64,32}*
  gemm_bf16_kernel<128,128,4,2,GLU,BK 64|32>        bf16-plain-glu-128x128w4x2k{64,32}*-129x14272x{64,96}
  gemm_bf16_kernel<64,128,2,2,..,CONV,BK 32|64>     bf16-rows-64x128w2x2k{32,64}*-66x200x{96,192} (all
                                                    six each), bf16-conv3-64x128w2x2*-69x70x{288,576}
  gemm_bf16_kernel<128,128,2,4,..,CONV,BK 32|64>    bf16-rows-128x128w2x4k{32,64}*-129x14331x{96,192}
                                                    (all six each), bf16-conv3-128x128w2x4*-138x14331x*
  gemm_bf16_kernel<256,256,4,2,..,BK 64>            bf16-plain-256x256w4x2k64pf1-257x131069x64
                                                    (NONE r0, RELU r1, SILU r0, GELU r1),
                                                    257x32765x2048 (K >= 2048, t256 = 256)
No case reaches
  gemm_f32_kernel<64,128,2,4,NONE,false,PF 2> and <64,128,2,4,RELU,true,PF 2>: the block needs
      384 tiles, a K >= 1024 case of it is 2.7 GFLOP of fp64 on the CPU; two of the four run, and
      all four run on the two other blocks;
  gemm_bf16_kernel<256,256,4,2> with (NONE, r1), (SILU, r1), (RELU, r0), (GELU, r0): the block
      needs t256 >= 1024, that is a C of 136 MB per case; every activation and both residual
      forms run on it, and all eight combinations on the three other bf16 blocks;
  the `launch<..., CONV = true, 32, PF = 2>` bodies dispatch_epi of gemm.hip names under `pf2`:
      pf2 is false for a gathered A, the branch never runs.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as KR
from test_gpu_kernels import PATTERN, _L, _padded, record, tune

pytestmark = pytest.mark.gpu

IDS = [KR.gemm_case_id(s) for s in KR.GEMM_CASES]


def _fill_op(op, _lib, keep, c, C, resid_dev):
    s = c['spec']
    M, N, K = c['M'], c['N'], c['K']
    if s['kind'] == 'plain':
        A = _padded(c['A'], K + 4)
        op.A, op.lda, op.a_elems = A.data_ptr(), K + 4, A.numel()
    else:
        A = c['buf'].cuda()
        off = np.ascontiguousarray(c['a_row_off'].numpy(), dtype=np.int64)
        op.A, op.lda, op.a_elems = A.data_ptr(), 0, A.numel()
        op.a_row_off = _lib.i64p(off)
        op.conv_C, op.conv_sy, op.conv_sx = c['conv_C'], c['conv_sy'], c['conv_sx']
        keep.append(off)
    W, bias = c['W'].contiguous().cuda(), c['bias'].contiguous().cuda()
    keep += [A, W, bias]
    op.W, op.bias, op.C = W.data_ptr(), bias.data_ptr(), C.data_ptr()
    op.M, op.N, op.K, op.ldc = M, N, K, C.shape[1]
    op.alpha, op.act, op.glu, op.precision = s['alpha'], s['act'], int(s['glu']), s['prec']
    if s['resid'] == 1:
        op.resid, op.ldr = resid_dev.data_ptr(), resid_dev.shape[1]
    elif s['resid'] == 2:
        op.resid, op.ldr = C.data_ptr(), C.shape[1]


def run_gemm(c):
    """One wn_op_gemm_ex call on a case of kernel_refs.make_gemm_case.  Returns (the bits of
    C[:M, :n_out] on the device, route).  Asserts that every other word of C kept PATTERN."""
    _lib, L = _L()
    s = c['spec']
    M, N = c['M'], c['N']
    n_out = N // 2 if s['glu'] else N
    ldc = n_out + (4 if s['glu'] else 5)
    C = torch.full((M + 3, ldc), PATTERN, dtype=torch.int32).cuda()
    resid_dev = None
    if s['resid'] == 1:
        resid_dev = _padded(c['resid'], N + 3)
    elif s['resid'] == 2:
        C[:M, :N] = c['resid'].cuda().view(torch.int32)
    op, keep = _lib.WnGemmOp(), []
    _fill_op(op, _lib, keep, c, C, resid_dev)
    route = ctypes.c_int32(-1)
    _lib.check(L.wn_op_gemm_ex(ctypes.byref(op), ctypes.byref(route),
                               torch.cuda.current_stream().cuda_stream), 'gemm_ex')
    torch.cuda.synchronize()
    out = C[:M, :n_out].clone()
    C[:M, :n_out] = PATTERN
    assert bool((C == PATTERN).all()), 'a store outside [0, M) x [0, N) of C'
    return out, route.value


def _expect_route(s, route=None):
    bm, bn, wgm, wgn, bk, pf = route or s['route']
    return KR.gemm_route_code(bm, bn, wgm, wgn, bk, pf, glu=s['glu'], conv=s['kind'] != 'plain',
                              prec=s['prec'], act=s['act'], resid=s['resid'] != 0)


def _check(name, c, refs, expect):
    ref, e_plain, scale = refs
    s = c['spec']
    out, route = run_gemm(c)
    assert route == expect, (name, hex(route), hex(expect))
    again, _ = run_gemm(c)
    assert torch.equal(out, again), name + ': two runs differ'
    got = out.view(torch.float32).cpu()
    assert torch.isfinite(got).all(), name
    if s['regime'] == 'coded':
        want = ref.float()
        bad = (got != want).sum().item()
        record(name, (got.double() - want.double()).abs().max().item(), e_plain, scale)
        assert bad == 0, (name, bad)
    else:
        record(name, (got.double() - ref).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('ci', range(len(KR.GEMM_CASES)), ids=IDS)
def test_gemm_case(ci):
    s = KR.GEMM_CASES[ci]
    c = KR.make_gemm_case(s)
    refs = KR.gemm_refs(c)
    _check('gemm[' + IDS[ci] + ']', c, refs, _expect_route(s))
    if s['tile1_route']:
        # the same problem without the 256-row block: the 128x128 block, the same bound
        with tune(gemm_tile_bf16=1):
            _check('gemm[' + IDS[ci] + '-tile1]', c, refs, _expect_route(s, s['tile1_route']))


def _refused(c, text, **change):
    """The call must fail with `text` in wn_last_error and leave every word of C alone."""
    _lib, L = _L()
    s = c['spec']
    n_out = c['N'] // 2 if s['glu'] else c['N']
    C = torch.full((c['M'] + 3, n_out + 5), PATTERN, dtype=torch.int32).cuda()
    resid_dev = _padded(c['resid'], c['N'] + 3) if s['resid'] == 1 else None
    op, keep = _lib.WnGemmOp(), []
    _fill_op(op, _lib, keep, c, C, resid_dev)
    for k, v in change.items():
        if k == 'a_row_off':
            keep.append(v)
            v = _lib.i64p(v)
        elif k == 'resid':
            keep.append(v)
            v = v.data_ptr()
        setattr(op, k, v)
    route = ctypes.c_int32(-1)
    status = L.wn_op_gemm_ex(ctypes.byref(op), ctypes.byref(route),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    msg = L.wn_last_error().decode('utf8', 'replace')
    assert status == -1 and text in msg, (status, msg)
    assert bool((C == PATTERN).all()), 'a refused call wrote to C'


def test_gemm_refusals():
    """What gemm_f32 and the hook refuse, before any launch."""
    S = KR._gemm_spec
    plain = KR.make_gemm_case(S('plain', 65, 67, 64, None))
    res = KR.make_gemm_case(S('plain', 65, 67, 64, None, resid=1))
    glu = KR.make_gemm_case(S('plain', 63, 128, 64, None, glu=True))
    rows = KR.make_gemm_case(S('rows', 66, 200, 96, None, lens=[37, 3, 95]))
    conv = KR.make_gemm_case(S('conv3', 69, 70, 288, None, lens=[31, 17], F1=7, conv_C=32))
    for prec in (0, 1):
        _refused(plain, 'K must be a multiple of 32', K=48, precision=prec)
        _refused(plain, 'lda must be a multiple of 4', lda=70, precision=prec)
        _refused(plain, 'lda is smaller than K', lda=60, precision=prec)
        _refused(plain, 'past a_elems', a_elems=64 * 68 + 63, precision=prec)
        _refused(plain, 'ldc is smaller', ldc=66, precision=prec)
        _refused(res, 'ldr is smaller', ldr=66, precision=prec)
        _refused(glu, 'N must be a multiple of 64', N=96, precision=prec)
        _refused(glu, 'no activation, residual or alpha', act=1, precision=prec)
        _refused(glu, 'no activation, residual or alpha', alpha=0.5, precision=prec)
        _refused(glu, 'no activation, residual or alpha', precision=prec,
                 resid=torch.zeros(63, 128).cuda(), ldr=128)
        _refused(glu, 'ldc is smaller', ldc=63, precision=prec)
        _refused(rows, 'no SiLU epilogue with a gathered A', act=1, precision=prec)
        _refused(conv, 'no SiLU epilogue with a gathered A', act=1, precision=prec)
        off = np.ascontiguousarray(rows['a_row_off'].numpy(), dtype=np.int64)
        for r in (0, 65):
            past, odd = off.copy(), off.copy()
            past[r] = rows['buf'].numel() - 92            # the last 4 floats of the row lie outside
            odd[r] += 2
            _refused(rows, 'past a_elems', a_row_off=past, precision=prec)
            _refused(rows, 'not a multiple of 4', a_row_off=odd, precision=prec)
        _refused(rows, 'past a_elems', a_elems=int(off.max()) + 95, precision=prec)
        coff = np.ascontiguousarray(conv['a_row_off'].numpy(), dtype=np.int64)
        # the last tap of the last row: (2 F1 + 2) pixels behind its first
        _refused(conv, 'past a_elems', a_elems=int(coff.max()) + (2 * 7 + 2) * 32 + 31, precision=prec)
        _refused(conv, 'multiples of 4', conv_sx=34, precision=prec)
        _refused(conv, 'K must be 9*C', conv_C=64, precision=prec)
