"""Operator tests of the stored-operand GEMMs -- gemm_bf16s_kernel (csrc/gemm_bf16s.hip),
gemm_lp_kernel on bf16 and MXFP8 operands and mx_quantize_kernel (csrc/gemm_bf16p.hip) -- through
wn_op_gemm_lowp_ex / wn_op_mx_quantize_ex, which hand the launchers the whole argument block
(strides, scale pitches, GLU), against the plain fp64 reference of tests/kernel_refs.py
(`ref_gemm_lowp` on the decoded operands, `mx_encode` / `mx_decode`; checked on the CPU in
tests/test_kernel_refs.py).  The cases are kernel_refs.GEMM_LOWP_CASES.

Every case
  * asserts the route the launcher reports (block, waves, K tile, GLU, activation, residual, kernel
    family, element type, C mode),
  * gives C as (M + 3, ldc) elements of PATTERN (PATTERN16 for a bf16 C, bytes 0xa5 for an MXFP8
    C), ldc = n_out + 4 / + 8 / + 16: everything outside [0, M) x [0, n_out) must still hold it;
    an MXFP8 C's scales are PATTERN dwords [ceil(N / 128)][pitch], and the entries of rows >= M
    and the bytes of blocks >= N / 32 of the last dword must still hold it,
  * has poison -- bf16 1e18, e4m3 byte 0x7e (448), scale byte 0xfe (2^127) -- in the pad columns of
    A (lda = K + 16), in 3 rows behind A and behind W, in the pad columns of the residual
    (ldr = N + 4) and in the scale entries of rows >= M / >= N (a_scale_pitch = c_scale_pitch =
    ceil(M / 256) * 256, the model's value, in every other case and M + 3 in the others;
    w_scale_pitch = N + 5 in some); the result must be finite,
  * runs twice and compares the bits.
Regimes: `unit` standard normal operands rounded to the storage type (MXFP8: rows of A scaled by
e^N(0,1), its k blocks by 2^randint(-6, 6)); `coded-hot` one-hot rows of A, 2^s(m) at k = (13 m +
5) mod K, against W[n][k] = ((37 n + 11 k) mod 17 - 8) 2^t(n, k / 32), integer bias and residual:
every output is ONE product, exact whatever the MFMA does inside a k-step, and wrong if a k block
meets another block's scale byte, another row's scale dword or another k; `coded-dense` A in
{-2..2} 2^s(m), W in {-8..8} 2^t(n), one scale per row: sums of at most 14 bits, exact in fp32,
wrong if a K tile is dropped, doubled or read from the other LDS buffer; `wide` biases that put
the SiLU / GELU arguments (GLU: the gates) at 0, +-20, +-88, +-90, +-104.
Bounds: bf16 operands, fp32 C: kernel_refs.bound(e_plain, scale) in its fp32 form (+ 4.7e-6 |alpha|
for gelu_e5 of the pipelined kernel).  bf16 C: the bits of the same case's fp32 C rounded on the
host, except -- one bf16 ulp -- where the fp32 C lies within that bound of a bf16 rounding
boundary (`unit` cases carry a bias of +4: near zero every absolute bound spans many boundaries;
under 2 % of the reference's elements are such, checked on the CPU); coded cases: no exception.
MXFP8 C: bytes and scale bytes == mx_encode of the same case's fp32 C.  MXFP8 `unit` / `wide`:
err <= 2e-5 S + 2e-5, S = max sum_k |a||w| (tests/test_gpu_fp8.py; the scaled MFMA aligns the
products of a k-step before it adds them, so e_plain is no yardstick: its ratio is recorded, not
asserted).  coded-*: rtol = atol = 0.

Kernel instantiation -> case ids (`every` = act 0..3 x r0 / r1, `acts` = act 0..3)
  gemm_lp_kernel<0,act,resid,0>   bf16-pipe-*-c32: every over M 1 / 255 / 256 / 257 / 300 / 1030 /
                                  1281, N 8 / 256 / 264 / 520, K 128 / 192 / 256 / 320; coded-hot,
                                  coded-dense, wide; 1030x264 (5 M panels, the last group of 1);
                                  bf16-pipe-tile0-*-257x24584x128 (the natural dispatch, t256 = 194)
  gemm_lp_kernel<0,act,false,1>   bf16-pipe-*-c16: acts, coded-hot, coded-dense
  gemm_lp_kernel<1,act,resid,0>   mx-pipe-*-c32: every over the same M and N, K 256 / 384 / 512 /
                                  640; coded-hot, coded-dense, wide
  gemm_lp_kernel<1,act,false,2>   mx-pipe-*-cmx: acts over N 32 / 288 / 544, coded-hot, wide
  gemm_bf16s_kernel<64,64,2,2,act,resid,false,false,64|32>     bf16-stored-64x64w2x2k{64,32}-*-c32:
                                  every at 333x200x{64,96}; 1, 2, 3, 5 K tiles (K 32 .. 320) coded
  gemm_bf16s_kernel<64,64,2,2,act,false,false,true,64|32>      ...-c16: acts at 333x200x{64,96}
  gemm_bf16s_kernel<128,128,2,4,act,resid,false,false,64|32>   bf16-stored-128x128w2x4k{64,32}-
                                  200x14332x{64,96}-*-c32 (t128 = 224): every, coded-hot, coded-dense
  gemm_bf16s_kernel<128,128,2,4,act,false,false,true,64|32>    ...-200x14336x{64,96}-*-c16: acts
  gemm_bf16s_kernel<64,128,2,2,NONE,false,true,false,64|32>    bf16-stored-glu-64x128w2x2*: N 64 /
                                  128 / 192 x M 1 / 63 / 130
  gemm_bf16s_kernel<128,128,4,2,NONE,false,true,false,64|32>   bf16-stored-glu-128x128w4x2*-
                                  129x14272x{64,96}
  gemm_bf16s_kernel<256,256,4,2,NONE,false,false,false,64>     bf16-stored-256x256w4x2k64-
                                  257x32764x2048: t256 = 256 and K >= 2048 under gemm_tile_bf16 = 0;
                                  N % 8 != 0, which the pipelined kernel does not take (a forced
                                  tile other than 0, 1 and 8 reaches the block too)
  mx_quantize_kernel              test_mx_quantize_ex
No case reaches
  gemm_bf16s_kernel<256,256,4,2> with any other epilogue (15 instantiations): the block needs
      t256 >= 256 with K >= 2048 -- 34 GFLOP of fp64 on the CPU per case, the size GEMM_CASES
      accepted once -- or t256 >= 1024, a C of 136 MB; its epilogue is gemm_epilogue, every form
      of which runs on the two other blocks, and its K loop is the one case above;
  gemm_lp_kernel<..., VAR != 0>: measurement variants (tools/bench_gemm.py --variants).

Ratios err / bound of one full run: profiles/r29a_gemm_lowp_error_ratios.txt.  Worst per kernel
family over the unit and wide cases: gemm_bf16s_kernel 64x64 0.052, 128x128 0.052, GLU 0.054,
256x256 (K = 2048) 0.211; gemm_lp_kernel on bf16 0.221 (GELU, K = 256), 0.044 on the natural
dispatch; gemm_lp_kernel on MXFP8 0.859 of 2e-5 S + 2e-5 (M = 1, N = 288, K = 256; every other
case under 0.35), and 13.9 against bound(e_plain, scale), which is recorded and not asserted.
All 49 coded cases were exact, coded-dense on the scaled MFMA included; no bf16 C differed from
the rounded fp32 C in any element.
"""
import ctypes

import pytest
import torch

import kernel_refs as KR
from test_gpu_kernels import PATTERN, PATTERN16, _L, _padded, record, tune

pytestmark = pytest.mark.gpu

IDS = [KR.gemm_lowp_case_id(s) for s in KR.GEMM_LOWP_CASES]
PATTERN8 = 0xa5
POISON_E4M3, POISON_E8M0 = 0x7e, 0xfe


def _cdiv(a, b):
    return -(-a // b)


def _operand(t, q, rows_pad, ld, et):
    """(rows, K) values (bf16) or bytes (MXFP8) -> device (rows + rows_pad, ld) in the storage
    type, poison everywhere else."""
    rows, K = t.shape
    if et:
        buf = torch.full((rows + rows_pad, ld), POISON_E4M3, dtype=torch.uint8)
        buf[:rows, :K] = q
    else:
        buf = torch.full((rows + rows_pad, ld), KR.POISON, dtype=torch.bfloat16)
        buf[:rows, :K] = t.to(torch.bfloat16)
    return buf.cuda()


def build_op(c, cm, keep):
    """The argument block of a case of kernel_refs.make_gemm_lowp_case with C mode `cm`, as the
    docstring lays the buffers out.  Returns (op, C, c_scale or None)."""
    _lib, _ = _L()
    s = c['spec']
    M, N, K, et = c['M'], c['N'], c['K'], s['et']
    n_out = N // 2 if s['glu'] else N
    lda = K + 16
    ldc = n_out + (4, 8, 16)[cm]
    A = _operand(c['A'], c.get('Aq'), 3, lda, et)
    W = _operand(c['W'], c.get('Wq'), 3, K, et)
    bias = c['bias'].contiguous().cuda()
    if cm == 0:
        C = torch.full((M + 3, ldc), PATTERN, dtype=torch.int32).cuda()
    elif cm == 1:
        C = torch.full((M + 3, ldc), PATTERN16, dtype=torch.int16).cuda()
    else:
        C = torch.full((M + 3, ldc), PATTERN8, dtype=torch.uint8).cuda()
    op = _lib.WnGemmLowpOp()
    op.A, op.W, op.bias, op.C = A.data_ptr(), W.data_ptr(), bias.data_ptr(), C.data_ptr()
    op.M, op.N, op.K, op.lda, op.ldc = M, N, K, lda, ldc
    op.alpha, op.act, op.glu, op.dtype, op.c_mode = s['alpha'], s['act'], int(s['glu']), 1 + et, cm
    op.a_bytes, op.w_bytes = A.numel() * A.element_size(), W.numel() * W.element_size()
    keep += [A, W, bias, C]
    if s['resid']:
        R = _padded(c['resid'], N + 4)
        op.resid, op.ldr = R.data_ptr(), N + 4
        keep.append(R)
    csc = None
    if et:
        pitch = _cdiv(M, 256) * 256 if s['model_pitch'] else M + 3
        a_sc = KR.mx_scale_dwords(c['AE'], pitch, POISON_E8M0).cuda()
        w_sc = KR.mx_scale_dwords(c['WE'], N + s['w_pad'], POISON_E8M0).cuda()
        op.a_scale, op.a_scale_pitch, op.a_scale_bytes = a_sc.data_ptr(), pitch, a_sc.numel() * 4
        op.w_scale, op.w_scale_pitch, op.w_scale_bytes = w_sc.data_ptr(), N + s['w_pad'], \
            w_sc.numel() * 4
        keep += [a_sc, w_sc]
        if cm == 2:
            csc = torch.full((_cdiv(N, 128), pitch), PATTERN, dtype=torch.int32).cuda()
            op.c_scale, op.c_scale_pitch, op.c_scale_bytes = csc.data_ptr(), pitch, csc.numel() * 4
            keep.append(csc)
    return op, C, csc


def run_lowp(c, cm):
    """One wn_op_gemm_lowp_ex call.  Returns (the bits of C[:M, :n_out] on the host, the E bytes
    (M, N / 32) of an MXFP8 C, route).  Asserts the frame of C and of the C scales."""
    _lib, L = _L()
    s = c['spec']
    M, N = c['M'], c['N']
    n_out = N // 2 if s['glu'] else N
    keep = []
    op, C, csc = build_op(c, cm, keep)
    route = ctypes.c_int32(-1)
    with tune(gemm_tile_bf16=s['tile']):
        _lib.check(L.wn_op_gemm_lowp_ex(ctypes.byref(op), ctypes.byref(route),
                                        torch.cuda.current_stream().cuda_stream), 'gemm_lowp_ex')
    torch.cuda.synchronize()
    out = C[:M, :n_out].clone()
    pat = (PATTERN, PATTERN16, PATTERN8)[cm]
    C[:M, :n_out] = pat
    assert bool((C == pat).all()), 'a store outside [0, M) x [0, n_out) of C'
    E = None
    if csc is not None:
        h = csc.cpu()
        E = KR.mx_scale_bytes(h, M, N // 32)
        own = torch.zeros(h.shape[0], h.shape[1], 4, dtype=torch.bool)
        for kb in range(N // 32):
            own[kb // 4, :M, kb % 4] = True
        pb = torch.full((h.shape[0], h.shape[1]), PATTERN, dtype=torch.int32).view(torch.uint8)
        assert torch.equal(h.view(torch.uint8).view(own.shape)[~own], pb.view(own.shape)[~own]), \
            'a store to a C-scale byte no (row, block) owns'
    return out.cpu(), E, route.value


_REFS = {}


def _refs(ci):
    """Cases are rebuilt from their spec; the references of the last case are kept for its second
    C mode."""
    if ci not in _REFS:
        _REFS.clear()
        c = KR.make_gemm_lowp_case(KR.GEMM_LOWP_CASES[ci])
        _REFS[ci] = (c, ) + KR.gemm_lowp_refs(c)
    return _REFS[ci]


def _extra(s):
    return KR.GELU_E5_ABS * abs(s['alpha']) if s['act'] == 3 and s['fam'] == KR.FAM_PIPELINED else 0.0


def _check_f32(name, c, refs):
    """The fp32-C run of a case against its reference; returns the fp32 C."""
    ref, e_plain, scale, S = refs
    s = c['spec']
    out, _, route = run_lowp(c, 0)
    expect = KR.lowp_route_code(dict(s, cm=0))
    assert route == expect, (name, hex(route & 0xffffffff), hex(expect & 0xffffffff))
    again, _, _ = run_lowp(c, 0)
    assert torch.equal(out, again), name + ': two runs differ'
    got = out.view(torch.float32)
    assert torch.isfinite(got).all(), name + ': not finite (poison was read)'
    err = (got.double() - ref).abs().max().item()
    if s['regime'].startswith('coded'):
        want = ref.float()
        bad = got != want
        record(name, err, e_plain, scale)
        assert not bad.any(), (name, int(bad.sum()), bad.nonzero()[:8].tolist(),
                               (got[bad][:8] - want[bad][:8]).tolist())
    elif s['et']:
        record(name, err, e_plain, scale, check=False)
        print(f'{name} err / (2e-5 S + 2e-5) = {err / (2e-5 * S + 2e-5):.3f}  S={S:.3e}')
        assert err <= 2e-5 * S + 2e-5, (name, err, S)
    else:
        record(name, err, e_plain, scale, extra=_extra(s))
    return got


@pytest.mark.parametrize('ci', range(len(KR.GEMM_LOWP_CASES)), ids=IDS)
def test_gemm_lowp_case(ci):
    s = KR.GEMM_LOWP_CASES[ci]
    c, *refs = _refs(ci)
    ref, e_plain, scale, S = refs
    name = 'gemm_lowp[' + IDS[ci] + ']'
    got32 = _check_f32(name if s['cm'] == 0 else name + '-as-c32', c, refs)
    if s['cm'] == 0:
        return
    out, E, route = run_lowp(c, s['cm'])
    assert route == KR.lowp_route_code(s), (name, hex(route & 0xffffffff))
    again, E2, _ = run_lowp(c, s['cm'])
    assert torch.equal(out, again), name + ': two runs differ'
    if s['cm'] == 1:
        want = got32.to(torch.bfloat16).view(torch.int16)
        bad = out != want
        near, _ = KR.bf16_tie_share(got32.double(), KR.bound(e_plain, scale) + _extra(s))
        print(f'{name} bf16 C: {int(bad.sum())} of {bad.numel()} differ from the rounded fp32 C; '
              f'{near.float().mean().item():.4f} of the elements lie within the bound of a boundary')
        if s['regime'].startswith('coded'):
            assert not bad.any() and torch.equal(out, ref.float().to(torch.bfloat16).view(torch.int16))
        else:
            assert not (bad & ~near).any(), (name, int((bad & ~near).sum()))
            assert ((out.int() - want.int()).abs()[bad] == 1).all(), name
    else:
        assert torch.equal(E, E2)
        wq, wE = KR.mx_encode(got32)
        assert torch.equal(E, wE), (name, (E != wE).nonzero()[:8].tolist())
        assert torch.equal(out, wq), (name, int((out != wq).sum()))
        if s['regime'].startswith('coded'):
            rq, rE = KR.mx_encode(ref.float())
            assert torch.equal(out, rq) and torch.equal(E, rE), name


def _refused(c, cm, text, **change):
    """The call must fail with `text` in wn_last_error and leave every word of C and of the C
    scales alone."""
    _lib, L = _L()
    keep = []
    op, C, csc = build_op(c, cm, keep)
    for k, v in change.items():
        if k.endswith('_off'):                       # a misaligned base: pointer + bytes
            k = k[:-4]
            v = (getattr(op, k) or 0) + v
        setattr(op, k, v)
    route = ctypes.c_int32(-1)
    status = L.wn_op_gemm_lowp_ex(ctypes.byref(op), ctypes.byref(route),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    msg = L.wn_last_error().decode('utf8', 'replace')
    assert status == -1 and text in msg, (text, change, status, msg)
    pat = (PATTERN, PATTERN16, PATTERN8)[cm]
    assert bool((C == pat).all()), 'a refused call wrote to C'
    assert csc is None or bool((csc == PATTERN).all()), 'a refused call wrote to the C scales'


def test_gemm_lowp_refusals():
    """Everything wn_op_gemm_lowp_ex refuses, before any launch."""
    S = KR._lowp_spec
    T, P = KR.FAM_STORED, KR.FAM_PIPELINED
    b = KR.make_gemm_lowp_case(S(T, 0, 65, 72, 64, (64, 64, 2, 2, 64), resid=1, act=1))
    b0 = KR.make_gemm_lowp_case(S(T, 0, 65, 72, 64, (64, 64, 2, 2, 64)))
    glu = KR.make_gemm_lowp_case(S(T, 0, 63, 128, 64, (64, 128, 2, 2, 64), glu=True))
    mx = KR.make_gemm_lowp_case(S(P, 1, 257, 288, 256, (256, 256, 2, 4, 128), resid=1))
    mx0 = KR.make_gemm_lowp_case(S(P, 1, 257, 288, 256, (256, 256, 2, 4, 128)))
    for c in (b, mx):
        _refused(c, 0, 'null operand', A=None)
        _refused(c, 0, 'empty problem', M=0)
        _refused(c, 0, 'dtype is 1', dtype=3)
        _refused(c, 0, 'c_mode is 0, 1 or 2', c_mode=3)
        _refused(c, 0, 'activation', act=4)
        _refused(c, 0, 'glu is 0 or 1', glu=2)
        _refused(c, 0, 'A and W must be 16-byte aligned', A_off=8)
        _refused(c, 0, 'A and W must be 16-byte aligned', W_off=4)
        _refused(c, 0, 'C must be 16-byte aligned', C_off=4)
        _refused(c, 0, 'bias and residual must be 16-byte aligned', bias_off=4)
        _refused(c, 0, 'bias and residual must be 16-byte aligned', resid_off=8)
        _refused(c, 0, 'lda is smaller than K', lda=c['K'] - 16)
        _refused(c, 0, 'ldc is smaller than the output row', ldc=c['N'] - 4)
        _refused(c, 0, 'ldc must be a multiple of 4', ldc=c['N'] + 2)
        _refused(c, 0, 'ldr is smaller than N', ldr=c['N'] - 4)
        _refused(c, 0, 'ldr must be a multiple of 4', ldr=c['N'] + 2)
        esz = 1 if c is mx else 2
        _refused(c, 0, 'past a_bytes', a_bytes=((c['M'] - 1) * (c['K'] + 16) + c['K']) * esz - 1)
        _refused(c, 0, 'past w_bytes', w_bytes=c['N'] * c['K'] * esz - 1)
        _refused(c, 1 if c is b else 2, 'no residual with a bf16 or MXFP8 C')
    _refused(b, 0, 'K must be a multiple of 32', K=48)
    _refused(b, 0, 'lda must be a multiple of 8', lda=68)
    _refused(b0, 0, 'an MXFP8 C needs MXFP8 operands', c_mode=2)
    _refused(b0, 1, 'ldc must be a multiple of 4', ldc=76)
    _refused(glu, 0, 'bf16 operands and an fp32 C only', c_mode=1)
    _refused(glu, 0, 'N must be a multiple of 64', N=96)
    _refused(glu, 0, 'no activation, residual or alpha', act=1)
    _refused(glu, 0, 'no activation, residual or alpha', alpha=0.5)
    R = torch.zeros(63, 128).cuda()
    _refused(glu, 0, 'no activation, residual or alpha', resid=R.data_ptr(), ldr=128)
    _refused(glu, 0, 'ldc is smaller than the output row', ldc=60)
    _refused(mx0, 0, 'a bf16 C needs bf16 operands', c_mode=1)
    _refused(mx0, 0, 'bf16 operands and an fp32 C only', glu=1)
    for cm in (0, 2):
        _refused(mx0, cm, 'K must be a multiple of 128, at least 256', K=192)
        _refused(mx0, cm, 'K must be a multiple of 128, at least 256', K=128)
        _refused(mx0, cm, 'N must be a multiple of 8', N=284)
        _refused(mx0, cm, 'lda must be a multiple of 16', lda=264)
        _refused(mx0, cm, 'null block scales', a_scale=None)
        _refused(mx0, cm, 'null block scales', w_scale=None)
        _refused(mx0, cm, 'scale arrays must be 4-byte aligned', a_scale_off=2)
        _refused(mx0, cm, 'a_scale_pitch is smaller than M', a_scale_pitch=256)
        _refused(mx0, cm, 'w_scale_pitch is smaller than N', w_scale_pitch=287)
        _refused(mx0, cm, 'past a_scale_bytes', a_scale_bytes=2 * 512 * 4 - 1)
        _refused(mx0, cm, 'past w_scale_bytes', w_scale_bytes=2 * 288 * 4 - 1)
        # an A of 2 GiB: what gemm_bf16p_supported rejects (the sizes are claims, nothing is read)
        _refused(mx0, cm, 'does not take', M=1 << 23, a_bytes=1 << 40, a_scale_pitch=1 << 23,
                 c_scale_pitch=1 << 23, a_scale_bytes=1 << 40, c_scale_bytes=1 << 40)
    _refused(mx0, 2, 'N must be a multiple of 32', N=280)
    _refused(mx0, 2, 'ldc must be a multiple of 4', ldc=296)
    _refused(mx0, 2, 'null C scales', c_scale=None)
    _refused(mx0, 2, 'c_scale_pitch is smaller than M', c_scale_pitch=256)
    _refused(mx0, 2, 'past c_scale_bytes', c_scale_bytes=3 * 512 * 4 - 1)


@pytest.mark.parametrize('K', [32, 160, 256, 544])
@pytest.mark.parametrize('rows', [1, 4, 5, 300])
def test_mx_quantize_ex(rows, K):
    """mx_quantize_kernel with ld = K + 4 and pitch = rows + 3, bit for bit against mx_encode:
    POISON in the pad columns of x, PATTERN8 in q behind row rows - 1, PATTERN in every scale
    byte no (row, block) owns."""
    _lib, L = _L()
    x = KR.mx_quantize_case(rows, K)
    xd = _padded(x, K + 4)
    q = torch.full((rows + 3, K), PATTERN8, dtype=torch.uint8).cuda()
    pitch, nk, nb = rows + 3, _cdiv(K, 128), K // 32
    sc = torch.full((nk, pitch), PATTERN, dtype=torch.int32).cuda()
    _lib.check(L.wn_op_mx_quantize_ex(xd.data_ptr(), K + 4, rows, K, q.data_ptr(), sc.data_ptr(),
                                      pitch, torch.cuda.current_stream().cuda_stream), 'mxq_ex')
    torch.cuda.synchronize()
    wq, wE = KR.mx_encode(x)
    h = sc.cpu()
    assert torch.equal(KR.mx_scale_bytes(h, rows, nb), wE)
    assert torch.equal(q[:rows].cpu(), wq) and bool((q[rows:] == PATTERN8).all())
    own = torch.zeros(nk, pitch, 4, dtype=torch.bool)
    for kb in range(nb):
        own[kb // 4, :rows, kb % 4] = True
    pb = torch.full((nk, pitch), PATTERN, dtype=torch.int32).view(torch.uint8).view(own.shape)
    assert torch.equal(h.view(torch.uint8).view(own.shape)[~own], pb[~own])


def test_mx_quantize_ex_refusals():
    _lib, L = _L()
    x = torch.zeros(8, 68).cuda()
    q = torch.full((8, 64), PATTERN8, dtype=torch.uint8).cuda()
    sc = torch.full((1, 11), PATTERN, dtype=torch.int32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    X, Q, SC = x.data_ptr(), q.data_ptr(), sc.data_ptr()
    for text, args in [('null argument', (None, 68, 8, 64, Q, SC, 11)),
                       ('empty problem', (X, 68, 0, 64, Q, SC, 11)),
                       ('K must be a multiple of 32', (X, 68, 8, 48, Q, SC, 11)),
                       ('ld must be a multiple of 4', (X, 66, 8, 64, Q, SC, 11)),
                       ('ld is smaller than K', (X, 60, 8, 64, Q, SC, 11)),
                       ('pitch is smaller than rows', (X, 68, 8, 64, Q, SC, 7)),
                       ('x must be 16-byte aligned', (X + 4, 68, 7, 64, Q, SC, 11)),
                       ('q and scale must be 4-byte aligned', (X, 68, 8, 64, Q + 2, SC, 11))]:
        status = L.wn_op_mx_quantize_ex(*args, st)
        torch.cuda.synchronize()
        msg = L.wn_last_error().decode('utf8', 'replace')
        assert status == -1 and text in msg, (text, status, msg)
        assert bool((q == PATTERN8).all()) and bool((sc == PATTERN).all())
