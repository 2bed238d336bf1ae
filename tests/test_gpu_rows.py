"""Operator tests of the kernels that own a complete row -- the LayerNorm family
(csrc/encoder_kernels.hip), the FFN reduce (csrc/ffn_fused.hip) and the row-LN GEMM
(csrc/gemm_rowln.hip) -- through the hooks wn_op_layernorm_ex / wn_op_layernorm2 /
wn_op_layernorm_mx / wn_op_ffn_reduce_ln / wn_op_gemm_rowln, against the plain fp64 references of
tests/kernel_refs.py (CPU checks: tests/test_kernel_refs.py).

In fp32 mode these kernels run between every pair of GEMMs of every layer; the whole-encoder
comparisons would let through a wrong column-to-lane map of w / b at a width the models do not use,
a write past row M or into the padding between D and the row stride, an eps in the wrong place, a
scale byte of layernorm_mx in the wrong slot of its dword.

Every case: tolerance KR.bound(e_plain, scale) under KR.cap_ok, both from the fp64 reference and
its fp32 evaluation; every output buffer one row longer than needed and pre-filled (KR.POISON, a
fixed pattern for bf16 / byte buffers), every element outside [0, M) x [0, D) must still hold
the fill; every call runs twice on fresh buffers and must give the same bits.

Kernel -> test:
  layernorm_kernel<1..20>              test_layernorm_f32 (all ten widths, strides, in place)
  layernorm_bf16out_kernel             test_layernorm_bf16out
  layernorm2_kernel, _bf16out_kernel   test_layernorm2
  layernorm_mx_kernel                  test_layernorm_mx, test_layernorm_mx_zero_block
  ffn_reduce_ln_kernel<4|8, 0|1|2>     test_ffn_reduce_ln, test_ffn_reduce_ln_counts_every_slice_once
  ffn_reduce_ln_img_kernel<4|8>        test_ffn_reduce_ln_img
  gemm_rowln_kernel                    test_gemm_rowln_packed, test_gemm_rowln_variants
"""
import functools
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead          # scale dwords
PATTERN16 = 0x7fde            # bf16 buffers
PATTERN8 = 0xa5               # byte buffers

LN_WIDTHS = [64, 128, 192, 256, 384, 512, 640, 768, 1024, 1280]
LN_ALL_REGIMES = (192, 256, 640)      # widths that run all five regimes
LN2_WIDTHS = [64, 128, 256, 512, 768, 1024, 1280]
MX_WIDTHS = [256, 512, 768, 1024, 1280]


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def record(name, err, e_plain, scale):
    """Prints the figures of a case (and appends them to the file WN_KERNEL_OPS_RATIOS names),
    then asserts the cap on the yardstick and the bound."""
    b = KR.bound(e_plain, scale)
    ratio = err / b if b > 0 else (0.0 if err == 0 else float('inf'))
    line = f'{name} err={err:.3e} bound={b:.3e} e_plain={e_plain:.3e} scale={scale:.3e} ' \
           f'ratio={ratio:.3f}'
    print(line)
    path = os.environ.get('WN_KERNEL_OPS_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')
    assert KR.cap_ok(e_plain, scale), line
    assert err <= b, line


def _bits(t):
    """A tensor's bytes (NaN-safe, sign-of-zero-exact comparisons)."""
    return t.contiguous().view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def twice(run):
    """run() -> tuple of host tensors (whole buffers); run on fresh buffers twice, bitwise equal."""
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert same_bits(u, v), f'output {i} differs between two runs of the same call'
    return a


def f32_buf(rows, ld, t=None):
    """Device (rows + 1, ld) fp32 buffer of KR.POISON with t in its top left corner."""
    buf = torch.full((rows + 1, ld), KR.POISON, dtype=torch.float32)
    if t is not None:
        buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


def check_fill(buf, M, D, fill, what):
    """Every element of the host buffer outside [0, M) x [0, D) still holds `fill`."""
    ref = torch.full_like(buf, fill)
    out = buf.clone()
    out[:M, :D] = ref[:M, :D]
    assert same_bits(out, ref), f'{what}: a write outside [0, {M}) x [0, {D})'


@functools.lru_cache(maxsize=None)
def rows_case(regime, M, D):
    c = KR.make_rows_case(regime, M, D, seed=1000 * KR.ROW_REGIMES.index(regime) + D + M)
    return c, KR.rows_refs(c), KR.rows2_refs(c)


def ln_regimes(D):
    return KR.ROW_REGIMES if D in LN_ALL_REGIMES else ('unit', 'offset')


# ---------------------------------------------------------------------------------------------
# LayerNorm


def run_ln(x, w, b, eps, ldx, ldy, bf16=False, inplace=False):
    """wn_op_layernorm_ex on x (M, D).  Returns the whole host output buffer (M + 1, ldy): fp32,
    or int16 (bf16 bits).  inplace: y is the x buffer (row stride ldx)."""
    _lib, L = _L()
    M, D = x.shape
    xd, wd, bd = f32_buf(M, ldx, x), w.cuda(), b.cuda()
    if inplace:
        yd, ldy = xd, ldx
    elif bf16:
        yd = torch.full((M + 1, ldy), PATTERN16, dtype=torch.int16, device='cuda')
    else:
        yd = f32_buf(M, ldy)
    _lib.check(L.wn_op_layernorm_ex(xd.data_ptr(), ldx, wd.data_ptr(), bd.data_ptr(),
                                    yd.data_ptr(), ldy, M, D, eps, int(bf16), _stream()), 'ln')
    torch.cuda.synchronize()
    out = yd.cpu()
    check_fill(out, M, D, PATTERN16 if bf16 else KR.POISON, 'layernorm y')
    if not inplace:
        assert same_bits(xd.cpu(), f32_buf(M, ldx, x).cpu()), 'layernorm changed x'
    return out


@pytest.mark.parametrize('pad', [(0, 0), (4, 8)], ids=['packed', 'strided'])
@pytest.mark.parametrize('D', LN_WIDTHS)
def test_layernorm_f32(D, pad):
    ldx, ldy = D + pad[0], D + pad[1]
    for M in (1, 4, 5, 37):
        for regime in ln_regimes(D):
            c, (ref, e, scale), _ = rows_case(regime, M, D)
            y, = twice(lambda: (run_ln(c['x'], c['w'], c['b'], c['eps'], ldx, ldy), ))
            y = y[:M, :D]
            record(f'layernorm D={D} M={M} {regime} ld={ldx}/{ldy}',
                   (y.double() - ref).abs().max().item(), e, scale)
            # y == x, as final_ffn calls it
            yi, = twice(lambda: (run_ln(c['x'], c['w'], c['b'], c['eps'], ldx, ldx,
                                        inplace=True), ))
            assert same_bits(yi[:M, :D], y), f'in place differs D={D} M={M} {regime}'


@pytest.mark.parametrize('D', LN_WIDTHS)
def test_layernorm_bf16out(D):
    """The bf16 store is the round-to-nearest-even conversion of the fp32 kernel's row."""
    for M in (1, 5, 37):
        for regime in ('unit', 'offset'):
            c = rows_case(regime, M, D)[0]
            y32 = run_ln(c['x'], c['w'], c['b'], c['eps'], D + 4, D + 8)[:M, :D]
            y16, = twice(lambda: (run_ln(c['x'], c['w'], c['b'], c['eps'], D + 4, D + 8,
                                         bf16=True), ))
            assert same_bits(y16[:M, :D], y32.bfloat16().view(torch.int16)), (D, M, regime)


def run_ln2(c, bf16, alias):
    """wn_op_layernorm2 on a rows case.  Returns (y1, y2) whole host buffers (M + 1, D)."""
    _lib, L = _L()
    M, D = c['M'], c['D']
    xd = f32_buf(M, D, c['x'])
    y1 = xd if alias else f32_buf(M, D)
    if bf16:
        y2 = torch.full((M + 1, D), PATTERN16, dtype=torch.int16, device='cuda')
    else:
        y2 = f32_buf(M, D)
    dev = [c[k].cuda() for k in ('w', 'b', 'w2', 'b2')]
    _lib.check(L.wn_op_layernorm2(xd.data_ptr(), *[t.data_ptr() for t in dev], y1.data_ptr(),
                                  y2.data_ptr(), M, D, c['eps'], int(bf16), _stream()), 'ln2')
    torch.cuda.synchronize()
    o1, o2 = y1.cpu(), y2.cpu()
    check_fill(o1, M, D, KR.POISON, 'layernorm2 y1')
    check_fill(o2, M, D, PATTERN16 if bf16 else KR.POISON, 'layernorm2 y2')
    if not alias:
        assert same_bits(xd.cpu(), f32_buf(M, D, c['x']).cpu()), 'layernorm2 changed x'
    return o1, o2


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16out'])
@pytest.mark.parametrize('D', LN2_WIDTHS)
def test_layernorm2(D, bf16):
    """y1 and y2 are the bits of two wn_op_layernorm calls (the kernels share ln_inplace), and
    y2 is LN(LN(x)) in fp64 within the bound."""
    for M in (1, 5, 37):
        for regime in ('unit', 'offset'):
            c, _, (ref2, e2, scale2) = rows_case(regime, M, D)
            want1 = run_ln(c['x'], c['w'], c['b'], c['eps'], D, D)[:M, :D]
            want2 = run_ln(want1, c['w2'], c['b2'], c['eps'], D, D)[:M, :D]
            record(f'layernorm2 D={D} M={M} {regime}',
                   (want2.double() - ref2).abs().max().item(), e2, scale2)
            if bf16:
                want2 = want2.bfloat16().view(torch.int16)
            for alias in (False, True):
                y1, y2 = twice(lambda: run_ln2(c, bf16, alias))
                assert same_bits(y1[:M, :D], want1), f'y1 D={D} M={M} {regime} alias={alias}'
                assert same_bits(y2[:M, :D], want2), f'y2 D={D} M={M} {regime} alias={alias}'


def scale_bytes(sc, M):
    """scale dwords [D/128][pitch] (host int32) -> E bytes [M][D/32]: byte (c >> 5) & 3 of dword
    [c >> 7][row]."""
    s = sc.numpy().view(np.uint32)
    nblk = 4 * s.shape[0]
    out = np.zeros((M, nblk), np.uint8)
    for kb in range(nblk):
        out[:, kb] = (s[kb // 4, :M] >> (8 * (kb % 4))) & 0xff
    return out


def run_ln_mx(x, w, b, eps, ldx, pitch):
    """wn_op_layernorm_mx.  Returns (q (M + 1, D) uint8, scale (D / 128, pitch) int32) on the
    host."""
    _lib, L = _L()
    M, D = x.shape
    xd, wd, bd = f32_buf(M, ldx, x), w.cuda(), b.cuda()
    q = torch.full((M + 1, D), PATTERN8, dtype=torch.uint8, device='cuda')
    sc = torch.full((D // 128, pitch), PATTERN, dtype=torch.int32, device='cuda')
    _lib.check(L.wn_op_layernorm_mx(xd.data_ptr(), ldx, wd.data_ptr(), bd.data_ptr(),
                                    q.data_ptr(), sc.data_ptr(), pitch, M, D, eps, _stream()),
               'ln_mx')
    torch.cuda.synchronize()
    q, sc = q.cpu(), sc.cpu()
    check_fill(q, M, D, PATTERN8, 'layernorm_mx q')
    assert (sc[:, M:] == PATTERN).all(), 'layernorm_mx: scale rows >= M changed'
    assert same_bits(xd.cpu(), f32_buf(M, ldx, x).cpu()), 'layernorm_mx changed x'
    return q, sc


def check_ln_mx(c, what):
    from oracle import wenet_oracle as O
    _lib, L = _L()
    M, D = c['M'], c['D']
    y = run_ln(c['x'], c['w'], c['b'], c['eps'], D + 4, D)[:M, :D].contiguous()
    q, sc = twice(lambda: run_ln_mx(c['x'], c['w'], c['b'], c['eps'], D + 4, M + 3))
    rq, rE = O.mx_quantize(y)
    np.testing.assert_array_equal(scale_bytes(sc, M), rE.numpy(), err_msg=what)
    np.testing.assert_array_equal(q[:M].numpy(), rq.view(torch.uint8).numpy(), err_msg=what)
    # ... and the library's own quantiser on the same rows
    yd = y.cuda()
    gq = torch.full((M, D), PATTERN8, dtype=torch.uint8, device='cuda')
    gs = torch.full((D // 128, M), PATTERN, dtype=torch.int32, device='cuda')
    _lib.check(L.wn_op_mx_quantize(yd.data_ptr(), M, D, gq.data_ptr(), gs.data_ptr(), _stream()),
               'mxq')
    torch.cuda.synchronize()
    assert same_bits(gq.cpu(), q[:M]), what
    assert same_bits(gs.cpu(), sc[:, :M].contiguous()), what
    return rE


@pytest.mark.parametrize('D', MX_WIDTHS)
def test_layernorm_mx(D):
    """Elements and scale bytes are the oracle's quantisation of the fp32 kernel's rows (held to
    fp64 by test_layernorm_f32), bit for bit."""
    for M in (1, 5, 37):
        for regime in ('unit', 'cols'):
            check_ln_mx(rows_case(regime, M, D)[0], f'D={D} M={M} {regime}')


@pytest.mark.parametrize('D', [256, 1280])
def test_layernorm_mx_zero_block(D):
    """w = b = 0 over one whole 32-column block: amax 0, scale byte 0 (the oracle defines it:
    test_kernel_refs.py::test_oracle_defines_the_scale_of_an_all_zero_mx_block)."""
    c = dict(rows_case('unit', 5, D)[0])
    blk = D // 32 - 3
    c['w'], c['b'] = c['w'].clone(), c['b'].clone()
    c['w'][32 * blk:32 * blk + 32] = 0.0
    c['b'][32 * blk:32 * blk + 32] = 0.0
    rE = check_ln_mx(c, f'zero block D={D}')
    assert (rE[:, blk] == 0).all() and (rE[:, blk - 1] > 0).all()


# ---------------------------------------------------------------------------------------------
# FFN reduce


def run_ffn_reduce(c, mode, img=False):
    """wn_op_ffn_reduce_ln on a case of KR.make_ffn_reduce_case (or a dict with the same keys).
    Returns host (x (M + 1, D), y (M + 1, D)) or, img, (x, image bytes + 3072 more)."""
    _lib, L = _L()
    M, D, S = c['M'], c['D'], c['S']
    xd = f32_buf(M, D, c['x'])
    # one slice more than S, poisoned: a slice counted past S shows
    Pd = torch.full((S + 1, M, D), KR.POISON, dtype=torch.float32)
    Pd[:S] = c['P']
    Pd = Pd.cuda()
    dev = [c[k].cuda() for k in ('fb2', 'w', 'b', 'w2', 'b2')]
    b2, w, b, w2, bb2 = [t.data_ptr() for t in dev]
    if img:
        nbytes = KR.x3_image_bytes(M, D)
        y3 = torch.full((nbytes + 3072, ), PATTERN8, dtype=torch.uint8, device='cuda')
        _lib.check(L.wn_op_ffn_reduce_ln(xd.data_ptr(), Pd.data_ptr(), S, b2, c['alpha'], w, b,
                                         w2, bb2, None, y3.data_ptr(), nbytes, M, D, c['eps'], 1,
                                         _stream()), 'ffn_reduce_ln_img')
        out = y3
    else:
        yd = f32_buf(M, D)
        _lib.check(L.wn_op_ffn_reduce_ln(xd.data_ptr(), Pd.data_ptr(), S, b2, c['alpha'], w, b,
                                         w2 if mode == 1 else None, bb2 if mode == 1 else None,
                                         yd.data_ptr(), None, 0, M, D, c['eps'], mode, _stream()),
                   'ffn_reduce_ln')
        out = yd
    torch.cuda.synchronize()
    xo, out = xd.cpu(), out.cpu()
    check_fill(xo, M, D, KR.POISON, 'ffn_reduce_ln x')
    if not img:
        check_fill(out, 0 if mode == 2 else M, D, KR.POISON, 'ffn_reduce_ln y')
    return xo, out


@functools.lru_cache(maxsize=None)
def ffn_case(M, D, S, alpha):
    return KR.make_ffn_reduce_case(M, D, S, alpha, seed=7 * M + D + 31 * S + int(alpha * 2))


@pytest.mark.parametrize('S', [1, 7, 8, 9, 16, 32])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('D', [256, 512])
def test_ffn_reduce_ln(D, mode, S):
    """S below, at and past one round of eight slice loads, and whole rounds."""
    for M in (1, 4, 5, 9):
        for alpha in (0.5, 16.0):
            c = ffn_case(M, D, S, alpha)
            (rx, ry), ex, ey = KR.ffn_reduce_refs(c, mode)
            x, y = twice(lambda: run_ffn_reduce(c, mode))
            name = f'ffn_reduce_ln D={D} mode={mode} S={S} M={M} alpha={alpha}'
            record(name + ' x', (x[:M].double() - rx).abs().max().item(), *ex)
            if mode != 2:
                record(name + ' y', (y[:M].double() - ry).abs().max().item(), *ey)


@pytest.mark.parametrize('S', [7, 8, 9, 16])
@pytest.mark.parametrize('D', [256, 512])
def test_ffn_reduce_ln_counts_every_slice_once(D, S):
    """P[s] = 2^s, x = 0, b2 = 0, alpha = 1: the new x is 2^S - 1 in every element, exactly."""
    M = 5
    c = dict(ffn_case(M, D, S, 0.5))
    c['P'] = (2.0 ** torch.arange(S, dtype=torch.float32)).view(S, 1, 1).expand(S, M, D).contiguous()
    c['x'], c['fb2'], c['alpha'] = torch.zeros(M, D), torch.zeros(D), 1.0
    x, _ = twice(lambda: run_ffn_reduce(c, 0))
    assert same_bits(x[:M], torch.full((M, D), float(2 ** S - 1)))


@pytest.mark.parametrize('S', [1, 9])
@pytest.mark.parametrize('M', [1, 8, 9, 33, 37])
@pytest.mark.parametrize('D', [256, 512])
def test_ffn_reduce_ln_img(D, M, S):
    """Blocks of 8 rows, a 32-row tile boundary, a partly filled last tile: x as mode 1 leaves
    it, the planes the exact split of mode 1's y, every image byte of the rows >= M untouched."""
    c = ffn_case(M, D, S, 0.5)
    x1, y1 = run_ffn_reduce(c, 1)
    x, img = twice(lambda: run_ffn_reduce(c, 1, img=True))
    assert same_bits(x, x1)
    img = img.numpy()
    h = KR.x3_decode(img, M, D)
    y = y1[:M].numpy()
    assert np.array_equal(((h[0] + h[1]) + h[2]).view(np.uint32), y.view(np.uint32))
    h0 = torch.from_numpy(y).bfloat16().float().numpy()
    h1 = torch.from_numpy(y - h0).bfloat16().float().numpy()
    assert np.array_equal(h[0].view(np.uint32), h0.view(np.uint32))
    assert np.array_equal(h[1].view(np.uint32), h1.view(np.uint32))
    owned = np.zeros(img.size, bool)
    off = KR.x3_offsets(M, D).reshape(-1)
    owned[off] = True
    owned[off + 1] = True
    assert (img[~owned] == PATTERN8).all(), 'an image byte outside the rows < M changed'


# ---------------------------------------------------------------------------------------------
# row-LN GEMM


def run_gemm_rowln(c, bias=True, resid=True, alpha=1.0, strided=False, resid_is_x=False,
                   y_is_a=False):
    """wn_op_gemm_rowln on a case of KR.make_gemm_rowln_case.  Returns host (x_out (M + 1, ldx),
    y (M + 1, ldy))."""
    _lib, L = _L()
    M, K = c['M'], c['K']
    lda, ldr, ldx, ldy = (K + 4, 260, 264, 268) if strided else (K, 256, 256, 256)
    Ad = f32_buf(M, lda, c['A'])
    Wd = c['W'].cuda()
    bd = c['bias'].cuda() if bias else None
    if resid_is_x:
        assert resid and ldr == ldx
        xd = f32_buf(M, ldx, c['resid'])
        rd = xd
    else:
        xd = f32_buf(M, ldx)
        rd = f32_buf(M, ldr, c['resid']) if resid else None
    if y_is_a:
        assert lda == ldy
        yd = Ad
    else:
        yd = f32_buf(M, ldy)
    lw, lb = c['ln_w'].cuda(), c['ln_b'].cuda()
    _lib.check(L.wn_op_gemm_rowln(Ad.data_ptr(), lda, Wd.data_ptr(), _ptr(bd), _ptr(rd), ldr,
                                  alpha, xd.data_ptr(), ldx, lw.data_ptr(), lb.data_ptr(),
                                  c['eps'], yd.data_ptr(), ldy, M, K, _stream()), 'gemm_rowln')
    torch.cuda.synchronize()
    xo, yo = xd.cpu(), yd.cpu()
    check_fill(xo, M, 256, KR.POISON, 'gemm_rowln x_out')
    check_fill(yo, M, 256, KR.POISON, 'gemm_rowln y')
    if not y_is_a:
        assert same_bits(Ad.cpu(), f32_buf(M, lda, c['A']).cpu()), 'gemm_rowln changed A'
    if rd is not None and not resid_is_x:
        assert same_bits(rd.cpu(), f32_buf(M, ldr, c['resid']).cpu()), 'gemm_rowln changed resid'
    return xo, yo


@functools.lru_cache(maxsize=None)
def rowln_case(M, K):
    return KR.make_gemm_rowln_case(M, K, seed=M + K)


@functools.lru_cache(maxsize=None)
def rowln_refs(M, K, bias, resid, alpha):
    return KR.gemm_rowln_refs(rowln_case(M, K), bias, resid, alpha)


def check_gemm_rowln(M, K, bias=True, resid=True, alpha=1.0, **kw):
    c = rowln_case(M, K)
    (rx, ry), ex, ey = rowln_refs(M, K, bias, resid, alpha)
    x, y = twice(lambda: run_gemm_rowln(c, bias, resid, alpha, **kw))
    name = f'gemm_rowln M={M} K={K} bias={int(bias)} resid={int(resid)} alpha={alpha} {kw}'
    record(name + ' x', (x[:M, :256].double() - rx).abs().max().item(), *ex)
    record(name + ' y', (y[:M, :256].double() - ry).abs().max().item(), *ey)
    return x[:M, :256], y[:M, :256]


@pytest.mark.parametrize('M', [1, 31, 32, 33, 95])
@pytest.mark.parametrize('K', [96, 128, 256, 512])
def test_gemm_rowln_packed(K, M):
    """K = 96 is three stages, exactly the number pre-issued; M around the 32-row block.  With
    resid == x_out (the model's form) the bits are those of the unaliased call."""
    x, y = check_gemm_rowln(M, K, alpha=0.5)
    xa, ya = check_gemm_rowln(M, K, alpha=0.5, resid_is_x=True)
    assert same_bits(xa, x) and same_bits(ya, y)


@pytest.mark.parametrize('K,M', [(96, 33), (256, 95)])
def test_gemm_rowln_variants(K, M):
    check_gemm_rowln(M, K, bias=False)
    check_gemm_rowln(M, K, resid=False)
    check_gemm_rowln(M, K, bias=False, resid=False, alpha=0.5)
    x, y = check_gemm_rowln(M, K, alpha=1.0)
    xs, ys = check_gemm_rowln(M, K, alpha=1.0, strided=True)
    assert same_bits(xs, x) and same_bits(ys, y)      # the strides change no arithmetic
    check_gemm_rowln(M, K, bias=False, alpha=0.5, strided=True)


@pytest.mark.parametrize('M', [33, 95])
def test_gemm_rowln_y_over_a(M):
    """K = 256, lda == ldy: y may be A (a block reads only the rows it writes)."""
    x, y = check_gemm_rowln(M, 256, alpha=0.5)
    xa, ya = check_gemm_rowln(M, 256, alpha=0.5, y_is_a=True)
    assert same_bits(xa, x) and same_bits(ya, y)
    xb, yb = check_gemm_rowln(M, 256, alpha=0.5, y_is_a=True, resid_is_x=True)
    assert same_bits(xb, x) and same_bits(yb, y)


# ---------------------------------------------------------------------------------------------
# rejections: every call below stops at the host checks, nothing is launched


def rejection_calls(L, p, s=None):
    """{hook: [(what, call, words of the message)]}: calls the hooks must refuse.  p: any address
    that is not null (a refused call never uses it)."""
    eps = 1e-5
    calls = {}

    def ln(x=p, ldx=256, w=p, b=p, y=p, ldy=256, M=4, D=256, bf16=0):
        return lambda: L.wn_op_layernorm_ex(x, ldx, w, b, y, ldy, M, D, eps, bf16, s)
    calls['layernorm_ex'] = [
        ('x null', ln(x=None), 'null'), ('w null', ln(w=None), 'null'),
        ('b null', ln(b=None), 'null'), ('y null', ln(y=None), 'null'),
        ('M = 0', ln(M=0), 'empty'), ('M < 0', ln(M=-1), 'empty'),
        ('width 320', ln(D=320, ldx=320, ldy=320), 'width'), ('width 0', ln(D=0), 'width'),
        ('width 1536', ln(D=1536, ldx=1536, ldy=1536), 'width'),
        ('ldx < D', ln(ldx=252), 'stride'), ('ldy < D', ln(ldy=252), 'stride'),
        ('ldx % 4', ln(ldx=258), 'stride'), ('ldy % 4', ln(ldy=257), 'stride'),
        ('ldy < D, bf16', ln(ldy=128, bf16=1), 'stride'),
    ]

    def ln2(x=p, w1=p, b1=p, w2=p, b2=p, y1=p, y2=p, M=4, D=256, bf16=0):
        return lambda: L.wn_op_layernorm2(x, w1, b1, w2, b2, y1, y2, M, D, eps, bf16, s)
    calls['layernorm2'] = [(f'{k} null', ln2(**{k: None}), 'null')
                           for k in ('x', 'w1', 'b1', 'w2', 'b2', 'y1', 'y2')] + [
        ('M = 0', ln2(M=0), 'empty'), ('width 192', ln2(D=192), 'width'),
        ('width 384, bf16', ln2(D=384, bf16=1), 'width'), ('width 640', ln2(D=640), 'width'),
    ]

    def mx(x=p, ldx=256, w=p, b=p, q=p, sc=p, pitch=4, M=4, D=256):
        return lambda: L.wn_op_layernorm_mx(x, ldx, w, b, q, sc, pitch, M, D, eps, s)
    calls['layernorm_mx'] = [(f'{k} null', mx(**{k: None}), 'null')
                             for k in ('x', 'w', 'b', 'q', 'sc')] + [
        ('M = 0', mx(M=0, pitch=0), 'empty'), ('width 128', mx(D=128), 'width'),
        ('width 384', mx(D=384, ldx=384), 'width'), ('width 1536', mx(D=1536, ldx=1536), 'width'),
        ('ldx < D', mx(ldx=252), 'stride'), ('ldx % 4', mx(ldx=258), 'stride'),
        ('pitch < M', mx(pitch=3), 'pitch'),
    ]

    def red(x=p, P=p, S=2, b2=p, w=p, b=p, w2=p, bb2=p, y=p, y3=None, y3_bytes=0, M=4, D=256,
            mode=1):
        return lambda: L.wn_op_ffn_reduce_ln(x, P, S, b2, 0.5, w, b, w2, bb2, y, y3, y3_bytes, M,
                                             D, eps, mode, s)
    img = KR.x3_image_bytes(4, 256)
    calls['ffn_reduce_ln'] = [(f'{k} null', red(**{k: None}), 'null')
                              for k in ('x', 'P', 'b2', 'w', 'b', 'w2', 'bb2', 'y')] + [
        ('y null, mode 0', red(y=None, mode=0), 'null'),
        ('M = 0', red(M=0), 'empty'), ('width 128', red(D=128), 'width'),
        ('width 768', red(D=768), 'width'), ('S = 0', red(S=0), 'S must'),
        ('S < 0', red(S=-8), 'S must'), ('mode 3', red(mode=3), 'mode'),
        ('mode -1', red(mode=-1), 'mode'),
        ('image, mode 0', red(y3=p, y3_bytes=img, mode=0), 'mode 1'),
        ('image, mode 2', red(y3=p, y3_bytes=img, mode=2), 'mode 1'),
        ('image too small', red(y3=p, y3_bytes=img - 1), 'y3_bytes'),
        ('image, negative size', red(y3=p, y3_bytes=-1), 'y3_bytes'),
        ('image, w2 null', red(y3=p, y3_bytes=img, w2=None), 'null'),
    ]

    def rl(A=p, lda=256, W=p, bias=p, resid=p, ldr=256, x=p, ldx=256, lw=p, lb=p, y=p, ldy=256,
           M=4, K=256):
        return lambda: L.wn_op_gemm_rowln(A, lda, W, bias, resid, ldr, 1.0, x, ldx, lw, lb, eps, y,
                                          ldy, M, K, s)
    calls['gemm_rowln'] = [(f'{k} null', rl(**{k: None}), 'null')
                           for k in ('A', 'W', 'x', 'lw', 'lb', 'y')] + [
        ('M = 0', rl(M=0), 'empty'), ('K % 32', rl(K=112, lda=112), 'K must'),
        ('K = 64', rl(K=64), 'K must'), ('K = 0', rl(K=0), 'K must'),
        ('lda < K', rl(lda=252), 'lda'), ('lda % 4', rl(lda=258), 'lda'),
        ('ldr < 256', rl(ldr=252), 'ldr'), ('ldx < 256', rl(ldx=252), 'ldr'),
        ('ldy < 256', rl(ldy=128), 'ldr'),
        ('A of 2 GiB', rl(M=2 ** 21, lda=256), '2 GiB'),
    ]
    return calls


@pytest.mark.parametrize('hook', ['layernorm_ex', 'layernorm2', 'layernorm_mx', 'ffn_reduce_ln',
                                  'gemm_rowln'])
def test_rejections(hook):
    """The refused calls get a real buffer, large enough for any of them, that must stay as it
    was."""
    _lib, L = _L()
    buf = torch.full((1 << 20, ), KR.POISON, dtype=torch.float32, device='cuda')
    for what, call, words in rejection_calls(L, buf.data_ptr(), _stream())[hook]:
        assert call() != 0, f'{hook}: {what} was accepted'
        msg = L.wn_last_error().decode()
        assert words in msg, f'{hook}: {what}: "{msg}"'
    torch.cuda.synchronize()
    assert (buf == KR.POISON).all()
