"""The six-product kernels (gemm_x6.hip, ffn_x6f.hip, gemm_x6r.hip, gemm_x6r512.hip), one plane
product at a time.  RUN THIS FILE FIRST after reorganising one of them.

One-term probes (tests/x6_probe.py; test_x6_probe.py shows on the CPU that they are sensitive):
every output of the hook is a single product a * w of general fp32 values, the accumulator holds
nothing else but exact zeros and the epilogue adds nothing inexact (bias 0, residual 0, alpha 1),
so the result is a * w to PROBE_RTOL = 2^-21 per element -- a kernel that loses or mis-pairs any
plane product at any k misses that on at least half of the elements it touches.

What sits behind a non-linear epilogue (LayerNorm outputs, the chained GLU, the feed-forward
module with its biases and SiLU) gets the dense yardstick rule of test_gpu_x6.py instead: the
error against fp64 is not larger than that of the same module on v_mfma_f32 GEMMs (wn_op_gemm)
with torch fp32 around them, margin 1.5x on the maximum and 1.2x on the rms."""
import functools

import pytest
import torch

import x6_probe as P
from kernel_refs import glu_perm as _glu_perm

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
KINDS = ('probe_w', 'probe_a')


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _tune:
    """wn_tune_set knobs for one case; back to `default` afterwards."""

    def __init__(self, key, value, default):
        self.key, self.value, self.default = key, value, default

    def __enter__(self):
        _lib, L = _L()
        _lib.check(L.wn_tune_set(self.key, self.value), 'tune')

    def __exit__(self, *exc):
        _L()[1].wn_tune_set(self.key, self.default)


@pytest.fixture(params=[1, 0], ids=['a_fp32', 'a_planes'])
def x6_af32(request):
    """Both forms of wn_op_gemm_x6's A operand: fp32 rows split in registers, and a plane image."""
    with _tune(b'x6_af32', request.param, 0):
        yield request.param


# (tune value, d_model): the GEMM pair at both widths, the kernel with the hidden tensor on chip
# where it exists
FFN_FORMS = [pytest.param(0, 256, id='gemm_pair-256'), pytest.param(0, 512, id='gemm_pair-512'),
             pytest.param(2, 256, id='hidden_on_chip-256')]


@pytest.fixture
def ffn_form(request):
    with _tune(b'ffn_x6f', request.param, 1):
        yield request.param


@functools.lru_cache(maxsize=None)
def _probe(kind, M, N, K, run=0, sample=None):
    """(A, W, ref) of a one-term case, built once and shared (CPU tensors, never modified)."""
    if kind == 'probe_w':
        A, W = P.dense(M, K, 101 + M + K, sample), P.probe_w(N, K, 103 + N + K, run, sample)[0]
    else:
        A, W = P.probe_a(M, K, 107 + M + K, run, sample)[0], P.dense(N, K, 109 + N + K, sample)
    ref = A.double() @ W.double().T          # one exact product per element
    assert (ref != 0).all()
    return A, W, ref


def _rows(kind, K, more=()):
    return (K + 1, ) if kind == 'probe_a' else (33, 130) + tuple(more)


def _check(tag, got, ref, worst):
    """Every element within PROBE_RTOL of the fp64 product; returns the running maximum."""
    got = got.cpu().double()
    rel = (got - ref).abs() / ref.abs()
    bad = int((rel > P.PROBE_RTOL).sum())
    assert bad == 0, (f'{tag}: {bad} of {rel.numel()} elements over 2^-21, max '
                      f'{rel.max().item() / ULP:.1f} x 2^-24')
    return max(worst, rel.max().item())


# ---- wn_op_gemm_x6 --------------------------------------------------------------------------------
def _x6(A, W, bm):
    _lib, L = _L()
    M, K = A.shape
    N = W.shape[0]
    C = torch.full((M, N), float('nan'), device='cuda')
    _lib.check(L.wn_op_gemm_x6(A.data_ptr(), W.data_ptr(), None, None, C.data_ptr(), M, N, K, 1.0,
                               0, bm, 1, _stream()), 'gemm_x6')
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,K', P.GEMM_NK)
@pytest.mark.parametrize('bm', [0, 120, 128, 129, 130, 256])
def test_gemm_x6_one_term(x6_af32, bm, N, K, kind):
    worst = 0.0
    for M in _rows(kind, K, (257, ) if bm == 256 else ()):
        R = N if kind == 'probe_w' else M
        for run in range(P.runs_to_cover(R, K)):
            A, W, ref = _probe(kind, M, N, K, run)
            Ad, Wd = A.cuda(), W.cuda()
            C = _x6(Ad, Wd, bm)
            worst = _check(f'gemm_x6 bm {bm} {M}x{N}x{K} {kind} run {run}', C, ref, worst)
            assert torch.equal(C, _x6(Ad, Wd, bm))             # race screen
    print(f'\n[gemm_x6 bm {bm} N {N} K {K} {kind}] max |err| / |a w| = {worst / ULP:.2f} x 2^-24')


# ---- wn_op_gemm_x6r (K = 256) ---------------------------------------------------------------------
def _x6r(A, W, b, epi, alpha=1.0, x=None, lw=None, lb=None):
    """(C, x_inout, y) of one launch; x_inout starts as `x` (zeros if None)."""
    _lib, L = _L()
    M, N = A.shape[0], W.shape[0]
    C = torch.full((M, N), float('nan'), device='cuda')
    y = torch.full((M, N), float('nan'), device='cuda')
    xo = torch.zeros((M, N), device='cuda') if x is None else x.clone()
    lw = torch.ones(N, device='cuda') if lw is None else lw
    lb = torch.zeros(N, device='cuda') if lb is None else lb
    _lib.check(L.wn_op_gemm_x6r(A.data_ptr(), W.data_ptr(), b.data_ptr(), xo.data_ptr(),
                                lw.data_ptr(), lb.data_ptr(), y.data_ptr(), C.data_ptr(), M, N,
                                epi, alpha, 1e-5, 1, _stream()), 'x6r')
    torch.cuda.synchronize()
    return C, xo, y


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,epi', [(n, 0) for n in P.X6R_N] + [(256, 1)])
def test_gemm_x6r_one_term(N, epi, kind):
    """epi 0: C; epi 1: x_inout (0 + 1 * (a w + 0)); its LayerNorm output is a dense case below."""
    worst = 0.0
    b = torch.zeros(N, device='cuda')
    for M in _rows(kind, 256):
        A, W, ref = _probe(kind, M, N, 256)
        Ad, Wd = A.cuda(), W.cuda()
        outs = [_x6r(Ad, Wd, b, epi)[epi] for _ in range(2)]
        worst = _check(f'x6r epi {epi} {M}x{N} {kind}', outs[0], ref, worst)
        assert torch.equal(outs[0], outs[1])
    print(f'\n[x6r epi {epi} N {N} {kind}] max |err| / |a w| = {worst / ULP:.2f} x 2^-24')


def test_gemm_x6r_glu_value_half_one_term():
    """epi 2 with the gates held at sigmoid(+40) == 1.0f exactly (gate weights 0, gate bias 40):
    the GLU output is the value pre-activation, a single product."""
    d, worst = 256, 0.0
    perm = _glu_perm(d)
    b = torch.cat([torch.zeros(d), torch.full((d, ), 40.0)])[perm].cuda()
    for M in (33, 130):
        A, Wv, ref = _probe('probe_w', M, d, 256)
        W = torch.cat([Wv, torch.zeros(d, 256)])[perm].contiguous().cuda()
        Ad = A.cuda()
        outs = [_x6r(Ad, W, b, 2)[0][:, :d] for _ in range(2)]
        worst = _check(f'x6r GLU values {M}', outs[0], ref, worst)
        assert torch.equal(outs[0], outs[1])
    print(f'\n[x6r epi 2 value half] max |err| / |a w| = {worst / ULP:.2f} x 2^-24')


def test_gemm_x6r_glu_gate_half_one_term():
    """epi 2 with the value pre-activation the constant 1.0 (weights 0, bias 1) and every gate
    pre-activation g a single product in [-20.25, -18.06] (operands in [4.25, 4.5), one of them
    negated): there sigmoid(g) ~ exp(g), so an error of 20 * 2^-17 in g -- a lost low-order
    product -- is a relative error of 1.5e-4 in the output.  Bound: 8x the maximum relative error
    of an fp32 CPU evaluation of sigmoid on the same pre-activations (the fp64-exact products
    rounded to fp32), the margin rule of test_gpu_kernels.py; that fp32 error measures 1.04e-6
    (rounding g to fp32 alone is up to 2^-20 = 9.5e-7 here), so the bound is 8.3e-6; the kernel
    measures 2.9e-6."""
    d, worst = 256, 0.0
    perm = _glu_perm(d)
    b = torch.cat([torch.ones(d), torch.zeros(d)])[perm].cuda()
    for M in (33, 130):
        A, Wg, g64 = _probe('probe_w', M, d, 256, 0, P.sample_range(4.25, 4.5))
        Wg, g64 = -Wg, -g64
        assert g64.min() >= -20.25 and g64.max() <= -18.0
        ref = torch.sigmoid(g64)
        f32 = torch.sigmoid(g64.float()).double()
        e32 = ((f32 - ref).abs() / ref).max().item()
        W = torch.cat([torch.zeros(d, 256), Wg])[perm].contiguous().cuda()
        Ad = A.cuda()
        outs = [_x6r(Ad, W, b, 2)[0][:, :d].cpu() for _ in range(2)]
        err = ((outs[0].double() - ref).abs() / ref).max().item()
        print(f'\n[x6r epi 2 gate half {M}] max rel |err| {err:.2e} / fp32 sigmoid {e32:.2e}')
        assert err <= 8 * e32
        assert torch.equal(outs[0], outs[1])
        worst = max(worst, err)


# ---- wn_op_gemm_x6r512 (K = 512) ------------------------------------------------------------------
def _x6r512(A, W, b, epi, W2, b2, alpha=1.0, x=None, lw=None, lb=None):
    """(C, x_inout, y); C is (M, N) for epi 0 and the (M, 512) GLU output for epi 3."""
    _lib, L = _L()
    M, N = A.shape[0], W.shape[0]
    C = torch.full((M, N), float('nan'), device='cuda')
    y = torch.full((M, N), float('nan'), device='cuda')
    xo = torch.zeros((M, N), device='cuda') if x is None else x.clone()
    lw = torch.ones(N, device='cuda') if lw is None else lw
    lb = torch.zeros(N, device='cuda') if lb is None else lb
    _lib.check(L.wn_op_gemm_x6r512(A.data_ptr(), W.data_ptr(), b.data_ptr(), xo.data_ptr(),
                                   lw.data_ptr(), lb.data_ptr(), y.data_ptr(), W2.data_ptr(),
                                   b2.data_ptr(), C.data_ptr(), M, N, epi, alpha, 1e-5, 1,
                                   _stream()), 'x6r512')
    torch.cuda.synchronize()
    return C, xo, y


@functools.lru_cache(maxsize=None)
def _glu512():
    """Dense pointwise_conv1 weights of the chained epilogue, reference order [values | gates]."""
    g = torch.Generator().manual_seed(512)
    return torch.randn(1024, 512, generator=g) / 512 ** 0.5, torch.randn(1024, generator=g) * 0.3


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N,epi', [(n, 0) for n in P.X6R512_N] + [(512, 1), (512, 3)])
@pytest.mark.parametrize('rows', [32, 64])
def test_gemm_x6r512_one_term(rows, N, epi, kind):
    """epi 0: C; epi 1 / 3: x_inout (epi 3: the one-term probe of its first GEMM; the chained GLU
    GEMM consumes LN(x), which no probe makes exact -- a dense case below)."""
    worst = 0.0
    b = torch.zeros(N, device='cuda')
    perm = _glu_perm(512)
    W2, b2 = (t[perm].contiguous().cuda() for t in _glu512())
    with _tune(b'x6r512_rows', rows, 0):
        for M in _rows(kind, 512):
            A, W, ref = _probe(kind, M, N, 512)
            Ad, Wd = A.cuda(), W.cuda()
            outs = [_x6r512(Ad, Wd, b, epi, W2, b2)[0 if epi == 0 else 1] for _ in range(2)]
            worst = _check(f'x6r512 rows {rows} epi {epi} {M}x{N} {kind}', outs[0], ref, worst)
            assert torch.equal(outs[0], outs[1])
    print(f'\n[x6r512 rows {rows} epi {epi} N {N} {kind}] max |err| / |a w| = '
          f'{worst / ULP:.2f} x 2^-24')


# ---- wn_op_ffn_x6 ---------------------------------------------------------------------------------
def _ffn(X, W1, b1, W2, b2, x, lw, lb, act, alpha):
    """(x_inout, y) of one call; x_inout starts as `x`."""
    _lib, L = _L()
    M, D = X.shape
    F = W1.shape[0]
    xo = x.clone()
    y = torch.full((M, D), float('nan'), device='cuda')
    _lib.check(L.wn_op_ffn_x6(X.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                              b2.data_ptr(), xo.data_ptr(), lw.data_ptr(), lb.data_ptr(),
                              y.data_ptr(), M, D, F, act, alpha, 1e-5, 1, _stream()), 'ffn_x6')
    torch.cuda.synchronize()
    return xo, y


@pytest.mark.parametrize('kind', ['w1', 'w2'])
@pytest.mark.parametrize('F', P.FFN_F)
@pytest.mark.parametrize('ffn_form,D', FFN_FORMS, indirect=['ffn_form'])
def test_ffn_x6_one_term(ffn_form, D, F, kind):
    """ReLU on positive operands (the identity), alpha 1, b1 = b2 = 0, x = 0: x_inout is one
    product per element.  'w1' probes the first contraction (and a0b0 / a1b0 / a2b0 of the
    second), 'w2' all six of the second; see x6_probe.ffn_probe."""
    worst = 0.0
    z = functools.partial(torch.zeros, device='cuda')
    for M in (33, 130):
        for run in range(P.ffn_probe_runs(D, F)):
            X, W1, W2, ref = P.ffn_probe(kind, M, D, F, 211 + M + D + F, run)
            t = [v.cuda() for v in (X, W1, W2)]
            outs = [_ffn(t[0], t[1], z(F), t[2], z(D), z(M, D), torch.ones(D, device='cuda'),
                         z(D), 2, 1.0)[0] for _ in range(2)]
            worst = _check(f'ffn_x6 form {ffn_form} {M} {D} {F} {kind} run {run}', outs[0], ref,
                           worst)
            assert torch.equal(outs[0], outs[1])
    print(f'\n[ffn_x6 form {ffn_form} D {D} F {F} {kind}] max |err| / |a w| = '
          f'{worst / ULP:.2f} x 2^-24')


# ---- dense yardstick rule ------------------------------------------------------------------------
# Measured on an MI355X (max |err| six-product / yardstick; rms six-product / yardstick), the worst
# case of each group -- the tests print all of them:
#   ffn_x6 GEMM pair      x 7.98e-07 / 1.94e-06, 1.34e-07 / 2.06e-07   y 1.00e-06 / 9.65e-07, 1.09e-07 / 1.46e-07
#   ffn_x6 hidden on chip x 4.47e-07 / 2.05e-06, 8.88e-08 / 2.34e-07   y 7.83e-07 / 9.65e-07, 9.43e-08 / 1.46e-07
#   x6r epi 1             x 1.27e-06 / 1.07e-06, 1.23e-07 / 1.47e-07   y 1.22e-06 / 1.22e-06, 1.30e-07 / 1.49e-07
#   x6r epi 2 (GLU)       C 1.79e-06 / 1.65e-06, 1.45e-07 / 1.68e-07
#   x6r512 epi 1 / 3      x 1.84e-06 / 1.37e-06, 1.72e-07 / 2.05e-07   y 1.97e-06 / 1.56e-06, 1.71e-07 / 1.95e-07
#   x6r512 epi 3 (GLU)    C 2.67e-06 / 2.71e-06, 2.26e-07 / 2.66e-07   (32- and 64-row blocks: the same bits)
# With one low-order product taken out of a kernel the rms goes to 8e-07 .. 1.7e-06 (6x .. 10x).
def _f32_gemm(A, W):
    """A W^T on v_mfma_f32 (wn_op_gemm), no epilogue."""
    _lib, L = _L()
    M, K = A.shape
    N = W.shape[0]
    A, W = A.contiguous(), W.contiguous()
    C = torch.empty((M, N), device='cuda')
    _lib.check(L.wn_op_gemm(A.data_ptr(), W.data_ptr(), None, None, C.data_ptr(), M, N, K, 1.0, 0,
                            _stream()), 'gemm')
    torch.cuda.synchronize()
    return C


def _yardstick(tag, got, f32, ref):
    """The project's rule for "this is an fp32 kernel" (test_gpu_x6.py): the error against fp64
    is not larger than the fp32 yardstick's, margin 1.5x on the maximum and 1.2x on the rms."""
    d6, d32 = got.cpu().double() - ref, f32.cpu().double() - ref
    e6, e32 = d6.abs().max().item(), d32.abs().max().item()
    r6, r32 = (d6 ** 2).mean().sqrt().item(), (d32 ** 2).mean().sqrt().item()
    print(f'\n[{tag}] max |err| x6 {e6:.2e} / f32 {e32:.2e}; rms {r6:.2e} / {r32:.2e}')
    assert e6 <= 1.5 * e32 + 1e-7, tag
    assert r6 <= 1.2 * r32 + 1e-8, tag


def _glu(pre, d):
    return pre[:, :d] * torch.sigmoid(pre[:, d:])


@pytest.mark.parametrize('act', ['silu', 'relu'])
@pytest.mark.parametrize('ffn_form,M,D,F', [
    pytest.param(f, *s, id=f'{n}-{s[0]}-{s[1]}-{s[2]}')
    for s in P.FFN_DENSE for f, n in ((0, 'gemm_pair'), (2, 'hidden_on_chip'))
    if f == 0 or s[1] == 256], indirect=['ffn_form'])
def test_ffn_x6_dense_is_an_fp32_module(ffn_form, M, D, F, act):
    fn = {'silu': torch.nn.functional.silu, 'relu': torch.relu}[act]
    cpu = P.ffn_dense_inputs(M, D, F, act)
    X, W1, b1, W2, b2, x, lw, lb = (t.double() for t in cpu)
    xr = x + 0.5 * (fn(X @ W1.T + b1) @ W2.T + b2)
    yr = torch.nn.functional.layer_norm(xr, (D, ), lw, lb, 1e-5)
    X, W1, b1, W2, b2, x, lw, lb = (t.cuda() for t in cpu)
    outs = [_ffn(X, W1, b1, W2, b2, x, lw, lb, {'silu': 1, 'relu': 2}[act], 0.5) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x32 = x + 0.5 * (_f32_gemm(fn(_f32_gemm(X, W1) + b1), W2) + b2)
    y32 = torch.nn.functional.layer_norm(x32, (D, ), lw, lb, 1e-5)
    tag = f'ffn_x6 form {ffn_form} {M} {D} {F} {act}'
    _yardstick(tag + ' x', outs[0][0], x32, xr)
    _yardstick(tag + ' y', outs[0][1], y32, yr)


def _rowln_inputs(M, d, seed):
    """Inputs scaled as test_gpu_ffn_fused.py scales them for the row-block kernels."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, d, generator=g)
    W = torch.randn(d, d, generator=g) / d ** 0.5
    b = torch.randn(d, generator=g) * 0.3
    x = torch.randn(M, d, generator=g)
    lw = 1.0 + 0.2 * torch.randn(d, generator=g)
    lb = 0.1 * torch.randn(d, generator=g)
    W2 = torch.randn(2 * d, d, generator=g) / d ** 0.5      # reference order: [values | gates]
    b2 = torch.randn(2 * d, generator=g) * 0.3
    return A, W, b, x, lw, lb, W2, b2


@pytest.mark.parametrize('M', [33, 130])
@pytest.mark.parametrize('epi', [1, 2])
def test_gemm_x6r_dense_is_an_fp32_kernel(epi, M):
    d = 256
    cpu = _rowln_inputs(M, d, 300 + M + epi)
    A, W, b, x, lw, lb, W2, b2 = (t.double() for t in cpu)
    Ad, Wd, bd, xd, lwd, lbd, W2d, b2d = (t.cuda() for t in cpu)
    tag = f'x6r epi {epi} {M}'
    if epi == 1:
        xr = x + 0.5 * (A @ W.T + b)
        yr = torch.nn.functional.layer_norm(xr, (d, ), lw, lb, 1e-5)
        outs = [_x6r(Ad, Wd, bd, 1, 0.5, xd, lwd, lbd) for _ in range(2)]
        assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
        x32 = xd + 0.5 * (_f32_gemm(Ad, Wd) + bd)
        y32 = torch.nn.functional.layer_norm(x32, (d, ), lwd, lbd, 1e-5)
        _yardstick(tag + ' x', outs[0][1], x32, xr)
        _yardstick(tag + ' y', outs[0][2], y32, yr)
        return
    perm = _glu_perm(d)
    cr = _glu(A @ W2.T + b2, d)
    outs = [_x6r(Ad, W2d[perm].contiguous(), b2d[perm].contiguous(), 2)[0][:, :d]
            for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    _yardstick(tag + ' GLU', outs[0], _glu(_f32_gemm(Ad, W2d) + b2d, d), cr)


@pytest.mark.parametrize('M', [33, 130])
@pytest.mark.parametrize('epi', [1, 3])
@pytest.mark.parametrize('rows', [32, 64])
def test_gemm_x6r512_dense_is_an_fp32_kernel(rows, epi, M):
    d = 512
    cpu = _rowln_inputs(M, d, 500 + M + epi)
    A, W, b, x, lw, lb, W2, b2 = (t.double() for t in cpu)
    Ad, Wd, bd, xd, lwd, lbd, W2d, b2d = (t.cuda() for t in cpu)
    perm = _glu_perm(d)
    xr = x + 0.5 * (A @ W.T + b)
    yr = torch.nn.functional.layer_norm(xr, (d, ), lw, lb, 1e-5)
    with _tune(b'x6r512_rows', rows, 0):
        outs = [_x6r512(Ad, Wd, bd, epi, W2d[perm].contiguous(), b2d[perm].contiguous(), 0.5, xd,
                        lwd, lbd) for _ in range(2)]
    for u, v in zip(*outs):
        assert torch.equal(u, v) or epi == 1 and torch.isnan(u).all()     # (epi 1 writes no C)
    x32 = xd + 0.5 * (_f32_gemm(Ad, Wd) + bd)
    y32 = torch.nn.functional.layer_norm(x32, (d, ), lwd, lbd, 1e-5)
    tag = f'x6r512 rows {rows} epi {epi} {M}'
    _yardstick(tag + ' x', outs[0][1], x32, xr)
    _yardstick(tag + ' y', outs[0][2], y32, yr)
    if epi == 3:
        cr = _glu(yr @ W2.T + b2, d)
        _yardstick(tag + ' GLU', outs[0][0][:, :d], _glu(_f32_gemm(y32, W2d) + b2d, d), cr)
