"""The skinny GEMM of the decoder step (csrc/gemm_skinny.hip, wn_op_gemm_skinny) against fp64.

C[M, N] = resid + act(A[M, K] W[N, K]^T + bias), M <= 256: every block height 1..8 tiles (M not a
multiple of 32, M = 1), N not a multiple of the 128-column block nor of 4, K from one tile to
tile counts the split does not divide (K = 384: 12 fp32 tiles, 6 bf16 tiles, split 5), the
auto split, no split and a forced one, the four epilogues, fp32 weights and the bf16 image.

Tolerance: the project's rule, kernel_refs.bound(e_plain, scale[, bf16]) -- e_plain is the error
of a plain torch fp32 evaluation of the same case (with the bf16 image: of its bf16-rounded
operands) against fp64, scale = max |C|.  The operand buffers carry POISON rows behind M / N and
the C buffer sentinel rows behind M: nothing of either may show.  Two calls give the same bits
(the split-K sum is ordered; the beam search's token parity depends on it)."""
import math

import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

MS = (1, 7, 33, 160, 256)
NS = (64, 211, 307, 1280)
KS = (32, 384, 1280, 1536)
SPLITS = (0, 1, 5)
EPILOGUES = ('none', 'bias_gelu', 'bias_relu', 'bias_resid')
ACT = {'none': 0, 'bias_gelu': 3, 'bias_relu': 2, 'bias_resid': 0}
SENTINEL = 777.0


def _case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    return A, W, bias, resid


def _plain(mm, bias, resid, epi):
    """The plain formula on the product `mm` = A W^T, in its dtype (the reference's own
    operations)."""
    dtype = mm.dtype
    y = mm
    if epi != 'none':
        y = y + bias.to(dtype)
    if epi == 'bias_gelu':
        y = torch.nn.functional.gelu(y)          # exact (erf) form
    if epi == 'bias_relu':
        y = torch.relu(y)
    if epi == 'bias_resid':
        y = y + resid.to(dtype)
    return y


def _run(L, dev, M, N, K, epi, w_bf16, split):
    """-> (C rows [0, M), the sentinel rows behind them), operands padded with POISON."""
    A, W, bias, resid = dev
    Ap = torch.full((M + 3, K), KR.POISON, device='cuda')
    Ap[:M] = A
    Wp = torch.full((N + 5, K), KR.POISON, device='cuda')
    Wp[:N] = W
    bp = torch.full((N + 5, ), KR.POISON, device='cuda')
    bp[:N] = bias
    rp = torch.full((M + 3, N), KR.POISON, device='cuda')
    rp[:M] = resid
    C = torch.full((M + 2, N), SENTINEL, device='cuda')
    st = L.wn_op_gemm_skinny(Ap.data_ptr(), Wp.data_ptr(),
                             bp.data_ptr() if epi != 'none' else None,
                             rp.data_ptr() if epi == 'bias_resid' else None, C.data_ptr(),
                             M, N, K, ACT[epi], int(w_bf16), split,
                             torch.cuda.current_stream().cuda_stream)
    assert st == 0, L.wn_last_error()
    torch.cuda.synchronize()
    return C[:M].cpu(), C[M:].cpu()


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_gemm_skinny_vs_fp64(M, N, K):
    from wenet_amd import _lib
    L = _lib.lib()
    host = _case(M, N, K, seed=M * 1000003 + N * 1009 + K)
    dev = tuple(t.cuda() for t in host)
    A, W, bias, resid = host
    worst = {}
    mm64 = A.double() @ W.double().t()      # computed once, shared by every epilogue below
    for w_bf16 in (False, True):
        Ar, Wr = (KR.bf16_representable(A), KR.bf16_representable(W)) if w_bf16 else (A, W)
        mm32 = Ar @ Wr.t()
        for epi in EPILOGUES:
            ref = _plain(mm64, bias, resid, epi)
            scale = ref.abs().max().item()
            e_plain = (_plain(mm32, bias, resid, epi).double() - ref).abs().max().item()
            assert KR.cap_ok(e_plain, scale, w_bf16), (e_plain, scale)
            tol = KR.bound(e_plain, scale, w_bf16)
            for split in SPLITS:
                got, tail = _run(L, dev, M, N, K, epi, w_bf16, split)
                what = (M, N, K, epi, 'bf16' if w_bf16 else 'fp32', split)
                assert torch.isfinite(got).all() and got.abs().max().item() < 1e6, what
                assert (tail == SENTINEL).all(), (what, 'rows behind M were written')
                err = (got.double() - ref).abs().max().item()
                print(f'skinny {what}: err {err:.3e} e_plain {e_plain:.3e} bound {tol:.3e}')
                assert err <= tol, (what, err, e_plain, tol)
                worst[(w_bf16, split)] = max(worst.get((w_bf16, split), 0.0), err / tol)
                if epi == 'bias_gelu':
                    again, _ = _run(L, dev, M, N, K, epi, w_bf16, split)
                    assert torch.equal(got, again), (what, 'two runs differ')
    assert worst


def test_gemm_skinny_refuses_more_than_256_rows():
    from wenet_amd import _lib
    L = _lib.lib()
    A = torch.zeros(257, 64, device='cuda')
    W = torch.zeros(64, 64, device='cuda')
    C = torch.full((257, 64), SENTINEL, device='cuda')
    st = L.wn_op_gemm_skinny(A.data_ptr(), W.data_ptr(), None, None, C.data_ptr(), 257, 64, 64,
                             0, 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st != 0 and b'256' in L.wn_last_error()
    assert (C == SENTINEL).all()
