"""One-term probes of the six-product kernels (gemm_x6.hip, ffn_x6f.hip, gemm_x6r.hip,
gemm_x6r512.hip): pure torch on the CPU, shared by test_x6_probe.py (which shows that the
instrument is sensitive) and test_gpu_x6_products.py (which points it at the kernels).

Every fp32 operand of those kernels is split exactly into three bf16 planes (csrc/x6.h split3,
restated as oracle.wenet_oracle.x6_planes) and six of the nine plane products are accumulated in
fp32: a0b0, a0b1, a1b0, a1b1, a0b2, a2b0.  A rewrite of such a kernel re-derives which plane of A
meets which plane of W at which k; the characteristic mistake is a missing or mis-paired
low-order product, about 2^-17 of a term, which a dense GEMM against fp64 hides under the
rounding noise of a K-term fp32 sum.

The probe removes that noise.  One operand is ONE-TERM (exactly one non-zero per row), the other
is dense, both hold general fp32 values (all three planes non-zero), so every output is a single
product  C[m, n] = a * w  in which all six plane products take part and next to which the
accumulator holds nothing but exact zeros.

The bound.  The six plane products are exact in fp32 (8 x 8 significand bits), the three omitted
ones (a1b2, a2b1, a2b2) are below 2^-25 of a*w together, and five fp32 additions add at most
5 * 2^-24 relative error, so

    |got - a*w| <= PROBE_RTOL * |a*w|,   PROBE_RTOL = 2^-21  (8 ulp),

per element against the fp64 product, no element excluded.  The CPU emulation stays within
1.5 * 2^-24 summing the small products first (what the kernels do) and 4.7 * 2^-24 in the
reverse order; the kernels themselves measure at most 2.6 * 2^-24 on an MI355X.  With a0b2, a1b1
or a2b0 omitted about three quarters of the elements exceed the bound (errors up to 2^-17), with
a0b1 or a1b0 omitted all of them do (test_x6_probe.py prints the shares)."""
import torch

from oracle import wenet_oracle as O

PROBE_RTOL = 2.0 ** -21

# (plane of A, plane of W) of the six products the kernels keep
PRODUCTS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))
LOW_ORDER = ((1, 1), (0, 2), (2, 0))
# summation orders: small products first (what the kernels do) and the reverse
ORDER_SMALL_FIRST = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
ORDER_LARGE_FIRST = tuple(reversed(ORDER_SMALL_FIRST))


def name(p):
    return f'a{p[0]}b{p[1]}'


def planes_nonzero(x):
    """Elementwise: planes 1 and 2 of x are both non-zero (plane 0 is zero only for x == 0)."""
    x0, x1, x2 = O.x6_planes(x)
    return (x0 != 0) & (x1 != 0) & (x2 != 0)


def sample_signed(n, g):
    """randn * 2^e, e uniform in [-12, 12]."""
    e = torch.randint(-12, 13, (n, ), generator=g).float()
    return torch.randn(n, generator=g) * torch.exp2(e)


def sample_positive(n, g):
    return sample_signed(n, g).abs()


def sample_range(lo, hi):
    """Uniform in [lo, hi): operands of a product that has to land in a narrow range."""
    def sample(n, g):
        return lo + (hi - lo) * torch.rand(n, generator=g)
    return sample


def general(shape, g, sample=None):
    """fp32 values with all three bf16 planes non-zero, drawn by `sample(n, g)` (default
    sample_signed).  The few draws with an empty plane (about 1 in 100: the low significand bits
    happen to be zero) are drawn again."""
    if sample is None:
        sample = sample_signed
    n = 1
    for s in shape:
        n *= s
    x = sample(n, g).float()
    for _ in range(64):
        bad = ~planes_nonzero(x)
        k = int(bad.sum())
        if k == 0:
            return x.reshape(shape)
        x[bad] = sample(k, g).float()
    raise RuntimeError('general(): the sampler keeps producing values with an empty plane')


def one_term_index(R, K, g, run=0):
    """pi (R,): column of the single non-zero of each row.  pi is a bijection onto [0, K) on every
    block of K consecutive rows (a fresh permutation per block); `run` shifts it by run * R
    positions, so that for R < K the runs 0 .. ceil(K / R) - 1 hit every k."""
    r = torch.arange(R)
    blocks = (R + K - 1) // K
    sig = torch.stack([torch.randperm(K, generator=g) for _ in range(blocks)])
    return sig[r // K, (r + run * R) % K]


def one_term(R, K, vals, pi):
    X = torch.zeros(R, K)
    X[torch.arange(R), pi] = vals
    return X


def runs_to_cover(R, K):
    return (K + R - 1) // R


def probe_w(N, K, seed, run=0, sample=None):
    """One-term weight W (N, K): W[n, pi[n]] = w[n] with w general.  Returns (W, pi, w); pair it
    with a dense general A (M, K): C[m, n] = A[m, pi[n]] * w[n]."""
    g = torch.Generator().manual_seed(seed)
    pi = one_term_index(N, K, g, run)
    w = general((N, ), g, sample)
    return one_term(N, K, w, pi), pi, w


def probe_a(M, K, seed, run=0, sample=None):
    """The transposed instrument: one-term A (M, K), to be paired with a dense general W (N, K):
    C[m, n] = a[m] * W[n, pi[m]].  With M >= K every (n, k) of the weight image is read through a
    product that is checked."""
    return probe_w(M, K, seed, run, sample)


def dense(R, K, seed, sample=None):
    return general((R, K), torch.Generator().manual_seed(seed), sample)


def selection(R, K, pi):
    """(R, K) of exact 1.0 entries at [r, pi[r]]: x * 1 keeps x0, x1, x2 times the single plane of
    1.0, so a six-product GEMM with it copies columns bit for bit."""
    return one_term(R, K, torch.ones(R), pi)


def emulate(A, W, drop=None, order=ORDER_SMALL_FIRST):
    """A @ W.T as the kernels form it: the six plane products, each an fp32 GEMM of bf16-valued
    planes (exact products), summed in fp32 in `order`; `drop` leaves one product out."""
    ap, wp = O.x6_planes(A), O.x6_planes(W)
    assert sorted(order) == sorted(PRODUCTS)
    out = torch.zeros(A.shape[0], W.shape[0])
    for i, j in order:
        if drop is not None and (i, j) == tuple(drop):
            continue
        out = out + ap[i] @ wp[j].T
    return out


def rel_err(got, A, W):
    """|got - a*w| / |a*w| per element against the fp64 product (one term per output: the fp64
    GEMM is that product, exactly), and the reference itself."""
    ref = A.double() @ W.double().T
    assert (ref != 0).all()
    return (got.double() - ref).abs() / ref.abs(), ref


def ffn_probe_runs(D, F):
    """F / D runs hit every hidden unit; F < D: D / F runs hit every k of the (F, D) weight."""
    return max(runs_to_cover(D, F), runs_to_cover(F, D))


def ffn_probe(kind, M, D, F, seed, run=0):
    """Operands of a feed-forward module act(X W1^T) W2^T (ReLU on positive operands: the
    identity) whose every output is ONE product; returns (X, W1, W2, ref) with ref in fp64.

    'w1': W1 (F, D) one-term with positive w, X dense positive, W2 (D, F) a selection of 1.0
    entries that copies the hidden units [run * D, (run + 1) * D) (mod F) to the output,
    ffn_probe_runs(D, F) runs: all six products of the first contraction, and a0b0 / a1b0 / a2b0 of the second.
    'w2': W1 a selection (the hidden tensor is a column permutation of X, exactly), W2 one-term
    with signed general values, shifted per run to hit every hidden unit: all six products of the
    second contraction, among them the three that 'w1' cannot see (a0b1, a1b1, a0b2)."""
    g = torch.Generator().manual_seed(seed)
    X = general((M, D), g, sample_positive)
    if kind == 'w1':
        W1 = one_term(F, D, general((F, ), g, sample_positive), one_term_index(F, D, g, run))
        W2 = selection(D, F, (run * D + torch.randperm(D, generator=g)) % F)
    else:
        W1 = selection(F, D, one_term_index(F, D, g, run))
        W2 = one_term(D, F, general((D, ), g), one_term_index(D, F, g, run))
    ref = (X.double() @ W1.double().T) @ W2.double().T      # one exact product per element
    assert (ref != 0).all()
    return X, W1, W2, ref


def ffn_dense_inputs(M, D, F, act):
    """Dense inputs of the feed-forward module, scaled as test_gpu_x6.py::test_ffn_x6_vs_fp64
    scales them: (X, W1, b1, W2, b2, x, ln_w, ln_b)."""
    g = torch.Generator().manual_seed(M + D + F + len(act))
    X = torch.randn(M, D, generator=g)
    W1 = torch.randn(F, D, generator=g) / D ** 0.5
    b1 = torch.randn(F, generator=g) * 0.3
    W2 = torch.randn(D, F, generator=g) / F ** 0.5
    b2 = torch.randn(D, generator=g) * 0.3
    x = torch.randn(M, D, generator=g)
    lw = 1.0 + 0.2 * torch.randn(D, generator=g)
    lb = 0.1 * torch.randn(D, generator=g)
    return X, W1, b1, W2, b2, x, lw, lb


def emulate_ffn(X, W1, b1, W2, b2, x, act, alpha, drop1=None, drop2=None):
    """The feed-forward module on emulated six-product GEMMs, everything else torch fp32:
    x + alpha * (act(X W1^T + b1) W2^T + b2)."""
    h = act(emulate(X, W1, drop1) + b1)
    return x + alpha * (emulate(h, W2, drop2) + b2)


# ---- the shapes test_gpu_x6_products.py runs (test_x6_probe.py checks the k coverage of each) ----
GEMM_NK = ((256, 256), (64, 48), (516, 48), (256, 2048))          # wn_op_gemm_x6
X6R_N = (256, 512, 768)                                            # wn_op_gemm_x6r, K = 256
X6R512_N = (512, 1536)                                             # wn_op_gemm_x6r512, K = 512
FFN_D = (256, 512)
FFN_F = (256, 1024)
# dense yardstick cases of the feed-forward module
FFN_DENSE = ((130, 256, 256), (130, 256, 2048), (130, 512, 1024))


def one_term_nk():
    """Every (rows, K) of a one-term weight in the GPU tests."""
    nk = set(GEMM_NK)
    nk |= {(n, 256) for n in X6R_N} | {(n, 512) for n in X6R512_N}
    for d in FFN_D:
        for f in FFN_F:
            nk |= {(f, d), (d, f)}
    return sorted(nk)
