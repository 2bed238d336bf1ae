"""The one-term probe of the six-product kernels (tests/x6_probe.py) on the CPU: before
test_gpu_x6_products.py trusts it, show on an emulation of the six plane products that the probe
passes when all six are there, in either summation order, and fails -- on at least half of its
elements -- as soon as any one of the five products other than a0b0 is left out."""
import pytest
import torch

import x6_probe as P

ULP = 2.0 ** -24
KINDS = ('probe_w', 'probe_a')
# (M, N, K): ragged, N < K, N > K with a partial last block of rows
SHAPES = ((33, 64, 48), (130, 256, 256), (49, 516, 48), (257, 256, 256))


def _operands(kind, M, N, K, run=0):
    if kind == 'probe_w':
        return P.dense(M, K, 11 + M + K), P.probe_w(N, K, 13 + N + K, run)[0]
    return P.probe_a(M, K, 17 + M + K, run)[0], P.dense(N, K, 19 + N + K)


@pytest.mark.parametrize('order', [P.ORDER_SMALL_FIRST, P.ORDER_LARGE_FIRST],
                         ids=['small_first', 'large_first'])
@pytest.mark.parametrize('kind', KINDS)
def test_all_six_products_stay_inside_the_bound(kind, order):
    worst = 0.0
    for M, N, K in SHAPES:
        A, W = _operands(kind, M, N, K)
        rel, _ = P.rel_err(P.emulate(A, W, None, order), A, W)
        worst = max(worst, rel.max().item())
        assert (rel <= P.PROBE_RTOL).all()
    print(f'\n[{kind}] all six: max |err| / |a w| = {worst / ULP:.2f} x 2^-24')
    assert worst > 0        # (a probe of bf16-exact values would give exactly 0)


@pytest.mark.parametrize('drop', [p for p in P.PRODUCTS if p != (0, 0)], ids=P.name)
@pytest.mark.parametrize('kind', KINDS)
def test_an_omitted_product_violates_the_bound_on_half_of_the_elements(kind, drop):
    for order in (P.ORDER_SMALL_FIRST, P.ORDER_LARGE_FIRST):
        for M, N, K in SHAPES:
            A, W = _operands(kind, M, N, K)
            rel, _ = P.rel_err(P.emulate(A, W, drop, order), A, W)
            share = (rel > P.PROBE_RTOL).float().mean().item()
            print(f'\n[{kind} {M}x{N}x{K}] without {P.name(drop)}: {100 * share:.1f} % of the '
                  f'elements over 2^-21, max {rel.max().item() / ULP:.0f} x 2^-24')
            assert share >= 0.5
            if drop in ((0, 1), (1, 0)):
                assert share == 1.0


@pytest.mark.parametrize('N,K', P.one_term_nk())
def test_every_k_is_hit_over_the_runs(N, K):
    runs = P.runs_to_cover(N, K)
    hit = torch.zeros(K, dtype=torch.bool)
    for run in range(runs):
        W, pi, w = P.probe_w(N, K, 5, run)
        assert ((W != 0).sum(1) == 1).all()                  # one term per row
        assert torch.equal(W[torch.arange(N), pi], w)
        for b in range(0, N - K + 1, K):                     # a bijection per block of K rows
            assert pi[b:b + K].sort().values.equal(torch.arange(K))
        hit[pi] = True
    assert hit.all()
    if N >= K:
        assert runs == 1


@pytest.mark.parametrize('kind', ['w1', 'w2'])
@pytest.mark.parametrize('D', P.FFN_D)
@pytest.mark.parametrize('F', P.FFN_F)
def test_ffn_probe_covers_every_hidden_unit(kind, D, F):
    runs = P.ffn_probe_runs(D, F)
    hit_h, hit_k1 = torch.zeros(F, dtype=torch.bool), torch.zeros(D, dtype=torch.bool)
    for run in range(runs):
        X, W1, W2, ref = P.ffn_probe(kind, 5, D, F, 23, run)
        assert ((W1 != 0).sum(1) == 1).all() and ((W2 != 0).sum(1) == 1).all()
        hit_h |= (W2 != 0).any(0)
        hit_k1 |= (W1 != 0).any(0)
        assert (X > 0).all() and (W1 >= 0).all()             # ReLU is the identity
    assert hit_h.all() and hit_k1.all()


def test_probe_values_have_three_planes():
    """A probe built from bf16-exact values (or values with an empty low plane) would test
    nothing: every w and every element of A has non-zero planes 1 and 2."""
    for N, K in P.GEMM_NK:
        W, pi, w = P.probe_w(N, K, 3)
        assert P.planes_nonzero(w).all()
        assert P.planes_nonzero(P.dense(33, K, 4)).all()
    gate = P.sample_range(4.25, 4.5)
    assert P.planes_nonzero(P.dense(33, 256, 6, gate)).all()
    assert P.planes_nonzero(P.probe_w(256, 256, 7, 0, gate)[2]).all()
    for kind in ('w1', 'w2'):
        X, W1, W2, _ = P.ffn_probe(kind, 33, 256, 1024, 8)
        assert P.planes_nonzero(X).all()
        one = W1 if kind == 'w1' else W2
        assert P.planes_nonzero(one[one != 0]).all()
    # the sampler really has to reject: plain draws do contain empty planes
    g = torch.Generator().manual_seed(1)
    assert not P.planes_nonzero(P.sample_signed(100000, g)).all()


@pytest.mark.parametrize('kind', ['w1', 'w2'])
def test_ffn_probe_sees_the_products_of_its_contraction(kind):
    """'w1' sees every product of the first contraction and a1b0 / a2b0 of the second, 'w2' every
    product of the second (among them a0b1, a1b1, a0b2, which 'w1' cannot see)."""
    M, D, F = 33, 256, 1024
    relu = torch.relu
    z = torch.zeros
    seen = {'w1': [(1, p) for p in P.PRODUCTS if p != (0, 0)] + [(2, (1, 0)), (2, (2, 0))],
            'w2': [(2, p) for p in P.PRODUCTS if p != (0, 0)]}[kind]
    for run in range(P.ffn_probe_runs(D, F)):
        X, W1, W2, ref = P.ffn_probe(kind, M, D, F, 29, run)

        def rel(drop1=None, drop2=None):
            got = P.emulate_ffn(X, W1, z(F), W2, z(D), z(M, D), relu, 1.0, drop1, drop2)
            return (got.double() - ref).abs() / ref.abs()
        assert (rel() <= P.PROBE_RTOL).all()
        for which, drop in seen:
            r = rel(drop, None) if which == 1 else rel(None, drop)
            share = (r > P.PROBE_RTOL).float().mean().item()
            print(f'\n[ffn {kind} run {run}] contraction {which} without {P.name(drop)}: '
                  f'{100 * share:.1f} % over 2^-21')
            assert share >= 0.5


@pytest.mark.parametrize('act', ['silu', 'relu'])
@pytest.mark.parametrize('M,D,F', P.FFN_DENSE)
def test_dense_yardstick_sees_an_omitted_low_order_product(M, D, F, act):
    """The dense instrument of test_gpu_x6_products.py (error against fp64 next to an fp32
    yardstick's, margin 1.2x on the rms): at its shapes and input scaling, leaving out any
    low-order product of either contraction raises the rms error of the emulated feed-forward
    module at least 5x over the healthy emulation."""
    fn = {'silu': torch.nn.functional.silu, 'relu': torch.relu}[act]
    t = P.ffn_dense_inputs(M, D, F, act)
    X, W1, b1, W2, b2, x = t[:6]
    ref = x.double() + 0.5 * (fn(X.double() @ W1.double().T + b1.double()) @ W2.double().T
                              + b2.double())

    def rms(drop1=None, drop2=None):
        got = P.emulate_ffn(X, W1, b1, W2, b2, x, fn, 0.5, drop1, drop2)
        return ((got.double() - ref) ** 2).mean().sqrt().item()
    healthy = rms()
    for drop in P.LOW_ORDER:
        for which in (1, 2):
            r = rms(drop, None) if which == 1 else rms(None, drop)
            print(f'\n[{M} {D} {F} {act}] contraction {which} without {P.name(drop)}: rms '
                  f'{r:.2e} = {r / healthy:.1f} x healthy {healthy:.2e}')
            assert r >= 5 * healthy
