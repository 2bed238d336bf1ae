"""Operator tests of the kernels behind decoders with heads of 32 -- attention_d32_kernel
(csrc/attention_d32.hip) through wn_op_attention_d32 and self_attn_step_d32_kernel
(csrc/attn_search.hip) through wn_op_attn_self_step with d = heads * 32 -- against the fp64
formulations of tests/attention_d32_refs.py.

Tolerance: the project's rule, err <= kernel_refs.bound(e_plain, scale) = 8 e_plain + 16 fp32 ulps
of the output scale, e_plain = the same plain formula in fp32; the cap (e_plain <= 1e-3 of the
scale) is asserted with it.  Exactness: the output starts as the pattern 0x7fc0dead and every
element no sequence owns still holds it; every batch lies between rows of +-1e18 and runs a second
time in reversed packing order, with the same bits per sequence; the step kernel changes only
out[n][d] and cache[step], and cache[step] is K | V of qkv bit for bit.
"""
import numpy as np
import pytest
import torch

import attention_d32_refs as D
import kernel_refs as KR
import paraformer_refs as PR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead
_REFS = {}


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def record(name, err, e_plain, scale):
    b = KR.bound(e_plain, scale)
    line = (f'{name} err={err:.3e} e_plain={e_plain:.3e} scale={scale:.3e} '
            f'ratio={err / b if b > 0 else 0.0:.3f}')
    print(line)
    assert KR.cap_ok(e_plain, scale), line
    assert err <= b, line


def _pattern(rows, ld):
    return torch.full((rows, ld), PATTERN, dtype=torch.int32).cuda()


def run_attention(c, pad=4, mask_mode=None):
    _lib, L = _L()
    d = c['d']
    ldo = d + pad
    bq = c['buf_q'].cuda()
    bk = bq if c['self_attn'] else c['buf_kv'].cuda()
    o = _pattern(c['q_rows'], ldo)
    order, q_off, q_len = PR.sorted_layout(c['q_offs'], c['q_lens'])
    kv_off = [c['kv_offs'][u] for u in order]
    kv_len = [c['kv_lens'][u] for u in order]
    qc, kc, vc = c['q_cols']
    _lib.check(L.wn_op_attention_d32(
        bq.data_ptr() + 4 * qc, bk.data_ptr() + 4 * kc, bk.data_ptr() + 4 * vc, c['ldq'],
        c['ldk'], c['ldk'], c['q_rows'], c['kv_rows'], o.data_ptr(), ldo,
        _lib.i32p(_i32(q_off)), _lib.i32p(_i32(q_len)), _lib.i32p(_i32(kv_off)),
        _lib.i32p(_i32(kv_len)), len(q_off), c['H'], c['scale'],
        c['mask_mode'] if mask_mode is None else mask_mode, _stream()), 'attention_d32')
    torch.cuda.synchronize()
    oc = o.cpu()
    own = torch.zeros(c['q_rows'], ldo, dtype=torch.bool)
    for (qo, ql, _, _) in c['seqs']:
        own[qo:qo + ql, :d] = True
    assert bool((oc[~own] == PATTERN).all()), 'attention_d32: a store outside the owned elements'
    return oc.view(torch.float32)[:, :d], own[:, 0]


def check_case(name):
    kw = D.ATTENTION_CASES[name]
    c = D.make_case(**kw)
    if name not in _REFS:          # one reference per case, shared and left alone
        _REFS[name] = D.case_refs(c)
    ref, e_plain, scale, _ = _REFS[name]
    out, own = run_attention(c)
    assert torch.isfinite(out[own]).all(), name
    record(f'attention_d32[{name}]', (out[own].double() - ref[own]).abs().max().item(), e_plain,
           scale)
    n = len(c['q_lens'])
    r = D.make_case(order=list(range(n))[::-1], **kw)
    out_r, _ = run_attention(r)
    for u in range(n):
        o0, o1, t = c['q_offs'][u], r['q_offs'][u], c['q_lens'][u]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: sequence {u} depends on where it is packed'


def test_causal_self_attention():
    """4 heads; sequences of 1, 31, 32, 33, 64 and 65 rows: one row, both sides of a key tile,
    both sides of two query groups."""
    check_case('causal')


def test_causal_padded_batch():
    """(rows, visible keys) = (9, 4), (9, 1), (33, 31): the padded batches of wn_decoder_forward;
    keys at or behind kv_len are hidden from every query, the padded query rows included."""
    check_case('padded')


@pytest.mark.parametrize('H', [1, 4, 8])
def test_cross_attention(H):
    """(q, kv) = (1, 3), (5, 32), (33, 70), (2, 1), (40, 125), ldq != ldk; 8 heads = 256 columns,
    the recipes' width."""
    check_case(f'cross_h{H}')


@pytest.mark.parametrize('regime', D.REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
@pytest.mark.parametrize('kind', ['cross', 'causal'])
def test_regimes(kind, regime):
    """4 heads, 33 queries over 70 keys (cross) and 65 rows (causal)."""
    check_case(f'{kind}_{regime[0]}_{regime[1]}')


def test_refusals():
    c = D.make_case('unit', None, 2, [5], mask_mode=1, seed=1)
    with pytest.raises(RuntimeError, match='mask_mode must be 0 .* or 1 .*not 2 \\(chunk window\\)'):
        run_attention(c, mask_mode=2)
    c['q_lens'] = [c['q_rows'] + 1]
    with pytest.raises(RuntimeError, match='attention_d32: query rows outside the buffer'):
        run_attention(c)
    c = D.make_case('unit', None, 2, [5], [4], seed=1)
    c['kv_offs'] = [c['kv_rows'] - 3]
    with pytest.raises(RuntimeError, match='attention_d32: key rows outside the buffer'):
        run_attention(c)
    c = D.make_case('unit', None, 2, [5], [4], seed=1)
    c['kv_lens'] = [0]
    with pytest.raises(RuntimeError, match='attention_d32: queries without keys'):
        run_attention(c)
    c = D.make_case('unit', None, 2, [5], [4], seed=1)
    c['ldq'] = c['ldq'] + 2
    with pytest.raises(RuntimeError, match='attention_d32: strides must be multiples of 4'):
        run_attention(c)


# ---------------------------------------------------------------------------------------------
# the step kernel at d = heads * 32


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_self_step(qkv, cache, path, H, step):
    """wn_op_attn_self_step on host tensors qkv (n, 3d), cache (max_len, n, 2d), path (n,
    max_len) with d = H * 32.  Returns out (n, d) fp32.  Asserts the exact conditions: the guard
    rows behind out keep the pattern, the cache changes in cache[step] only, and cache[step] =
    K | V of qkv."""
    _lib, L = _L()
    n, d = qkv.shape[0], H * 32
    max_len = path.shape[1]
    dq, dc, dp = qkv.contiguous().cuda(), cache.contiguous().cuda(), path.contiguous().cuda()
    out = _pattern(n + 3, d)
    _lib.check(L.wn_op_attn_self_step(dq.data_ptr(), d, H, n, dc.data_ptr(), step, dp.data_ptr(),
                                      max_len, out.data_ptr(), _stream()), 'attn_self_step')
    torch.cuda.synchronize()
    oc, cc = out.cpu(), dc.cpu()
    assert bool((oc[n:] == PATTERN).all()), 'a store behind the n x d block of out'
    keep = torch.ones(max_len, dtype=torch.bool)
    keep[step] = False
    assert torch.equal(_bits(cc[keep]), _bits(cache[keep])), 'a store outside cache[step]'
    assert torch.equal(_bits(cc[step]), _bits(qkv[:, d:])), 'cache[step] is not K | V of qkv'
    return oc[:n].view(torch.float32)


def check_step(name):
    case = D.make_step_case(**D.STEP_CASES[name])
    if ('step', name) not in _REFS:
        _REFS[('step', name)] = D.step_refs(case)
    ref, e_plain, scale, _ = _REFS[('step', name)]
    out = run_self_step(case['qkv'], case['cache'], case['path'], case['H'], case['step'])
    assert torch.isfinite(out).all(), name
    record(f'self_step_d32[{name}]', (out.double() - ref).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('name', sorted(D.STEP_CASES))
def test_self_step(name):
    """(H, n, length) = (1, 1, 1), (4, 5, 2), (8, 30, 63), (1, 5, 64), (4, 30, 65), (8, 5, 129) in
    `unit` and `peaked` 10; the needle at 0, 63, 64 and the last key of 129; 6 utterances x 5
    hypotheses behind a prompt of 3 (the paths of the prompted search)."""
    check_step(name)


def test_self_step_refuses_other_widths():
    _lib, L = _L()
    z = torch.zeros(4, 3 * 48).cuda()
    cache = torch.zeros(2, 4, 96).cuda()
    path = torch.zeros(4, 2, dtype=torch.int32).cuda()
    out = torch.zeros(4, 48).cuda()
    assert L.wn_op_attn_self_step(z.data_ptr(), 48, 1, 4, cache.data_ptr(), 0, path.data_ptr(), 2,
                                  out.data_ptr(), _stream()) == -1
    msg = L.wn_last_error()
    assert b'heads * 64' in msg and b'heads * 32' in msg
