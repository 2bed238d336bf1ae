"""Operator tests of the FireRedASR-AED encoder kernels (csrc/firered.hip) through the hooks
wn_op_attention_relshift / wn_op_firered_frontend, against the plain fp64 references of
tests/firered_refs.py (pinned to the reference's modules on the CPU, tests/test_firered_host.py).

Tolerance of every case, the rule of tests/test_gpu_kernels.py: err <= 8 * e_plain + 16 fp32 ulps
of the output scale (kernel_refs.bound), e_plain = the error of the plain fp32 evaluation of the
same formula on the same inputs, itself capped at 1e-3 of the scale (kernel_refs.cap_ok; asserted
on the CPU for every case too).  Output buffers start as a bit pattern that every element no
sequence owns must still hold; input rows no sequence owns hold +-1e18.

What the cases reach in attention_relshift_kernel<2>:
  ragged     q_len 1, 31, 32, 33, 65, 100 in one batch: one key tile, exactly 32 / 33, three and
             four tiles, a dead second wave (<= 32 queries), queries past the end in a live wave,
             band rows in front of and behind the table at the first and the last tile
  one        a single T = 1: a one-row table, every other band row predicated off
  sign       position rows 40 times larger for distances r < 0: a mirrored distance or a band
             row off by one misses the bound by > 1000 x (asserted on the CPU)
  table      a table sized for 300 frames under sequences of 70 and 5
  alone / batched   T = 97 alone, and inside a batch whose longest has 200: bit-identical
and dwconv_kernel<40>, the conv module of d_model 1280 (2560 channels, LayerNorm over them,
K = 33): test_dwconv_2560, on the cases of tests/test_gpu_kernels.py's test_dwconv.
"""
import ctypes

import numpy as np
import pytest
import torch

import firered_refs as FR
import kernel_refs as KR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _padded(t, ld, fill=KR.POISON):
    rows, d = t.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float32)
    buf[:, :d] = t
    return buf.cuda()


def record(name, err, e_plain, scale):
    b = KR.bound(e_plain, scale)
    line = (f'{name} err={err:.3e} e_plain={e_plain:.3e} scale={scale:.3e} '
            f'ratio={err / b if b > 0 else 0.0:.3f}')
    print(line)
    assert KR.cap_ok(e_plain, scale), line
    assert err <= b, line


def run_relshift(case, pads=(4, 8, 12, 4, 4)):
    """wn_op_attention_relshift on a case of firered_refs.make_relshift_case -> O (rows, d) fp32
    on the host.  Asserts that no element outside the owned rows / the first d columns of O
    changed."""
    _lib, L = _L()
    H, d = case['H'], case['H'] * 64
    ldq, ldk, ldv, ldo, ldp = (d + p for p in pads)
    Q, K, V = _padded(case['q'], ldq), _padded(case['k'], ldk), _padded(case['v'], ldv)
    P = _padded(case['P'], ldp)
    bu, bv = case['bias_u'].contiguous().cuda(), case['bias_v'].contiguous().cuda()
    O = torch.full((case['rows'], ldo), PATTERN, dtype=torch.int32).cuda()
    off, ln = _i32([s[0] for s in case['seqs']]), _i32([s[1] for s in case['seqs']])
    _lib.check(L.wn_op_attention_relshift(
        Q.data_ptr(), K.data_ptr(), V.data_ptr(), ldq, ldk, ldv, case['rows'], P.data_ptr(), ldp,
        case['P'].shape[0], case['p_center'], bu.data_ptr(), bv.data_ptr(), O.data_ptr(), ldo,
        _lib.i32p(off), _lib.i32p(ln), len(off), H, case['scale'],
        torch.cuda.current_stream().cuda_stream), 'attention_relshift')
    torch.cuda.synchronize()
    Oc = O.cpu()
    owned = torch.zeros(case['rows'], ldo, dtype=torch.bool)
    owned[case['own'], :d] = True
    assert bool((Oc[~owned] == PATTERN).all()), 'a store outside the owned rows / columns of O'
    return Oc.view(torch.float32)[:, :d]


@pytest.mark.parametrize('name', sorted(FR.RELSHIFT_CASES))
def test_attention_relshift(name):
    case = FR.make_relshift_case(**FR.RELSHIFT_CASES[name])
    ref, e_plain, scale, _ = FR.relshift_refs(case)
    out = run_relshift(case).double()
    own = case['own']
    assert torch.isfinite(out[own]).all(), name
    record(f'relshift[{name}]', (out[own] - ref[own]).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('H', [2, 20])
def test_attention_relshift_alone_equals_batched(H):
    """The distance does not depend on the batch: T = 97 alone and the same rows inside a batch
    whose longest sequence has 200 frames (one table, sized for 200) give the same bits."""
    batch = FR.make_relshift_case(H=H, lens=[200, 97, 40], seed=30 + H, t_table=200)
    o, T = batch['seqs'][1]
    alone = dict(batch)
    alone.update(seqs=[(o, T)])
    own = torch.zeros(batch['rows'], dtype=torch.bool)
    own[o:o + T] = True
    alone['own'] = own
    out_b = run_relshift(batch)
    out_a = run_relshift(alone)
    assert torch.equal(out_a[o:o + T].view(torch.int32), out_b[o:o + T].view(torch.int32))
    # and a table of another size (the same rows around another centre)
    small = dict(alone)
    small.update(P=batch['P'][200 - 97:200 + 96].contiguous(), p_center=96)
    out_s = run_relshift(small)
    assert torch.equal(out_s[o:o + T].view(torch.int32), out_b[o:o + T].view(torch.int32))
    ref, e_plain, scale, _ = FR.relshift_refs(batch)
    bo = batch['own']
    record(f'relshift[batch200-h{H}]', (out_b[bo].double() - ref[bo]).abs().max().item(),
           e_plain, scale)


def run_frontend(c, lens, feats, out_off, out_rows, pad=4):
    _lib, L = _L()
    C, Fd = c['C'], c['F']
    F2 = ((Fd - 3) // 2 + 1 - 3) // 2 + 1
    ldo = C * F2 + pad
    dev = lambda t: t.contiguous().cuda()
    w1 = dev(c['w1'].view(C, 9).t())                                  # [9][C]
    w2 = dev(c['w2'].permute(2, 3, 1, 0).reshape(9, C, C))            # [tap][c_in][c_out]
    mean, istd = (dev(c['mean']), dev(c['istd'])) if c['mean'] is not None else (None, None)
    b1, b2, fd = dev(c['b1']), dev(c['b2']), dev(feats)
    O = torch.full((out_rows, ldo), PATTERN, dtype=torch.int32).cuda()
    out_len = np.zeros(len(lens), dtype=np.int32)
    _lib.check(L.wn_op_firered_frontend(
        fd.data_ptr(), mean.data_ptr() if mean is not None else None,
        istd.data_ptr() if istd is not None else None, w1.data_ptr(), b1.data_ptr(),
        w2.data_ptr(), b2.data_ptr(), O.data_ptr(), ldo, out_rows, _lib.i32p(_i32(lens)),
        _lib.i32p(_i32(out_off)), _lib.i32p(out_len), len(lens), feats.shape[1], Fd, C,
        torch.cuda.current_stream().cuda_stream), 'firered_frontend')
    torch.cuda.synchronize()
    return O.cpu(), out_len, C * F2


def test_firered_frontend():
    """Lengths 7, 61, 97, 290 (and 1: one frame already yields one) in one batch, poisoned
    padding, gaps between the utterances' output rows; then every utterance alone: same bits."""
    lens = FR.FRONTEND_LENS
    c = FR.make_frontend_case(lens, seed=5)
    ref, e_plain, scale = FR.frontend_refs(c)
    t2 = [FR.firered_out_len(n) for n in lens]
    off, rows = KR.pack_layout(t2, 2, 3)
    O, out_len, width = run_frontend(c, lens, c['feats'], off, rows)
    assert list(out_len) == t2
    owned = torch.zeros(O.shape, dtype=torch.bool)
    err = 0.0
    for b, n in enumerate(t2):
        owned[off[b]:off[b] + n, :width] = True
        got = O[off[b]:off[b] + n, :width].view(torch.float32).double()
        assert torch.isfinite(got).all()
        err = max(err, (got - ref[b]).abs().max().item())
    assert bool((O[~owned] == PATTERN).all()), 'a store outside the owned rows / columns'
    record('firered_frontend', err, e_plain, scale)
    for b, n in enumerate(lens):
        Oa, la, _ = run_frontend(c, [n], c['feats'][b:b + 1, :n], [0], t2[b])
        assert la[0] == t2[b]
        assert torch.equal(Oa[:, :width], O[off[b]:off[b] + t2[b], :width]), n


@pytest.mark.parametrize('K,causal', [(33, False), (15, False), (8, True)])
def test_dwconv_2560(K, causal):
    """wn_op_dwconv at D = 2560 (E = 40 values per lane, tap groups of 2): lengths around the
    kernel size, on both sides of the tap-group edges, poisoned rows between the utterances."""
    _lib, L = _L()
    lens = [1, 2, 3, max(K - 1, 1), K, K + 1, 0, 70]
    c = KR.make_dwconv_case(2560, K, causal, 0, lens, seed=2560 + K, gap=1, lead=2, t_extra=3,
                            pad_ld=4, tail=3)
    ref, e_plain, scale = KR.dwconv_refs(c)
    D, M = c['D'], c['M']
    ldx, ldy = D + 4, D + 8
    x = _padded(c['x'], ldx)
    y = torch.full((M, ldy), PATTERN, dtype=torch.int32).cuda()
    t = {k: c[k].contiguous().cuda() for k in ('wt', 'bias', 'cpad', 'ln_w', 'ln_b')}
    _lib.check(L.wn_op_dwconv(x.data_ptr(), ldx, t['wt'].data_ptr(), t['bias'].data_ptr(),
                              t['cpad'].data_ptr(), t['ln_w'].data_ptr(), t['ln_b'].data_ptr(),
                              0, y.data_ptr(), ldy, _lib.i32p(_i32(c['off'])),
                              _lib.i32p(_i32(c['lens'])), len(lens), M, D, K, int(causal),
                              c['t_max'], c['eps'], torch.cuda.current_stream().cuda_stream),
               'dwconv')
    torch.cuda.synchronize()
    yc = y.cpu()
    owned = torch.zeros(M, ldy, dtype=torch.bool)
    owned[c['own'], :D] = True
    assert bool((yc[~owned] == PATTERN).all()), 'a store outside the owned rows / columns of y'
    got = yc.view(torch.float32)[:, :D].double()
    own = c['own']
    assert torch.isfinite(got[own]).all()
    record(f'dwconv2560[K{K}-c{int(causal)}]', (got[own] - ref[own]).abs().max().item(), e_plain,
           scale)
