"""Operator tests of the Paraformer kernels (csrc/attention_d128.hip, csrc/paraformer.hip) through
the hooks wn_op_attention_d128 / wn_op_lfr_front / wn_op_layernorm_wide / wn_op_cif_alpha /
wn_op_cif_fire, against the plain fp64 restatements of tests/paraformer_refs.py (checked on the
CPU in tests/test_paraformer_host.py).

Tolerance of every case, the rule of tests/test_gpu_kernels.py: err <= 8 * e_plain + 16 fp32 ulps
of the output scale (kernel_refs.bound) with the cap on the yardstick (kernel_refs.cap_ok), e_plain
= the error of the plain fp32 evaluation of the same formula on the same inputs.  Utterances are
packed between rows of +-1e18 and run a second time in reversed packing order: per utterance the
two results are the same bits, so no row of a neighbour is ever read.  Output buffers start as a
bit pattern that every element no utterance owns must still hold.  The fire frames, fire counts
and token numbers of cif_fire must equal the fp32 chain's exactly.
"""
import math

import numpy as np
import pytest
import torch

import kernel_refs as KR
import paraformer_refs as PR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead


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


def _check_unowned(y_cpu, owned, what):
    assert bool((y_cpu[~owned] == PATTERN).all()), f'{what}: a store outside the owned elements'


# ---------------------------------------------------------------------------------------------
# attention_d128


def run_attention(c, pad=4):
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
    _lib.check(L.wn_op_attention_d128(
        bq.data_ptr() + 4 * qc, bk.data_ptr() + 4 * kc, bk.data_ptr() + 4 * vc, c['ldq'],
        c['ldk'], c['ldk'], c['q_rows'], c['kv_rows'], o.data_ptr(), ldo,
        _lib.i32p(_i32(q_off)), _lib.i32p(_i32(q_len)), _lib.i32p(_i32(kv_off)),
        _lib.i32p(_i32(kv_len)), len(q_off), c['H'], c['scale'], _stream()), 'attention_d128')
    torch.cuda.synchronize()
    oc = o.cpu()
    own = torch.zeros(c['q_rows'], ldo, dtype=torch.bool)
    for (qo, ql, _, _) in c['seqs']:
        own[qo:qo + ql, :d] = True
    _check_unowned(oc, own, 'attention_d128')
    return oc.view(torch.float32)[:, :d], own[:, 0]


def _attention_both_orders(q_lens, kv_lens, seed, name):
    c = PR.make_attention_d128_case(2, q_lens, kv_lens, seed=seed)
    ref, e_plain, scale = PR.attention_d128_refs(c)
    out, own = run_attention(c)
    assert torch.isfinite(out[own]).all(), name
    record(name, (out[own].double() - ref[own]).abs().max().item(), e_plain, scale)
    n = len(q_lens)
    r = PR.make_attention_d128_case(2, q_lens, kv_lens, seed=seed, order=list(range(n))[::-1])
    out_r, _ = run_attention(r)
    for u in range(n):
        o0, o1, t = c['q_offs'][u], r['q_offs'][u], q_lens[u]
        assert torch.equal(out[o0:o0 + t].view(torch.int32), out_r[o1:o1 + t].view(torch.int32)), \
            f'{name}: utterance {u} depends on where it is packed'


def test_attention_d128_self():
    """2 heads x 128; sequences of 1, 31, 33 and 65 rows: one row, a tile less a key, a tile and a
    key (two tiles, two query groups), two tiles and a key (a second block)."""
    _attention_both_orders([1, 31, 33, 65], None, 11, 'attention_d128[self]')


def test_attention_d128_cross():
    """(q, kv) = (1, 3), (5, 32), (33, 70), (2, 1): tokens against frames, ldq != ldk."""
    _attention_both_orders([1, 5, 33, 2], [3, 32, 70, 1], 12, 'attention_d128[cross]')


def test_attention_d128_refusals():
    _lib, L = _L()
    c = PR.make_attention_d128_case(2, [5], None, seed=1)
    c['q_lens'] = [c['q_rows'] + 1]
    with pytest.raises(RuntimeError, match='outside the buffer'):
        run_attention(c)
    c = PR.make_attention_d128_case(2, [5], [4], seed=1)
    c['kv_lens'] = [0]
    with pytest.raises(RuntimeError, match='queries without keys'):
        run_attention(c)


# ---------------------------------------------------------------------------------------------
# lfr_front

LFR_N = [1, 5, 6, 7, 24, 97]
LFR_F, LFR_M, LFR_STEP, LFR_D, LFR_LD = 80, 7, 6, 560, 576


def _lfr_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = [3.0 * torch.randn(n, LFR_F, generator=g) + 1.0 for n in LFR_N]
    return dict(feats=feats, mean=torch.randn(LFR_D, generator=g),
                istd=0.5 + torch.rand(LFR_D, generator=g),
                pe=PR.whisper_sinusoids(32, LFR_D).float(),
                ln_w=1.0 + 0.2 * torch.randn(LFR_D, generator=g),
                ln_b=0.1 * torch.randn(LFR_D, generator=g), xscale=math.sqrt(512.0), eps=1e-5)


def run_lfr(c, order):
    """The utterances as rows `order` of a (B, T, F) batch padded with +-1e18, output rows packed
    in that order with a gap.  Returns (rows by utterance, as int32 bit patterns)."""
    _lib, L = _L()
    B, T = len(LFR_N), max(LFR_N) + 2
    sign = torch.where(torch.arange(LFR_F) % 2 == 0, 1.0, -1.0) * PR.POISON
    feats = sign.repeat(B, T, 1)
    lens, out_off, at = [], [], 1
    for slot, u in enumerate(order):
        n = LFR_N[u]
        feats[slot, :n] = c['feats'][u]
        lens.append(n)
        out_off.append(at)
        at += PR.lfr_rows(n) + 2
    out = _pattern(at, LFR_LD)
    out_len = np.zeros(B, dtype=np.int32)
    dev = {k: c[k].cuda() for k in ('mean', 'istd', 'pe', 'ln_w', 'ln_b')}
    fd = feats.contiguous().cuda()
    _lib.check(L.wn_op_lfr_front(
        fd.data_ptr(), dev['mean'].data_ptr(), dev['istd'].data_ptr(), dev['pe'].data_ptr(),
        dev['pe'].shape[0], dev['ln_w'].data_ptr(), dev['ln_b'].data_ptr(), out.data_ptr(),
        LFR_LD, at, _lib.i32p(_i32(lens)), _lib.i32p(_i32(out_off)), _lib.i32p(out_len), B, T,
        LFR_F, LFR_M, LFR_STEP, c['xscale'], c['eps'], _stream()), 'lfr_front')
    torch.cuda.synchronize()
    oc = out.cpu()
    own = torch.zeros(at, LFR_LD, dtype=torch.bool)
    res = {}
    for slot, u in enumerate(order):
        rows = PR.lfr_rows(LFR_N[u])
        assert out_len[slot] == rows
        own[out_off[slot]:out_off[slot] + rows] = True
        res[u] = oc[out_off[slot]:out_off[slot] + rows]
    _check_unowned(oc, own, 'lfr_front')
    return res


def test_lfr_front():
    c = _lfr_inputs(3)
    a = run_lfr(c, list(range(len(LFR_N))))
    b = run_lfr(c, list(range(len(LFR_N)))[::-1])
    for u, n in enumerate(LFR_N):
        args = (c['feats'][u], c['mean'], c['istd'], c['pe'], c['ln_w'], c['ln_b'], c['xscale'],
                c['eps'], LFR_M, LFR_STEP)
        ref = PR.ref_lfr_front(*args)
        plain = PR.ref_lfr_front(*args, fp32=True)
        out = a[u].view(torch.float32)
        assert bool((a[u][:, LFR_D:] == 0).all()), 'columns 560..575 must be exact zeros'
        record(f'lfr_front[n={n}]', (out[:, :LFR_D].double() - ref).abs().max().item(),
               (plain - ref).abs().max().item(), ref.abs().max().item())
        assert torch.equal(a[u], b[u]), f'lfr_front: utterance of {n} frames depends on its slot'


# ---------------------------------------------------------------------------------------------
# layernorm_wide


@pytest.mark.parametrize('D,Dpad,M', [(2048, 2048, 1), (2048, 2048, 5), (560, 576, 1),
                                      (560, 576, 5)])
def test_layernorm_wide(D, Dpad, M):
    _lib, L = _L()
    c = KR.make_rows_case('unit', M, D, seed=D + M)
    ldx, ldy = D + 8, Dpad + 4
    x = torch.full((M, ldx), PR.POISON)
    x[:, :D] = c['x']
    xd, w, b = x.cuda(), c['w'].cuda(), c['b'].cuda()
    y = _pattern(M, ldy)
    _lib.check(L.wn_op_layernorm_wide(xd.data_ptr(), ldx, w.data_ptr(), b.data_ptr(),
                                      y.data_ptr(), ldy, M, D, Dpad, c['eps'], _stream()),
               'layernorm_wide')
    torch.cuda.synchronize()
    yc = y.cpu()
    assert bool((yc[:, Dpad:] == PATTERN).all()), 'a store behind Dpad'
    assert bool((yc[:, D:Dpad] == 0).all()), 'the padding columns must be exact zeros'
    ref, e_plain, scale = KR.rows_refs(c)
    record(f'layernorm_wide[D={D},M={M}]',
           (yc.view(torch.float32)[:, :D].double() - ref).abs().max().item(), e_plain, scale)


def test_layernorm_wide_refusals():
    _lib, L = _L()
    x = torch.zeros(1, 4096).cuda()
    with pytest.raises(RuntimeError, match='2048'):
        _lib.check(L.wn_op_layernorm_wide(x.data_ptr(), 4096, x.data_ptr(), x.data_ptr(),
                                          x.data_ptr(), 4096, 1, 2052, 2052, 1e-5, _stream()),
                   'layernorm_wide')


# ---------------------------------------------------------------------------------------------
# cif_alpha

CIF_LENS = [1, 2, 33]


def _cif_weights(d, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(conv_w=torch.randn(d, d, 3, generator=g) / math.sqrt(3 * d),
                conv_b=0.1 * torch.randn(d, generator=g),
                out_w=torch.randn(d, generator=g) / math.sqrt(d) * 3.0,
                out_b=0.1 * torch.randn(1, generator=g))


def run_cif_alpha(hs, w, order, smooth=1.0, noise=0.0):
    _lib, L = _L()
    d = hs[0].shape[1]
    buf, offs, total = PR.pack_rows(hs, order, gap=2, lead=1, ld=d + 4)
    alpha = _pattern(total, 1)
    idx, off, ln = PR.sorted_layout(offs, [h.shape[0] for h in hs])
    bd = buf.cuda()
    cw = PR.conv_w_tap_major(w['conv_w']).cuda()
    cb, ow, ob = w['conv_b'].cuda(), w['out_w'].cuda(), w['out_b'].cuda()
    _lib.check(L.wn_op_cif_alpha(bd.data_ptr(), d + 4, total, d, cw.data_ptr(), cb.data_ptr(),
                                 ow.data_ptr(), ob.data_ptr(), smooth, noise, alpha.data_ptr(),
                                 _lib.i32p(_i32(off)), _lib.i32p(_i32(ln)), len(off), _stream()),
               'cif_alpha')
    torch.cuda.synchronize()
    ac = alpha.cpu()
    own = torch.zeros(total, 1, dtype=torch.bool)
    for u, h in enumerate(hs):
        own[offs[u]:offs[u] + h.shape[0]] = True
    _check_unowned(ac, own, 'cif_alpha')
    return [ac[offs[u]:offs[u] + h.shape[0], 0] for u, h in enumerate(hs)]


@pytest.mark.parametrize('d', [256, 512])
def test_cif_alpha(d):
    g = torch.Generator().manual_seed(d)
    hs = [torch.randn(t, d, generator=g) for t in CIF_LENS]
    w = _cif_weights(d, d + 1)
    a = run_cif_alpha(hs, w, None)
    b = run_cif_alpha(hs, w, list(range(len(hs)))[::-1])
    for u, h in enumerate(hs):
        args = (h, w['conv_w'], w['conv_b'], w['out_w'], w['out_b'], 1.0, 0.0)
        ref, plain = PR.ref_cif_alpha(*args), PR.ref_cif_alpha(*args, fp32=True)
        out = a[u].view(torch.float32).double()
        assert bool(((out >= 0) & (out <= 1)).all())
        record(f'cif_alpha[d={d},T={h.shape[0]}]', (out - ref).abs().max().item(),
               (plain - ref).abs().max().item(), 1.0)
        assert torch.equal(a[u], b[u]), f'cif_alpha: utterance {u} depends on where it is packed'


# ---------------------------------------------------------------------------------------------
# cif_fire

TAIL = 0.45


def run_cif_fire(hs, alphas, order, cap_extra=1):
    """Returns per utterance (embedding rows as int32 bits, fire frames, n_fire, token_num)."""
    _lib, L = _L()
    d = hs[0].shape[1]
    n = len(hs)
    buf, offs, total = PR.pack_rows(hs, order, gap=2, lead=1, ld=d + 4)
    al = torch.full((total, ), PR.POISON)
    for u in range(n):
        al[offs[u]:offs[u] + hs[u].shape[0]] = torch.as_tensor(alphas[u], dtype=torch.float32)
    idx, off, ln = PR.sorted_layout(offs, [h.shape[0] for h in hs])
    caps = [ln[i] + cap_extra for i in range(n)]          # at most one fire per frame, + the tail
    emb_off, at = [], 1
    for i in range(n):
        emb_off.append(at)
        at += caps[i] + 1
    lde = d + 4
    emb = _pattern(at, lde)
    fire_t = np.zeros(at, dtype=np.int32)
    n_fire, tok = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    bd, ad = buf.cuda(), al.cuda()
    _lib.check(L.wn_op_cif_fire(bd.data_ptr(), d + 4, total, d, ad.data_ptr(),
                                _lib.i32p(_i32(off)), _lib.i32p(_i32(ln)), n, 1.0, TAIL,
                                emb.data_ptr(), lde, at, _lib.i32p(_i32(emb_off)),
                                _lib.i32p(_i32(caps)), _lib.i32p(fire_t), _lib.i32p(n_fire),
                                _lib.i32p(tok), _stream()), 'cif_fire')
    torch.cuda.synchronize()
    ec = emb.cpu()
    own = torch.zeros(at, lde, dtype=torch.bool)
    res = {}
    for i, u in enumerate(idx):
        k = max(int(n_fire[i]), int(tok[i]))
        assert k <= caps[i]
        own[emb_off[i]:emb_off[i] + k, :d] = True
        res[u] = (ec[emb_off[i]:emb_off[i] + int(n_fire[i]), :d],
                  fire_t[emb_off[i]:emb_off[i] + int(n_fire[i])].tolist(), int(n_fire[i]),
                  int(tok[i]))
    _check_unowned(ec, own, 'cif_fire')
    return res


@pytest.mark.parametrize('d', [256, 512])
def test_cif_fire(d):
    names = list(PR.CIF_ALPHA_ROWS)
    g = torch.Generator().manual_seed(d)
    alphas = [PR.CIF_ALPHA_ROWS[k] for k in names]
    # a 40-frame row of free alphas whose every fire decision is far from the threshold
    for seed in range(100):
        a = torch.rand(40, generator=torch.Generator().manual_seed(seed)).mul(0.9).add(0.02)
        if PR.fire_margin(a.numpy(), TAIL) >= 1e-3:
            alphas.append(a.numpy().tolist())
            names.append('free40')
            break
    hs = [torch.randn(len(a), d, generator=g) for a in alphas]
    r0 = run_cif_fire(hs, alphas, None)
    r1 = run_cif_fire(hs, alphas, list(range(len(hs)))[::-1])
    for u, name in enumerate(names):
        a32 = np.asarray(alphas[u], dtype=np.float32)
        assert PR.fire_margin(a32, TAIL) >= 1e-3
        fires, _, _, n_tok = PR.cif_chain(a32, np.float32(TAIL), np.float32)
        emb, f_t, n_fire, tok = r0[u]
        assert (f_t, n_fire, tok) == (fires, len(fires), n_tok), name
        ref, fires64, _ = PR.ref_cif_embeds(hs[u], a32, TAIL)
        plain, _, _ = PR.ref_cif_embeds(hs[u], a32, np.float32(TAIL), fp32=True)
        assert fires64 == fires
        if len(fires):
            out = emb.view(torch.float32).double()
            record(f'cif_fire[d={d},{name}]', (out - ref).abs().max().item(),
                   (plain - ref).abs().max().item(), max(ref.abs().max().item(), 1e-30))
        assert torch.equal(emb, r1[u][0]) and r1[u][1:] == r0[u][1:], \
            f'cif_fire: utterance {name} depends on where it is packed'
    assert r0[names.index('no_fire')][2] == 0
    assert r0[names.index('tail_only')][1] == [2]
    assert r0[names.index('consecutive')][1][:3] == [1, 2, 3]


def test_cif_fire_refusals():
    d = 256
    hs = [torch.randn(3, d)]
    with pytest.raises(RuntimeError, match=r'outside \[0, 1\]'):
        run_cif_fire(hs, [[0.5, 1.5, 0.2]], None)
    _lib, L = _L()
    x = torch.zeros(8, d).cuda()
    one = _i32([0])
    z = np.zeros(8, dtype=np.int32)
    with pytest.raises(RuntimeError, match='threshold must be 1.0'):
        _lib.check(L.wn_op_cif_fire(x.data_ptr(), d, 8, d, x.data_ptr(), _lib.i32p(one),
                                    _lib.i32p(_i32([3])), 1, 0.9, TAIL, x.data_ptr(), d, 8,
                                    _lib.i32p(one), _lib.i32p(_i32([4])), _lib.i32p(z),
                                    _lib.i32p(z), _lib.i32p(z), _stream()), 'cif_fire')
