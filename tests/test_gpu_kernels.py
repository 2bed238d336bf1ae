"""Operator tests of the four kernel families that are not GEMMs -- attention, depthwise conv +
norm + SiLU, CMVN + conv1 + ReLU, CTC log-softmax + top-k -- through the hooks wn_op_attention /
wn_op_dwconv / wn_op_conv1 / wn_op_ctc_rows (the model's own launchers and dispatch), against the
plain fp64 references of tests/kernel_refs.py (checked against the oracle on the CPU,
tests/test_kernel_refs.py).

Why: the whole-model tests feed attention the scores of random-init models.  Measured on
`synthetic.make_state_dict` weights behind a LayerNorm (six configs): q and k entries have a
standard deviation of 0.58, the scores q.k / 8 one of 0.335, all of them inside [-1.7, 2.3] -- a
nearly flat softmax whose running maximum hardly moves after the first key tile.  The rescale of
the accumulator, the merge of the key halves / stages and the deferred rescale are then executed
with factors of ~1.  The regimes below make them matter:
  unit        standard normal q, k, v (today's regime)
  peaked      scores of a standard deviation of 10 and 30
  ascending / descending   +-1 per key (the maximum moves in every tile) and +-0.375 per key
              (12 per tile: past the deferred-rescale threshold of 8 in log2 units)
  needle      one key leads by > 40: key 0, 31, 32, the last one, the first key of the second
              half of the key split, the last visible key under the mask
  shifted     every score +-80, V = 100 + unit noise
  tied        q = 0: the output is the plain mean of the visible value rows

Tolerance of every case: err <= margin * e_plain + floor, e_plain = the error of the plain fp32
(bf16) evaluation of the same formula on the same inputs; margin 8 (fp32, six-product) / 4 (bf16),
floor 16 fp32 ulps (2^-9 for bf16) of the output scale -- max |v| over the sequences' keys for
attention, max |ref| otherwise -- and e_plain itself capped at 1e-3 (1e-2) of the scale.  Output
buffers start as a bit pattern that every element no sequence owns must still hold; input rows
no sequence owns hold +-1e18.

Kernel instantiation -> cases that reach it (every attention case asserts the form the dispatch
reports):
  attention_kernel<2,false,1>        test_attention_fp32_forms[plain-1-*], heads, cross, long_h20
  attention_kernel<2,false,2>        test_attention_fp32_forms[plain-2-*], cross[ks2]
  attention_kernel<2,true,1|2>       test_attention_fp32_forms[relpos-*], masks[relpos]
  attention_kernel<2,false,1|2,true> test_attention_fp32_forms[fold-*], regimes[fold], masks[fold]
  (pre-folded kbias form of <2,false,KS> + relpos_fold_kernel)   test_attention_fp32_forms[prefold-*]
  attention_x6_kernel + pack pass    regimes[x6-g0|g1], masks[x6], long[x6]
  attention_bf16_kernel nw 2 / 4 / 8 (fp32 and bf16 inputs, rel-pos)   test_attention_bf16_register
                                     regimes[bf16reg], masks[bf16reg], cross[bf16]
  attention_bf16_dma_kernel<4|8>     test_attention_bf16_dma (defer 80 / 0), regimes[bf16dma], long
  dwconv_kernel<1,2,4,8,12,16,20>, dwconv_tiled_kernel<4|8>            test_dwconv
  cmvn_conv1_kernel, cmvn_conv1_x3_kernel                              test_conv1
  ctc_row_kernel, ctc_row_wave2_kernel<8|72|96>                        test_ctc_rows
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead
PATTERN16 = 0x7fde

KIND = dict(plain=0, relpos=1, fold=2, x6=3, bf16=4, dma=5)
FOLD, PREFOLD, QKV_BF16, O_BF16 = 1, 2, 4, 8


def form_code(kind, ks=1, nw=2, relpos=False, in16=False, kbias=False):
    return KIND[kind] | ks << 4 | nw << 8 | int(relpos) << 12 | int(in16) << 13 | int(kbias) << 14


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


@contextlib.contextmanager
def tune(**kw):
    _lib, L = _L()
    old = {}
    v = ctypes.c_int32(0)
    for k in kw:
        _lib.check(L.wn_tune_get(None, k.encode(), ctypes.byref(v)), 'tune_get')
        old[k] = v.value
    try:
        for k, val in kw.items():
            _lib.check(L.wn_tune_set(k.encode(), val), 'tune_set')
        yield
    finally:
        for k, val in old.items():
            L.wn_tune_set(k.encode(), val)


def record(name, err, e_plain, scale, bf16=False, extra=0.0, check=True):
    """Prints the figures of a case, appends its ratio err / bound to the file
    WN_KERNEL_OPS_RATIOS names (profiles/r21a_kernel_ops_error_ratios.txt is one such run,
    r23a_frontend_error_ratios.txt one of tests/test_gpu_frontend.py), then
    asserts the cap on the yardstick and the bound.  extra: a documented absolute error of the
    kernel's own formula, added to the bound; check=False: figures only (a kernel whose
    arithmetic e_plain is no yardstick for, asserted by its caller against another bound)."""
    b = KR.bound(e_plain, scale, bf16) + extra
    ratio = err / b if b > 0 else (0.0 if err == 0 else float('inf'))
    line = f'{name} err={err:.3e} e_plain={e_plain:.3e} scale={scale:.3e} ratio={ratio:.3f}'
    print(line)
    path = os.environ.get('WN_KERNEL_OPS_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')
    if not check:
        return
    assert KR.cap_ok(e_plain, scale, bf16), line
    assert err <= b, line


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _padded(t, ld, fill=KR.POISON):
    """(rows, d) -> device (rows, ld) with the pad columns poisoned."""
    rows, d = t.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float32)
    buf[:, :d] = t
    return buf.cuda()


# ---------------------------------------------------------------------------------------------
# attention

_REFS = {}


def _case_refs(key, make, bf16):
    """Cases are rebuilt from their key; the references of a key are computed once."""
    if key not in _REFS:
        if len(_REFS) > 6:
            _REFS.clear()
        case = make()
        _REFS[key] = (case, ) + KR.attention_refs(case, bf16)
    return _REFS[key]


def run_attention(case, flags=0, precision=0, galign=0, pads=(0, 0, 0, 4)):
    """Runs wn_op_attention on a case of kernel_refs.make_attention_case.  Returns (O as fp64
    (q_rows, d), form).  Asserts that no element outside the owned rows / the first d columns
    of O changed."""
    _lib, L = _L()
    H, d = case['H'], case['H'] * 64
    seqs = case['seqs']
    ldq, ldk, ldv, ldo = (d + p for p in pads)
    dev = dict(q=_padded(case['q'], ldq), k=_padded(case['k'], ldk), v=_padded(case['v'], ldv))
    if case['pos'] is not None:
        dev.update(pos=case['pos'].cuda(), bu=case['bias_u'].contiguous().cuda(),
                   bv=case['bias_v'].contiguous().cuda())
    o16 = bool(flags & O_BF16)
    if o16:
        O = torch.full((case['q_rows'], ldo), PATTERN16, dtype=torch.int16).cuda()
    else:
        O = torch.full((case['q_rows'], ldo), PATTERN, dtype=torch.int32).cuda()
    arr = [_i32([s[i] for s in seqs]) for i in range(5)]
    op = _lib.WnAttentionOp()
    op.Q, op.K, op.V = dev['q'].data_ptr(), dev['k'].data_ptr(), dev['v'].data_ptr()
    op.ldq, op.ldk, op.ldv = ldq, ldk, ldv
    op.q_rows, op.kv_rows = case['q_rows'], case['kv_rows']
    if case['pos'] is not None:
        op.P, op.ldp, op.p_rows = dev['pos'].data_ptr(), d, case['pos'].shape[0]
        op.p_off = _lib.i32p(arr[4])
        op.bias_u, op.bias_v = dev['bu'].data_ptr(), dev['bv'].data_ptr()
    op.O, op.ldo = O.data_ptr(), ldo
    op.q_off, op.q_len = _lib.i32p(arr[0]), _lib.i32p(arr[1])
    op.kv_off, op.kv_len = _lib.i32p(arr[2]), _lib.i32p(arr[3])
    op.n_seq, op.n_heads = len(seqs), H
    op.mask_mode, op.chunk_size, op.left_chunks = case['mask_mode'], case['chunk'], case['left']
    op.scale = case['scale']
    op.flags, op.precision, op.x6_galign = flags, precision, galign
    form = ctypes.c_int32(-1)
    _lib.check(L.wn_op_attention(ctypes.byref(op), ctypes.byref(form),
                                 torch.cuda.current_stream().cuda_stream), 'attention')
    torch.cuda.synchronize()
    Oc = O.cpu()
    owned = torch.zeros(case['q_rows'], ldo, dtype=torch.bool)
    owned[case['own_q'], :d] = True
    assert bool((Oc[~owned] == (PATTERN16 if o16 else PATTERN)).all()), \
        'a store outside the owned rows / columns of O'
    out = Oc.view(torch.bfloat16).float() if o16 else Oc.view(torch.float32)
    return out[:, :d].double(), form.value


def check_attention(name, key, make, expect_form, bf16=False, **run_kw):
    case, ref, e_plain, scale, w = _case_refs(key, make, bf16)
    out, form = run_attention(case, precision=1 if bf16 else 0, **run_kw)
    assert form == expect_form, (name, hex(form), hex(expect_form))
    own = case['own_q']
    assert torch.isfinite(out[own]).all(), name
    err = (out[own] - ref[own]).abs().max().item()
    record(name, err, e_plain, scale, bf16)
    return w


BATCH_A = [1, 2, 31, 32, 0, 33, 63, 64, 65]          # below the automatic key split
BATCH_B = [127, 128, 0, 129, 255, 257]               # x6 / key split territory
REGIME_IDS = [f'{r}-{p}' for r, p in KR.ATTENTION_REGIMES]


def _assert_non_flat(regime, w, case_is_masked_needle=False):
    if regime in KR.NON_FLAT and not case_is_masked_needle:
        share = (w > 0.5).double().mean().item()
        assert share >= KR.NON_FLAT[regime], (regime, share)


@pytest.mark.parametrize('xcd', [1, 0])
@pytest.mark.parametrize('split', [1, 2])
@pytest.mark.parametrize('form', ['plain', 'relpos', 'fold', 'prefold'])
def test_attention_fp32_forms(form, split, xcd):
    """Every fp32 v_mfma_f32 form x key split x block order, on both packed batches, unit and
    peaked data."""
    relpos = form != 'plain'
    flags = {'plain': 0, 'relpos': 0, 'fold': FOLD, 'prefold': PREFOLD}[form]
    expect = form_code('plain' if form == 'prefold' else form, ks=split, kbias=form == 'prefold')
    for bi, lens in enumerate((BATCH_A, BATCH_B)):
        for regime, param in (('unit', None), ('peaked', 10.0)):
            key = ('forms', relpos, bi, regime)
            make = lambda: KR.regime_case(regime, param, H=4, q_lens=lens, relpos=relpos,
                                          seed=3 + bi)
            with tune(attn_split=split, attn_xcd=xcd, attn_x6=0):
                check_attention(f'attn_fp32[{form}-ks{split}-xcd{xcd}-b{bi}-{regime}]', key, make,
                                expect, flags=flags, pads=(4, 8, 12, 4))


@pytest.mark.parametrize('H', [1, 8, 20])
def test_attention_heads(H):
    for relpos, flags, kind in ((False, 0, 'plain'), (True, FOLD, 'fold')):
        key = ('heads', H, relpos)
        make = lambda: KR.regime_case('peaked', 10.0, H=H, q_lens=BATCH_A, relpos=relpos, seed=H)
        with tune(attn_x6=0):
            check_attention(f'attn_heads[{kind}-h{H}]', key, make, form_code(kind, ks=1), flags=flags)
    # bf16: register-staged with fp32 inputs, and bf16 Q | K | V
    make = lambda: KR.regime_case('peaked', 10.0, H=H, q_lens=BATCH_A, seed=H, bf16=True)
    check_attention(f'attn_heads[bf16-h{H}]', ('heads16', H), make, form_code('bf16', nw=2),
                    bf16=True)
    check_attention(f'attn_heads[bf16in-h{H}]', ('heads16', H), make,
                    form_code('bf16', nw=2, in16=True), bf16=True, flags=QKV_BF16 | O_BF16,
                    pads=(0, 0, 0, 8))


def _regime_forms():
    # (id, kwargs of the case, bf16, tune knobs, run kwargs, expected form)
    return [
        ('fold', dict(relpos=True), False, dict(attn_x6=0, attn_split=2), dict(flags=FOLD),
         form_code('fold', ks=2)),
        ('x6-g0', dict(relpos=True), False, dict(attn_x6=1), dict(flags=FOLD, galign=0),
         form_code('x6', ks=2)),
        ('x6-g1', dict(relpos=True), False, dict(attn_x6=1), dict(flags=FOLD, galign=1),
         form_code('x6', ks=2)),
        ('bf16reg', dict(relpos=True), True, dict(attn_bf16_nw=4), dict(),
         form_code('bf16', nw=4, relpos=True)),
        ('bf16dma', dict(), True, dict(attn_bf16_nw=4), dict(flags=QKV_BF16 | O_BF16),
         form_code('dma', nw=4, in16=True)),
    ]


@pytest.mark.parametrize('fi', range(5), ids=[f[0] for f in _regime_forms()])
@pytest.mark.parametrize('regime', KR.ATTENTION_REGIMES, ids=REGIME_IDS)
def test_attention_regimes(regime, fi):
    fid, ckw, bf16, knobs, rkw, expect = _regime_forms()[fi]
    key = ('regimes', regime, bf16, tuple(sorted(ckw)))
    make = lambda: KR.regime_case(regime[0], regime[1], H=4, q_lens=BATCH_B, seed=17, bf16=bf16,
                                  **ckw)
    with tune(**knobs):
        w = check_attention(f'attn_regimes[{fid}-{regime[0]}-{regime[1]}]', key, make, expect,
                            bf16=bf16, **rkw)
    # (ramps of bf16-representable keys tie above 256: the weights are judged on the fp32 cases)
    if not bf16:
        _assert_non_flat(regime, w)


MASKS = [(1, 0, -1)] + [(2, c, l) for c in (1, 4, 16) for l in (-1, 0, 1, 3)]
MASK_REGIMES = [('unit', None), ('peaked', 10.0), ('needle', 'last_visible'), ('ascending', 1.0)]


@pytest.mark.parametrize('form', ['relpos', 'fold', 'x6', 'bf16reg', 'bf16in'])
@pytest.mark.parametrize('mi', range(len(MASKS)), ids=[f'm{m}c{c}l{l}' for m, c, l in MASKS])
def test_attention_masks(mi, form):
    mode, chunk, left = MASKS[mi]
    regime = MASK_REGIMES[mi % 4]
    bf16 = form.startswith('bf16')
    relpos = form != 'bf16in'
    lens = [65, 2, 0, 130, 31, 200]
    key = ('masks', mi, bf16, relpos)
    make = lambda: KR.regime_case(regime[0], regime[1], H=4, q_lens=lens, relpos=relpos,
                                  mask_mode=mode, chunk=chunk, left=left, seed=23 + mi, bf16=bf16)
    knobs, rkw, expect = {
        'relpos': (dict(attn_x6=0, attn_split=1), dict(), form_code('relpos', ks=1)),
        'fold': (dict(attn_x6=0), dict(flags=FOLD), form_code('fold', ks=2)),
        'x6': (dict(attn_x6=2), dict(flags=FOLD, galign=mi % 2), form_code('x6', ks=2)),
        'bf16reg': (dict(), dict(), form_code('bf16', nw=2, relpos=True)),
        # (a mask keeps bf16 Q | K | V on the register-staged kernel)
        'bf16in': (dict(attn_bf16_nw=8), dict(flags=QKV_BF16),
                   form_code('bf16', nw=8, in16=True)),
    }[form]
    with tune(**knobs):
        w = check_attention(f'attn_masks[{form}-m{mode}c{chunk}l{left}-{regime[0]}]', key, make,
                            expect, bf16=bf16, **rkw)
    if not bf16:
        _assert_non_flat(regime, w)


@pytest.mark.parametrize('nw', [2, 4, 8])
def test_attention_bf16_register(nw):
    """attention_bf16_kernel with 2 / 4 / 8 waves: fp32 inputs with and without the rel-pos term,
    bf16 inputs (attn_bf16_dma = 0 keeps them off the DMA kernel)."""
    for regime, param in (('unit', None), ('peaked', 10.0), ('descending', 1.0)):
        for relpos in (False, True):
            key = ('bf16reg', regime, relpos)
            make = lambda: KR.regime_case(regime, param, H=4, q_lens=BATCH_B, relpos=relpos,
                                          seed=29, bf16=True)
            with tune(attn_bf16_nw=nw):
                check_attention(f'attn_bf16reg[nw{nw}-{regime}-relpos{int(relpos)}]', key, make,
                                form_code('bf16', nw=nw, relpos=relpos), bf16=True,
                                pads=(4, 8, 12, 4))
        key = ('bf16reg', regime, False)
        make = lambda: KR.regime_case(regime, param, H=4, q_lens=BATCH_B, seed=29, bf16=True)
        with tune(attn_bf16_nw=nw, attn_bf16_dma=0):
            check_attention(f'attn_bf16reg[nw{nw}-{regime}-in16]', key, make,
                            form_code('bf16', nw=nw, in16=True), bf16=True,
                            flags=QKV_BF16 | O_BF16, pads=(0, 0, 0, 8))


@pytest.mark.parametrize('defer', [80, 0])
@pytest.mark.parametrize('nw', [4, 8])
def test_attention_bf16_dma(nw, defer):
    """The LDS-DMA kernel with the deferred rescale on (threshold 8.0) and off; the +-0.375 per
    key ramps move the maximum by 12 per tile, the +-1 ramps by 32."""
    for regime, param in (('unit', None), ('ascending', 0.375), ('ascending', 1.0),
                          ('descending', 0.375), ('peaked', 30.0), ('needle', 'second_half')):
        key = ('dma', regime, param)
        make = lambda: KR.regime_case(regime, param, H=4, q_lens=BATCH_B + [33, 1], seed=31,
                                      bf16=True)
        with tune(attn_bf16_nw=nw, attn_bf16_defer=defer):
            check_attention(f'attn_bf16dma[nw{nw}-defer{defer}-{regime}-{param}]', key, make,
                            form_code('dma', nw=nw, in16=True), bf16=True,
                            flags=QKV_BF16 | O_BF16, pads=(0, 0, 0, 8))


@pytest.mark.parametrize('regime', [('unit', None), ('peaked', 10.0), ('needle', 'last'),
                                    ('shifted', 80.0), ('tied', None)],
                         ids=lambda r: f'{r[0]}-{r[1]}')
def test_attention_cross(regime):
    """Decoder-style cross attention: q_len 1 .. 40 against kv_len up to 300, separate layouts."""
    q_lens, kv_lens = [1, 40, 7, 0, 33], [300, 77, 1, 0, 129]
    for bf16 in (False, True):
        key = ('cross', regime, bf16)
        make = lambda: KR.regime_case(regime[0], regime[1], H=4, q_lens=q_lens, kv_lens=kv_lens,
                                      seed=37, bf16=bf16)
        if bf16:
            check_attention(f'attn_cross[bf16-{regime[0]}]', key, make, form_code('bf16', nw=2),
                            bf16=True)
            check_attention(f'attn_cross[bf16in-{regime[0]}]', key, make,
                            form_code('bf16', nw=2, in16=True), bf16=True, flags=QKV_BF16)
        else:
            for ks in (1, 2):
                with tune(attn_split=ks):
                    check_attention(f'attn_cross[ks{ks}-{regime[0]}]', key, make,
                                    form_code('plain', ks=ks), pads=(4, 0, 8, 4))


@pytest.mark.parametrize('regime', [('unit', None), ('peaked', 30.0), ('ascending', 1.0),
                                    ('shifted', -80.0)], ids=lambda r: f'{r[0]}-{r[1]}')
def test_attention_long(regime):
    """1500 frames next to a short sequence: the automatic choices of every mode."""
    lens = [1500, 33]
    key = ('long', regime, False)
    make = lambda: KR.regime_case(regime[0], regime[1], H=2, q_lens=lens, relpos=True, seed=41)
    with tune(attn_x6=0):      # automatic key split (max_q_len >= 128 with the rel-pos term)
        check_attention(f'attn_long[fold-{regime[0]}]', key, make, form_code('fold', ks=2),
                        flags=FOLD)
    for g in (0, 1):
        check_attention(f'attn_long[x6-g{g}-{regime[0]}]', key, make, form_code('x6', ks=2),
                        flags=FOLD, galign=g)
    key = ('long', regime, True)
    make = lambda: KR.regime_case(regime[0], regime[1], H=2, q_lens=lens, relpos=True, seed=41,
                                  bf16=True)
    check_attention(f'attn_long[bf16reg-{regime[0]}]', key, make,
                    form_code('bf16', nw=8, relpos=True), bf16=True)
    key = ('long-plain', regime, True)
    make = lambda: KR.regime_case(regime[0], regime[1], H=2, q_lens=lens, seed=41, bf16=True)
    # (the DMA kernel keeps four waves for long sequences too)
    check_attention(f'attn_long[bf16dma-{regime[0]}]', key, make,
                    form_code('dma', nw=4, in16=True), bf16=True, flags=QKV_BF16 | O_BF16,
                    pads=(0, 0, 0, 8))


def test_attention_long_h20():
    """The Whisper-large shape: 20 heads, 1500 frames, no rel-pos term."""
    make = lambda: KR.regime_case('peaked', 10.0, H=20, q_lens=[1500], seed=43)
    check_attention('attn_h20[plain]', ('h20', False), make, form_code('plain', ks=1))
    make = lambda: KR.regime_case('peaked', 10.0, H=20, q_lens=[1500], seed=43, bf16=True)
    check_attention('attn_h20[bf16dma]', ('h20', True), make, form_code('dma', nw=4, in16=True),
                    bf16=True, flags=QKV_BF16 | O_BF16, pads=(0, 0, 0, 8))


def test_attention_rejects_bad_arguments():
    _lib, L = _L()
    case = KR.regime_case('unit', None, H=1, q_lens=[5])

    def call(**kw):
        c = dict(case)
        c.update(kw)
        try:
            run_attention(c)
        except (RuntimeError, AssertionError) as e:
            return str(e)
        return None

    # keys past the end of the K / V buffer, a sequence with queries and no keys, a chunk mask
    # without a chunk size: refused on the host, nothing is launched
    assert 'key rows outside' in call(seqs=[(5, 5, 5, 60, 0)])
    assert 'queries without keys' in call(seqs=[(5, 5, 5, 0, 0)])
    assert 'query rows outside' in call(seqs=[(10, 5, 5, 5, 0)])
    assert 'position rows outside' in call(
        **{**KR.regime_case('unit', None, H=1, q_lens=[5], relpos=True), 'seqs': [(5, 5, 5, 5, 9)]})
    assert 'chunk size' in call(mask_mode=2, chunk=0)
    assert 'mask mode' in call(mask_mode=3)


# ---------------------------------------------------------------------------------------------
# depthwise conv


def run_dwconv(c):
    _lib, L = _L()
    D, M = c['D'], c['M']
    ldx, ldy = D + c['pad_ld'], D + 2 * c['pad_ld']
    x = _padded(c['x'], ldx)
    y = torch.full((M, ldy), PATTERN, dtype=torch.int32).cuda()
    t = {k: c[k].contiguous().cuda() for k in ('wt', 'bias', 'cpad', 'ln_w', 'ln_b')}
    off, lens = _i32(c['off']), _i32(c['lens'])
    _lib.check(L.wn_op_dwconv(x.data_ptr(), ldx, t['wt'].data_ptr(), t['bias'].data_ptr(),
                              t['cpad'].data_ptr(), t['ln_w'].data_ptr(), t['ln_b'].data_ptr(),
                              c['norm_mode'], y.data_ptr(), ldy, _lib.i32p(off), _lib.i32p(lens),
                              len(lens), M, D, c['K'], int(c['causal']), c['t_max'], c['eps'],
                              torch.cuda.current_stream().cuda_stream), 'dwconv')
    torch.cuda.synchronize()
    yc = y.cpu()
    owned = torch.zeros(M, ldy, dtype=torch.bool)
    owned[c['own'], :D] = True
    assert bool((yc[~owned] == PATTERN).all()), 'a store outside the owned rows / columns of y'
    return yc.view(torch.float32)[:, :D]


DW_K = [(2, True), (7, True), (8, True), (9, True), (16, True), (17, True), (3, False),
        (7, False), (9, False), (15, False), (17, False), (31, False), (33, False)]


@pytest.mark.parametrize('norm_mode', [0, 1])
@pytest.mark.parametrize('K,causal', DW_K)
@pytest.mark.parametrize('D', [64, 128, 256, 512, 768, 1024, 1280])
def test_dwconv(D, K, causal, norm_mode):
    """Every width (E = 1 .. 20) on both sides of every tap-group edge (groups of 8; of 4 for
    E > 8), lengths around the kernel size packed so that 4-row tiles straddle utterances."""
    i = K + D // 64 + norm_mode
    lens = [1, 2, 3, 4, 5, max(K - 1, 1), K, K + 1, 0, 100]
    c = KR.make_dwconv_case(D, K, causal, norm_mode, lens, seed=D + K, gap=i % 2, lead=(i // 2) % 3,
                            t_extra=3 * (i % 2), pad_ld=4 * (1 + i % 2), tail=3)
    if c['M'] % 16 == 0:
        c = KR.make_dwconv_case(D, K, causal, norm_mode, lens, seed=D + K, gap=i % 2,
                                lead=(i // 2) % 3, t_extra=3 * (i % 2), pad_ld=4 * (1 + i % 2),
                                tail=4)
    assert c['M'] % 16 != 0
    ref, e_plain, scale = KR.dwconv_refs(c)
    own = c['own']
    got = run_dwconv(c)
    name = f'dwconv[D{D}-K{K}-{"causal" if causal else "sym"}-norm{norm_mode}]'
    if D in (256, 512):
        # the tiled kernel and the row-per-wave kernel: bit for bit
        with tune(dwconv_tiled=0):
            got0 = run_dwconv(c)
        assert torch.equal(got[own].view(torch.int32), got0[own].view(torch.int32)), name
    assert torch.isfinite(got[own]).all(), name
    record(name, (got[own].double() - ref[own]).abs().max().item(), e_plain, scale)


@pytest.mark.parametrize('K,causal', [(8, True), (15, False)])
@pytest.mark.parametrize('D', [64, 128, 256, 512, 768, 1024, 1280])
def test_dwconv_common_offset(D, K, causal):
    """Rows of +-50 + unit noise: the LayerNorm has to cancel the offset."""
    c = KR.make_dwconv_case(D, K, causal, 0, [5, 100, K, 3], seed=D, gap=1, lead=1, t_extra=2,
                            pad_ld=4, offset=50.0)
    ref, e_plain, scale = KR.dwconv_refs(c)
    got = run_dwconv(c)
    own = c['own']
    record(f'dwconv_offset[D{D}-K{K}]', (got[own].double() - ref[own]).abs().max().item(),
           e_plain, scale)


def test_dwconv_rejects_bad_arguments():
    _lib, L = _L()
    c = KR.make_dwconv_case(64, 3, False, 0, [4])
    for kw, msg in ((dict(D=96), 'unsupported width'), (dict(K=4), 'odd size'),
                    (dict(lens=[400]), 'rows outside'), (dict(t_max=2), 't_max')):
        cc = dict(c)
        cc.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            run_dwconv(cc)


# ---------------------------------------------------------------------------------------------
# CMVN + conv1 + ReLU


def run_conv1(c, plane):
    _lib, L = _L()
    feats = c['feats'].cuda()
    mean = c['mean'].cuda() if c['mean'] is not None else None
    istd = c['istd'].cuda() if c['istd'] is not None else None
    w9 = c['w'].reshape(c['C'], 9).t().contiguous().cuda()           # [9][C] tap-major
    bias = c['bias'].cuda()
    out = torch.full((c['rows'], c['F1'], c['C']), PATTERN, dtype=torch.int32).cuda()
    off, lens = _i32(c['off']), _i32(c['t1_lens'])
    _lib.check(L.wn_op_conv1(feats.data_ptr(), mean.data_ptr() if mean is not None else None,
                             istd.data_ptr() if istd is not None else None, w9.data_ptr(),
                             bias.data_ptr(), out.data_ptr(), _lib.i32p(off), _lib.i32p(lens),
                             c['B'], c['T'], c['F'], c['C'], c['rows'], int(plane),
                             torch.cuda.current_stream().cuda_stream), 'conv1')
    torch.cuda.synchronize()
    oc = out.cpu()
    owned = torch.zeros(c['rows'], dtype=torch.bool)
    for o, n in zip(c['off'], c['t1_lens']):
        owned[o:o + n] = True
    assert bool((oc[~owned] == PATTERN).all()), 'a store into frames no utterance owns'
    return oc.view(torch.float32), owned


@pytest.mark.parametrize('cmvn', [True, False])
@pytest.mark.parametrize('C', [32, 64, 256, 512, 1280])
@pytest.mark.parametrize('Fdim', [7, 23, 80, 127, 128])
def test_conv1(Fdim, C, cmvn):
    """t1_len 1, 2, 15, 16, 17 around the 16 frames a block of the plane kernel walks, an empty
    utterance in the middle; the plane-image form equals the fp32 form bit for bit."""
    c = KR.make_conv1_case(Fdim, C, [17, 1, 0, 16, 2, 15], cmvn=cmvn, seed=Fdim * 7 + C)
    ref, e_plain, scale = KR.conv1_refs(c)
    got, owned = run_conv1(c, plane=False)
    err = max((got[o:o + n].double() - r).abs().max().item()
              for o, n, r in zip(c['off'], c['t1_lens'], ref) if n)
    assert torch.isfinite(got[owned]).all()
    assert c['F1'] <= 64 and C % 32 == 0          # every listed shape has the plane form
    got3, _ = run_conv1(c, plane=True)
    name = f'conv1[F{Fdim}-C{C}-cmvn{int(cmvn)}]'
    assert torch.equal(got3[owned].view(torch.int32), got[owned].view(torch.int32)), name
    record(name, err, e_plain, scale)


def test_conv1_rejects_bad_arguments():
    c = KR.make_conv1_case(23, 32, [3])
    for kw, msg in ((dict(F=129), 'feature dim'), (dict(T=6), 'too short'),
                    (dict(t1_lens=[500]), 'frames outside')):
        cc = dict(c)
        cc.update(kw)
        with pytest.raises(RuntimeError, match=msg):
            run_conv1(cc, plane=False)
    cc = dict(c)
    cc['C'], cc['w'], cc['bias'] = 48, torch.zeros(48, 1, 3, 3), torch.zeros(48)
    with pytest.raises(RuntimeError, match='plane image shape'):
        run_conv1(cc, plane=True)


# ---------------------------------------------------------------------------------------------
# CTC rows


def run_ctc(x, k, blank, penalty, want_logp, ld_pad=3):
    _lib, L = _L()
    M, V = x.shape
    ld = V + ld_pad
    xd = _padded(x, ld)
    val = torch.full((M, k), PATTERN, dtype=torch.int32).cuda()
    idx = torch.full((M, k), -7, dtype=torch.int32).cuda()
    ld_out = V + 5
    logp = torch.full((M, ld_out), PATTERN, dtype=torch.int32).cuda() if want_logp else None
    _lib.check(L.wn_op_ctc_rows(xd.data_ptr(), ld, M, V, k, blank, penalty, val.data_ptr(),
                                idx.data_ptr(), logp.data_ptr() if want_logp else None, ld_out,
                                torch.cuda.current_stream().cuda_stream), 'ctc_rows')
    torch.cuda.synchronize()
    lp = None
    if want_logp:
        lc = logp.cpu()
        assert bool((lc[:, V:] == PATTERN).all()), 'a store past column V of logp'
        lp = lc.view(torch.float32)[:, :V].double()
    return val.cpu().view(torch.float32).double(), idx.cpu().long(), lp


def check_ctc(name, x, k, blank, penalty, want_logp, wave):
    M, V = x.shape
    logp, rval, ridx, e_plain, scale = KR.ctc_refs(x, blank, penalty, k)
    with tune(ctc_wave=wave):
        val, idx, lp = run_ctc(x, k, blank, penalty, want_logp)
    tol = KR.bound(e_plain, scale)
    assert torch.isfinite(val).all(), name
    err = (val - rval).abs().max().item()
    # indices: exact where the fp64 neighbours of the sorted row are further apart than the value
    # tolerance, otherwise any valid answer
    srt = logp.sort(dim=1, descending=True).values[:, :min(k + 1, V)]
    gaps = srt[:, :-1] - srt[:, 1:]                       # (M, k) or (M, k - 1) when k == V
    clear = torch.ones(M, k, dtype=torch.bool)
    clear[:, :gaps.shape[1]] &= gaps > tol                # gap below rank r
    clear[:, 1:] &= gaps[:, :k - 1] > tol                 # gap above rank r
    assert bool((idx[clear] == ridx[clear]).all()), name
    assert bool(((idx >= 0) & (idx < V)).all()), name
    assert all(len(set(r.tolist())) == k for r in idx), name + ': repeated index'
    assert ((logp.gather(1, idx) - val).abs().max().item() <= tol) or V == 1, name
    assert bool((val[:, :-1] >= val[:, 1:]).all()), name
    if lp is not None:
        assert torch.isfinite(lp).all(), name
        err = max(err, (lp - logp).abs().max().item())
        assert torch.logsumexp(lp, dim=1).abs().max().item() <= tol + 16 * KR.ULP32, name
    record(name, err, e_plain, scale)
    return idx, clear.all(dim=1)


CTC_V = [1, 2, 63, 64, 65, 511, 512, 513, 4233, 4607, 4608, 4609, 5002, 6144, 6145, 11008, 30720]
CTC_REGIMES = ['randn', 'shift_up', 'shift_down', 'spread', 'ties']


@pytest.mark.parametrize('V', CTC_V)
def test_ctc_rows(V):
    """Both sides of every dispatch edge (V = 512, 4608, 6144; k = 16; with / without logp;
    ctc_wave), every regime, the wave kernels against the block kernel."""
    vi = CTC_V.index(V)
    ks = sorted({k for k in (1, 4, 10, 16, 17) if k <= V} | ({V} if V <= 65 else set()))
    for ki, k in enumerate(ks):
        M = [1, 3, 4, 5][(vi + ki) % 4]
        blank, penalty = [(0, 0.0), (0, 1.5), (V // 2, 1.5), (V - 1, 0.0)][(vi + ki) % 4]
        x = KR.make_ctc_case(CTC_REGIMES[(vi + ki) % 5], M, V, blank=blank, seed=V + k)
        tag = f'V{V}-k{k}-M{M}-b{blank}-p{penalty}'
        got = {}
        for wave in (1, 0):
            for want_logp in (False, True):
                got[(wave, want_logp)] = check_ctc(f'ctc[{tag}-wave{wave}-logp{int(want_logp)}]',
                                                   x, k, blank, penalty, want_logp, wave)
        idx_w, untied = got[(1, False)]
        idx_b, _ = got[(0, False)]
        assert torch.equal(idx_w[untied], idx_b[untied]), tag


@pytest.mark.parametrize('regime', CTC_REGIMES)
@pytest.mark.parametrize('V', [4233, 5002])
def test_ctc_rows_regimes(V, regime):
    x = KR.make_ctc_case(regime, 37, V, blank=0, seed=V)
    for wave, want_logp in ((1, False), (0, False), (0, True)):
        check_ctc(f'ctc_regime[V{V}-{regime}-wave{wave}-logp{int(want_logp)}]', x, 10, 0, 1.5,
                  want_logp, wave)


@pytest.mark.parametrize('V', [512, 4233])
def test_ctc_rows_many_rows(V):
    x = KR.make_ctc_case('randn', 4097, V, blank=0, seed=V)
    for wave, want_logp in ((1, False), (0, True)):
        check_ctc(f'ctc_rows4097[V{V}-wave{wave}]', x, 10, 0, 0.0, want_logp, wave)


def test_ctc_rows_rejects_bad_arguments():
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match='top-k'):
        run_ctc(x, 9, 0, 0.0, False)
    with pytest.raises(RuntimeError, match='blank'):
        run_ctc(x, 2, 8, 0.0, False)
    with pytest.raises(RuntimeError, match='too large'):
        run_ctc(torch.zeros(1, 30721), 4, 0, 0.0, True)
