"""Operator tests of the subsampling front ends behind conv1, against fp64, on every route.

Conformer (Conv2dSubsampling4, csrc/model.hip subsample_conv2d4) through the hook wn_op_conv2d4,
which stops after the front end, hands out conv1's activations as conv2 read them, conv2's output
and the packed rows, and reports the route the launch code took.  Three comparisons per case
(tests/kernel_refs.py frontend_refs; CPU checks in tests/test_kernel_refs.py):
  c2       against ref_conv2 of the GPU's own c1     -- conv2 alone: the pixel / row tables, the
           tap order, the weight reorder [d][(ky 3 + kx) d + c] and its plane image, the tiles
  x_proj   against ref_sub_out of the GPU's own c2   -- the projection alone: the c f -> f c
           permutation of out.0.weight, the K slices and their reduction, the sqrt(d) scale
  x_chain  against the oracle's global_cmvn + conv2d_subsampling4 in fp64 from the features
with the yardstick of test_gpu_kernels.py: err <= 8 e_plain + 16 fp32 ulps of the scale, e_plain
(the fp32 CPU evaluation of the same step against fp64) capped at 1e-3 of the scale.  e_plain is
2-5e-7 of the scale here, the bound ~5e-6: 200 times tighter than the 1e-3 of
test_encoder_layers_vs_oracle.

Every case asserts the route code it was written for, runs twice (bit equality), checks the
lengths, and poisons the feature frames at and beyond 4 l2 + 3 of every utterance (what no kept
output frame reads).

Route -> cases (kind / tile / projection as reported):
  v_mfma_f32 gathered GEMM, linear()                      small[*-f32]
  six-product, plane image, one launch of 128-row tiles   small[*-planes128], small[*-planes0],
                                                          projection[*], tiles[d64-below-two-rounds],
                                                          tiles[d512-m3500]
  six-product, fp32 gather, 128-row tiles                 small[*-af32]
  six-product, fp32 gather, 256-row tiles + 128-row rest  tiles[d64-m3500-af32]
  plane image, 256-row tiles + K-slice tail (4 slices)    tiles[d64-m3500], tiles[d256-m3500]
  plane image, one launch of 256-row tiles                tiles[d64-three-rounds]
  projection as K slices + ffn_reduce_ln                  projection[*-above], tiles[d256 / d512]
  projection as linear()                                  everything else

x6_conv_bm = 0 does not mean 256-row tiles at every size, and the cases assert what the launch
code reports: below two rounds of 256 tiles gemm_x6_bm() picks 128-row tiles (M F2 < 65 536 runs
as ONE launch of 128-row tiles), and at N = 512 the split into 256-row tiles + remainder is not
taken at all (N > 256): gemm_x6_bm() again picks one launch of 128-row tiles for 66 500 rows.  A
launch of 256-row tiles alone needs >= 512 tiles: tiles[d64-three-rounds].  With the plane image
the remainder never runs as 128-row tiles from the model (the K-slice scratch is always there and
9 d / 16 k blocks always divide by 2 or 3); the fp32 gather reaches that launch.

Whisper (Conv1dSubsampling2 in encode_transformer): wn_encode with wn_debug_set n_layers = 0,
skip_after_norm = 1 against the oracle's conv1d_subsampling2 in fp64 on the zero-padded batch.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as KR
from test_gpu_kernels import _L, record, tune

pytestmark = pytest.mark.gpu

F32, AF32, PLANES = 0, 1, 2                      # conv2 kind
T128, T256, T256_REM128, T256_KTAIL = 0, 1, 2, 3  # tile form


def route(kind, tile=T128, slices=0, sub_out=0, linear_x6=0):
    return kind | tile << 4 | slices << 8 | sub_out << 12 | linear_x6 << 13 | 1 << 16


_MODELS = {}


def _model(F_in, d, whisper=False):
    """One model per (F, d): tiny_lite / whisper_tiny_like with one block."""
    from gpu_util import make_model
    key = (F_in, d, whisper)
    if key not in _MODELS:
        configs, sd = KR.frontend_model_parts(F_in, d, whisper)
        _MODELS[key] = (sd, make_model(configs, sd))
    return _MODELS[key]


def _lens_of(l2, extra):
    """Feature lengths with l2 output frames: 4 l2 + 3 + extra, extra in 0..3 (0 -> 6 - extra)."""
    return [4 * n + 3 + e if n else 6 - e for n, e in zip(l2, extra)]


def _run(model, feats_dev, lens, F_in, d):
    """wn_op_conv2d4 -> (c1, c2, x on the CPU, enc_lens, route code); outputs start as NaN."""
    _lib, L = _L()
    l2 = KR.sub4_lens(lens)
    M, M1 = sum(l2), sum(2 * n + 1 for n in l2 if n)
    F1 = (F_in - 1) // 2
    F2 = (F1 - 1) // 2
    nan = float('nan')
    c1 = torch.full((M1, F1, d), nan, device='cuda')
    c2 = torch.full((M, F2, d), nan, device='cuda')
    x = torch.full((M, d), nan, device='cuda')
    enc = np.full(len(lens), -1, np.int32)
    code = ctypes.c_int32(-1)
    B, T, _ = feats_dev.shape
    _lib.check(L.wn_op_conv2d4(model._h, feats_dev.data_ptr(), _lib.i32p(np.asarray(lens, np.int32)),
                               B, T, c1.data_ptr(), c2.data_ptr(), x.data_ptr(), _lib.i32p(enc),
                               ctypes.byref(code), None), 'wn_op_conv2d4')
    return c1.cpu(), c2.cpu(), x.cpu(), enc.tolist(), code.value


def _split(t, sizes):
    return list(torch.split(t, sizes))


def _err(got, ref):
    return max([(g.double() - r).abs().max().item() for g, r in zip(got, ref) if r.numel()] +
               [0.0])


def _case(name, F_in, d, feats, lens, want_route, utts=None):
    """Runs one case twice, asserts route / lengths / bit equality and the three comparisons.
    Returns (c1, c2, x, per-utterance c2 references of the evaluated utterances, utts)."""
    sd, model = _model(F_in, d)
    l2 = KR.sub4_lens(lens)
    dev = feats.cuda()
    c1, c2, x, enc, code = _run(model, dev, lens, F_in, d)
    assert code == want_route, f'{name}: route {code:#x}, written for {want_route:#x}'
    assert enc == l2, name
    c1b, c2b, xb, encb, codeb = _run(model, dev, lens, F_in, d)
    assert codeb == code and encb == enc
    assert torch.equal(c1, c1b) and torch.equal(c2, c2b) and torch.equal(x, xb), \
        f'{name}: two runs differ'
    assert torch.isfinite(c1).all() and torch.isfinite(c2).all() and torch.isfinite(x).all(), name
    c1l = _split(c1, [2 * n + 1 if n else 0 for n in l2])
    c2l = _split(c2, l2)
    xl = _split(x, l2)
    refs, utts = KR.frontend_refs(feats, lens, sd, d, c1l, c2l, utts)
    for what, got in (('c2', c2l), ('x_proj', xl), ('x_chain', xl)):
        ref, e_plain, scale = refs[what]
        record(f'frontend[{name} {what}]', _err([got[b] for b in utts], ref), e_plain, scale)
    return c1, c2, x, refs, utts


# ---------------------------------------------------------------------------------------------
# small shapes, every conv2 kind

SMALL_T = 90
SMALL_LENS = [7, 6, 10, 11, 0, 75, SMALL_T]      # l2 = 1, 0, 1, 2, 0, 18, 21: M = 43

# (tune settings, conv2 kind where F1 <= 64)
SMALL_ROUTES = [
    ('f32', dict(gemm_x6=0), F32),
    ('planes128', dict(gemm_x6=2, x6_conv_bm=128), PLANES),
    ('planes0', dict(gemm_x6=2, x6_conv_bm=0), PLANES),
    ('af32', dict(gemm_x6=2, x6_conv_af32=1), AF32),
]


@pytest.mark.parametrize('F_in,d', [(23, 64), (80, 128), (81, 64), (128, 64), (80, 256), (80, 512)])
def test_small_every_kind(F_in, d):
    """One ragged batch -- a single output frame, two empty utterances in the middle, both sides
    of the 4 k + 7 step, one utterance that fills the tensor -- on the four tune settings.
    F = 23: F1 = 11, F2 = 5; F = 81: an even F1 = 40 (ne = 20 = F2 + 1); F = 128: F1 = 63, the
    last width the plane form takes.  M = 43 stays below every size threshold: 128-row tiles,
    linear() as the v_mfma_f32 GEMM.  c1 must be the same bits on every route."""
    lens = SMALL_LENS
    assert KR.sub4_lens(lens) == [1, 0, 1, 2, 0, 18, 21]
    feats = KR.make_frontend_feats(lens, F_in, seed=F_in + d)
    assert (F_in - 1) // 2 <= 64
    c1_first = None
    for tag, knobs, kind in SMALL_ROUTES:
        with tune(**knobs):
            c1, _, _, _, _ = _case(f'small F{F_in} d{d} {tag}', F_in, d, feats, lens, route(kind))
        if c1_first is None:
            c1_first = c1
        assert torch.equal(c1, c1_first), f'F{F_in} d{d} {tag}: c1 differs from the fp32 route'


# ---------------------------------------------------------------------------------------------
# the output projection as K slices / as linear()


@pytest.mark.parametrize('d', [256, 512])
def test_projection_both_forms(d):
    """M = 515: sub_out_linear (K slices + ffn_reduce_ln); the same batch with the last utterance
    six frames shorter, M = 509 < 512: linear().  Default tune set (the shipped routes: plane
    image, one launch of 128-row tiles)."""
    l2 = [200, 0, 1, 150, 164]
    extra = [0, 1, 2, 3, 1]
    lens = _lens_of(l2, extra)
    feats = KR.make_frontend_feats(lens, 80, seed=d)
    _case(f'projection d{d} above', 80, d, feats, lens, route(PLANES, sub_out=1))
    l2b = l2[:-1] + [158]
    lens_b = _lens_of(l2b, extra)
    assert sum(l2) == 515 and sum(l2b) == 509
    feats_b = KR.make_frontend_feats(lens_b, 80, seed=d, T=feats.shape[1])
    _case(f'projection d{d} below', 80, d, feats_b, lens_b, route(PLANES, sub_out=0))


# ---------------------------------------------------------------------------------------------
# tile forms of the 256-row conv2 (x6_conv_bm = 0)

# M = 3500 -> 66 500 GEMM rows = 259 full 256-row tiles + 196 rows: t256 = 260, one round of 256
# tiles + 4, the last one partial.  Rows from 65 536 on (frame 3449, row 5 of it) are the tail.
L2_3500 = [120, 1100, 1, 0, 900, 130, 950, 250, 49]
EXTRA_3500 = [0, 1, 2, 3, 3, 2, 1, 0, 3]
FULL_ROWS = 256 * 256


def _batch_3500(seed):
    assert sum(L2_3500) == 3500
    lens = _lens_of(L2_3500, EXTRA_3500)
    return KR.make_frontend_feats(lens, 80, seed=seed), lens


def _tail_err(c2, refs, utts, l2):
    """max |c2 - ref| over the GEMM rows from FULL_ROWS on, and the rows it covered."""
    off = np.concatenate([[0], np.cumsum(l2)])
    err, rows = 0.0, 0
    for r, b in zip(refs['c2'][0], utts):
        lo, hi = off[b] * 19, off[b + 1] * 19           # GEMM rows of utterance b
        if hi <= FULL_ROWS:
            continue
        s = max(FULL_ROWS, lo)
        got = c2.reshape(-1, c2.shape[-1])[s:hi].double()
        want = r.reshape(-1, r.shape[-1])[s - lo:]
        err = max(err, (got - want).abs().max().item())
        rows += hi - s
    return err, rows


@pytest.mark.parametrize('d', [64, 256])
def test_tiles_k_slice_tail(d):
    """256-row tiles + the last four tiles as 4 K slices (conv_tail_reduce_kernel, the `part`
    scratch), d = 64 and the production width 256 -- and the one-launch 128-row form on the same
    inputs: the rows below 256 * full are the same bits (test_conv2_tile_forms_agree's claim, on
    c2 itself), the tail rows are inside the bound in both forms."""
    feats, lens = _batch_3500(seed=d + 1)
    sub = 1 if d == 256 else 0
    with tune(x6_conv_bm=0):
        _, c2, _, refs, utts = _case(f'tiles d{d} m3500 ktail', 80, d, feats, lens,
                                     route(PLANES, T256_KTAIL, slices=4, sub_out=sub))
    with tune(x6_conv_bm=128):
        # (fp64 on the first tiles, the middle and the tail: the full tiles are the bits above)
        _, c2b, _, refs_b, utts_b = _case(f'tiles d{d} m3500 one-launch', 80, d, feats, lens,
                                          route(PLANES, T128, sub_out=sub), utts=[0, 2, 5, 7, 8])
    flat, flat_b = c2.reshape(-1, d), c2b.reshape(-1, d)
    assert flat.shape[0] == 66500
    assert torch.equal(flat[:FULL_ROWS], flat_b[:FULL_ROWS]), 'full tiles differ between the forms'
    for tag, t, r, u in (('ktail', c2, refs, utts), ('one-launch', c2b, refs_b, utts_b)):
        _, e_plain, scale = r['c2']
        err, rows = _tail_err(t, r, u, L2_3500)
        assert rows == 66500 - FULL_ROWS
        record(f'frontend[tiles d{d} m3500 {tag} c2 tail rows]', err, e_plain, scale)


def test_tiles_fp32_gather_remainder():
    """x6_conv_af32 = 1 at the same row counts: 256-row tiles, the remainder as 128-row tiles
    (the fp32 gather has no K-slice tail)."""
    feats, lens = _batch_3500(seed=7)
    with tune(x6_conv_bm=0, x6_conv_af32=1):
        _case('tiles d64 m3500 af32', 80, 64, feats, lens, route(AF32, T256_REM128))


def test_tiles_d512():
    """N = 512 > 256: no split into 256-row tiles + remainder; gemm_x6_bm() picks one launch of
    128-row tiles for 260 x 2 tiles.  fp64 on a subset of the utterances (the first tiles, the
    middle, the rows from 65 536 on)."""
    feats, lens = _batch_3500(seed=9)
    with tune(x6_conv_bm=0):
        _case('tiles d512 m3500', 80, 512, feats, lens, route(PLANES, T128, sub_out=1),
              utts=[0, 2, 5, 7, 8])


def test_tiles_below_two_rounds():
    """M F2 = 11 400 rows < 65 536 under x6_conv_bm = 0: gemm_x6_bm() keeps 128-row tiles below
    two rounds of 256-row tiles."""
    l2 = [100, 0, 1, 300, 150, 49]
    lens = _lens_of(l2, [3, 0, 1, 2, 0, 1])
    feats = KR.make_frontend_feats(lens, 80, seed=11)
    with tune(x6_conv_bm=0):
        _case('tiles d64 below-two-rounds', 80, 64, feats, lens, route(PLANES, T128))


def test_tiles_256_only():
    """182 210 rows = 712 256-row tiles: two rounds + 200, more than half a round, so no second
    launch; 128-row tiles would take as long (6 half rounds each) and the tie keeps 256-row
    tiles: ONE launch of 256-row tiles, the last tile partial."""
    l2 = [2000, 1, 0, 2500, 1800, 1289, 2000]
    assert sum(l2) == 9590
    lens = _lens_of(l2, [0, 1, 2, 3, 1, 0, 2])
    feats = KR.make_frontend_feats(lens, 80, seed=13)
    with tune(x6_conv_bm=0):
        _case('tiles d64 three-rounds', 80, 64, feats, lens, route(PLANES, T256))


# ---------------------------------------------------------------------------------------------
# rejections of the hook


def test_hook_rejections():
    _lib, L = _L()
    _, conf = _model(23, 64)
    _, whisper = _model(80, 384, whisper=True)
    feats = torch.zeros(2, 8, 80, device='cuda')
    out = torch.zeros(4096, device='cuda')
    code = ctypes.c_int32(0)

    def call(model, f, lens, T):
        return L.wn_op_conv2d4(model._h, f.data_ptr(), _lib.i32p(np.asarray(lens, np.int32)),
                               len(lens), T, None, None, out.data_ptr(), None,
                               ctypes.byref(code), None)

    f23 = torch.zeros(2, 8, 23, device='cuda')
    for fn, msg in ((lambda: call(whisper, feats, [8, 8], 8), 'Conformer'),
                    (lambda: call(conf, f23, [6, 6], 6), 'at least 7 frames'),
                    (lambda: call(conf, f23, [8, 9], 8), 'length out of range'),
                    (lambda: L.wn_op_conv2d4(conf._h, None, None, 2, 8, None, None, None, None,
                                             ctypes.byref(code), None), 'null argument')):
        assert fn() == -1
        assert msg in L.wn_last_error().decode(), L.wn_last_error().decode()
    # the handle is usable afterwards
    assert call(conf, f23, [8, 7], 8) == 0 and code.value == route(F32)


# ---------------------------------------------------------------------------------------------
# Whisper front end


def _whisper_run(model, feats_dev, lens):
    _lib, L = _L()
    try:
        _lib.check(L.wn_debug_set(model._h, b'n_layers', 0), 'dbg')
        _lib.check(L.wn_debug_set(model._h, b'skip_after_norm', 1), 'dbg')
        enc, mask = model._forward_encoder(feats_dev, torch.tensor(lens, dtype=torch.int32))
    finally:
        L.wn_debug_set(model._h, b'n_layers', -1)
        L.wn_debug_set(model._h, b'skip_after_norm', 0)
    return enc.cpu(), mask.squeeze(1).sum(1).tolist()


@pytest.mark.parametrize('F_in', [80, 128])
@pytest.mark.parametrize('T', [12, 13, 300, 301])
def test_whisper_frontend(F_in, T):
    """pad_feats_kernel, the two gathered-row GEMMs with GELU (F = 80: K = 240 padded to 256), the
    right-pad rule of an utterance with L == T, both parities of T, the positional rows; lengths
    0, 1, 2, 3 beside.  The padding frames stay zeros: the reference reads them."""
    sd, model = _model(F_in, 384, whisper=True)
    lens = [T, 0, 1, 2, 3, T - 1, T // 2, 7]
    g = torch.Generator().manual_seed(T + F_in)
    feats = torch.randn(len(lens), T, F_in, generator=g)
    for b, n in enumerate(lens):
        feats[b, n:] = 0.0
    ref, e_plain, scale = KR.whisper_frontend_refs(feats, lens, sd)
    l2 = KR.sub2_lens(lens, T)
    dev = feats.cuda()
    enc, got_lens = _whisper_run(model, dev, lens)
    enc_b, _ = _whisper_run(model, dev, lens)
    assert got_lens == l2
    assert torch.equal(enc, enc_b), 'two runs differ'
    assert enc.shape == (len(lens), (T - 1) // 2 + 1, 384)
    for b, n in enumerate(l2):
        assert not enc[b, n:].any(), f'utterance {b}: rows behind its length are not zero'
    record(f'frontend[whisper F{F_in} T{T}]', _err([enc[b, :n] for b, n in enumerate(l2)], ref),
           e_plain, scale)
