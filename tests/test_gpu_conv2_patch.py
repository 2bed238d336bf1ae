"""conv2 with conv1's patch computed in LDS (csrc/conv2_patch.hip, conv2 kind 3) through the hook
wn_op_conv2d4, with the yardstick and the helpers of tests/test_gpu_frontend.py: conv2 against
fp64 from the conv1 activations, the projection against fp64 from conv2's output, the chain
against the oracle from the features -- err <= 8 e_plain + 16 fp32 ulps of the scale -- the
route code, the lengths and two runs giving the same bits (_case).  On top of that every case
is run on the fall-back route (x6_conv_patch = 0: conv1's plane image + the gathered conv2) and
must give the same bits: both walk K as (channel chunk, tap) with the same six plane products
per k block, on operands that are the same bits.

x6_conv_patch = 2 takes the kernel at every size (the default takes it from 131 072 GEMM rows
on); gemm_x6 = 2 takes the six-product kernels below 4096 rows.  d = 256, F = 80: F1 = 39, F2 =
19, 128-row tiles.  The feature frames no kept output frame reads hold NaN.

Every case is also run through wn_op_conv2_patch_into, where conv2_patch_kernel itself writes a
caller's buffer: a PATTERN frame of three output frames in front of and behind C must come back
intact (the row guard of the last tile), and C and the packed rows are the bits of the hook run.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as KR
from test_gpu_frontend import PLANES, _case, _lens_of, _model, _run, route
from test_gpu_kernels import _L, tune

PATCH = 3
F_IN, D, F2 = 80, 256, 19
FORCE = dict(gemm_x6=2, x6_conv_patch=2)
FALLBACK = dict(gemm_x6=2, x6_conv_patch=0)


PATTERN = -7.25


def _framed(model, feats_dev, lens):
    """conv2_patch_kernel writing into a framed buffer -> (c2, x on the CPU); asserts the frame."""
    _lib, L = _L()
    M = sum(KR.sub4_lens(lens))
    pad = 3 * F2 * D
    buf = torch.full((2 * pad + M * F2 * D, ), PATTERN, device='cuda')
    x = torch.full((M, D), float('nan'), device='cuda')
    code = ctypes.c_int32(-1)
    B, T, _ = feats_dev.shape
    _lib.check(L.wn_op_conv2_patch_into(model._h, feats_dev.data_ptr(),
                                        _lib.i32p(np.asarray(lens, np.int32)), B, T,
                                        buf.data_ptr() + 4 * pad, x.data_ptr(),
                                        ctypes.byref(code), None), 'wn_op_conv2_patch_into')
    assert code.value & 15 == PATCH
    out = buf.cpu()
    assert (out[:pad] == PATTERN).all(), 'stores in front of C'
    assert (out[-pad:] == PATTERN).all(), 'stores behind C'
    return out[pad:-pad].reshape(M, F2, D), x.cpu()


def _feats(lens, seed):
    feats = KR.make_frontend_feats(lens, F_IN, seed=seed)
    for b, l2 in enumerate(KR.sub4_lens(lens)):
        feats[b, (4 * l2 + 3 if l2 else 0):] = float('nan')
    return feats


# (name, lens, projection runs as K slices, tiles / what it exercises)
CASES = [
    ('one-frame', [7], 0),                       # 19 rows: one output frame, a partial tile
    ('two-frames', [11], 0),
    ('ragged', [7, 39, 67, 131], 0),             # l2 = 1, 9, 16, 32: 1102 rows, tiles cross
                                                 # utterance boundaries, the last tile partial
    ('full-last-tile', [4 * 128 + 3], 0),        # 128 frames: 2432 rows = 19 tiles exactly
    ('one-row-last-tile', [4 * 27 + 3], 0),      # 27 frames: 513 rows = 4 tiles + 1 row
    ('boundaries-and-empties', [7, 6, 7, 7, 7, 11, 15, 0], 0),   # l2 = 1, 0, 1, 1, 1, 2, 3, 0: one
                                                 # tile over five boundaries and an empty
                                                 # utterance, 20 conv1 frames in its patch
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,lens,sub', CASES, ids=[c[0] for c in CASES])
def test_patch_kernel(name, lens, sub):
    l2 = KR.sub4_lens(lens)
    rows = sum(l2) * F2
    if name == 'full-last-tile':
        assert rows % 128 == 0
    if name == 'one-row-last-tile':
        assert rows % 128 == 1
    feats = _feats(lens, seed=len(lens) + rows)
    with tune(**FORCE):
        c1, c2, x, _, _ = _case(f'patch {name}', F_IN, D, feats, lens, route(PATCH, sub_out=sub))
    with tune(**FALLBACK):
        c1f, c2f, xf, _, _ = _case(f'patch {name} fall-back', F_IN, D, feats, lens,
                                   route(PLANES, sub_out=sub))
    assert torch.equal(c1, c1f), f'{name}: c1 differs from the plane image'
    assert torch.equal(c2, c2f), f'{name}: conv2 differs from the fall-back route'
    assert torch.equal(x, xf), f'{name}: the packed rows differ from the fall-back route'
    _, model = _model(F_IN, D)
    with tune(**FORCE):
        c2k, xk = _framed(model, feats.cuda(), lens)
    assert torch.equal(c2k, c2), f'{name}: the framed run differs'
    assert torch.equal(xk, x), f'{name}: the packed rows of the framed run differ'


@pytest.mark.gpu
def test_patch_too_many_frames_falls_back():
    """Fourteen utterances of one output frame: the second tile (output frames 6 .. 13) would read
    3 x 8 = 24 conv1 frames > 21, so the batch takes the plane-image route even when the patch
    kernel is forced, and the framed hook refuses it without touching the buffer."""
    lens = [7] * 14
    _lib, L = _L()
    assert L.wn_conv2_patch_max_frames(_lib.i32p(np.asarray(KR.sub4_lens(lens), np.int32)), 14,
                                       F2) == 24
    feats = _feats(lens, seed=14)
    with tune(**FORCE):
        _case('patch too-many-frames', F_IN, D, feats, lens, route(PLANES))
        _, model = _model(F_IN, D)
        buf = torch.full((14 * F2 * D, ), PATTERN, device='cuda')
        code = ctypes.c_int32(-1)
        assert L.wn_op_conv2_patch_into(model._h, feats.cuda().data_ptr(),
                                        _lib.i32p(np.asarray(lens, np.int32)), 14, 7,
                                        buf.data_ptr(), None, ctypes.byref(code), None) == -1
        assert 'kind 3' in L.wn_last_error().decode()
    assert (buf == PATTERN).all()


@pytest.mark.gpu
def test_patch_one_hot_taps():
    """conv2's weight as nine one-hot rows -- output channel k reads tap k of input channel
    29 k + 3 (nine different channel chunks), bias 0 -- pins the (channel chunk, tap) order of
    the weight image and the tap windows of the patch: c2[t, f, k] must be c1[2 t + ky, 2 f + kx,
    channel] EXACTLY (x = h0 + h1 + h2 times 1.0, summed small to large, is x)."""
    from gpu_util import make_model
    configs, sd = KR.frontend_model_parts(F_IN, D)
    sd = dict(sd)
    w = torch.zeros_like(sd['encoder.embed.conv.2.weight'])            # (C, C, 3, 3)
    chans = [(29 * k + 3) % D for k in range(9)]
    assert len({c // 16 for c in chans}) == 9
    for k, ci in enumerate(chans):
        w[k, ci, k // 3, k % 3] = 1.0
    sd['encoder.embed.conv.2.weight'] = w
    sd['encoder.embed.conv.2.bias'] = torch.zeros_like(sd['encoder.embed.conv.2.bias'])
    model = make_model(configs, sd)
    lens = [7, 39, 67, 131]
    l2 = KR.sub4_lens(lens)
    feats = _feats(lens, seed=9).cuda()
    with tune(**FORCE):
        c1, c2, x, _, code = _run(model, feats, lens, F_IN, D)
        c1b, c2b, xb, _, _ = _run(model, feats, lens, F_IN, D)
        c2k, xk = _framed(model, feats, lens)
    assert code == route(PATCH)
    assert torch.equal(c1, c1b) and torch.equal(c2, c2b) and torch.equal(x, xb), 'two runs differ'
    assert torch.equal(c2k, c2) and torch.equal(xk, x), 'the framed run differs'
    c1l = torch.split(c1, [2 * n + 1 for n in l2])
    c2l = torch.split(c2, l2)
    for b, n in enumerate(l2):
        for k, ci in enumerate(chans):
            ky, kx = k // 3, k % 3
            want = c1l[b][ky:ky + 2 * n:2, kx:kx + 2 * F2:2, ci]
            assert torch.equal(c2l[b][:, :, k], want), f'utterance {b}, tap {k}'
        assert not c2l[b][:, :, 9:].any()


def test_max_frames_matches_numpy():
    """conv2_patch_max_frames (host code, no GPU) against a restatement: packed conv1 frames are
    consecutive, 2 l2 + 1 per utterance with output frames; a tile of 128 GEMM rows reads from the
    first conv1 frame of its first output frame to the third of its last."""
    from wenet_amd import _lib
    L = _lib.lib()

    def restated(l2, F2):
        first = []                       # first conv1 frame of every output frame
        o1 = 0
        for n in l2:
            first += [o1 + 2 * t for t in range(n)]
            o1 += 2 * n + 1 if n else 0
        rows = len(first) * F2
        return max([first[min(r + 127, rows - 1) // F2] + 3 - first[r // F2]
                    for r in range(0, rows, 128)] + [0])

    cases = [([1], 19, 3), ([2], 19, 5), ([128], 19, 17), ([27], 19, 17),
             ([1, 9, 16, 32], 19, None), ([1, 0, 1, 1, 1, 2, 3, 0], 19, 20), ([1] * 14, 19, 24),
             ([0, 0, 5, 0], 19, 11), ([40, 40], 5, None), ([0, 0], 19, 0)]
    for l2, F2_, want in cases:
        got = L.wn_conv2_patch_max_frames(_lib.i32p(np.asarray(l2, np.int32)), len(l2), F2_)
        assert got == restated(l2, F2_), (l2, F2_)
        if want is not None:
            assert got == want, (l2, F2_)
    assert L.wn_conv2_patch_max_frames(_lib.i32p(np.asarray([-1], np.int32)), 1, 19) == -1


def test_kperm_matches_numpy():
    """The k-block order of the permuted weight image (host code, no GPU): destination block
    (chunk, tap) takes the tap-major image's block tap * kbc + chunk."""
    from wenet_amd import _lib
    L = _lib.lib()
    for kbc, taps in ((16, 9), (4, 9), (1, 9), (16, 1), (3, 2)):
        got = np.full(kbc * taps, -1, np.int32)
        assert L.wn_conv2_kperm(kbc, taps, _lib.i32p(got)) == 0
        want = np.arange(taps * kbc, dtype=np.int32).reshape(taps, kbc).T.reshape(-1)
        assert np.array_equal(got, want)
        assert sorted(got.tolist()) == list(range(kbc * taps))
    assert L.wn_conv2_kperm(0, 9, _lib.i32p(np.zeros(1, np.int32))) == -1
