"""The Conv2dSubsampling6 front end (csrc/conv2d6.hip, one launch for CMVN + conv1 + conv2) through
the hook wn_op_conv2d6 against a plain fp64 evaluation of its three layers with
torch.nn.functional.conv2d on the CPU, one utterance at a time on its own frames.  The bound is
the one of the Conv2dSubsampling4 front-end tests (test_gpu_kernels.record): err <= 8 e_plain +
16 fp32 ulps of the largest |output|, e_plain = the same evaluation in fp32, under its cap.

The kernel writes the caller's c2 [M][12][d]: a PATTERN frame around it must come back intact.
Every frame no kept output frame reads (the padding included) holds 1e30: a kernel that read one
would be off by far more than the bound.  The batch must give each utterance the bits it gets alone.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from gpu_util import make_model
from test_gpu_kernels import record, tune

F_IN, F2, PATTERN, BIG = 80, 12, -7.25, 1.0e30
_PARTS = {}


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _parts(d, cmvn):
    """(configs, state dict) of tiny_conv2d6 at width d with one block."""
    if (d, cmvn) not in _PARTS:
        from wenet_amd import synthetic as S
        configs = S.make_configs('tiny_conv2d6')
        ec = configs['encoder_conf']
        ec['output_size'], ec['attention_heads'], ec['num_blocks'] = d, d // 64, 1
        configs['decoder_conf']['attention_heads'] = d // 64
        if not cmvn:
            configs['cmvn'] = None
        sd = {k: torch.as_tensor(v) for k, v in S.make_state_dict(configs, 3).items()}
        _PARTS[(d, cmvn)] = (configs, sd)
    return _PARTS[(d, cmvn)]


def _l2(L):
    return max(0, ((L - 1) // 2 - 2) // 3)


def _feats(lens, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(len(lens), max(max(lens), 11), F_IN, generator=g) * 3.0 + 11.0
    for b, n in enumerate(lens):
        feats[b, (6 * _l2(n) + 5 if _l2(n) else 0):] = BIG
    return feats


def _ref(feats, lens, sd, d, dt):
    """[(c2 (l2, 12, d), x (l2, d))] per utterance with output frames, evaluated in `dt`."""
    w = {k: sd['encoder.embed.' + k].to(dt) for k in
         ('conv.0.weight', 'conv.0.bias', 'conv.2.weight', 'conv.2.bias', 'linear.weight',
          'linear.bias')}
    out = []
    for b, n in enumerate(lens):
        if _l2(n) == 0:
            continue
        x = feats[b, :n].to(dt)
        if 'encoder.global_cmvn.mean' in sd:
            x = (x - sd['encoder.global_cmvn.mean'].to(dt)) * sd['encoder.global_cmvn.istd'].to(dt)
        y = torch.relu(Fn.conv2d(x[None, None], w['conv.0.weight'], w['conv.0.bias'], stride=2))
        y = torch.relu(Fn.conv2d(y, w['conv.2.weight'], w['conv.2.bias'], stride=3))[0]
        assert y.shape == (d, _l2(n), F2)
        proj = Fn.linear(y.permute(1, 0, 2).reshape(_l2(n), d * F2), w['linear.weight'],
                         w['linear.bias']) * math.sqrt(d)
        out.append((y.permute(1, 2, 0).contiguous(), proj))
    return out


def _run(model, feats, lens, d):
    """The hook on a framed buffer -> (c2 (M, 12, d), x (M, d)) on the CPU; asserts the frame and
    the lengths."""
    _lib, L = _L()
    M = sum(_l2(n) for n in lens)
    pad = 2 * F2 * d
    buf = torch.full((2 * pad + M * F2 * d, ), PATTERN, device='cuda')
    x = torch.full((M, d), float('nan'), device='cuda')
    enc = np.full(len(lens), -1, np.int32)
    dev = feats.cuda()
    _lib.check(L.wn_op_conv2d6(model._h, dev.data_ptr(), _lib.i32p(np.asarray(lens, np.int32)),
                               len(lens), dev.shape[1], buf.data_ptr() + 4 * pad, x.data_ptr(),
                               _lib.i32p(enc), None), 'wn_op_conv2d6')
    assert enc.tolist() == [_l2(n) for n in lens]
    out = buf.cpu()
    assert (out[:pad] == PATTERN).all() and (out[-pad:] == PATTERN).all(), 'stores outside c2'
    return out[pad:-pad].reshape(M, F2, d), x.cpu()


def _check(what, got, feats, lens, sd, d):
    ref, plain = _ref(feats, lens, sd, d, torch.float64), _ref(feats, lens, sd, d, torch.float32)
    for i, name in enumerate(('c2', 'x')):
        r64 = torch.cat([r[i] for r in ref])
        assert torch.isfinite(got[i]).all(), f'{what} {name}: not finite'
        record(f'{what} {name}', (got[i].double() - r64).abs().max().item(),
               (torch.cat([r[i] for r in plain]).double() - r64).abs().max().item(),
               r64.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('cmvn', [True, False], ids=['cmvn', 'nocmvn'])
@pytest.mark.parametrize('d', [256, 512])
def test_conv2d6_against_fp64(d, cmvn):
    _lib, L = _L()
    ft = L.wn_conv2d6_ft(d)                             # the shipped frames per tile
    assert ft in (5, 8, 10)
    # l2 = 1, FT - 1, none (10 frames), FT, FT + 1, 2 FT + 1; the shorter ones have padding
    lens = [11] + [6 * n + 5 for n in (ft - 1, )] + [10] + \
           [6 * n + 5 for n in (ft, ft + 1, 2 * ft + 1)]
    lens[4] += 4                                        # frames of its own that no output reads
    configs, sd = _parts(d, cmvn)
    model = make_model(configs, sd)
    feats = _feats(lens, seed=d + cmvn)
    c2, x = _run(model, feats, lens, d)
    _check(f'conv2d6 d={d} cmvn={cmvn}', (c2, x), feats, lens, sd, d)
    o = 0
    for b, n in enumerate(lens):
        if _l2(n) == 0:
            continue
        c2b, xb = _run(model, feats[b:b + 1, :max(n, 11)], [n], d)
        assert torch.equal(c2b, c2[o:o + _l2(n)]), f'utterance {b}: c2 differs from the batch'
        assert torch.equal(xb, x[o:o + _l2(n)]), f'utterance {b}: x differs from the batch'
        o += _l2(n)


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(25))
def test_conv2d6_one_tap(tap):
    """conv2's weight nonzero at ONE (ky, kx): a wrong tap offset, residue order or k-block order
    of the weight image reads another pixel of conv1's output."""
    d, lens = 256, [17]                                 # l2 = 2
    configs, sd = _parts(d, True)
    sd = dict(sd)
    w = torch.zeros_like(sd['encoder.embed.conv.2.weight'])
    w[:, :, tap // 5, tap % 5] = sd['encoder.embed.conv.2.weight'][:, :, tap // 5, tap % 5] * 5.0
    sd['encoder.embed.conv.2.weight'] = w
    feats = _feats(lens, seed=tap)
    got = _run(make_model(configs, sd), feats, lens, d)
    _check(f'conv2d6 tap {tap}', got, feats, lens, sd, d)


@pytest.mark.gpu
@pytest.mark.parametrize('d,ft,wide', [(256, 5, 0), (256, 8, 0), (256, 10, 0), (512, 5, 1), (512, 8, 1),
                                       (512, 10, 1), (512, 5, 2), (512, 8, 2), (512, 10, 2)])
def test_conv2d6_variants(d, ft, wide):
    """Every built (frames per tile, column split) behind the tune keys conv2d6_ft / conv2d6_wide
    (1: two column halves, 2: eight waves; ft 10 has column halves only), on lengths around ITS
    tile size.  All walk K in the same order: the bits of the shipped form."""
    lens = [6 * n + 5 for n in (1, ft - 1, ft, ft + 1, 2 * ft + 1)]
    configs, sd = _parts(d, True)
    model = make_model(configs, sd)
    feats = _feats(lens, seed=ft)
    with tune(conv2d6_ft=ft, conv2d6_wide=wide):
        c2, x = _run(model, feats, lens, d)
    _check(f'conv2d6 d={d} ft={ft} wide={wide}', (c2, x), feats, lens, sd, d)
    c2s, xs = _run(model, feats, lens, d)
    assert torch.equal(c2, c2s) and torch.equal(x, xs), 'differs from the shipped form'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['bf16', 'fp8'])
def test_conv2d6_low_precision_handles_keep_the_front_end(dtype):
    """A bf16 / fp8 handle runs the same kernel: c2 is the fp32 handle's bits."""
    d, lens = 256, [11, 59, 107]
    configs, sd = _parts(d, True)
    feats = _feats(lens, seed=1)
    c2, _ = _run(make_model(configs, sd), feats, lens, d)
    low = make_model(configs, sd)
    low.set_compute_dtype(dtype)
    assert torch.equal(_run(low, feats, lens, d)[0], c2)
