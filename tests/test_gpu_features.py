"""Operator tests of the two feature front ends against fp64: wn_fbank (csrc/fbank.hip, tables of
csrc/fbank_tables.h) and wn_log_mel (csrc/logmel.hip, the two fp32 GEMMs, the tables built in
csrc/cabi_encode.hip), on the inputs and under the rule of tests/frontend_refs.py (CPU checks of
both: tests/test_frontend_refs.py).

Every case: FR.accept(kernel, fp64 reference, plain fp32 evaluation) -- max-abs error and p99 of
the absolute error each within 4 x the plain fp32 error of that case + 2 ulp.  The parity tests of
tests/test_gpu_parity.py (agreement with the reference's recorded outputs, p99 < 2e-3 and
max < 5e-2) would pass a mel weight 1 % off, a doubled window[1], a floor at max - 7.9 or a
maximum taken over the batch; tests/test_frontend_refs.py shows this rule rejecting each of them
by 180 x and more.

Through ASRModel.compute_fbank / compute_log_mel_spectrogram where the public method reaches the
case, through the C entry points where it cannot: a PCM pointer 12 bytes into its allocation with
NaNs around the samples, max_frames three past the longest utterance, an output buffer pre-filled
with NaN and followed by guard floats.

GPU-measured figures (MI355X; ratio = error / tolerance, the larger of the max-abs and p99 one):
  case                                       err   e_plain       p99 p99_plain  ratio
  fbank white                          4.812e-05 4.812e-05 7.905e-06 8.141e-06  0.245
  fbank white_quiet                    3.729e-05 3.753e-05 8.872e-06 8.890e-06  0.245
  fbank white_dc                       2.637e-05 2.542e-05 8.756e-06 8.969e-06  0.250
  fbank tone_floor                     5.406e-04 5.406e-04 3.005e-04 3.002e-04  0.250
  fbank chirp_top                      1.368e-01 1.368e-01 5.555e-02 5.555e-02  0.250
  fbank chirp_top (carrying filters)   3.139e-06 9.985e-07 3.127e-06 9.874e-07  0.403
  fbank impulse                        4.861e-06 4.861e-06 2.442e-06 2.262e-06  0.209
  fbank silence                        5.206e-07 4.330e-07 5.206e-07 4.330e-07  0.143
  fbank const                          5.206e-07 4.330e-07 5.206e-07 4.330e-07  0.143
  fbank len400                         7.739e-06 8.341e-06 7.461e-06 7.865e-06  0.212
  fbank len559                         3.912e-06 3.822e-06 3.841e-06 3.655e-06  0.208
  fbank len560                         1.255e-05 4.916e-06 4.217e-06 3.743e-06  0.534
  fbank len561                         8.410e-06 7.219e-06 6.907e-06 6.271e-06  0.257
  fbank ragged[0]                      1.588e-04 1.588e-04 8.576e-06 8.366e-06  0.249
  fbank ragged[3]                      4.454e-05 4.358e-05 7.173e-06 7.255e-06  0.250
  logmel80 white                       6.434e-07 5.242e-07 1.702e-07 1.575e-07  0.290
  logmel128 white                      6.257e-07 6.257e-07 1.807e-07 1.660e-07  0.239
  logmel80 ramp                        5.383e-06 5.383e-06 1.351e-06 1.351e-06  0.247
  logmel128 ramp                       7.032e-06 7.032e-06 2.156e-06 2.076e-06  0.252
  logmel80 one_frame                   2.225e-07 1.629e-07 1.653e-07 1.528e-07  0.289
  logmel128 one_frame                  3.055e-07 3.055e-07 2.160e-07 2.155e-07  0.228
  logmel80 tone_floor                  1.431e-06 1.550e-06 5.548e-07 4.984e-07  0.249
  logmel128 tone_floor                 1.931e-06 2.050e-06 7.943e-07 7.790e-07  0.237
  logmel80 silence                     0.000e+00 0.000e+00 0.000e+00 0.000e+00  0.000
  logmel128 silence                    0.000e+00 0.000e+00 0.000e+00 0.000e+00  0.000
  logmel80 silence_then_noise          3.824e-07 4.420e-07 1.860e-07 1.370e-07  0.237
  logmel128 silence_then_noise         4.126e-07 4.443e-07 1.946e-07 1.703e-07  0.212
  logmel80 len319                      1.559e-07 1.559e-07 1.324e-07 1.271e-07  0.211
  logmel128 len319                     2.203e-07 2.203e-07 1.594e-07 2.094e-07  0.220
  logmel80 len320                      2.519e-07 2.519e-07 2.247e-07 1.758e-07  0.273
  logmel128 len320                     3.011e-06 3.011e-06 2.504e-07 2.366e-07  0.248
  logmel80 len479                      3.308e-07 2.712e-07 1.840e-07 1.616e-07  0.275
  logmel128 len479                     6.929e-07 6.929e-07 3.282e-07 2.430e-07  0.301
  logmel80 len480                      1.726e-06 1.726e-06 1.761e-07 2.167e-07  0.246
  logmel128 len480                     1.815e-06 1.696e-06 2.247e-07 2.217e-07  0.263
  logmel80 level_step[0]               1.700e-07 1.700e-07 1.391e-07 1.391e-07  0.185
  logmel80 level_step[1]               4.074e-07 3.887e-07 3.028e-07 2.090e-07  0.282
  logmel128 level_step[0]              6.514e-07 6.514e-07 2.300e-07 1.960e-07  0.229
  logmel128 level_step[1]              6.369e-07 5.343e-07 2.857e-07 2.835e-07  0.268
  logmel80 ragged[0]                   2.575e-07 2.575e-07 1.815e-07 1.729e-07  0.224
  logmel80 ragged[1]                   2.325e-07 2.325e-07 2.182e-07 1.711e-07  0.272
  logmel80 ragged[2]                   2.321e-07 2.321e-07 1.635e-07 1.426e-07  0.237
  logmel80 ragged[3]                   2.297e-07 3.452e-07 1.899e-07 2.080e-07  0.200
  logmel128 ragged[0]                  4.612e-07 4.612e-07 2.237e-07 2.093e-07  0.235
  logmel128 ragged[1]                  2.171e-06 2.051e-06 1.745e-06 1.658e-06  0.261
  logmel128 ragged[2]                  1.022e-06 1.022e-06 2.177e-07 1.953e-07  0.243
  logmel128 ragged[3]                  8.189e-07 8.189e-07 2.385e-07 2.654e-07  0.241

(level_step_rev repeats level_step with the utterances swapped, figure for figure; every
utterance of the log-mel ragged batch run alone gave the bits of its rows in the batch.)  The fp32
yardsticks follow the kernels' own summation order (tests/frontend_refs.py says why), so on most
cases the kernel's error IS e_plain and the ratio sits at 0.25; with the first yardsticks
(torch.fft.rfft; a k = 0, 1, 2, ... chain) the ratios were 0.08 - 0.70 with two excesses, fbank
ragged[0] 1.04 and logmel128 len320 1.80, each the draw of one near-cancelled element.

Kernel fix these tests forced: logmel_log_kernel took log10f of the clamped value, and the device
log10f(1e-10f) is -10.000001, so digital silence (all the padding of pad_or_trim) came out as
-1.5000002 where the definition gives -1.5.  The clamp's logarithm is now the constant -10.
"""
import numpy as np
import pytest
import torch

import frontend_refs as FR
from gpu_util import cached_model

pytestmark = pytest.mark.gpu

N_MELS = [80, 128]
SKEW, LEAD, TAIL, GUARD = 3, 512, 512, 64      # floats
SENTINEL = 12345.0
EXTRA_FRAMES = 3


def _model():
    return cached_model('tiny_sym', 0)[2]


def _fbank(ws):
    feats, nfr = _model().compute_fbank(ws)
    return feats.cpu().numpy(), nfr.tolist()


def _logmel(ws, n_mels):
    feats, nfr = _model().compute_log_mel_spectrogram(ws, n_mels)
    return feats.cpu().numpy(), nfr.tolist()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _raw(kind, ws, n_mels=80):
    """wn_fbank / wn_log_mel on a packed batch laid out to catch a stray access: the PCM pointer
    SKEW floats into its allocation (not 16-byte aligned), LEAD NaNs in front of the first
    utterance and TAIL behind the last, max_frames EXTRA_FRAMES past the longest utterance, the
    output pre-filled with NaN and followed by GUARD sentinel floats.
    -> ((B, max_frames, F) features, n_frames, guard floats)."""
    from wenet_amd import _lib
    L, model = _lib.lib(), _model()
    B = len(ws)
    count = FR.fbank_frames if kind == 'fbank' else FR.logmel_frames
    F = 80 if kind == 'fbank' else n_mels
    offs = np.zeros((B + 1, ), dtype=np.int64)
    offs[0] = LEAD
    offs[1:] = LEAD + np.cumsum([len(w) for w in ws])
    host = np.full((SKEW + int(offs[B]) + TAIL, ), np.nan, dtype=np.float32)
    for i, w in enumerate(ws):
        host[SKEW + offs[i]:SKEW + offs[i + 1]] = w
    dev = torch.from_numpy(host).cuda()
    pcm = dev.data_ptr() + 4 * SKEW
    assert pcm % 16 != 0
    max_frames = max(count(len(w)) for w in ws) + EXTRA_FRAMES
    out = torch.full((B * max_frames * F + GUARD, ), float('nan'), dtype=torch.float32)
    out[B * max_frames * F:] = SENTINEL
    out = out.cuda()
    nfr = np.full((B, ), -1, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    if kind == 'fbank':
        _lib.check(L.wn_fbank(model._h, pcm, _lib.i64p(offs), B, out.data_ptr(), max_frames,
                              _lib.i32p(nfr), stream), 'wn_fbank')
    else:
        _lib.check(L.wn_log_mel(model._h, pcm, _lib.i64p(offs), B, n_mels, out.data_ptr(),
                                max_frames, _lib.i32p(nfr), stream), 'wn_log_mel')
    torch.cuda.synchronize()
    got, n = out.cpu().numpy(), B * max_frames * F
    return got[:n].reshape(B, max_frames, F), nfr.tolist(), got[n:]


def _check_ragged(what, feats, nfr, guard, refs):
    assert nfr == [r.shape[0] for r, _ in refs]
    assert np.all(guard == np.float32(SENTINEL)), f'{what}: a write past the output'
    assert not np.isnan(feats).any(), f'{what}: NaN (a row never written, or a sample read ' \
                                      f'outside its utterance)'
    for b, (ref, plain) in enumerate(refs):
        assert np.all(feats[b, nfr[b]:] == 0), f'{what}[{b}]: rows past n_frames are not zero'
        FR.accept(feats[b, :nfr[b]], ref, plain, f'{what}[{b}]')


# ---------------------------------------------------------------------------------------------
# Kaldi fbank


@pytest.mark.parametrize('name', ['white', 'white_quiet', 'white_dc', 'tone_floor', 'chirp_top',
                                  'impulse', 'silence', 'const'])
def test_fbank_case(name):
    (w, ), ((ref, plain), ) = FR.CASES_FBANK[name], FR.fbank_refs(name)
    feats, nfr = _fbank([w])
    assert nfr == [ref.shape[0]] and feats.shape == (1, ref.shape[0], 80)
    got = feats[0]
    FR.accept(got, ref, plain, f'fbank {name}')
    if name == 'chirp_top':
        # the low filters hold only the leakage of the chirp and set the error of the whole case:
        # the filters that carry the signal (within 3 decades of the peak) under their own bar
        FR.accept(got, ref, plain, 'fbank chirp_top (carrying filters)',
                  where=ref > ref.max() - 7.0)
    if name in ('silence', 'const'):
        # logf(FLT_EPSILON) in every element, within 1 ulp of fp32 at 15.9
        assert np.abs(got.astype(np.float64) - float(FR.LOG_EPS32)).max() <= 2.0 ** -20
    if name == 'impulse':
        assert np.abs(got[[0, 3]].astype(np.float64) - float(FR.LOG_EPS32)).max() <= 2.0 ** -20


@pytest.mark.parametrize('n', list(FR.FBANK_FRAME_COUNTS))
def test_fbank_frame_count(n):
    (w, ), ((ref, plain), ) = FR.CASES_FBANK[f'len{n}'], FR.fbank_refs(f'len{n}')
    feats, nfr = _fbank([w])
    assert nfr == [FR.FBANK_FRAME_COUNTS[n]] == [ref.shape[0]]
    if nfr[0] == 0:
        assert np.all(feats == 0)
    else:
        assert feats.shape[1] == nfr[0]
        FR.accept(feats[0], ref, plain, f'fbank len{n}')


def test_fbank_ragged_batch():
    ws, refs = FR.CASES_FBANK['ragged'], FR.fbank_refs('ragged')
    feats, nfr, guard = _raw('fbank', ws)
    assert feats.shape[1] == 23 + EXTRA_FRAMES
    _check_ragged('fbank ragged', feats, nfr, guard, refs)
    # one block computes one frame from that frame's samples alone: bit for bit the same alone
    for b, w in enumerate(ws):
        if nfr[b] == 0:
            continue        # len399 of test_fbank_frame_count is the zero-frame call
        alone, n1 = _fbank([w])
        assert n1 == [nfr[b]]
        assert _bits_equal(alone[0, :nfr[b]], feats[b, :nfr[b]]), \
            f'utterance {b} alone differs from its rows in the batch'


# ---------------------------------------------------------------------------------------------
# Whisper log-mel


@pytest.mark.parametrize('n_mels', N_MELS)
@pytest.mark.parametrize('name', ['white', 'ramp', 'one_frame', 'tone_floor', 'silence',
                                  'silence_then_noise'])
def test_logmel_case(name, n_mels):
    (w, ), ((ref, plain), ) = FR.CASES_LOGMEL[name], FR.logmel_refs(name, n_mels)
    feats, nfr = _logmel([w], n_mels)
    assert nfr == [ref.shape[0]] and feats.shape == (1, ref.shape[0], n_mels)
    got = feats[0]
    FR.accept(got, ref, plain, f'logmel{n_mels} {name}')
    if name == 'silence':
        assert np.all(got == np.float32(-1.5))
    if name == 'silence_then_noise':
        # the silent frames sit at this utterance's floor, above the -1.5 of the clamp
        assert np.all(got[:3] == got[0, 0]) and got[0, 0] > -1.5
    if name == 'tone_floor':
        share = float((got == got.min()).mean())
        print(f'logmel{n_mels} tone_floor: {share:.2f} of the kernel\'s elements at the floor')
        assert 0.50 <= share <= 0.95


@pytest.mark.parametrize('n_mels', N_MELS)
@pytest.mark.parametrize('n', list(FR.LOGMEL_FRAME_COUNTS))
def test_logmel_frame_count(n, n_mels):
    (w, ), ((ref, plain), ) = FR.CASES_LOGMEL[f'len{n}'], FR.logmel_refs(f'len{n}', n_mels)
    feats, nfr = _logmel([w], n_mels)
    assert nfr == [FR.LOGMEL_FRAME_COUNTS[n]] == [ref.shape[0]] == [feats.shape[1]]
    FR.accept(feats[0], ref, plain, f'logmel{n_mels} len{n}')


@pytest.mark.parametrize('n_mels', N_MELS)
@pytest.mark.parametrize('name', ['level_step', 'level_step_rev'])
def test_logmel_level_step(name, n_mels):
    """A loud and a quiet utterance in one call, in both orders: each floors at its own maximum."""
    ws, refs = FR.CASES_LOGMEL[name], FR.logmel_refs(name, n_mels)
    feats, nfr = _logmel(ws, n_mels)
    assert nfr == [r.shape[0] for r, _ in refs]
    for b, (ref, plain) in enumerate(refs):
        FR.accept(feats[b, :nfr[b]], ref, plain, f'logmel{n_mels} {name}[{b}]')
        assert np.all(feats[b, nfr[b]:] == 0)


@pytest.mark.parametrize('n_mels', N_MELS)
def test_logmel_ragged_batch(n_mels):
    ws, refs = FR.CASES_LOGMEL['ragged'], FR.logmel_refs('ragged', n_mels)
    feats, nfr, guard = _raw('logmel', ws, n_mels)
    assert feats.shape[1] == 10 + EXTRA_FRAMES
    _check_ragged(f'logmel{n_mels} ragged', feats, nfr, guard, refs)
    # alone, the GEMMs run another M (their tile choice may differ): the bar, not the bits
    for b, (w, (ref, plain)) in enumerate(zip(ws, refs)):
        alone, n1 = _logmel([w], n_mels)
        assert n1 == [nfr[b]]
        FR.accept(alone[0], ref, plain, f'logmel{n_mels} ragged[{b}] alone')
        print(f'logmel{n_mels} ragged[{b}] alone: bitwise equal to its rows in the batch: '
              f'{_bits_equal(alone[0], feats[b, :nfr[b]])}')
