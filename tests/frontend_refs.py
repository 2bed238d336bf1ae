"""Plain references of the two feature front ends -- the Kaldi fbank (csrc/fbank.hip, tables of
csrc/fbank_tables.h) and the Whisper log-mel spectrogram (csrc/logmel.hip and the two fp32 GEMMs
wn_log_mel issues) -- the acceptance rule of their operator tests and the inputs those tests run
(tests/test_frontend_refs.py on the CPU, tests/test_gpu_features.py on the GPU).

Both definitions are restated here from their text (processor.py:226-256 with
runtime/core/frontend/fbank.h:91-163,221-226,250-327; processor.py:320-369); nothing is imported
from the oracle.  `fbank64` / `logmel64` evaluate them in fp64.  The PARAMETERS of the operators
are data, taken as the fp32 numbers the definition itself holds: the povey window, the 0.97, the
HTK mel weights -- including which FFT bins lie inside a triangle, which fbank.h decides with fp32
comparisons -- the periodic Hann window and the Slaney mel matrix.

`fbank32` / `logmel32` evaluate the same formulas in fp32, in the FORMULATION of the kernels (an
honest fp32 evaluation, written from the kernels' text, never from their output):
  * fbank32: the frame sum as a 64-lane butterfly per wave, the 512-point transform as a radix-2
    decimation-in-time FFT with an fp32 twiddle table, the mel step as a chain over the FFT bins
    of a triangle; a * b + c rounds once where the compiled kernel fuses it;
  * logmel32: the 400-point DFT as an fp32 matrix product with fp32 cos / -sin tables over
    K = 400 (not an FFT), then the mel step as an fp32 matrix product, every output one fused
    multiply-add chain in the k order of the matrix-core GEMM (csrc/gemm.hip).
A first version used torch.fft.rfft (fbank) and a k = 0, 1, 2, ... chain with rounded products
(log-mel).  Outputs that are near-cancellations of a frame's spectrum (white noise: a mel bin
4 - 5 decades under its neighbours) carry an error of about one ulp of the SPECTRUM's scale times
a draw that differs between summation orders; the max-abs error of a case is that one draw, and
the kernels exceeded 4 x the other order's draw on two of ~70 case comparisons (ratios 1.04, 1.80)
while sitting at 0.1 - 0.7 elsewhere.  With the kernels' own order the yardstick is the error of
the operation the kernel performs.  The distance of these from the fp64 evaluation is the
yardstick `e_plain` of `accept`.

Every function takes keyword "mutations" (a wrong divisor, a shifted frame, ...): the CPU tests
apply them to the fp32 side to show that `accept` rejects each of them by a wide margin.

No GPU in here.
"""
import functools
import math

import numpy as np
import torch

FLT_EPSILON = float(np.finfo(np.float32).eps)
LOG_EPS32 = np.float32(math.log(FLT_EPSILON))     # what a silent fbank frame must hold
FACTOR = 4.0      # another summation order (tests/test_gpu_transducer.py, tests/test_gpu_rows.py)

FRAME_LEN, FRAME_SHIFT, NFFT = 400, 160, 512
N_FFT, HOP = 400, 160


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------
# the acceptance rule


def ulp32(m):
    """Spacing of fp32 at magnitude m."""
    m = float(m)
    if m < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(m)) - 23)


def measure(got, ref64, plain32, where=None):
    """The figures of one case: max-abs and p99 errors of `got` and of the plain fp32 evaluation
    against fp64, and the tolerance FACTOR * e_plain + 2 ulp(largest |output|) of each.  `where`:
    a bool mask (chosen from ref64 alone) that restricts the case to a part of its elements."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    plain = np.asarray(plain32, dtype=np.float64)
    assert got.shape == ref.shape == plain.shape, (got.shape, ref.shape, plain.shape)
    if where is not None:
        got, ref, plain = got[where], ref[where], plain[where]
    if ref.size == 0:
        return dict(err=0.0, e_plain=0.0, tol=0.0, err99=0.0, e99=0.0, tol99=0.0, ratio=0.0)
    d = np.abs(got - ref)
    d[~np.isfinite(got)] = np.inf
    dp = np.abs(plain - ref)
    floor = 2.0 * ulp32(np.abs(ref).max())
    err, e_plain = float(d.max()), float(dp.max())
    err99, e99 = float(np.percentile(d, 99)), float(np.percentile(dp, 99))
    tol, tol99 = FACTOR * e_plain + floor, FACTOR * e99 + floor
    return dict(err=err, e_plain=e_plain, tol=tol, err99=err99, e99=e99, tol99=tol99,
                ratio=max(err / tol, err99 / tol99))


def accept(got, ref64, plain32, what='', where=None):
    """The project's rule for a kernel against fp64: err <= 4 * e_plain + 2 ulp, on the max-abs
    error of the case and on the p99 of the absolute error (a small bias in every element).
    Prints the figures; returns (err, e_plain, ratio), ratio = err / tolerance (the larger of the
    max and the p99 one)."""
    m = measure(got, ref64, plain32, where)
    line = (f'{what} err={m["err"]:.3e} e_plain={m["e_plain"]:.3e} tol={m["tol"]:.3e} '
            f'p99={m["err99"]:.3e} p99_plain={m["e99"]:.3e} ratio={m["ratio"]:.3f}')
    print(line)
    assert m['err'] <= m['tol'], line
    assert m['err99'] <= m['tol99'], line
    return m['err'], m['e_plain'], m['ratio']


# ---------------------------------------------------------------------------------------------
# Kaldi fbank


def fbank_frames(n):
    return 0 if n < FRAME_LEN else 1 + (n - FRAME_LEN) // FRAME_SHIFT   # fbank.h:254-255


@functools.lru_cache(maxsize=None)
def povey_window():
    """fbank.h:150-156, rounded to fp32 as the table holds it."""
    i = np.arange(FRAME_LEN, dtype=np.float64)
    return np.power(0.5 - 0.5 * np.cos(2.0 * math.pi / (FRAME_LEN - 1) * i), 0.85) \
        .astype(np.float32)


def _mel32(f):
    """1127 * logf(1 + f / 700) in fp32 steps (fbank.h:196-213); logf as the correctly rounded
    value."""
    x = np.float32(1.0) + np.float32(f) / np.float32(700.0)
    return np.float32(1127.0) * np.float32(math.log(float(x)))


@functools.lru_cache(maxsize=None)
def mel_banks(nbins=80):
    """HTK triangles 20 Hz .. 8 kHz on the 512-point grid (fbank.h:91-148), every step in fp32:
    dense (nbins, 256) fp32."""
    bin_w = np.float32(16000.0) / np.float32(NFFT)
    mlo, mhi = _mel32(20.0), _mel32(8000.0)
    delta = np.float32((mhi - mlo) / np.float32(nbins + 1))
    mels = [_mel32(bin_w * np.float32(i)) for i in range(NFFT // 2)]
    out = np.zeros((nbins, NFFT // 2), dtype=np.float32)
    for b in range(nbins):
        left = np.float32(mlo + np.float32(b) * delta)
        center = np.float32(mlo + np.float32(b + 1) * delta)
        right = np.float32(mlo + np.float32(b + 2) * delta)
        for i, mf in enumerate(mels):
            if mf > left and mf < right:
                out[b, i] = (mf - left) / (center - left) if mf <= center \
                    else (right - mf) / (right - center)
    return out


def _fbank(pcm, dt, mel_w=None, window=None, dc_div=400.0, preemph=0.97, shift=0,
           log_floor=FLT_EPSILON):
    x = torch.as_tensor(np.asarray(pcm, dtype=np.float32)).to(dt) * 32768.0
    n = x.numel()
    T = fbank_frames(n)
    if T == 0:
        return np.zeros((0, 80), dtype=np.float64)
    idx = torch.arange(T)[:, None] * FRAME_SHIFT + torch.arange(FRAME_LEN)[None, :] + shift
    data = x[idx.clamp(max=n - 1)]
    data = data - data.sum(dim=1, keepdim=True) / dc_div
    c = _f32(preemph)
    pre = torch.empty_like(data)
    pre[:, 1:] = data[:, 1:] - c * data[:, :-1]
    pre[:, 0] = data[:, 0] - c * data[:, 0]
    w = torch.from_numpy(povey_window() if window is None else window).to(dt)
    spec = torch.fft.rfft(pre * w, n=NFFT, dim=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:, :NFFT // 2]
    mw = torch.from_numpy(mel_banks() if mel_w is None else mel_w).to(dt)
    mel = power @ mw.t()
    floor = torch.tensor(_f32(log_floor), dtype=dt)
    return torch.log(torch.maximum(mel, floor)).double().numpy()


def fbank64(pcm, **mut):
    """(T, 80) fp64: the definition in fp64 on the fp32 parameters."""
    return _fbank(pcm, torch.float64, **mut)


def fbank32_fft(pcm, **mut):
    """The formula in torch fp32 with a library fp32 FFT and torch's own sums: the yardstick of an
    implementation built that way (the oracle, the reference's C++ fbank)."""
    return _fbank(pcm, torch.float32, **mut)


def fma32(a, b, c):
    """a * b + c rounded once to fp32 (the product of two fp32 is exact in fp64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) +
            np.asarray(c, np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fft512_tables():
    k = np.arange(NFFT // 2, dtype=np.float64)
    rev = np.array([int(format(i, '09b')[::-1], 2) for i in range(NFFT)])
    return (np.cos(2.0 * math.pi * k / NFFT).astype(np.float32),
            (-np.sin(2.0 * math.pi * k / NFFT)).astype(np.float32), rev)


def fbank32(pcm, mel_w=None, window=None, dc_div=400.0, preemph=0.97, shift=0,
            log_floor=FLT_EPSILON):
    """The same formula in fp32 throughout, in the formulation of csrc/fbank.hip (module
    docstring); the logarithm is the correctly rounded one."""
    f32 = np.float32
    x = np.asarray(pcm, dtype=f32) * f32(32768.0)
    n = x.shape[0]
    T = fbank_frames(n)
    if T == 0:
        return np.zeros((0, 80), dtype=np.float64)
    idx = np.arange(T)[:, None] * FRAME_SHIFT + np.arange(FRAME_LEN)[None, :] + shift
    data = np.zeros((T, NFFT), dtype=f32)
    data[:, :FRAME_LEN] = x[np.minimum(idx, n - 1)]
    # frame sum: thread t holds samples t and t + 256, xor butterfly over the 64 lanes of a wave,
    # then the four waves in order
    part = (data[:, :256] + data[:, 256:]).reshape(T, 4, 64)
    while part.shape[2] > 1:
        h = part.shape[2] // 2
        part = part[:, :, :h] + part[:, :, h:]
    part = part[:, :, 0]
    mean = (((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]) / f32(dc_div)
    data = data[:, :FRAME_LEN] - mean[:, None]
    prev = np.concatenate([data[:, :1], data[:, :-1]], axis=1)
    w = povey_window() if window is None else np.asarray(window, dtype=f32)
    pre = fma32(prev, -f32(preemph), data) * w[None, :]
    cos, msin, rev = _fft512_tables()
    re, im = np.zeros((T, NFFT), dtype=f32), np.zeros((T, NFFT), dtype=f32)
    re[:, rev[:FRAME_LEN]] = pre
    t = np.arange(NFFT // 2)
    for st in range(9):
        half = 1 << st
        k = t & (half - 1)
        i0 = ((t >> st) << (st + 1)) + k
        i1 = i0 + half
        c, sn = cos[k << (8 - st)], msin[k << (8 - st)]
        xr, xi = re[:, i1], im[:, i1]
        tr = fma32(xr, c, -(xi * sn))
        ti = fma32(xr, sn, xi * c)
        ur, ui = re[:, i0], im[:, i0]
        re[:, i0], re[:, i1] = ur + tr, ur - tr
        im[:, i0], im[:, i1] = ui + ti, ui - ti
    re, im = re[:, :NFFT // 2], im[:, :NFFT // 2]
    power = fma32(re, re, im * im)
    mw = mel_banks() if mel_w is None else np.asarray(mel_w, dtype=f32)
    mel = np.zeros((T, mw.shape[0]), dtype=f32)
    for b in range(mw.shape[0]):
        nz = np.nonzero(mw[b])[0]
        e = np.zeros((T, ), dtype=f32)
        for i in range(nz[0], nz[-1] + 1):
            e = fma32(mw[b, i], power[:, i], e)
        mel[:, b] = e
    return np.log(np.maximum(mel, f32(log_floor)).astype(np.float64)).astype(f32) \
        .astype(np.float64)


# ---------------------------------------------------------------------------------------------
# Whisper log-mel


@functools.lru_cache(maxsize=None)
def hann_window(denominator=N_FFT):
    """torch.hann_window(400) (periodic), rounded to fp32."""
    n = np.arange(N_FFT, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * math.pi * n / denominator)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def slaney_mel(n_mels):
    """librosa.filters.mel(16000, 400, n_mels) (Slaney scale: linear below 1 kHz, log above; area
    normalisation), computed in fp64, rounded to fp32: (n_mels, 201)."""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz2mel(f):
        return min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    def mel2hz(m):
        return min_log_hz * math.exp(logstep * (m - min_log_mel)) if m >= min_log_mel \
            else f_sp * m
    lo, hi = hz2mel(0.0), hz2mel(8000.0)
    edges = [mel2hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    w = np.zeros((n_mels, N_FFT // 2 + 1), dtype=np.float64)
    for i in range(n_mels):
        for k in range(N_FFT // 2 + 1):
            f = 8000.0 * k / (N_FFT // 2)
            lower = (f - edges[i]) / (edges[i + 1] - edges[i])
            upper = (edges[i + 2] - f) / (edges[i + 2] - edges[i + 1])
            w[i, k] = max(0.0, min(lower, upper)) * 2.0 / (edges[i + 2] - edges[i])
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _dft_tables():
    """cos / -sin of 2 pi k n / 400, k 0..200, as (400, 201) fp64."""
    k = np.arange(N_FFT // 2 + 1)[None, :]
    n = np.arange(N_FFT)[:, None]
    ph = 2.0 * math.pi * ((k * n) % N_FFT).astype(np.float64) / N_FFT
    return np.cos(ph), -np.sin(ph)


def matmul32(a, b):
    """(M, K) @ (K, N) in fp32 as csrc/gemm.hip accumulates it: every output one chain of fused
    multiply-adds from 0, over k in the order the 32x32x2 matrix-core steps take it (within
    every 8: k, k + 4, k + 1, k + 5, ...)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k0 in range(0, K, 8):
        for s in range(4):
            for k in (k0 + s, k0 + 4 + s):
                if k < K:
                    acc = fma32(a[:, k:k + 1], b[k:k + 1, :], acc)
    return acc


def logmel_frames(n):
    return n // HOP     # 1 + n // hop STFT frames, the last one dropped


def _logmel_log(pcm, n_mels, fp32, edge_repeat=False, hann_denominator=N_FFT, drop_first=False,
                clamp=1e-10, window=None, fft=False):
    """log10(max(mel power, clamp)) of the kept frames: (T, n_mels) in the working precision.
    `window`: another fp32 table in place of hann_window() (a definition that holds its own).
    `fft` (fp32 only): the transform as an fp32 FFT instead of the matrix product -- the yardstick
    of an implementation that calls torch.stft, whose rounding noise is spread differently over
    the bins of a frame that holds one strong tone."""
    ft = np.float32 if fp32 else np.float64
    x = np.asarray(pcm, dtype=np.float32).astype(ft)
    n = x.shape[0]
    assert n > N_FFT // 2, 'reflect padding needs more than 200 samples'
    T = 1 + n // HOP
    j = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :] - N_FFT // 2     # center=True
    rep = 1 if edge_repeat else 0
    j = np.where(j < 0, -j - rep, j)                                             # reflect
    j = np.where(j >= n, 2 * (n - 1) - j + rep, j)
    if window is None:
        window = hann_window(hann_denominator)
    frames = x[j] * np.asarray(window, dtype=np.float32).astype(ft)[None, :]
    cos, msin = _dft_tables()
    if fp32 and fft:
        spec = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames)), dim=1)
        re, im = spec.real.numpy(), spec.imag.numpy()
    elif fp32:
        re = matmul32(frames, cos.astype(np.float32))
        im = matmul32(frames, msin.astype(np.float32))
    else:
        re, im = frames @ cos, frames @ msin
    power = fma32(im, im, re * re) if fp32 else re * re + im * im
    power = power[1:] if drop_first else power[:-1]
    mw = slaney_mel(n_mels)
    mel = matmul32(power, mw.T) if fp32 else power @ mw.T.astype(np.float64)
    # fp32: the correctly rounded log10 (NumPy's own fp32 log10 is 1 ulp off at the clamp)
    return np.log10(np.maximum(mel, ft(clamp)).astype(np.float64)).astype(ft)


def _logmel_norm(log_spec, umax, span=8.0):
    ft = log_spec.dtype.type
    return ((np.maximum(log_spec, ft(umax) - ft(span)) + ft(4.0)) / ft(4.0)).astype(np.float64)


def logmel_max(pcm, n_mels, fp32=False, **mut):
    """The maximum the floor of this utterance hangs from."""
    mut.pop('span', None)
    ls = _logmel_log(pcm, n_mels, fp32, **mut)
    return float(ls.max()) if ls.size else -math.inf


def _logmel(pcm, n_mels, fp32, umax=None, span=8.0, **mut):
    ls = _logmel_log(pcm, n_mels, fp32, **mut)
    if ls.shape[0] == 0:
        return np.zeros((0, n_mels), dtype=np.float64)
    return _logmel_norm(ls, ls.max() if umax is None else umax, span)


def logmel64(pcm, n_mels, **mut):
    """(n // 160, n_mels) fp64.  `umax` replaces the utterance's own maximum (the batch-maximum
    mutant and the input condition that goes with it)."""
    return _logmel(pcm, n_mels, False, **mut)


def logmel32(pcm, n_mels, **mut):
    return _logmel(pcm, n_mels, True, **mut)


# ---------------------------------------------------------------------------------------------
# inputs: name -> list of waveforms (one call of the front end); fixed seeds


def _rng(tag):
    return np.random.Generator(np.random.PCG64([tag, 77]))


def _white(n, sigma, tag):
    return (sigma * _rng(tag).standard_normal(n)).astype(np.float32)


def _tone(n, noise, tag):
    t = np.arange(n, dtype=np.float64) / 16000.0
    return (0.3 * np.sin(2.0 * math.pi * 1000.0 * t) +
            noise * _rng(tag).standard_normal(n)).astype(np.float32)


def _chirp(n, f0, f1):
    t = np.arange(n, dtype=np.float64) / 16000.0
    dur = n / 16000.0
    return (0.3 * np.sin(2.0 * math.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / dur))) \
        .astype(np.float32)


def _impulse(n, at, v):
    x = np.zeros(n, dtype=np.float32)
    x[at] = v
    return x


FBANK_FRAME_COUNTS = {399: 0, 400: 1, 559: 1, 560: 2, 561: 2}
LOGMEL_FRAME_COUNTS = {319: 1, 320: 2, 479: 2, 480: 3}


def _fbank_cases():
    c = {
        'white': [_white(4000, 0.1, 1)],
        'white_quiet': [_white(4000, 1e-4, 2)],
        'white_dc': [_white(4000, 0.1, 1) + np.float32(0.5)],
        'tone_floor': [_tone(2000, 1e-3, 3)],
        'chirp_top': [_chirp(2000, 3000.0, 7900.0)],
        'impulse': [_impulse(880, 437, 0.5)],
        'silence': [np.zeros(880, dtype=np.float32)],
        'const': [np.full(880, 0.25, dtype=np.float32)],
    }
    for n in FBANK_FRAME_COUNTS:
        c[f'len{n}'] = [_white(n, 0.1, 10 + n)]
    c['ragged'] = [_white(n, 0.1, 20 + i) for i, n in enumerate((4000, 0, 399, 561))]
    return c


def _logmel_cases():
    loud = _white(1000, 0.3, 31)
    quiet = _tone(2000, 1e-5, 32) * np.float32(1e-3)
    c = {
        'white': [_white(1000, 0.1, 33)],
        'ramp': [(0.3 * np.arange(1000) / 1000.0).astype(np.float32) + _white(1000, 0.01, 34)],
        'one_frame': [_white(201, 0.1, 35)],
        'tone_floor': [_tone(2000, 1e-5, 32)],
        'level_step': [loud, quiet],
        'level_step_rev': [quiet, loud],
        'silence': [np.zeros(800, dtype=np.float32)],
        'silence_then_noise': [np.concatenate([np.zeros(800, dtype=np.float32),
                                               _white(800, 0.1, 36)])],
    }
    for n in LOGMEL_FRAME_COUNTS:
        c[f'len{n}'] = [_white(n, 0.1, 40 + n)]
    c['ragged'] = [_white(n, 0.1, 50 + i) for i, n in enumerate((1000, 201, 1600, 320))]
    return c


CASES_FBANK = _fbank_cases()
CASES_LOGMEL = _logmel_cases()
FBANK_SINGLE = [k for k, v in CASES_FBANK.items() if len(v) == 1]
LOGMEL_SINGLE = [k for k, v in CASES_LOGMEL.items() if len(v) == 1]


@functools.lru_cache(maxsize=None)
def fbank_refs(name):
    """[(ref64, plain32)] per utterance of the case; computed once, never written to."""
    out = [(fbank64(w), fbank32(w)) for w in CASES_FBANK[name]]
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def logmel_refs(name, n_mels):
    out = [(logmel64(w, n_mels), logmel32(w, n_mels)) for w in CASES_LOGMEL[name]]
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out
