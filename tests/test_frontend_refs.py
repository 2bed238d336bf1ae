"""CPU checks of tests/frontend_refs.py, the references and the acceptance rule of the feature
front-end operator tests (tests/test_gpu_features.py).

(a) The fp64 references are the definition: the oracle's fbank and log-mel (fp32 restatements of
    the reference's text) and the committed outputs of the reference's own C++ fbank pass `accept`
    against them -- two honest fp32 implementations, so the bar is not too tight for one either.
(b) The rule bites: every mutant of the fp32 implementation (a mel weight 1 % off, window[1]
    doubled, a wrong DC divisor, ...) is rejected on at least one case with an error of at least
    ten times that case's tolerance, while the unmutated one passes everywhere.
(c) The inputs do what they are there for: the floor case is mostly floor, the level step makes
    the per-utterance maximum matter, digital silence lands exactly on the two clamps.
"""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import frontend_refs as FR

N_MELS = [80, 128]


def _oracle():
    from oracle import wenet_oracle as O
    return O


# ---------------------------------------------------------------------------------------------
# (a) the references are the definition


def test_parameter_tables_are_the_definitions():
    """The restated fp32 parameters against the oracle's: the povey window and the Slaney matrix
    bit for bit; the HTK weights with the same FFT bins inside every triangle (the weights
    themselves move with the last bit of the fp32 logarithm in the mel scale); the periodic Hann
    window within 2 ulp of torch.hann_window, which evaluates the cosine in fp32."""
    O = _oracle()
    assert np.array_equal(FR.povey_window(), O.povey_window())
    mine, theirs = FR.mel_banks(), O.mel_banks()
    assert np.array_equal(mine != 0, theirs != 0)
    assert (mine != 0).sum(axis=1).min() >= 1
    assert np.abs(mine - theirs).max() < 5e-5
    for n in N_MELS:
        assert np.array_equal(FR.slaney_mel(n), O.slaney_mel_filters(16000, 400, n))
    assert np.abs(FR.hann_window() - torch.hann_window(400).numpy()).max() <= 2.0 ** -22


@pytest.mark.parametrize('name', list(FR.CASES_FBANK))
def test_fbank64_is_the_oracle_fbank(name):
    """The yardstick of the oracle (NumPy sums, a library FFT) is the library-FFT form of the fp32
    evaluation, as the kernel's is the kernel's form: on an 80-element case the max-abs error is
    the draw of one ill-conditioned element, and the draws of two summation orders differ by more
    than the factor of the rule now and then (frontend_refs.py)."""
    O = _oracle()
    for i, (w, (ref, _)) in enumerate(zip(FR.CASES_FBANK[name], FR.fbank_refs(name))):
        got = O.fbank(w)
        assert got.shape[0] == ref.shape[0] == FR.fbank_frames(len(w))
        FR.accept(got, ref, FR.fbank32_fft(w), f'oracle.fbank {name}[{i}]')


def test_fbank64_is_the_reference_cpp_fbank():
    """tests/golden/fbank_*.npz: outputs of the reference's C++ fbank, a second fp32
    implementation; waveforms rebuilt from `meta` as test_fbank_vs_reference_cpp_golden does."""
    from wenet_amd import synthetic as S
    paths = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'fbank_*.npz')))
    assert len(paths) >= 4
    with_frames = 0
    for p in paths:
        z = np.load(p)
        meta = json.loads(bytes(z['meta']).decode())
        w = S.make_audio(meta['samples'], seed=meta['seed'])
        ref = FR.fbank64(w)
        assert ref.shape[0] == z['feats'].shape[0] == meta['frames']
        if ref.shape[0]:
            with_frames += 1
            FR.accept(z['feats'], ref, FR.fbank32_fft(w), f'C++ fbank {meta["case"]}')
    assert with_frames >= 3


@pytest.mark.parametrize('n_mels', N_MELS)
def test_logmel64_is_the_oracle_log_mel(n_mels):
    """The oracle multiplies by torch.hann_window(400), whose fp32 cosine is up to 2 ulp off the
    rounded window the kernel's table holds.  An output that is a near-cancellation of the
    transform magnifies that difference of DATA beyond any rounding bar, so both references take
    the oracle's window here: the comparison is about the formula.  The oracle's transform is
    torch.stft, an fp32 FFT, so the fp32 yardstick is the FFT form of logmel32 (on the 1 kHz tone
    the FFT is up to 4.2 x noisier in the far bins than the matrix product the kernel runs)."""
    O = _oracle()
    win = torch.hann_window(400).numpy()
    for name, ws in FR.CASES_LOGMEL.items():
        for i, w in enumerate(ws):
            got = O.log_mel_spectrogram(w, n_mels)
            ref = FR.logmel64(w, n_mels, window=win)
            assert got.shape[0] == ref.shape[0] == FR.logmel_frames(len(w))
            FR.accept(got, ref, FR.logmel32(w, n_mels, window=win, fft=True),
                      f'oracle.log_mel {n_mels} {name}[{i}]')


# ---------------------------------------------------------------------------------------------
# (b) the checker bites


def _mel_edge_off():
    w = FR.mel_banks().copy()
    w[0, np.nonzero(w[0])[0][0]] *= np.float32(1.01)      # the rising edge of the first triangle
    return w


def _window1_doubled():
    w = FR.povey_window().copy()
    w[1] *= np.float32(2.0)
    return w


FBANK_MUTANTS = {
    'mel_edge_weight_x1.01': dict(mel_w=_mel_edge_off()),
    'window1_x2': dict(window=_window1_doubled()),
    'dc_divisor_512': dict(dc_div=512.0),
    'preemphasis_0.96': dict(preemph=0.96),
    'frame_start_plus_1': dict(shift=1),
    'log_floor_1e-10': dict(log_floor=1e-10),
}


def _rejected_by(figures):
    """figures: [(case, measure dict)].  The mutant must fail `accept` on a case whose max-abs
    error is at least 10 x the tolerance of that case; returns the widest margin."""
    best = max(figures, key=lambda f: f[1]['err'] / f[1]['tol'])
    margin = best[1]['err'] / best[1]['tol']
    print(f'rejected on {best[0]}: err={best[1]["err"]:.3e} tol={best[1]["tol"]:.3e} '
          f'margin={margin:.1f}x')
    assert margin >= 10.0, (best[0], best[1])
    return best[0]


@pytest.mark.parametrize('mutant', list(FBANK_MUTANTS))
def test_fbank_mutant_is_rejected(mutant):
    figures = []
    for name, ws in FR.CASES_FBANK.items():
        for i, (w, (ref, plain)) in enumerate(zip(ws, FR.fbank_refs(name))):
            if ref.shape[0]:
                bad = FR.fbank32(w, **FBANK_MUTANTS[mutant])
                figures.append(((name, i), FR.measure(bad, ref, plain)))
    name, i = _rejected_by(figures)
    ref, plain = FR.fbank_refs(name)[i]
    with pytest.raises(AssertionError):
        FR.accept(FR.fbank32(FR.CASES_FBANK[name][i], **FBANK_MUTANTS[mutant]), ref, plain, mutant)


def _batch_max(ws, n_mels):
    umax = max(FR.logmel_max(w, n_mels, fp32=True) for w in ws)
    return [FR.logmel32(w, n_mels, umax=umax) for w in ws]


def _per_utterance(**mut):
    return lambda ws, n_mels: [FR.logmel32(w, n_mels, **mut) for w in ws]


LOGMEL_MUTANTS = {
    'reflect_with_edge_repeat': _per_utterance(edge_repeat=True),
    'symmetric_hann': _per_utterance(hann_denominator=399),
    'first_frame_dropped': _per_utterance(drop_first=True),
    'floor_max_minus_7.9': _per_utterance(span=7.9),
    'batch_maximum': _batch_max,
    'clamp_1e-8': _per_utterance(clamp=1e-8),
}


@pytest.mark.parametrize('n_mels', N_MELS)
@pytest.mark.parametrize('mutant', list(LOGMEL_MUTANTS))
def test_logmel_mutant_is_rejected(mutant, n_mels):
    figures, outs = [], {}
    for name, ws in FR.CASES_LOGMEL.items():
        bad = LOGMEL_MUTANTS[mutant](ws, n_mels)
        for i, (ref, plain) in enumerate(FR.logmel_refs(name, n_mels)):
            figures.append(((name, i), FR.measure(bad[i], ref, plain)))
            outs[(name, i)] = bad[i]
    key = _rejected_by(figures)
    ref, plain = FR.logmel_refs(key[0], n_mels)[key[1]]
    with pytest.raises(AssertionError):
        FR.accept(outs[key], ref, plain, mutant)


def test_unmutated_fp32_is_accepted_everywhere():
    for name in FR.CASES_FBANK:
        for i, (ref, plain) in enumerate(FR.fbank_refs(name)):
            FR.accept(plain, ref, plain, f'fbank32 {name}[{i}]')
    for n_mels in N_MELS:
        for name in FR.CASES_LOGMEL:
            for i, (ref, plain) in enumerate(FR.logmel_refs(name, n_mels)):
                FR.accept(plain, ref, plain, f'logmel32 {n_mels} {name}[{i}]')


def test_accept_rejects_nan_and_a_small_bias():
    """A NaN anywhere fails; so does a bias in every element that stays under the max-abs bar of
    the case (the p99 half of the rule)."""
    ref, plain = FR.fbank_refs('white')[0]
    bad = plain.copy()
    bad[3, 7] = np.nan
    with pytest.raises(AssertionError):
        FR.accept(bad, ref, plain, 'nan')
    m = FR.measure(plain, ref, plain)
    assert m['tol99'] < 0.8 * m['tol']
    biased = ref + 0.5 * (m['tol99'] + m['tol'])
    assert FR.measure(biased, ref, plain)['err'] <= m['tol']
    with pytest.raises(AssertionError):
        FR.accept(biased, ref, plain, 'bias')


# ---------------------------------------------------------------------------------------------
# (c) conditions on the inputs, fp64 side only


def test_frame_counts_of_the_cases():
    for n, t in FR.FBANK_FRAME_COUNTS.items():
        assert FR.fbank_frames(n) == t == FR.fbank_refs(f'len{n}')[0][0].shape[0]
    for n, t in FR.LOGMEL_FRAME_COUNTS.items():
        assert FR.logmel_frames(n) == t == FR.logmel_refs(f'len{n}', 80)[0][0].shape[0]
    assert [r.shape[0] for r, _ in FR.fbank_refs('ragged')] == [23, 0, 0, 2]
    assert [r.shape[0] for r, _ in FR.logmel_refs('ragged', 80)] == [6, 1, 10, 2]
    assert FR.logmel_refs('one_frame', 80)[0][0].shape[0] == 1
    assert all(len(w) <= 4000 for c in (FR.CASES_FBANK, FR.CASES_LOGMEL)
               for ws in c.values() for w in ws)


def _floor_share(ref):
    return float((ref == ref.min()).mean())


@pytest.mark.parametrize('n_mels', N_MELS)
def test_floor_case_is_mostly_floor(n_mels):
    w = FR.CASES_LOGMEL['tone_floor'][0]
    ref = FR.logmel_refs('tone_floor', n_mels)[0][0]
    lo = (FR.logmel_max(w, n_mels) - 8.0 + 4.0) / 4.0
    assert ref.min() == lo                       # the minimum IS the floor, not a small value
    share = _floor_share(ref)
    print(f'tone_floor {n_mels}: {share:.2f} of the elements at the floor')
    assert 0.50 <= share <= 0.95


@pytest.mark.parametrize('n_mels', N_MELS)
def test_level_step_needs_the_per_utterance_maximum(n_mels):
    """With the batch maximum in place of its own, the quiet utterance's reference moves by more
    than 100 x its tolerance -- in either order of the batch."""
    for name, quiet in (('level_step', 1), ('level_step_rev', 0)):
        ws = FR.CASES_LOGMEL[name]
        maxima = [FR.logmel_max(w, n_mels) for w in ws]
        assert maxima[quiet] < maxima[1 - quiet] - 2.0
        ref, plain = FR.logmel_refs(name, n_mels)[quiet]
        moved = np.abs(FR.logmel64(ws[quiet], n_mels, umax=max(maxima)) - ref).max()
        tol = FR.measure(plain, ref, plain)['tol']
        print(f'{name} {n_mels}: batch maximum moves the quiet utterance by {moved:.3e}, '
              f'tolerance {tol:.3e}')
        assert moved > 100.0 * tol


def test_silence_lands_on_the_clamps():
    for name in ('silence', 'const'):
        ref = FR.fbank_refs(name)[0][0]
        assert ref.shape == (4, 80)
        assert np.all(ref == math.log(FR.FLT_EPSILON))
    for n_mels in N_MELS:
        ref = FR.logmel_refs('silence', n_mels)[0][0]
        assert ref.shape == (5, n_mels)
        assert np.all(ref == -1.5)


@pytest.mark.parametrize('n_mels', N_MELS)
def test_silent_frames_before_noise_sit_at_the_floor(n_mels):
    """silence_then_noise: the frames of the silent half hold (max - 8 + 4) / 4, above the -1.5 of
    the clamp."""
    w = FR.CASES_LOGMEL['silence_then_noise'][0]
    ref = FR.logmel_refs('silence_then_noise', n_mels)[0][0]
    lo = (FR.logmel_max(w, n_mels) - 8.0 + 4.0) / 4.0
    assert lo > -1.5
    assert np.all(ref[:3] == lo)                 # frames centred at 0, 160, 320: zeros only
    assert np.all(ref[6:] > lo)


def test_impulse_frames():
    """impulse: the sample lies in frames 1 and 2 (at window positions 277 and 117); frames 0
    and 3 are digital silence."""
    ref = FR.fbank_refs('impulse')[0][0]
    floor = math.log(FR.FLT_EPSILON)
    assert np.all(ref[[0, 3]] == floor)
    assert np.all(ref[[1, 2]] > floor)
    assert np.abs(ref[1] - ref[2]).max() > 1e-2


def test_chirp_carries_the_top_filters():
    ref = FR.fbank_refs('chirp_top')[0][0]
    assert ref[:, 60:].max(axis=0).min() > ref.max() - 7.0
