// Host tables of the Kaldi fbank kernel (fbank.hip; runtime/core/frontend/fbank.h:91-163): the
// povey window, the 512-point twiddles and the mel filter bank as CSR rows.  Built by every
// wn_model_create* entry point, whatever its encoder.
#pragma once
#include <math.h>

#include <vector>

namespace wn {

struct FbankTables {
  std::vector<float> window;    // [400]
  std::vector<float> twiddle;   // [256][2] cos, -sin of 2 pi k / 512
  std::vector<float> mel_w;     // CSR weights
  std::vector<int> mel_start, mel_len, mel_off;   // [n_mel]
  bool ok = true;               // false: a bin without an FFT bin (e.g. 128 bins)
};

inline FbankTables make_fbank_tables(int nbins) {
  FbankTables t;
  t.window.resize(400);
  t.twiddle.resize(512);
  t.mel_start.resize(nbins); t.mel_len.resize(nbins); t.mel_off.resize(nbins);
  const double a = 2.0 * M_PI / 399.0;
  for (int i = 0; i < 400; ++i) t.window[i] = (float)pow(0.5 - 0.5 * cos(a * i), 0.85);
  for (int k = 0; k < 256; ++k) {
    t.twiddle[2 * k] = (float)cos(2.0 * M_PI * k / 512.0);
    t.twiddle[2 * k + 1] = (float)-sin(2.0 * M_PI * k / 512.0);
  }
  auto mel = [](float f) { return 1127.0f * logf(1.0f + f / 700.0f); };
  const int nfft_bins = 256;
  const float bin_w = 16000.0f / 512.0f;
  const float mlo = mel(20.0f), mhi = mel(8000.0f);
  const float delta = (mhi - mlo) / (float)(nbins + 1);
  for (int b = 0; b < nbins; ++b) {
    const float left = mlo + b * delta, center = mlo + (b + 1) * delta,
                right = mlo + (b + 2) * delta;
    int first = -1, last = -1;
    std::vector<float> row(nfft_bins, 0.f);
    for (int i = 0; i < nfft_bins; ++i) {
      const float mf = mel(bin_w * i);
      if (mf > left && mf < right) {
        row[i] = mf <= center ? (mf - left) / (center - left)
                              : (right - mf) / (right - center);
        if (first < 0) first = i;
        last = i;
      }
    }
    if (first < 0) { t.ok = false; first = last = 0; }
    t.mel_start[b] = first; t.mel_len[b] = last + 1 - first; t.mel_off[b] = (int)t.mel_w.size();
    for (int i = first; i <= last; ++i) t.mel_w.push_back(row[i]);
  }
  return t;
}

}  // namespace wn
