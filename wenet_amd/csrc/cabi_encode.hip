// C ABI (include/wenet_amd.h), features -> encoder output: wn_encode and the streaming chunk
// calls over the engine (model.hip), and the audio front ends (resampler, Kaldi fbank, Whisper
// log-mel) with their tables.
#include "model_state.h"

namespace wn {
namespace {

int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// Fill a table of the shared model block that is built on first use.  The caller holds
// ModelData::lazy; `slot` stays empty until the finished buffer is swapped in, so a failed
// build is tried again by the next call and a set slot is never written again.
int publish_table(DevBuf& slot, const std::vector<float>& v) {
  DevBuf nb;
  WN_TRY(nb.ensure(v.size() * sizeof(float)));
  WN_HIP(hipMemcpy(nb.p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  slot.swap(nb);
  return 0;
}

// librosa.filters.mel(sr=16000, n_fft=400, n_mels) (slaney scale + norm), the
// matrix processor.py:360-361 multiplies with (librosa is third party: its
// published algorithm is restated; the test oracle restates it independently in
// numpy).  Row-major [n_mels][LOGMEL_K2].
std::vector<float> slaney_mel_matrix(int n_mels) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, logstep = log(6.4) / 27.0;
  const double min_log_mel = min_log_hz / f_sp;
  auto hz2mel = [&](double f) {
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
  };
  auto mel2hz = [&](double mm) {
    return mm >= min_log_mel ? min_log_hz * exp(logstep * (mm - min_log_mel)) : f_sp * mm;
  };
  const int nb = 201;
  std::vector<double> mel_f(n_mels + 2);
  const double m_lo = hz2mel(0.0), m_hi = hz2mel(8000.0);
  for (int i = 0; i < n_mels + 2; ++i)
    mel_f[i] = mel2hz(m_lo + (m_hi - m_lo) * i / (double)(n_mels + 1));
  std::vector<float> w((size_t)n_mels * LOGMEL_K2, 0.f);
  for (int i = 0; i < n_mels; ++i) {
    const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int k = 0; k < nb; ++k) {
      const double f = 8000.0 * k / 200.0;
      const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
      const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
      const double v = std::max(0.0, std::min(lower, upper));
      w[(size_t)i * LOGMEL_K2 + k] = (float)(v * enorm);
    }
  }
  return w;
}

}  // namespace
}  // namespace wn

// ===========================================================================
extern "C" {

int wn_encode(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host,
              int32_t B, int32_t T, int32_t chunk, int32_t left,
              float* enc_out_dev, int32_t* enc_lens_host, void* stream) {
  WN_CHECK(m && feats_dev && feat_lens_host, "wn_encode: null argument");
  WN_ENTER(m);
  // the encode gate is one-shot: whatever way this call ends (an argument check included), it
  // does not stay on the handle for a later call to wait on an event that may be gone by then
  struct GateDrop { wn_model* m; ~GateDrop() { m->enc_gate = nullptr; } } gate_drop{m};
  m->pb_valid = false;
  PrecisionScope prec_scope(m);
  WN_CHECK(!m->data->layers.empty() || !m->data->tf_layers.empty() || m->pf.on || m->sv.on,
           "wn_encode: this handle has no weights");
  WN_CHECK(B > 0, "wn_encode: empty batch");
  WN_CHECK(chunk != 0, "decoding_chunk_size must not be 0 (asr_model.py:310)");
  if (m->sv.on) {
    // (stored query ids serve one encode, however it ends: encode_sensevoice takes them first)
    struct QidDrop { wn_model* m; ~QidDrop() { m->sv.qid.clear(); } } qid_drop{m};
    WN_CHECK(chunk < 0, "chunk decoding is not implemented for the SenseVoice encoder (it "
                        "attends over the full utterance)");
    WN_CHECK(m->prec == PREC_F32, "wn_encode: a SenseVoice handle stays fp32");
    WN_CHECK(T >= 1, "wn_encode: empty features");
    WN_HIP(hipSetDevice(m->device));
    WN_TRY(encode_gate_wait(m, (hipStream_t)stream));
    return encode_sensevoice(m, feats_dev, feat_lens_host, B, T, enc_out_dev, enc_lens_host,
                             (hipStream_t)stream);
  }
  if (m->pf.on) {
    WN_CHECK(chunk < 0, "chunk decoding is not implemented for the Paraformer encoder (it "
                        "attends over the full utterance)");
    WN_CHECK(m->prec == PREC_F32, "wn_encode: a Paraformer handle stays fp32");
    WN_CHECK(T >= 1, "wn_encode: empty features");
    WN_HIP(hipSetDevice(m->device));
    WN_TRY(encode_gate_wait(m, (hipStream_t)stream));
    return encode_paraformer(m, feats_dev, feat_lens_host, B, T, enc_out_dev, enc_lens_host,
                             (hipStream_t)stream);
  }
  if (m->fr.on) {
    WN_CHECK(chunk < 0, "chunk decoding is not implemented for the FireRed encoder (the "
                        "reference: firedasr don't support streaming)");
    WN_CHECK(m->prec == PREC_F32, "wn_encode: a FireRed handle stays fp32");
    WN_CHECK(T >= 1, "wn_encode: empty features");
    WN_HIP(hipSetDevice(m->device));
    WN_TRY(encode_gate_wait(m, (hipStream_t)stream));
    return encode_firered(m, feats_dev, feat_lens_host, B, T, enc_out_dev, enc_lens_host,
                          (hipStream_t)stream);
  }
  if (m->bf.on) {
    WN_CHECK(m->prec == PREC_F32, "wn_encode: a Branchformer handle stays fp32");
    WN_CHECK(T >= 7, "wn_encode: at least 7 frames are needed by Conv2dSubsampling4");
    WN_HIP(hipSetDevice(m->device));
    return encode_branchformer(m, feats_dev, feat_lens_host, B, T, chunk, left, enc_out_dev,
                               enc_lens_host, (hipStream_t)stream);
  }
  if (m->sq.on) {
    WN_CHECK(m->prec == PREC_F32, "wn_encode: a Squeezeformer handle stays fp32");
    WN_CHECK(T >= 7, "wn_encode: at least 7 frames are needed by the conv2d front end");
    WN_HIP(hipSetDevice(m->device));
    return encode_squeezeformer(m, feats_dev, feat_lens_host, B, T, chunk, left, enc_out_dev,
                                enc_lens_host, (hipStream_t)stream);
  }
  if (m->ef.on) {
    WN_CHECK(m->prec == PREC_F32, "wn_encode: an Efficient Conformer handle stays fp32");
    WN_CHECK(T >= (m->ef.c.front_rate == 4 ? 7 : 3),
             "wn_encode: at least 7 (conv2d) / 3 (conv2d2) frames are needed by the front end");
    WN_HIP(hipSetDevice(m->device));
    return encode_efficonformer(m, feats_dev, feat_lens_host, B, T, chunk, left, enc_out_dev,
                                enc_lens_host, (hipStream_t)stream);
  }
  if (m->cfg.encoder_type == 1) {
    WN_CHECK(chunk < 0 && m->cfg.static_chunk_size <= 0,
             "chunk decoding is not implemented for the transformer encoder");
    WN_CHECK(T >= 1, "wn_encode: empty features");
    WN_HIP(hipSetDevice(m->device));
    WN_TRY(encode_gate_wait(m, (hipStream_t)stream));
    return encode_transformer(m, feats_dev, feat_lens_host, B, T, enc_out_dev,
                              enc_lens_host, (hipStream_t)stream);
  }
  WN_CHECK(T >= 7, "wn_encode: at least 7 frames are needed by Conv2dSubsampling4");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int d = c.d_model;
  const int Tp = ((T - 1) / 2 - 1) / 2;
  WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, enc_lens_host, 0, s));
  WN_TRY(encode_gate_wait(m, s));     // (paths that did not consume the gate behind conv1)
  const int M = m->rows;
  if (M > 0) {
    WN_TRY(encoder_layers(m, chunk, left, s));
  }
  if (enc_out_dev) {
    if (M > 0) {
      WN_TRY(scatter_padded(m->enc.as<float>(), d, m->d_off.as<int>(), m->d_len.as<int>(), B, Tp,
                            d, enc_out_dev, s));
    } else if (Tp > 0) {
      WN_HIP(hipMemsetAsync(enc_out_dev, 0, (size_t)B * Tp * d * sizeof(float), s));
    }
  }
  return 0;
}

int wn_encode_chunk_batch(wn_model* m, int32_t n_sess, const float* feats_dev, int32_t time,
                          const int32_t* offsets_host, int32_t required_cache_size,
                          const float* const* att_cache_dev, const int32_t* cache_t1_host,
                          const float* const* cnn_cache_dev, float* out_dev,
                          float* const* new_att_cache_dev, float* const* new_cnn_cache_dev,
                          int32_t* chunk_out, int32_t* new_cache_t1_out, void* stream) {
  WN_CHECK(m && feats_dev && out_dev && offsets_host && cache_t1_host && n_sess >= 1,
           "wn_encode_chunk: null argument");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  WN_CHECK(!m->data->layers.empty() && m->cfg.encoder_type == 0,
           "wn_encode_chunk: needs a Conformer encoder");
  WN_CHECK(!m->fr.on, "wn_encode_chunk: the FireRed encoder does not stream");
  WN_CHECK(!m->bf.on, "wn_encode_chunk: no chunk-by-chunk path for a Branchformer encoder (the "
                      "cgMLP conv cache)");
  WN_CHECK(!m->sq.on, "wn_encode_chunk: no chunk-by-chunk path for a Squeezeformer encoder (the "
                      "time reduction's caches)");
  WN_CHECK(!m->ef.on, "wn_encode_chunk: no chunk-by-chunk path for an Efficient Conformer encoder "
                      "(the rate-mixed attention cache)");
  WN_CHECK(time >= 7, "wn_encode_chunk: at least 7 frames are needed by Conv2dSubsampling4");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int R = ((time - 1) / 2 - 1) / 2;
  const int lorder = c.causal ? c.cnn_kernel - 1 : 0;
  std::vector<ChunkSess> sess(n_sess);
  std::vector<int32_t> lens(n_sess, time);
  for (int b = 0; b < n_sess; ++b) {
    const int offset = offsets_host[b], t1c = cache_t1_host[b];
    WN_CHECK(offset >= 0 && t1c >= 0 && t1c <= offset,
             "wn_encode_chunk: need 0 <= cache_t1 <= offset");
    WN_CHECK(t1c == 0 || (att_cache_dev && att_cache_dev[b]), "wn_encode_chunk: att_cache is null");
    WN_CHECK(offset + R <= c.max_pos, "wn_encode_chunk: offset beyond the positional table");
    const int key = t1c + R;
    // encoder.py:258-263
    const int next_start = required_cache_size < 0 ? 0
                           : required_cache_size == 0 ? key
                           : std::max(key - required_cache_size, 0);
    const int nt = key - next_start;
    WN_CHECK(nt == 0 || (new_att_cache_dev && new_att_cache_dev[b]),
             "wn_encode_chunk: new_att_cache is null");
    WN_CHECK(lorder == 0 || (new_cnn_cache_dev && new_cnn_cache_dev[b]),
             "wn_encode_chunk: new_cnn_cache is null");
    ChunkSess& ss = sess[b];
    ss.att_cache = t1c > 0 ? att_cache_dev[b] : nullptr;
    // nt == 0: the kernel writes no cache rows, any non-null pointer will do
    ss.new_att = nt > 0 ? new_att_cache_dev[b] : out_dev;
    ss.cnn_cache = (cnn_cache_dev && lorder > 0) ? cnn_cache_dev[b] : nullptr;
    ss.new_cnn = lorder > 0 ? new_cnn_cache_dev[b] : nullptr;
    ss.t1 = t1c; ss.next_start = next_start; ss.nt = nt; ss.kv_off = 0;
    if (new_cache_t1_out) new_cache_t1_out[b] = nt;
  }
  WN_TRY(subsample_conv2d4(m, feats_dev, lens.data(), n_sess, time, nullptr,
                           offsets_host[0], s));
  WN_CHECK(m->rows == n_sess * R, "wn_encode_chunk: internal row count");
  WN_TRY(encoder_layers_chunk(m, n_sess, R, offsets_host, sess, out_dev, s));
  m->rows = 0; m->B = 0;  // the handle holds no decodable batch after a chunk call
  if (chunk_out) *chunk_out = R;
  return 0;
}

int wn_encode_chunk(wn_model* m, const float* feats_dev, int32_t time, int32_t offset,
                    int32_t required_cache_size, const float* att_cache_dev,
                    int32_t cache_t1, const float* cnn_cache_dev, float* out_dev,
                    float* new_att_cache_dev, float* new_cnn_cache_dev,
                    int32_t* chunk_out, int32_t* new_cache_t1_out, void* stream) {
  return wn_encode_chunk_batch(m, 1, feats_dev, time, &offset, required_cache_size,
                               &att_cache_dev, &cache_t1, &cnn_cache_dev, out_dev,
                               &new_att_cache_dev, &new_cnn_cache_dev, chunk_out,
                               new_cache_t1_out, stream);
}

int wn_set_encoder_out(wn_model* m, const float* enc_out_dev,
                       const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                       void* stream) {
  WN_CHECK(m && enc_out_dev && enc_lens_host && B > 0 && Tp > 0,
           "wn_set_encoder_out: bad argument");
  WN_ENTER(m);
  m->pb_valid = false;
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  std::vector<int> off(B), len(B);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(enc_lens_host[b] >= 0 && enc_lens_host[b] <= Tp, "length > Tp");
    off[b] = b * Tp; len[b] = enc_lens_host[b];
  }
  WN_TRY(set_layout(m, B, Tp, off, len, B * Tp, s));
  WN_TRY(m->stage.end(s));
  const size_t bytes = (size_t)B * Tp * m->cfg.d_model * sizeof(float);
  WN_TRY(m->enc.ensure(bytes));
  WN_HIP(hipMemcpyAsync(m->enc.p, enc_out_dev, bytes, hipMemcpyDeviceToDevice, s));
  return 0;
}

int64_t wn_resample_length(int64_t n_in, int32_t orig_freq, int32_t new_freq) {
  if (n_in <= 0 || orig_freq <= 0 || new_freq <= 0) return 0;
  const int g = gcd_int(orig_freq, new_freq);
  const int64_t o = orig_freq / g, n = new_freq / g;
  return (n * n_in + o - 1) / o;  // ceil(new * length / orig)
}

int wn_resample(wn_model* m, const float* pcm_dev, int64_t n_in, int32_t orig_freq,
                int32_t new_freq, float* out_dev, int64_t n_out, void* stream) {
  WN_CHECK(m && pcm_dev && out_dev, "wn_resample: null argument");
  WN_ENTER(m);
  WN_CHECK(orig_freq > 0 && new_freq > 0 && n_in > 0, "wn_resample: bad rate or length");
  WN_CHECK(n_out == wn_resample_length(n_in, orig_freq, new_freq),
           "wn_resample: n_out must be wn_resample_length(n_in, orig, new)");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  if (orig_freq == new_freq) {  // Resample.forward returns the input unchanged
    WN_HIP(hipMemcpyAsync(out_dev, pcm_dev, (size_t)n_in * sizeof(float),
                          hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const int g = gcd_int(orig_freq, new_freq);
  const int orig = orig_freq / g, nnew = new_freq / g;
  // sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99 (the defaults of
  // torchaudio.transforms.Resample); taps in fp64, stored fp32
  const double lpw = 6.0, rolloff = 0.99;
  const double base = std::min(orig, nnew) * rolloff;
  const int width = (int)std::ceil(lpw * orig / base);
  const int K = 2 * width + orig;
  const DevBuf* buf = nullptr;
  {
    const ModelData& W = *m->data;
    std::lock_guard<std::mutex> lock(W.lazy);
    DevBuf& slot = W.rs_taps[{orig, nnew}];
    buf = &slot;
    if (!slot.p) {
      std::vector<float> taps((size_t)nnew * K);
      const double pi = 3.14159265358979323846;
      for (int i = 0; i < nnew; ++i) {
        for (int k = 0; k < K; ++k) {
          double t = (-(double)i / nnew + (double)(k - width) / orig) * base;
          t = std::min(std::max(t, -lpw), lpw);
          const double c = std::cos(t * pi / lpw / 2.0);
          const double win = c * c;
          const double tp = t * pi;
          const double sinc = tp == 0.0 ? 1.0 : std::sin(tp) / tp;
          taps[(size_t)i * K + k] = (float)(sinc * win * (base / orig));
        }
      }
      WN_TRY(publish_table(slot, taps));
    }
  }
  return resample_sinc(pcm_dev, n_in, buf->as<float>(), K, width, orig, nnew, out_dev,
                       n_out, s);
}

int wn_fbank(wn_model* m, const float* pcm_dev, const int64_t* sample_off_host,
             int32_t B, float* feats_dev, int32_t max_frames,
             int32_t* n_frames_host, void* stream) {
  WN_CHECK(m && pcm_dev && sample_off_host && feats_dev && n_frames_host && B > 0,
           "wn_fbank: bad argument");
  WN_ENTER(m);
  const ModelData& W = *m->data;
  WN_CHECK(W.fbank_ok, "wn_fbank: no Kaldi fbank for this feature dimension "
                        "(Whisper models use log-mel, processor.py:320-369)");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  std::vector<int> nfr(B);
  std::vector<int64_t> off(B);
  for (int b = 0; b < B; ++b) {
    const int64_t n = sample_off_host[b + 1] - sample_off_host[b];
    WN_CHECK(n >= 0, "wn_fbank: sample offsets must be non-decreasing");
    nfr[b] = n < 400 ? 0 : (int)(1 + (n - 400) / 160);   // fbank.h:254-255
    WN_CHECK(nfr[b] <= max_frames, "wn_fbank: max_frames too small");
    off[b] = sample_off_host[b];
    n_frames_host[b] = nfr[b];
  }
  if (max_frames == 0) return 0;
  WN_TRY(m->stage.begin((size_t)B * 16 + 1024));
  WN_TRY(m->stage.put(m->fb_off, off.data(), off.size() * sizeof(int64_t), s));
  WN_TRY(m->stage.put(m->fb_nfr, nfr.data(), nfr.size() * sizeof(int), s));
  WN_TRY(m->stage.end(s));
  FbankArgs a;
  a.pcm = pcm_dev; a.sample_off = m->fb_off.as<int64_t>();
  a.n_frames = m->fb_nfr.as<int>(); a.B = B; a.max_frames = max_frames;
  a.n_mel = m->cfg.feat_dim; a.window = W.fb_window; a.twiddle = W.fb_twiddle;
  const int* tab = W.fb_tab_i.as<int>();
  a.mel_start = tab; a.mel_len = tab + a.n_mel; a.mel_off = tab + 2 * a.n_mel;
  a.mel_w = W.fb_mel_w; a.feats = feats_dev;
  return fbank_kaldi(a, s);
}

int wn_log_mel(wn_model* m, const float* pcm_dev, const int64_t* sample_off_host,
               int32_t B, int32_t n_mels, float* feats_dev, int32_t max_frames,
               int32_t* n_frames_host, void* stream) {
  WN_CHECK(m && pcm_dev && sample_off_host && feats_dev && n_frames_host && B > 0,
           "wn_log_mel: bad argument");
  WN_ENTER(m);
  WN_CHECK(n_mels >= 1 && n_mels <= 256, "wn_log_mel: num_mel_bins");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  std::vector<int> nfr(B), foff(B), row_utt;
  std::vector<int64_t> off(B + 1);
  int rows = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = sample_off_host[b + 1] - sample_off_host[b];
    // torch.stft(center=True) reflects n_fft/2 samples: needs n > 200
    WN_CHECK(n > 200, "wn_log_mel: an utterance needs more than 200 samples");
    nfr[b] = (int)(n / 160);          // 1 + n // hop frames, the last one dropped
    WN_CHECK(nfr[b] <= max_frames, "wn_log_mel: max_frames too small");
    off[b] = sample_off_host[b];
    foff[b] = rows;
    rows += nfr[b];
    n_frames_host[b] = nfr[b];
    for (int t = 0; t < nfr[b]; ++t) row_utt.push_back(b);
  }
  off[B] = sample_off_host[B];
  if (max_frames == 0) return 0;
  // ---- tables (once per model, shared by its clones) ---------------------------
  const ModelData& W = *m->data;
  const DevBuf* melw = nullptr;
  {
    std::lock_guard<std::mutex> lock(W.lazy);
    if (!W.lm_dft.p) {
      // [402][416] cos / -sin rows, then the periodic hann window [400]
      std::vector<float> t((size_t)LOGMEL_NS * LOGMEL_K1 + 400, 0.f);
      for (int k = 0; k <= 200; ++k)
        for (int n = 0; n < 400; ++n) {
          const double ph = 2.0 * M_PI * (double)((k * n) % 400) / 400.0;
          t[(size_t)k * LOGMEL_K1 + n] = (float)cos(ph);
          t[(size_t)(201 + k) * LOGMEL_K1 + n] = (float)-sin(ph);
        }
      for (int n = 0; n < 400; ++n)
        t[(size_t)LOGMEL_NS * LOGMEL_K1 + n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / 400.0));
      WN_TRY(publish_table(W.lm_dft, t));
    }
    DevBuf& slot = W.lm_mel[n_mels];
    melw = &slot;
    if (!slot.p) WN_TRY(publish_table(slot, slaney_mel_matrix(n_mels)));
  }
  if (rows == 0) {
    WN_HIP(hipMemsetAsync(feats_dev, 0, (size_t)B * max_frames * n_mels * sizeof(float), s));
    return 0;
  }
  WN_TRY(m->stage.begin((size_t)B * 32 + (size_t)rows * 4 + 4096));
  WN_TRY(m->stage.put(m->lm_off, off.data(), off.size() * sizeof(int64_t), s));
  WN_TRY(m->stage.put(m->lm_foff, foff.data(), foff.size() * sizeof(int), s));
  WN_TRY(m->stage.put(m->lm_nfr, nfr.data(), nfr.size() * sizeof(int), s));
  WN_TRY(m->stage.put(m->lm_rowutt, row_utt.data(), row_utt.size() * sizeof(int), s));
  WN_TRY(m->stage.end(s));
  WN_TRY(m->lm_frames.ensure((size_t)rows * LOGMEL_K1 * sizeof(float)));
  WN_TRY(m->lm_spec.ensure((size_t)rows * LOGMEL_NS * sizeof(float)));
  WN_TRY(m->lm_pw.ensure((size_t)rows * LOGMEL_K2 * sizeof(float)));
  WN_TRY(m->lm_melout.ensure((size_t)rows * n_mels * sizeof(float)));
  WN_TRY(m->lm_umax.ensure((size_t)B * sizeof(float)));
  LogMelArgs a;
  a.pcm = pcm_dev; a.sample_off = m->lm_off.as<int64_t>();
  a.row_utt = m->lm_rowutt.as<int>(); a.frame_off = m->lm_foff.as<int>();
  a.window = W.lm_dft.as<float>() + (size_t)LOGMEL_NS * LOGMEL_K1;
  a.frames = m->lm_frames.as<float>();
  WN_TRY(logmel_frames(a, rows, s));
  GemmArgs g1;  // DFT: [rows, 416] x [402, 416]^T
  g1.A = m->lm_frames.as<float>(); g1.W = W.lm_dft.as<float>();
  g1.C = m->lm_spec.as<float>(); g1.M = rows; g1.N = LOGMEL_NS; g1.K = LOGMEL_K1;
  g1.lda = LOGMEL_K1; g1.ldc = LOGMEL_NS;
  WN_TRY(gemm_f32(g1, s));
  WN_TRY(logmel_power(m->lm_spec.as<float>(), m->lm_pw.as<float>(), rows, s));
  GemmArgs g2;  // mel: [rows, 224] x [n_mels, 224]^T
  g2.A = m->lm_pw.as<float>(); g2.W = melw->as<float>();
  g2.C = m->lm_melout.as<float>(); g2.M = rows; g2.N = n_mels; g2.K = LOGMEL_K2;
  g2.lda = LOGMEL_K2; g2.ldc = n_mels;
  WN_TRY(gemm_f32(g2, s));
  return logmel_finish(m->lm_melout.as<float>(), n_mels, m->lm_foff.as<int>(),
                       m->lm_nfr.as<int>(), m->lm_umax.as<float>(), B, max_frames,
                       feats_dev, s);
}

}  // extern "C"
