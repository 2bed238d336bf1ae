// C ABI (include/wenet_amd.h), utterance-normalised fbank (compute_w2vbert_fbank,
// dataset/processor.py:259-272) over the kernels of utt_norm.hip: wn_utt_normalize behind wn_fbank,
// the switch that lets wn_encode on a W2v-BERT (shaw) handle take raw fbank, and the two operator
// hooks.  The statistics workspace belongs to the handle and grows on demand.
#include "model_state.h"

int utt_stats_handle(wn_model* m, const float* feats_dev, int max_len, int B, int T, int F,
                     hipStream_t s) {
  using namespace wn;
  UttStatsArgs a;
  a.n_slab = cdiv(max_len, UTT_SLAB);
  WN_TRY(m->utt_ws.ensure((size_t)B * std::max(a.n_slab, 1) * 3 * F * sizeof(float)));
  WN_TRY(m->utt_mean.ensure((size_t)B * F * sizeof(float)));
  WN_TRY(m->utt_std.ensure((size_t)B * F * sizeof(float)));
  a.feats = feats_dev; a.len = m->utt_len.as<int>(); a.ws = m->utt_ws.as<float>();
  a.mean = m->utt_mean.as<float>(); a.std = m->utt_std.as<float>();
  a.B = B; a.T = T; a.F = F;
  return utt_stats(a, s);
}

namespace wn {
namespace {

// the checks every entry shares; the longest length comes back
int check_lens(const int32_t* lens, int B, int T, const std::string& who, int* max_len) {
  *max_len = 0;
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens[b] >= 0 && lens[b] <= T, who + ": a length outside [0, T] (len > T)");
    *max_len = std::max(*max_len, (int)lens[b]);
  }
  return 0;
}

// host ints -> a hook's own device buffer (the hooks synchronise: test entry points)
int upload_hook_ints(DevBuf& buf, const std::vector<int>& v, hipStream_t s) {
  WN_TRY(buf.ensure(v.size() * sizeof(int)));
  WN_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace
}  // namespace wn

extern "C" {

int wn_utt_normalize(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int32_t B,
                     int32_t T, int32_t F, float* out_dev, void* stream) {
  WN_CHECK(m && feats_dev && feat_lens_host && out_dev, "wn_utt_normalize: null argument");
  WN_ENTER(m);
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F >= 1, "wn_utt_normalize: B / T / F");
  WN_CHECK(F <= 128, "wn_utt_normalize: F > 128");
  WN_CHECK(F % 4 == 0, "wn_utt_normalize: F % 4 != 0");
  WN_CHECK((((uintptr_t)feats_dev | (uintptr_t)out_dev) & 15) == 0,
           "wn_utt_normalize: feats and out must be 16-byte aligned");
  int max_len = 0;
  WN_TRY(check_lens(feat_lens_host, B, T, "wn_utt_normalize", &max_len));
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  WN_TRY(m->stage.begin((size_t)B * sizeof(int32_t) + 1024));
  WN_TRY(m->stage.put(m->utt_len, feat_lens_host, (size_t)B * sizeof(int32_t), s));
  WN_TRY(m->stage.end(s));
  WN_TRY(utt_stats_handle(m, feats_dev, max_len, B, T, F, s));
  return utt_normalize(feats_dev, m->utt_len.as<int>(), m->utt_mean.as<float>(),
                       m->utt_std.as<float>(), out_dev, B, T, F, s);
}

int wn_model_set_utt_norm_input(wn_model* m, int32_t on) {
  WN_CHECK(m, "wn_model_set_utt_norm_input: null argument");
  WN_ENTER(m);
  WN_CHECK(m->sh.on, "wn_model_set_utt_norm_input: a W2v-BERT (shaw) handle only (the family "
                     "whose features are utterance-normalised)");
  m->sh.utt_input = on != 0;
  return 0;
}

int wn_op_utt_stats(const float* feats, const int32_t* lens, int32_t B, int32_t T, int32_t F,
                    float* mean, float* std_out, void* stream) {
  WN_CHECK(feats && lens && mean && std_out, "utt_stats: null argument");
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F >= 1, "utt_stats: B / T / F");
  WN_CHECK(F <= 128, "utt_stats: F > 128 (two bins per lane)");
  int max_len = 0;
  WN_TRY(check_lens(lens, B, T, "utt_stats", &max_len));
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, ws;
  WN_TRY(upload_hook_ints(desc, std::vector<int>(lens, lens + B), s));
  UttStatsArgs a;
  a.n_slab = cdiv(max_len, UTT_SLAB);
  WN_TRY(ws.ensure((size_t)B * std::max(a.n_slab, 1) * 3 * F * sizeof(float)));
  a.feats = feats; a.len = desc.as<int>(); a.ws = ws.as<float>(); a.mean = mean; a.std = std_out;
  a.B = B; a.T = T; a.F = F;
  return utt_stats(a, s);
}

int wn_op_stack_frames_ln_utt(const float* feats, const float* umean, const float* ustd,
                              const float* mean, const float* istd, const float* ln_w,
                              const float* ln_b, float* out, int32_t ldo, int32_t out_rows,
                              const int32_t* lens, const int32_t* out_off, int32_t* out_len,
                              int32_t B, int32_t T, int32_t F, void* stream) {
  WN_CHECK(feats && umean && ustd && ln_w && ln_b && out && lens && out_off && out_len,
           "stack_frames_ln_utt: null argument");
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F >= 1 && out_rows > 0,
           "stack_frames_ln_utt: B / T / F");
  WN_CHECK(F <= 128, "stack_frames_ln_utt: F > 128 (2 F values per row)");
  int max_len = 0;
  WN_TRY(check_lens(lens, B, T, "stack_frames_ln_utt", &max_len));
  std::vector<int> h((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    out_len[b] = lens[b] / 2;
    h[b] = out_off[b]; h[B + b] = out_len[b];
    // rows of ascending, disjoint ranges inside the buffer
    WN_CHECK(out_off[b] >= (b ? out_off[b - 1] + out_len[b - 1] : 0) &&
                 (int64_t)out_off[b] + out_len[b] <= out_rows,
             "stack_frames_ln_utt: rows outside the buffer, unordered or overlapping");
  }
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(upload_hook_ints(desc, h, s));
  StackFramesUttArgs a;
  a.k.feats = feats; a.k.mean = mean; a.k.istd = istd; a.k.ln_w = ln_w; a.k.ln_b = ln_b;
  a.k.out = out; a.k.ldo = ldo; a.k.off = desc.as<int>(); a.k.len = a.k.off + B;
  a.k.B = B; a.k.T = T; a.k.F = F; a.k.max_len = max_len / 2; a.k.eps = 1e-5f;
  a.umean = umean; a.ustd = ustd;
  return stack_frames_ln_utt(a, s);
}

}  // extern "C"
