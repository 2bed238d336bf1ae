// SenseVoice Small (wenet/models/sensevoice/): the front end that lays the four query rows of an
// utterance in front of its LFR rows.  The layer stacks behind it run on the Paraformer's kernels
// (cabi_sensevoice.hip).  fp32.
#include "kernels.h"

namespace wn {

namespace {

// Queries | LFR + CMVN, then position + LayerNorm of layer 0: one wave per output row, column
// c = 64 j + lane (lfr_front_kernel's layout).  The row before the norm never leaves the
// registers.  Every bound comes from len[b] / qid[b], which the host validated.
constexpr int SV_E = LFR_MAX_D / 64;

__global__ __launch_bounds__(256) void sv_front_kernel(SvFrontArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int n_fr = a.len[b];
  if (n_fr <= 0 || t >= SV_QUERY + (n_fr + a.n - 1) / a.n) return;
  const int D = a.m * a.F;
  const bool query = t < SV_QUERY;
  const int first = a.n * (t - SV_QUERY) - (a.m - 1) / 2;
  const float* fb = a.feats + (int64_t)b * a.T * a.F;
  const float* er = a.embed + (int64_t)(query ? a.qid[b * SV_QUERY + t] : 0) * D;
  const float* pe = a.pe + (int64_t)(t + 1) * D;      // positions start at 1, queries included
  float v[SV_E];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < SV_E; ++j) {
    const int c = j * 64 + lane;
    float x = 0.f;
    if (c < D) {
      if (query) {
        x = er[c];
      } else {
        const int f = c / a.F;
        int idx = first + f;
        idx = idx < 0 ? 0 : (idx > n_fr - 1 ? n_fr - 1 : idx);
        x = fb[(int64_t)idx * a.F + (c - f * a.F)];
        if (a.mean) x = (x - a.mean[c]) * a.istd[c];
      }
      x = x * a.xscale + pe[c];
      sum += x;
    }
    v[j] = x;
  }
  const float mean = wave_sum(sum) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < SV_E; ++j) {
    const float dlt = v[j] - mean;
    if (j * 64 + lane < D) q += dlt * dlt;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + a.eps);
  float* yr = a.out + (int64_t)(a.off[b] + t) * a.ldo;
#pragma unroll
  for (int j = 0; j < SV_E; ++j) {
    const int c = j * 64 + lane;
    if (c < D) yr[c] = (v[j] - mean) * rstd * a.ln_w[c] + a.ln_b[c];
    else if (c < a.ldo) yr[c] = 0.f;
  }
}

}  // namespace

int sv_front(const SvFrontArgs& a, hipStream_t s) {
  WN_CHECK(a.feats && a.embed && a.pe && a.ln_w && a.ln_b && a.out && a.len && a.off && a.qid,
           "sv_front: null argument");
  WN_CHECK(!a.mean == !a.istd, "sv_front: mean and istd come together");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.T > 0 && a.F > 0 && a.m > 0 && a.n > 0 &&
               a.max_rows > SV_QUERY, "sv_front: shape");
  WN_CHECK(a.m * a.F <= LFR_MAX_D && a.ldo >= a.m * a.F && a.ldo <= LFR_MAX_D,
           "sv_front: m * F <= ldo <= 576");
  dim3 g(cdiv(a.max_rows, 4), a.B), t(256);
  hipLaunchKernelGGL(sv_front_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
