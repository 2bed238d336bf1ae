// Paraformer kernels besides the d_k = 128 attention (attention_d128.hip): the LFR front end, a
// LayerNorm for wide rows, and the CIF predictor (the staged 3-tap image of its conv GEMM, the
// alpha rows, the integrate-and-fire scan).  fp32.
#include <algorithm>

#include "kernels.h"

namespace wn {

namespace {

// ===========================================================================
// LFR + CMVN + position + LayerNorm of layer 0: one wave per output row, column c = 64 j + lane.
// The row before the norm is never used again, so it never leaves the registers.
constexpr int LFR_E = LFR_MAX_D / 64;

__global__ __launch_bounds__(256) void lfr_front_kernel(LfrFrontArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int n_fr = a.len[b];
  if (n_fr <= 0 || t >= (n_fr + a.n - 1) / a.n) return;
  const int D = a.m * a.F;
  const int first = a.n * t - (a.m - 1) / 2;
  const float* fb = a.feats + (int64_t)b * a.T * a.F;
  const float* pe = a.pe + (int64_t)(t + 1) * D;      // positions start at 1
  float v[LFR_E];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < LFR_E; ++j) {
    const int c = j * 64 + lane;
    float x = 0.f;
    if (c < D) {
      const int f = c / a.F;
      int idx = first + f;
      idx = idx < 0 ? 0 : (idx > n_fr - 1 ? n_fr - 1 : idx);
      x = fb[(int64_t)idx * a.F + (c - f * a.F)];
      if (a.mean) x = (x - a.mean[c]) * a.istd[c];
      x = x * a.xscale + pe[c];
      sum += x;
    }
    v[j] = x;
  }
  const float mean = wave_sum(sum) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < LFR_E; ++j) {
    const float dlt = v[j] - mean;
    if (j * 64 + lane < D) q += dlt * dlt;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + a.eps);
  float* yr = a.out + (int64_t)(a.off[b] + t) * a.ldo;
#pragma unroll
  for (int j = 0; j < LFR_E; ++j) {
    const int c = j * 64 + lane;
    if (c < D) yr[c] = (v[j] - mean) * rstd * a.ln_w[c] + a.ln_b[c];
    else if (c < a.ldo) yr[c] = 0.f;
  }
}

// ===========================================================================
// LayerNorm, one wave per row, quad q = 64 j + lane of the row; D <= 2048.
constexpr int LNW_E = 8;

__global__ __launch_bounds__(256) void layernorm_wide_kernel(
    const float* x, int ldx, const float* __restrict__ w, const float* __restrict__ b, float* y,
    int ldy, int M, int D, int Dpad, float eps) {   // (y may be x: a wave reads its row first)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (int64_t)row * ldx;
  f32x4 v[LNW_E];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < LNW_E; ++j) {
    const int c = (j * 64 + lane) * 4;
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < D) v[j] = *reinterpret_cast<const f32x4*>(xr + c);
    sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  }
  const float mean = wave_sum(sum) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < LNW_E; ++j) {
    if ((j * 64 + lane) * 4 < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dlt = v[j][e] - mean;
        q += dlt * dlt;
      }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  float* yr = y + (int64_t)row * ldy;
#pragma unroll
  for (int j = 0; j < LNW_E; ++j) {
    const int c = (j * 64 + lane) * 4;
    if (c < D) {
      const f32x4 ww = *reinterpret_cast<const f32x4*>(w + c);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(b + c);
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (v[j][e] - mean) * rstd * ww[e] + bb[e];
      *reinterpret_cast<f32x4*>(yr + c) = r;
    } else if (c < Dpad) {
      *reinterpret_cast<f32x4*>(yr + c) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// ===========================================================================
// CIF.  The staged image of the conv GEMM: one thread per float4 of [M][3 d].
__global__ __launch_bounds__(256) void cif_stage3_kernel(
    const float* __restrict__ h, int ldh, float* __restrict__ img,
    const int* __restrict__ row_utt, const int* __restrict__ off, const int* __restrict__ len,
    int M, int d) {
  const int per_row = 3 * d / 4;
  const int64_t total = (int64_t)M * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / per_row);
    const int c = (int)(i - (int64_t)r * per_row) * 4;
    const int tap = c / d;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int u = row_utt[r];
    if (u >= 0) {
      const int t = r - off[u] + tap - 1;
      if (t >= 0 && t < len[u])
        v = *reinterpret_cast<const f32x4*>(h + (int64_t)(off[u] + t) * ldh + (c - tap * d));
    }
    *reinterpret_cast<f32x4*>(img + (int64_t)r * 3 * d + c) = v;
  }
}

__global__ __launch_bounds__(256) void cif_alpha_rows_kernel(
    const float* __restrict__ y, int ldy, const float* __restrict__ w,
    const float* __restrict__ b, float smooth, float noise, float* __restrict__ alpha,
    const int* __restrict__ row_utt, int M, int d) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || row_utt[row] < 0) return;
  const float* yr = y + (int64_t)row * ldy;
  float acc = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(yr + c);
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + c);
    acc += (a4[0] * w4[0] + a4[1] * w4[1]) + (a4[2] * w4[2] + a4[3] * w4[3]);
  }
  acc = wave_sum(acc) + b[0];
  if (lane == 0) alpha[row] = fmaxf(sigmoid_f(acc) * smooth - noise, 0.f);
}

// The scan.  Every thread carries the scalar chain (the same fp32 operations on the same values,
// so the same fire decisions in every lane) and CIF_MAX_D / 256 channels of the running frame.
// __fadd_rn / __fsub_rn / __fmul_rn: no contraction anywhere in the chain or into the compare.
constexpr int CIF_E = CIF_MAX_D / 256;

__global__ __launch_bounds__(256) void cif_fire_kernel(CifFireArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.len[b] > 0 ? a.len[b] : 0;
  const int o = a.off[b], eo = a.emb_off[b], cap = a.emb_cap[b];
  float fr[CIF_E], hn[CIF_E];
#pragma unroll
  for (int e = 0; e < CIF_E; ++e) { fr[e] = 0.f; hn[e] = 0.f; }
  float a_next = a.tail;
  if (T > 0) {
    a_next = a.alpha[o];
#pragma unroll
    for (int e = 0; e < CIF_E; ++e)
      if (e * 256 + tid < a.d) hn[e] = a.h[(int64_t)o * a.ldh + e * 256 + tid];
  }
  float integrate = 0.f;
  double sum = 0.0;
  int k = 0;
  for (int t = 0; t <= T; ++t) {       // exactly len + 1 steps
    const float al = a_next;
    float hv[CIF_E];
#pragma unroll
    for (int e = 0; e < CIF_E; ++e) { hv[e] = hn[e]; hn[e] = 0.f; }
    a_next = a.tail;
    if (t + 1 < T) {                   // the next frame's loads go out ahead of this frame's chain
      a_next = a.alpha[o + t + 1];
#pragma unroll
      for (int e = 0; e < CIF_E; ++e)
        if (e * 256 + tid < a.d) hn[e] = a.h[(int64_t)(o + t + 1) * a.ldh + e * 256 + tid];
    }
    sum += (double)al;
    const float completion = __fsub_rn(1.0f, integrate);
    integrate = __fadd_rn(integrate, al);
    const bool fire = integrate >= 1.0f;
    if (fire) integrate = __fsub_rn(integrate, 1.0f);
    const float cur = fire ? completion : al;
    const float remain = __fsub_rn(al, cur);
#pragma unroll
    for (int e = 0; e < CIF_E; ++e) fr[e] = __fadd_rn(fr[e], __fmul_rn(cur, hv[e]));
    if (fire) {
      if (k < cap) {
#pragma unroll
        for (int e = 0; e < CIF_E; ++e)
          if (e * 256 + tid < a.d) a.emb[(int64_t)(eo + k) * a.lde + e * 256 + tid] = fr[e];
        if (tid == 0) a.fire_t[eo + k] = t;
      }
      ++k;
#pragma unroll
      for (int e = 0; e < CIF_E; ++e) fr[e] = __fmul_rn(remain, hv[e]);
    }
  }
  const int n_tok = (int)floor(sum);
  // (the reference pads the embeddings with zero rows up to its token count, cif.py:283-292)
  for (int r = k; r < n_tok && r < cap; ++r) {
#pragma unroll
    for (int e = 0; e < CIF_E; ++e)
      if (e * 256 + tid < a.d) a.emb[(int64_t)(eo + r) * a.lde + e * 256 + tid] = 0.f;
    if (tid == 0) a.fire_t[eo + r] = -1;
  }
  if (tid == 0) {
    a.n_fire[b] = k;
    a.token_num[b] = n_tok;
  }
}

}  // namespace

int lfr_front(const LfrFrontArgs& a, hipStream_t s) {
  WN_CHECK(a.feats && a.pe && a.ln_w && a.ln_b && a.out && a.len && a.off,
           "lfr_front: null argument");
  WN_CHECK(!a.mean || a.istd, "lfr_front: CMVN needs mean and istd");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.T > 0 && a.F > 0 && a.m > 0 && a.n > 0 && a.max_rows > 0,
           "lfr_front: shape");
  WN_CHECK(a.m * a.F <= LFR_MAX_D && a.ldo >= a.m * a.F && a.ldo <= LFR_MAX_D,
           "lfr_front: m * F <= ldo <= 576");
  dim3 g(cdiv(a.max_rows, 4), a.B), t(256);
  hipLaunchKernelGGL(lfr_front_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int layernorm_wide(const float* x, int ldx, const float* w, const float* b, float* y, int ldy,
                   int M, int D, int Dpad, float eps, hipStream_t s) {
  WN_CHECK(x && w && b && y, "layernorm_wide: null argument");
  WN_CHECK(M > 0, "layernorm_wide: empty");
  WN_CHECK(D > 0 && D % 4 == 0 && Dpad % 4 == 0 && D <= Dpad && Dpad <= LNW_E * 256,
           "layernorm_wide: D <= Dpad <= 2048, multiples of 4");
  WN_CHECK(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= D && ldy >= Dpad,
           "layernorm_wide: row strides");
  hipLaunchKernelGGL(layernorm_wide_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, x, ldx, w, b, y,
                     ldy, M, D, Dpad, eps);
  WN_HIP(hipGetLastError());
  return 0;
}

int cif_stage3(const float* h, int ldh, float* img, const int* row_utt, const int* off,
               const int* len, int M, int d, hipStream_t s) {
  WN_CHECK(h && img && row_utt && off && len, "cif_stage3: null argument");
  WN_CHECK(M > 0 && d > 0 && d % 4 == 0 && ldh % 4 == 0 && ldh >= d, "cif_stage3: shape");
  const int64_t items = (int64_t)M * (3 * d / 4);
  const int blocks = (int)std::min<int64_t>(cdiv64(items, 256), 65535);
  hipLaunchKernelGGL(cif_stage3_kernel, dim3(blocks), dim3(256), 0, s, h, ldh, img, row_utt, off,
                     len, M, d);
  WN_HIP(hipGetLastError());
  return 0;
}

int cif_alpha_rows(const float* y, int ldy, const float* w, const float* b, float smooth,
                   float noise, float* alpha, const int* row_utt, int M, int d, hipStream_t s) {
  WN_CHECK(y && w && b && alpha && row_utt, "cif_alpha_rows: null argument");
  WN_CHECK(M > 0 && d > 0 && d % 4 == 0 && ldy % 4 == 0 && ldy >= d, "cif_alpha_rows: shape");
  hipLaunchKernelGGL(cif_alpha_rows_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, y, ldy, w, b,
                     smooth, noise, alpha, row_utt, M, d);
  WN_HIP(hipGetLastError());
  return 0;
}

int cif_fire(const CifFireArgs& a, hipStream_t s) {
  WN_CHECK(a.h && a.alpha && a.off && a.len && a.emb_off && a.emb_cap && a.emb && a.fire_t &&
               a.n_fire && a.token_num, "cif_fire: null argument");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.d > 0 && a.d <= CIF_MAX_D && a.ldh >= a.d &&
               a.lde >= a.d, "cif_fire: shape");
  hipLaunchKernelGGL(cif_fire_kernel, dim3(a.B), dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
