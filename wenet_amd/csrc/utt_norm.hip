// Utterance-normalised fbank, the features of the W2v-BERT 2.0 family (compute_w2vbert_fbank,
// dataset/processor.py:259-272):
//     std, mean = torch.std_mean(mat, dim=0);  mat = mat.subtract(mean).divide(std)
// per utterance and per mel bin over ALL len[b] frames of the utterance, std unbiased (M2 / (n - 1)).
// Input is the padded (B, T, F) tensor wn_fbank leaves in HBM, F <= 128.  An utterance of 30 s is
// 3000 x 80 floats = 960 KB: it does not fit a CU's LDS, so the statistics are a pass of their own
// and the division is done by whoever reads the features next -- utt_normalize (a second padded
// tensor, or in place) or stack_frames_ln_utt (the front end of the shaw encoders, which then
// never sees a normalised tensor in HBM).
//
// utt_stats_kernel, grid (n_slab, B), 4 waves.  A block owns UTT_SLAB = 128 frames of ONE
// utterance, wave w the 32 frames slab * 128 + 32 w ..; a lane owns the bins lane and lane + 64, so
// a frame is one coalesced row read of F floats (two loads per lane, the second live on F - 64
// lanes).  Frames are taken four at a time -- eight independent loads in flight per lane -- and fed
// one by one to Welford's update.  Per bin a lane keeps THREE numbers next to the (wave-uniform)
// count: p, the running mean of the raw values, p += (x - p) / n; and Welford's (m, M2) of the
// values LESS k, the utterance's own first frame of that bin: v = x - k, d = v - m, m += d / n,
// M2 += d * (v - m).  Why both: the running mean of a bin of mean 1e3 moves on a grid of 6e-5, and
// an M2 accumulated against it is off by 1e-5 of a std of 1 -- two hundred times the error of the
// plain fp32 formula; against v the mean is of the std's size and M2 keeps its digits.  The mean
// itself is NOT taken as k + m: for a bin of mean 0 that sum cancels and carries the rounding of
// values of size |k|; p has no such term.  No sum of raw squares is ever formed.  1 / n is one
// reciprocal per frame shared by the lane's two bins.  The four waves' triples go through LDS and
// threads 0 .. F - 1 merge them per bin by Chan's pairwise formula in WAVE ORDER 0, 1, 2, 3 (M2
// with the difference of the shifted means); the counts are not stored, they follow from len[b]
// and the frame index.  The block writes its slab's triple to ws[b][slab][0 | 1 | 2][f].  Slabs
// start at multiples of 128 counted from the utterance's own first frame and k is the utterance's
// own frame 0, so the partition -- and with it every rounding -- depends on the utterance alone, not
// on T, B or its place in the batch.  Blocks past the utterance's end return at once.
//
// utt_stats_finish_kernel, grid B, 128 threads, thread = bin: merges the cdiv(len, 128) slab
// triples in SLAB ORDER with the same formula and writes mean[b][f] = p, std[b][f] = sqrt(M2 / (n -
// 1)).  No atomics, no arrival counter: the order is fixed, an utterance gives the same bits alone,
// batched and at any place of the batch.  len[b] < 2 writes nothing (and yields no encoder row).
//
// utt_normalize_kernel, grid (cdiv(T F / 4, 256), B): a float4 of one frame per thread (F % 4 == 0),
// (x - mean) / std with IEEE division -- a constant bin gives 0 / 0 = NaN as the reference does;
// frames at or behind len[b] are written as zeros without a read.  stack_frames_ln_utt_kernel is
// stack_frames_ln_kernel (attention_shaw.hip) with the utterance's statistics rows in front of the
// optional CMVN: one wave per output row, up to four values per lane, two-pass LayerNorm in
// registers; the sibling leaves the CMVN-only kernel and its bits alone.
//
// LDS: utt_stats_kernel only, 4 waves x 3 x 128 floats = 6 KB static.  Banks (64 of 4 bytes): the
// partial stores are ds_write_b32 at w * 384 + c * 128 + lane (+ 64), 64 consecutive dwords per
// instruction; the merge reads dword w * 384 + c * 128 + tid, consecutive across a wave: no
// conflicts in either.  The compiler reports for gfx950: utt_stats_kernel 64 VGPRs, finish 27,
// normalize 30, stack_frames_ln_utt 19; no scratch in any; occupancy 8 waves per SIMD, the limit
// of the CU, for all four.  Untuned: the slab size and the unroll of four were chosen by
// reasoning (128 frames x 80 bins = 40 KB per block, 24 blocks for 30 s), not by measurement.
#include "kernels.h"

namespace wn {

namespace {

constexpr int WAVE_FRAMES = UTT_SLAB / 4;      // 32 frames per wave

// a partial of one bin: the mean of the raw values, and Welford's (mean, M2) of the values less k
struct Part { float p, m, S; };

// Chan et al.: a <- a + b with counts na, nb > 0
__device__ __forceinline__ void chan_merge(float& na, Part& a, float nb, const Part& b) {
  const float n = na + nb, r = nb / n, d = b.m - a.m;
  a.p += (b.p - a.p) * r;
  a.m += d * r;
  a.S += b.S + d * d * (na * nb / n);
  na = n;
}

__device__ __forceinline__ void welford(float x, float k, float rn, Part& a) {
  a.p += (x - a.p) * rn;
  const float v = x - k, d = v - a.m;
  a.m += d * rn;
  a.S += d * (v - a.m);
}

__global__ __launch_bounds__(256) void utt_stats_kernel(UttStatsArgs a) {
  __shared__ float part[4][3][128];     // [wave][mean | shifted mean | M2][bin]
  const int u = blockIdx.y, slab = blockIdx.x;
  const int len = a.len[u], t_slab = slab * UTT_SLAB;
  if (t_slab >= len) return;            // block-uniform
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t0 = t_slab + w * WAVE_FRAMES;
  const int nw = min(max(len - t0, 0), WAVE_FRAMES);       // frames of this wave, all < len <= T
  const int F = a.F;
  const float* x0 = a.feats + (int64_t)u * a.T * F;        // frame 0 exists: len > t_slab >= 0
  const float* x = x0 + (int64_t)t0 * F;
  const bool h0 = lane < F, h1 = lane + 64 < F;
  const float k0 = h0 ? x0[lane] : 0.f, k1 = h1 ? x0[lane + 64] : 0.f;
  Part a0 = {0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f};
  int t = 0;
  for (; t + 4 <= nw; t += 4) {
    float v0[4], v1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* r = x + (int64_t)(t + j) * F;
      v0[j] = h0 ? r[lane] : 0.f;
      v1[j] = h1 ? r[lane + 64] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float rn = 1.0f / (float)(t + j + 1);
      welford(v0[j], k0, rn, a0);
      welford(v1[j], k1, rn, a1);
    }
  }
  for (; t < nw; ++t) {
    const float* r = x + (int64_t)t * F;
    const float rn = 1.0f / (float)(t + 1);
    welford(h0 ? r[lane] : 0.f, k0, rn, a0);
    welford(h1 ? r[lane + 64] : 0.f, k1, rn, a1);
  }
  part[w][0][lane] = a0.p; part[w][0][lane + 64] = a1.p;
  part[w][1][lane] = a0.m; part[w][1][lane + 64] = a1.m;
  part[w][2][lane] = a0.S; part[w][2][lane + 64] = a1.S;
  __syncthreads();
  const int f = threadIdx.x;
  if (f >= F) return;
  // wave 0 of a live block has at least one frame
  float n = (float)min(len - t_slab, WAVE_FRAMES);
  Part acc = {part[0][0][f], part[0][1][f], part[0][2][f]};
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const int nk = min(max(len - t_slab - k * WAVE_FRAMES, 0), WAVE_FRAMES);
    if (nk > 0) chan_merge(n, acc, (float)nk, Part{part[k][0][f], part[k][1][f], part[k][2][f]});
  }
  float* o = a.ws + ((int64_t)u * a.n_slab + slab) * 3 * F;
  o[f] = acc.p;
  o[F + f] = acc.m;
  o[2 * F + f] = acc.S;
}

__global__ __launch_bounds__(128) void utt_stats_finish_kernel(UttStatsArgs a) {
  const int u = blockIdx.x, f = threadIdx.x;
  const int len = a.len[u], F = a.F;
  if (f >= F || len < 2) return;
  const float* p = a.ws + (int64_t)u * a.n_slab * 3 * F;
  float n = (float)min(len, UTT_SLAB);
  Part acc = {p[f], p[F + f], p[2 * F + f]};
  for (int sl = 1; sl * UTT_SLAB < len; ++sl) {
    const float* q = p + (int64_t)sl * 3 * F;
    chan_merge(n, acc, (float)min(len - sl * UTT_SLAB, UTT_SLAB),
               Part{q[f], q[F + f], q[2 * F + f]});
  }
  a.mean[(int64_t)u * F + f] = acc.p;
  a.std[(int64_t)u * F + f] = sqrtf(acc.S / (n - 1.0f));
}

__global__ __launch_bounds__(256) void utt_normalize_kernel(const float* feats, const int* len,
                                                            const float* mean, const float* std,
                                                            float* out, int T, int F) {
  const int u = blockIdx.y;
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;       // T F < 2^31 (checked)
  if (e >= T * F) return;
  const int t = e / F, f = e - t * F, n = len[u];
  const int64_t at = (int64_t)u * T * F + e;
  float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < n) {
    if (n < 2) {
      y.x = y.y = y.z = y.w = __builtin_nanf("");
    } else {
      const float4 x = *reinterpret_cast<const float4*>(feats + at);
      const float4 m = *reinterpret_cast<const float4*>(mean + (int64_t)u * F + f);
      const float4 s = *reinterpret_cast<const float4*>(std + (int64_t)u * F + f);
      y.x = (x.x - m.x) / s.x; y.y = (x.y - m.y) / s.y;
      y.z = (x.z - m.z) / s.z; y.w = (x.w - m.w) / s.w;
    }
  }
  *reinterpret_cast<float4*>(out + at) = y;
}

// stack_frames_ln_kernel with (x - umean[u][f]) / ustd[u][f] in front of the optional CMVN
__global__ __launch_bounds__(256) void stack_frames_ln_utt_kernel(StackFramesUttArgs b) {
  const StackFramesArgs& a = b.k;
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.len[u]) return;
  const int n = 2 * a.F;
  const float* x = a.feats + ((int64_t)u * a.T + 2 * t) * a.F;
  const float* um = b.umean + (int64_t)u * a.F;
  const float* us = b.ustd + (int64_t)u * a.F;
  float v[4];
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = lane + 64 * e;
    v[e] = 0.f;
    if (i < n) {
      const int f = i < a.F ? i : i - a.F;
      v[e] = (x[i] - um[f]) / us[f];
      if (a.mean) v[e] = (v[e] - a.mean[f]) * a.istd[f];
    }
    sum += v[e];
  }
#pragma unroll
  for (int x2 = 32; x2 > 0; x2 >>= 1) sum += __shfl_xor(sum, x2, 64);
  const float mu = sum / (float)n;
  float var = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dlt = lane + 64 * e < n ? v[e] - mu : 0.f;
    var += dlt * dlt;
  }
#pragma unroll
  for (int x2 = 32; x2 > 0; x2 >>= 1) var += __shfl_xor(var, x2, 64);
  const float rstd = rsqrtf(var / (float)n + a.eps);
  float* y = a.out + (int64_t)(a.off[u] + t) * a.ldo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = lane + 64 * e;
    if (i < n) y[i] = (v[e] - mu) * rstd * a.ln_w[i] + a.ln_b[i];
  }
}

}  // namespace

int utt_stats(const UttStatsArgs& a, hipStream_t s) {
  WN_CHECK(a.feats && a.len && a.ws && a.mean && a.std, "utt_stats: null argument");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.T > 0 && a.F >= 1, "utt_stats: B / T / F");
  WN_CHECK(a.F <= 128, "utt_stats: F > 128 (two bins per lane)");
  WN_CHECK(a.n_slab >= 0 && (int64_t)a.n_slab * UTT_SLAB < (int64_t)a.T + UTT_SLAB,
           "utt_stats: more slabs than T frames hold");
  if (a.n_slab == 0) return 0;
  hipLaunchKernelGGL(utt_stats_kernel, dim3(a.n_slab, a.B), dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  hipLaunchKernelGGL(utt_stats_finish_kernel, dim3(a.B), dim3(128), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int utt_normalize(const float* feats, const int* len, const float* mean, const float* std,
                  float* out, int B, int T, int F, hipStream_t s) {
  WN_CHECK(feats && len && mean && std && out, "utt_normalize: null argument");
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F >= 1, "utt_normalize: B / T / F");
  WN_CHECK(F <= 128, "utt_normalize: F > 128");
  WN_CHECK(F % 4 == 0, "utt_normalize: F % 4 != 0 (a float4 of one frame per thread)");
  WN_CHECK((int64_t)T * F < (1ll << 31), "utt_normalize: T * F must stay below 2^31");
  WN_CHECK((((uintptr_t)feats | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)out) & 15) == 0,
           "utt_normalize: feats, mean, std and out must be 16-byte aligned");
  hipLaunchKernelGGL(utt_normalize_kernel, dim3(cdiv(T * F / 4, 256), B), dim3(256), 0, s, feats,
                     len, mean, std, out, T, F);
  WN_HIP(hipGetLastError());
  return 0;
}

int stack_frames_ln_utt(const StackFramesUttArgs& b, hipStream_t s) {
  const StackFramesArgs& a = b.k;
  WN_CHECK(a.feats && a.ln_w && a.ln_b && a.out && a.off && a.len && b.umean && b.ustd,
           "stack_frames_ln_utt: null argument");
  WN_CHECK((a.mean == nullptr) == (a.istd == nullptr),
           "stack_frames_ln_utt: mean and istd come together");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.T > 0 && a.F >= 1, "stack_frames_ln_utt: B / T / F");
  WN_CHECK(a.F <= 128, "stack_frames_ln_utt: F > 128 (2 F values per row)");
  WN_CHECK(a.ldo >= 2 * a.F, "stack_frames_ln_utt: output stride");
  if (a.max_len <= 0) return 0;
  WN_CHECK(2 * a.max_len <= a.T,
           "stack_frames_ln_utt: a row would read past its utterance's frames");
  hipLaunchKernelGGL(stack_frames_ln_utt_kernel, dim3(cdiv(a.max_len, 4), a.B), dim3(256), 0, s,
                     b);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
