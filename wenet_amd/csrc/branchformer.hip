// Branchformer / E-Branchformer kernels (wenet/models/branchformer/cgmlp.py,
// e_branchformer/encoder_layer.py), fp32, on the packed [rows][channels] layout of the encoder:
//   csgu_gate      the middle of the convolutional gating MLP: LayerNorm over the gate half of
//                  h = GELU(channel_proj1(x)), depthwise conv over time, * the other half
//   merge_dwconv   y = c + depthwise_conv_fusion(c) over the concatenated branches
// Both run one tiled depthwise conv: a workgroup owns CSGU_TILE frames x 64 channels of ONE
// utterance, stages its CSGU_TILE + K - 1 input frames in LDS once (an input row comes from HBM
// (CSGU_TILE + K - 1) / CSGU_TILE times, not K times) and adds the taps in ascending order.
// Tiles start at the utterance's own first frame and a frame outside [0, len) is the conv's
// padding, whatever lies in the neighbouring rows of the packed buffer: a result depends on
// nothing but the utterance's own frames, in any batch, at any place in it.
#include "kernels.h"

namespace wn {

namespace {

constexpr int DWT_CH = 64;            // channels per workgroup: one per lane of a wave
constexpr int DWT_THREADS = 256;      // 4 waves, each CSGU_TILE / 4 output frames

// (mean, rstd) of the gate half of every row: one wave per row, the row in registers
__global__ __launch_bounds__(256) void csgu_stats_kernel(const float* __restrict__ g, int ldx,
                                                         int M, int C, float eps,
                                                         float2* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* p = g + (int64_t)row * ldx;
  const int n = C / 64;               // <= 16
  float v[16];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = j < n ? p[j * 64 + lane] : 0.f;
    sum += v[j];
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float d = j < n ? v[j] - mean : 0.f;
    sq += d * d;
  }
  const float var = wave_sum(sq) / (float)C;
  if (lane == 0) stats[row] = make_float2(mean, 1.0f / sqrtf(var + eps));
}

// MODE 0: csgu_gate (stats / ln_w / ln_b set: the staged value is the normalised one; r set:
// the result is multiplied by it).  MODE 1: merge_dwconv (the centre frame is added).
// grid (C / 64, tiles of the longest utterance, B); dynamic LDS: (CSGU_TILE + 2 K - 1) x 64
// floats = the input frames, then the K x 64 taps.
template <int MODE>
__global__ __launch_bounds__(DWT_THREADS) void dwconv_tile_kernel(DwTileArgs a) {
  extern __shared__ __align__(16) float dwt_lds[];
  const int b = blockIdx.z;
  const int len = a.len[b];
  const int t0 = blockIdx.y * CSGU_TILE;
  if (t0 >= len) return;
  const int row0 = a.off[b];
  const int c0 = blockIdx.x * DWT_CH;
  const int K = a.K;
  const int left = a.causal ? K - 1 : (K - 1) / 2;
  const int n_in = CSGU_TILE + K - 1;
  float* s_in = dwt_lds;                       // [n_in][64]
  float* s_w = dwt_lds + n_in * DWT_CH;        // [K][64]
  const int tid = threadIdx.x;
  // taps [K][C] -> LDS
  for (int i = tid; i < K * (DWT_CH / 4); i += DWT_THREADS) {
    const int k = i / (DWT_CH / 4), q = i % (DWT_CH / 4);
    *reinterpret_cast<float4*>(s_w + k * DWT_CH + q * 4) =
        *reinterpret_cast<const float4*>(a.wt + (int64_t)k * a.C + c0 + q * 4);
  }
  // input frames t0 - left .. t0 - left + n_in - 1 of THIS utterance; outside [0, len): padding
  for (int i = tid; i < n_in * (DWT_CH / 4); i += DWT_THREADS) {
    const int j = i / (DWT_CH / 4), q = i % (DWT_CH / 4);
    const int t = t0 - left + j;
    const int c = c0 + q * 4;
    float4 v;
    if (t >= 0 && t < len) {
      const int64_t row = row0 + t;
      v = *reinterpret_cast<const float4*>(a.x + row * a.ldx + c);
      if (MODE == 0) {
        const float2 st = a.stats[row];
        const float4 w = *reinterpret_cast<const float4*>(a.ln_w + c);
        const float4 bb = *reinterpret_cast<const float4*>(a.ln_b + c);
        v.x = (v.x - st.x) * st.y * w.x + bb.x;
        v.y = (v.y - st.x) * st.y * w.y + bb.y;
        v.z = (v.z - st.x) * st.y * w.z + bb.z;
        v.w = (v.w - st.x) * st.y * w.w + bb.w;
      }
    } else if (MODE == 0 && a.causal) {
      // the reference pads in FRONT of the LayerNorm: a zero frame leaves it as its bias
      v = *reinterpret_cast<const float4*>(a.ln_b + c);
    } else {
      v = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    *reinterpret_cast<float4*>(s_in + j * DWT_CH + q * 4) = v;
  }
  __syncthreads();
  constexpr int PER = CSGU_TILE / (DWT_THREADS / 64);   // output frames per wave
  const int lane = tid & 63;
  const int o0 = (tid >> 6) * PER;
  float acc[PER];
#pragma unroll
  for (int o = 0; o < PER; ++o) acc[o] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float w = s_w[k * DWT_CH + lane];
#pragma unroll
    for (int o = 0; o < PER; ++o) acc[o] = fmaf(w, s_in[(o0 + o + k) * DWT_CH + lane], acc[o]);
  }
  const int c = c0 + lane;
  const float bias = a.bias[c];
#pragma unroll
  for (int o = 0; o < PER; ++o) {
    const int t = t0 + o0 + o;
    if (t >= len) break;
    const int64_t row = row0 + t;
    float y = acc[o] + bias;
    if (MODE == 0) {
      if (a.r) y *= a.r[row * a.ldr + c];
    } else {
      y += s_in[(o0 + o + left) * DWT_CH + lane];
      // optional residual behind the merge (the Paraformer's FSMN blocks); null for the
      // E-Branchformer callers, whose sum stays as it was
      if (a.r) y += a.r[row * a.ldr + c];
    }
    a.y[row * a.ldy + c] = y;
  }
}

__global__ __launch_bounds__(256) void csgu_mul_kernel(const float* __restrict__ r, int ldr,
                                                       const float* __restrict__ g, int ldg,
                                                       float* __restrict__ y, int ldy, int M,
                                                       int C4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)M * C4) return;
  const int64_t row = i / C4;
  const int c = (int)(i % C4) * 4;
  const float4 rv = *reinterpret_cast<const float4*>(r + row * ldr + c);
  const float4 gv = *reinterpret_cast<const float4*>(g + row * ldg + c);
  *reinterpret_cast<float4*>(y + row * ldy + c) =
      make_float4(rv.x * gv.x, rv.y * gv.y, rv.z * gv.z, rv.w * gv.w);
}

int dwt_check(const DwTileArgs& a, const char* who) {
  const std::string w(who);
  WN_CHECK(a.x && a.wt && a.bias && a.y && a.off && a.len, w + ": null argument");
  WN_CHECK(a.C >= 64 && a.C % 64 == 0, w + ": channels must be a multiple of 64");
  WN_CHECK(a.K >= 1 && a.K <= CSGU_MAX_K && (a.causal || a.K % 2 == 1),
           w + ": 1 <= K <= 63, odd unless causal");
  WN_CHECK(a.ldx % 4 == 0 && a.ldx >= a.C && a.ldy >= a.C, w + ": row strides");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.max_len > 0, w + ": empty batch");
  WN_CHECK(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.wt & 15) == 0,
           w + ": x and the taps must be 16-byte aligned");
  return 0;
}

template <int MODE>
int dwt_launch(const DwTileArgs& a, hipStream_t s) {
  const size_t lds = (size_t)(CSGU_TILE + 2 * a.K - 1) * DWT_CH * sizeof(float);   // <= 40 KB
  const dim3 grid(a.C / DWT_CH, cdiv(a.max_len, CSGU_TILE), a.B);
  hipLaunchKernelGGL((dwconv_tile_kernel<MODE>), grid, dim3(DWT_THREADS), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int csgu_gate(const DwTileArgs& a, hipStream_t s) {
  WN_TRY(dwt_check(a, "csgu_gate"));
  WN_CHECK(a.C <= CSGU_MAX_C, "csgu_gate: at most 1024 gate channels");
  WN_CHECK(a.ln_w && a.ln_b && a.stats && a.M > 0, "csgu_gate: null argument");
  WN_CHECK(!a.r || a.ldr >= a.C, "csgu_gate: row stride of r");
  WN_CHECK(((uintptr_t)a.ln_w & 15) == 0 && ((uintptr_t)a.ln_b & 15) == 0,
           "csgu_gate: the norm's weight and bias must be 16-byte aligned");
  hipLaunchKernelGGL(csgu_stats_kernel, dim3(cdiv(a.M, 4)), dim3(256), 0, s, a.x, a.ldx, a.M,
                     a.C, a.eps, a.stats);
  WN_HIP(hipGetLastError());
  return dwt_launch<0>(a, s);
}

int merge_dwconv(const DwTileArgs& a, hipStream_t s) {
  WN_TRY(dwt_check(a, "merge_dwconv"));
  WN_CHECK(a.y != a.x, "merge_dwconv: not in place (a tile reads its neighbours' frames)");
  WN_CHECK(!a.r || a.ldr >= a.C, "merge_dwconv: row stride of r");
  return dwt_launch<1>(a, s);
}

int csgu_mul(const float* r, int ldr, const float* g, int ldg, float* y, int ldy, int M, int C,
             hipStream_t s) {
  WN_CHECK(r && g && y && M > 0 && C > 0 && C % 4 == 0 && ldr % 4 == 0 && ldg % 4 == 0 &&
               ldy % 4 == 0,
           "csgu_mul: shapes");
  hipLaunchKernelGGL(csgu_mul_kernel, dim3((unsigned)cdiv64((int64_t)M * (C / 4), 256)),
                     dim3(256), 0, s, r, ldr, g, ldg, y, ldy, M, C / 4);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
