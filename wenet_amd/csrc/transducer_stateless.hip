// The stateless predictors of a hybrid transducer (EmbeddingPredictor and ConvPredictor,
// wenet/models/transducer/predictor.py:209-495) as one kernel per predictor advance, fp32 only.
//
// A stateless predictor's output is a function of the last C = history_size + 1 tokens of a
// hypothesis, so a whole advance -- the C embedding rows, the position-weighted mix (or the
// depthwise conv), ffn, LayerNorm, the activation and joint.pred_ffn -- is one launch that writes
// the row of pred_proj; nothing recurrent is kept, gathered or scattered.
//  * rnnt_stateless_kernel<KC>   SL_ROWS (4) consecutive rows per workgroup of 16 waves.  The rows
//    whose `advance` flag is set stage their window in LDS; the two linears then run one wave per
//    output column, which keeps its weight row in registers (KC 64-lane chunks) and walks the
//    group's rows, four columns at a time so that their loads are in flight together: ffn.weight
//    and joint.pred_ffn.weight are read once per group, not per row.
//    Every output element is one reduction in one order (a lane's fmaf chain over ascending k,
//    then the wave butterfly), whatever the group holds: a row's bits depend neither on M nor on
//    its place in the group nor on the other rows.  A row that does not advance is not written.
// The window is an explicit (M, C) id array, or the tail of a token row the search keeps anyway
// (tokens / tok_len), preceded by the blank and then by -1 (the zero vector: the reference's
// zero-initialised history before the leading blank).
#include "kernels.h"

namespace wn {
namespace {

constexpr int SL_ROWS = 4;         // rows of one workgroup
constexpr int SL_COLS = 4;         // output columns a wave has in flight
constexpr int SL_THREADS = 1024;   // 16 waves
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_CMAX = 16;        // context and heads at most

// y[r][n] = W[n] . x[r] + b[n] for the group's live rows; x rows in LDS (pitch E).  A wave takes
// SL_COLS columns at a time so that their weight loads are in flight together; every column is
// summed as if it were alone.
template <int KC, bool TO_GLOBAL>
__device__ __forceinline__ void sl_linear(const float* __restrict__ W, const float* __restrict__ b,
                                          int N, int E, const float* x, float* y, int64_t ldy,
                                          const int* live, int n_live, int lane, int wave) {
  for (int n0 = wave; n0 < N; n0 += SL_WAVES * SL_COLS) {
    float w[SL_COLS][KC];
    float bias[SL_COLS];
#pragma unroll
    for (int j = 0; j < SL_COLS; ++j) {
      const int n = n0 + j * SL_WAVES;
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        const int k = i * 64 + lane;
        w[j][i] = (n < N && k < E) ? W[(int64_t)n * E + k] : 0.0f;
      }
      bias[j] = (b && n < N) ? b[n] : 0.0f;
    }
    for (int a = 0; a < n_live; ++a) {
      const int r = live[a];
      const float* xr = x + r * E;
      float s[SL_COLS];
#pragma unroll
      for (int j = 0; j < SL_COLS; ++j) s[j] = 0.0f;
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        const int k = i * 64 + lane;
        if (k < E) {
          const float xv = xr[k];
#pragma unroll
          for (int j = 0; j < SL_COLS; ++j) s[j] = fmaf(w[j][i], xv, s[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < SL_COLS; ++j) s[j] = wave_sum(s[j]);
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SL_COLS; ++j) {
          const int n = n0 + j * SL_WAVES;
          if (n >= N) continue;
          if constexpr (TO_GLOBAL) y[(int64_t)r * ldy + n] = s[j] + bias[j];
          else y[r * E + n] = s[j] + bias[j];
        }
      }
    }
  }
}

template <int KC>
__global__ __launch_bounds__(SL_THREADS) void rnnt_stateless_kernel(RnntStatelessArgs p) {
  if (p.n_active && *p.n_active == 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_ids[SL_ROWS][SL_CMAX];
  __shared__ float s_w[SL_ROWS][SL_CMAX][SL_CMAX];     // [row][head][c]
  __shared__ float s_ws[SL_ROWS][SL_CMAX];
  __shared__ int s_live[SL_ROWS];
  __shared__ int s_nlive;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = p.E, C = p.C;
  float* bufA = reinterpret_cast<float*>(smem);          // [SL_ROWS][E]
  float* bufB = bufA + SL_ROWS * E;                      // [SL_ROWS][E]
  const int m0 = blockIdx.x * SL_ROWS;

  // ---- the live rows of this group and their windows -------------------------------------------
  if (tid == 0) {
    int n = 0;
    for (int r = 0; r < SL_ROWS; ++r) {
      const int m = m0 + r;
      if (m < p.M && (!p.advance || p.advance[m] != 0)) s_live[n++] = r;
    }
    s_nlive = n;
  }
  if (tid < SL_ROWS * SL_CMAX) {
    const int r = tid / SL_CMAX, c = tid % SL_CMAX, m = m0 + r;
    int id = -1;
    if (m < p.M && c < C) {
      if (p.ctx) {
        id = p.ctx[(int64_t)m * C + c];
      } else {
        const int tr = p.tok_row ? p.tok_row[m] : m;
        const int pos = max(p.tok_len[tr], 0) - C + c;
        if (pos >= 0) { if (pos < p.ld_tok) id = p.tokens[(int64_t)tr * p.ld_tok + pos]; }
        else if (pos == -1) id = p.blank;
      }
      if (id < 0 || id >= p.V) id = -1;
    }
    s_ids[r][c] = id;
  }
  __syncthreads();
  const int n_live = s_nlive;
  if (n_live == 0) return;

  // ---- the mix of the window into bufA ---------------------------------------------------------
  if (p.kind == 1) {
    // w[h][c] = sum_e x[c][e] pos[h][e][c]: one wave per (row, head, c)
    const int per_row = p.heads * C;
    for (int it = wave; it < n_live * per_row; it += SL_WAVES) {
      const int r = s_live[it / per_row], hc = it % per_row, h = hc / C, c = hc % C;
      const int id = s_ids[r][c];
      float s = 0.0f;
      if (id >= 0) {
        const float* x = p.embed + (int64_t)id * E;
        const float* q = p.pos + (int64_t)h * E * C + c;
        for (int e = lane; e < E; e += 64) s = fmaf(x[e], q[(int64_t)e * C], s);
      }
      s = wave_sum(s);
      if (lane == 0) s_w[r][h][c] = s;
    }
    __syncthreads();
    if (tid < SL_ROWS * SL_CMAX) {
      const int r = tid / SL_CMAX, c = tid % SL_CMAX;
      float s = 0.0f;
      if (c < C)
        for (int h = 0; h < p.heads; ++h) s += s_w[r][h][c];
      s_ws[r][c] = s;
    }
    __syncthreads();
    const float div = (float)(p.heads * C);
    for (int it = tid; it < n_live * E; it += SL_THREADS) {
      const int r = s_live[it / E], e = it % E;
      float s = 0.0f;
      for (int c = 0; c < C; ++c) {
        const int id = s_ids[r][c];
        if (id >= 0) s = fmaf(s_ws[r][c], p.embed[(int64_t)id * E + e], s);
      }
      bufA[r * E + e] = s / div;
    }
    __syncthreads();
    sl_linear<KC, false>(p.ffn_w, p.ffn_b, E, E, bufA, bufB, 0, s_live, n_live, lane, wave);
  } else {
    for (int it = tid; it < n_live * E; it += SL_THREADS) {
      const int r = s_live[it / E], e = it % E;
      float s = 0.0f;
      for (int c = 0; c < C; ++c) {
        const int id = s_ids[r][c];
        if (id >= 0) s = fmaf(p.embed[(int64_t)id * E + e], p.conv_w[(int64_t)e * C + c], s);
      }
      if (p.conv_b) s += p.conv_b[e];
      bufB[r * E + e] = s;
    }
  }
  __syncthreads();

  // ---- LayerNorm + activation, bufB -> bufA: one wave per row, two passes -----------------------
  for (int a = wave; a < n_live; a += SL_WAVES) {
    const int r = s_live[a];
    const float* x = bufB + r * E;
    float s = 0.0f;
    for (int e = lane; e < E; e += 64) s += x[e];
    const float mean = wave_sum(s) / (float)E;
    float q = 0.0f;
    for (int e = lane; e < E; e += 64) { const float d = x[e] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + p.eps);
    for (int e = lane; e < E; e += 64) {
      const float v = (x[e] - mean) * rstd * p.norm_w[e] + p.norm_b[e];
      bufA[r * E + e] = p.act == 0 ? v * sigmoid_f(v) : fmaxf(v, 0.0f);
    }
  }
  __syncthreads();

  // ---- joint.pred_ffn into the rows of pred_proj -----------------------------------------------
  sl_linear<KC, true>(p.pj_w, p.pj_b, p.J, E, bufA, p.out + (int64_t)m0 * p.ldo, p.ldo, s_live,
                      n_live, lane, wave);
}

template <int KC>
int sl_launch(const RnntStatelessArgs& a, hipStream_t s) {
  const size_t lds = (size_t)2 * SL_ROWS * a.E * sizeof(float);
  WN_MAX_DYN_LDS(rnnt_stateless_kernel<KC>, lds);
  hipLaunchKernelGGL(rnnt_stateless_kernel<KC>, dim3(cdiv(a.M, SL_ROWS)), dim3(SL_THREADS), lds, s,
                     a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int rnnt_stateless_step(const RnntStatelessArgs& a, hipStream_t s) {
  WN_CHECK(a.kind == 1 || a.kind == 2, "rnnt_stateless_step: kind must be 1 (embedding) or 2 (conv)");
  WN_CHECK(a.embed && a.norm_w && a.norm_b && a.pj_w && a.out && a.M >= 1 && a.V >= 1,
           "rnnt_stateless_step: null / empty operand");
  WN_CHECK(a.kind == 1 ? (a.pos && a.ffn_w) : a.conv_w != nullptr,
           "rnnt_stateless_step: null predictor weight");
  WN_CHECK(a.ctx || (a.tokens && a.tok_len && a.ld_tok >= 1),
           "rnnt_stateless_step: neither context ids nor token rows");
  WN_CHECK(a.E >= 1 && a.E <= 1024 && a.J >= 1 && a.J <= 1024 && a.ldo >= a.J,
           "rnnt_stateless_step: widths must be in [1, 1024]");
  WN_CHECK(a.C >= 1 && a.C <= SL_CMAX && a.heads >= 1 && a.heads <= SL_CMAX,
           "rnnt_stateless_step: context and heads must be in [1, 16]");
  WN_CHECK(a.act == 0 || a.act == 1, "rnnt_stateless_step: activation 0 (swish) or 1 (relu)");
  // (the chunk count only bounds the registers: a lane sums its chunks in ascending order in
  // every instantiation)
  if (a.E <= 128) return sl_launch<2>(a, s);
  if (a.E <= 384) return sl_launch<6>(a, s);
  return sl_launch<16>(a, s);
}

}  // namespace wn
