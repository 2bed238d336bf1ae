// RNN-T greedy search with frame lookahead (wenet/models/transducer/search/greedy_search.py:6-54
// for a whole batch in lock-step), fp32 only.
//
// The joint output depends on the predictor only through pred_out, and pred_out changes only
// when a non-blank symbol is emitted.  A step therefore evaluates the joint for the next F
// frames of every utterance under its current predictor output (one GEMM with M = B x F rows),
// takes the arg-max of each and lets the advance kernel consume the window up to and including
// its first non-blank frame.  Kernels:
//  * rnnt_linear_kernel   y[b] = W1 x1[b] + b1 (+ W2 x2[b] + b2) for the rows whose `advance`
//    flag is set: the LSTM gate sums, the predictor's projection and joint.pred_ffn (M = B
//    rows).  One wave per output column keeps its weight rows in registers and walks the
//    rows; every row is summed in the same order whatever the batch holds;
//  * rnnt_cell_kernel     the LSTM cell (gate order i, f, g, o as torch.nn.LSTM), in place on
//    the advancing rows; the others keep h and c bit for bit;
//  * rnnt_joint_kernel    tanh(enc_proj[row] + pred_proj[b]) built on its way into LDS, times
//    ffn_out.weight^T on v_mfma_f32_32x32x2_f32, 32 rows x 128 columns per block; the epilogue
//    keeps a (max, index) per row and column block -- the (M, V) logits are never written (the
//    beam search's instantiation, rnnt_joint_rows, writes them instead: transducer_beam.hip).
//    Every row is summed in one fixed order in every block (four interleaved fmaf chains over
//    ascending k -- the f32 MFMA is an fmaf chain per output element -- added in a fixed order;
//    no K split across blocks), so a row's logits depend neither on M nor on the row's place in
//    the window nor on the other utterances;
//  * rnnt_advance_kernel  one wave per utterance reduces the column-block partials (lowest
//    index on ties and the first NaN before any number, as torch.argmax; rnnt_reduce_row, which
//    rnnt_reduce_kernel runs on its own for the operator hook), scans the window in frame order, applies the emission
//    rule, appends tokens and writes the next step's row map, `advance`, `done`, `n_active`.
// Plain stream-ordered launches; every kernel of a finished batch returns on n_active == 0.
#include "rnnt_argmax.h"
#include "rnnt_joint_tile.h"

namespace wn {
namespace {

constexpr int RL_KC = 16;          // 64-lane chunks of a weight row kept in registers: K <= 1024

__global__ __launch_bounds__(256) void rnnt_linear_kernel(RnntLinearArgs p) {
  if (p.n_active && *p.n_active == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= p.N) return;
  float w1[RL_KC], w2[RL_KC];
#pragma unroll
  for (int i = 0; i < RL_KC; ++i) {
    const int k = i * 64 + lane;
    w1[i] = k < p.K1 ? p.W1[(int64_t)n * p.K1 + k] : 0.0f;
    w2[i] = (p.W2 && k < p.K2) ? p.W2[(int64_t)n * p.K2 + k] : 0.0f;
  }
  float bias = p.b1 ? p.b1[n] : 0.0f;
  if (p.b2) bias += p.b2[n];
  for (int b = 0; b < p.B; ++b) {
    if (p.advance && p.advance[b] == 0) continue;
    const int r1 = p.x1_rows ? p.x1_rows[b] : b;
    const float* x1 = p.x1 + (int64_t)r1 * p.ldx1;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < RL_KC; ++i) {
      const int k = i * 64 + lane;
      if (k < p.K1) s1 = fmaf(w1[i], x1[k], s1);
    }
    if (p.W2) {
      const float* x2 = p.x2 + (int64_t)b * p.ldx2;
#pragma unroll
      for (int i = 0; i < RL_KC; ++i) {
        const int k = i * 64 + lane;
        if (k < p.K2) s2 = fmaf(w2[i], x2[k], s2);
      }
    }
    s1 = wave_sum(s1);
    if (p.W2) s1 += wave_sum(s2);
    if (lane == 0) p.y[(int64_t)b * p.ldy + n] = s1 + bias;
  }
}

// gates [B][4H] (i | f | g | o) -> c, h in place on the advancing rows
__global__ __launch_bounds__(256) void rnnt_cell_kernel(const float* __restrict__ gates, float* h,
                                                        float* c, const int* __restrict__ advance,
                                                        int B, int H,
                                                        const int* __restrict__ n_active) {
  if (n_active && *n_active == 0) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * H) return;
  const int b = idx / H, j = idx - b * H;
  if (advance && advance[b] == 0) return;
  const float* g = gates + (int64_t)b * 4 * H;
  const float gi = sigmoid_f(g[j]), gf = sigmoid_f(g[H + j]);
  const float gg = tanhf(g[2 * H + j]), go = sigmoid_f(g[3 * H + j]);
  const float cn = gf * c[idx] + gi * gg;
  c[idx] = cn;
  h[idx] = go * tanhf(cn);
}

// argmax_merge, rnnt_reduce_row: rnnt_argmax.h

// FULL: the epilogue keeps the logits of every live row (p.logits, pitch p.ldl) instead of a
// (max, index) per column block -- the beam search's instantiation.  The GEMM body is the one
// text for both, so a row's logits are the same bits in either.
template <bool FULL>
__global__ __launch_bounds__(256) void rnnt_joint_kernel(RnntJointArgs p) {
  if (p.n_active && *p.n_active == 0) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red_v[4][JT_ROWS];
  __shared__ int red_i[4][JT_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * JT_ROWS;
  // A rows of this block and this wave's 32 x 32 logits without the bias (rnnt_joint_tile.h)
  rnnt_joint_stage_a(smem, p.enc_proj, p.lde, p.pred_proj, p.ldp, p.row_enc, p.row_pred, p.M, p.J,
                     m0, tid);
  __syncthreads();
  const int n0 = blockIdx.x * JT_COLS + wave * 32;
  const f32x16 acc = rnnt_joint_tile_sums(smem, p.W, p.J, p.V, n0, lane);

  // C / D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int col = n0 + (lane & 31);
  const float bias = col < p.V ? p.bias[col] : 0.0f;
  if constexpr (FULL) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < p.M && col < p.V && p.row_enc[m] >= 0)
        p.logits[(int64_t)m * p.ldl + col] = acc[r] + bias;
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = col < p.V ? acc[r] + bias : -INFINITY;
    int i = col;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {          // the 32 lanes of this half-wave
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      argmax_merge(v, i, ov, oi);
    }
    if ((lane & 31) == 0) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      red_v[wave][row] = v;
      red_i[wave][row] = i;
    }
  }
  __syncthreads();
  if (tid < JT_ROWS && m0 + tid < p.M) {
    const int m = m0 + tid;
    float v = red_v[0][tid];
    int i = red_i[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) argmax_merge(v, i, red_v[w][tid], red_i[w][tid]);
    if (p.row_enc[m] < 0) { v = -INFINITY; i = -1; }
    const int64_t o = (int64_t)m * gridDim.x + blockIdx.x;
    p.part_max[o] = v;
    p.part_idx[o] = i;
  }
}

// row map of utterance b's next window; lane-strided over the F frames
__device__ __forceinline__ void rnnt_write_map(const RnntState& st, int b, int F, int t, bool done,
                                               int lane) {
  const int len = st.len[b], off = st.off[b];
  for (int f = lane; f < F; f += 64) {
    st.row_enc[b * F + f] = (!done && t + f < len) ? off + t + f : -1;
    st.row_pred[b * F + f] = b;
  }
}

__global__ __launch_bounds__(1024) void rnnt_init_kernel(RnntState st, int B, int F, int blank) {
  __shared__ int live;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += 16) {
    const bool done = st.len[b] <= 0;
    if (lane == 0) {
      st.t[b] = 0; st.cnt[b] = 0; st.n_tok[b] = 0;
      st.last_tok[b] = blank;
      st.done[b] = done;
      st.advance[b] = !done;       // the predictor's first step: the blank id on a zero state
      if (!done) atomicAdd(&live, 1);
    }
    rnnt_write_map(st, b, F, 0, done, lane);
  }
  __syncthreads();
  if (threadIdx.x == 0) { *st.n_active = live; *st.steps = 0; }
}

__global__ __launch_bounds__(1024) void rnnt_advance_kernel(
    const float* __restrict__ part_max, const int* __restrict__ part_idx, int ncb, int V,
    RnntState st, int B, int F, int blank, int n_steps) {
  __shared__ int live;
  const int active_in = *st.n_active;
  if (active_in == 0) return;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += 16) {
    if (st.done[b]) continue;      // (advance[b] is 0 and the row map inert since it finished)
    const int len = st.len[b];
    int t = st.t[b], cnt = st.cnt[b];
    const int nwin = min(F, len - t);
    int first = -1, tok = blank;
    for (int f = 0; f < nwin && first < 0; ++f) {     // frame order; F <= 16
      const int64_t base = (int64_t)(b * F + f) * ncb;
      float v;
      int i;
      rnnt_reduce_row(part_max, part_idx, base, ncb, lane, v, i);
      // a token is a row of the embedding table: anything outside [0, V) is read as blank
      if (i != blank && (unsigned)i < (unsigned)V) { first = f; tok = i; }
    }
    bool adv = false;
    if (first < 0) {
      t += nwin; cnt = 0;
    } else {
      if (first > 0) cnt = 0;
      t += first;
      const int n = st.n_tok[b];
      if (lane == 0) {
        if (n < st.max_tok) st.tokens[(int64_t)b * st.max_tok + n] = tok;
        st.n_tok[b] = n + 1;
        st.last_tok[b] = tok;
      }
      cnt += 1;
      if (cnt >= n_steps) { t += 1; cnt = 0; }
      adv = true;
    }
    const bool done = t >= len;
    if (lane == 0) {
      st.t[b] = t; st.cnt[b] = cnt;
      st.done[b] = done;
      st.advance[b] = adv && !done;
      if (!done) atomicAdd(&live, 1);
    }
    rnnt_write_map(st, b, F, t, done, lane);
  }
  __syncthreads();
  if (threadIdx.x == 0) { *st.n_active = live; *st.steps += 1; }
}

// the column-block reduction of the advance kernel on its own: one wave per row
__global__ __launch_bounds__(256) void rnnt_reduce_kernel(const float* __restrict__ part_max,
                                                          const int* __restrict__ part_idx,
                                                          int ncb, int M, float* out_max,
                                                          int* out_idx) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float v;
  int i;
  rnnt_reduce_row(part_max, part_idx, (int64_t)m * ncb, ncb, lane, v, i);
  if (lane == 0) { out_max[m] = v; out_idx[m] = i; }
}

}  // namespace

int rnnt_linear(const RnntLinearArgs& a, hipStream_t s) {
  WN_CHECK(a.x1 && a.W1 && a.y && a.B >= 1 && a.N >= 1, "rnnt_linear: null / empty operand");
  WN_CHECK(a.K1 >= 1 && a.K1 <= 64 * RL_KC && (!a.W2 || (a.x2 && a.K2 >= 1 && a.K2 <= 64 * RL_KC)),
           "rnnt_linear: input widths must be in [1, 1024]");
  hipLaunchKernelGGL(rnnt_linear_kernel, dim3(cdiv(a.N, 4)), dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_cell(const float* gates, float* h, float* c, const int* advance, int B, int H,
              const int* n_active, hipStream_t s) {
  hipLaunchKernelGGL(rnnt_cell_kernel, dim3(cdiv(B * H, 256)), dim3(256), 0, s, gates, h, c,
                     advance, B, H, n_active);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_joint_col_blocks(int V) { return cdiv(V, JT_COLS); }

int rnnt_joint_argmax(const RnntJointArgs& a, hipStream_t s) {
  WN_CHECK(a.enc_proj && a.pred_proj && a.row_enc && a.row_pred && a.W && a.bias && a.part_max &&
           a.part_idx, "rnnt_joint_argmax: null operand");
  WN_CHECK(a.M >= 1 && a.V >= 1, "rnnt_joint_argmax: empty");
  WN_CHECK(a.J >= 32 && a.J % 32 == 0 && a.J <= 1024,
           "rnnt_joint_argmax: join_dim must be a multiple of 32 in [32, 1024]");
  WN_CHECK(a.lde % 4 == 0 && a.ldp % 4 == 0, "rnnt_joint_argmax: row pitches must be multiples of 4");
  const size_t lds = (size_t)JT_ROWS * (a.J * 4 + 16);
  WN_MAX_DYN_LDS(rnnt_joint_kernel<false>, lds);
  hipLaunchKernelGGL(rnnt_joint_kernel<false>, dim3(cdiv(a.V, JT_COLS), cdiv(a.M, JT_ROWS)),
                     dim3(256), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_joint_rows(const RnntJointArgs& a, hipStream_t s) {
  WN_CHECK(a.enc_proj && a.pred_proj && a.row_enc && a.row_pred && a.W && a.bias && a.logits,
           "rnnt_joint_rows: null operand");
  WN_CHECK(a.M >= 1 && a.V >= 1 && a.ldl >= a.V, "rnnt_joint_rows: empty, or a pitch below V");
  WN_CHECK(a.J >= 32 && a.J % 32 == 0 && a.J <= 1024,
           "rnnt_joint_rows: join_dim must be a multiple of 32 in [32, 1024]");
  WN_CHECK(a.lde % 4 == 0 && a.ldp % 4 == 0, "rnnt_joint_rows: row pitches must be multiples of 4");
  const size_t lds = (size_t)JT_ROWS * (a.J * 4 + 16);
  WN_MAX_DYN_LDS(rnnt_joint_kernel<true>, lds);
  hipLaunchKernelGGL(rnnt_joint_kernel<true>, dim3(cdiv(a.V, JT_COLS), cdiv(a.M, JT_ROWS)),
                     dim3(256), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_init(const RnntState& st, int B, int F, int blank, hipStream_t s) {
  hipLaunchKernelGGL(rnnt_init_kernel, dim3(1), dim3(1024), 0, s, st, B, F, blank);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_advance(const float* part_max, const int* part_idx, int ncb, int V, const RnntState& st,
                 int B, int F, int blank, int n_steps, hipStream_t s) {
  WN_CHECK(ncb >= 1 && ncb == rnnt_joint_col_blocks(V), "rnnt_advance: ncb is not V's block count");
  hipLaunchKernelGGL(rnnt_advance_kernel, dim3(1), dim3(1024), 0, s, part_max, part_idx, ncb, V,
                     st, B, F, blank, n_steps);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_reduce_partials(const float* part_max, const int* part_idx, int ncb, int M,
                         float* out_max, int* out_idx, hipStream_t s) {
  WN_CHECK(part_max && part_idx && out_max && out_idx && ncb >= 1 && M >= 1,
           "rnnt_reduce_partials: null / empty operand");
  hipLaunchKernelGGL(rnnt_reduce_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, part_max, part_idx,
                     ncb, M, out_max, out_idx);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
