// Teacher-forced transducer score: -RNN-T loss of given hypotheses under the encoder output
// (wenet/models/transducer/transducer.py:161-186, _cal_transducer_score).  The reference builds
// the (beam, T', U + 1, V) joint logits and hands them to rnnt_loss; here the hypotheses of an
// utterance go into a prefix trie (rnnt_trie.h, host) and
//  * rnnt_gather_kernel   one GEMM row per (frame, trie node): the A tile
//    tanh(enc_proj + pred_proj) and the k loop on v_mfma_f32_32x32x2_f32 are rnnt_joint_kernel's
//    own (rnnt_joint_tile.h: one text, so a logit is the same bits as in the searches).  A block
//    owns a tile of 32 rows and walks ALL of V in passes of 128 columns, keeping a running
//    (max, sum of exponentials) per row and writing only logit - logsumexp at the row's listed
//    columns (the blank and the tokens of the node's children).  Nothing of size M x V or
//    M x V / 128 is written.  A 32-row block re-reads all of ffn_out from L2, which argued for a
//    larger tile; measured, a 64-row tile (161 VGPRs + 128 AGPRs, one wave per SIMD against
//    three) was 15-21 % slower at the bench shape and a 128-row one spills to scratch, so
//    neither is kept (docs/LOG_round15.md).
//    Order of summation: the 32 columns of a wave's group are reduced by a butterfly over the
//    lanes (place = column mod 32), the groups of a wave (columns = wave mod 4 of the 128
//    pass) merge in ascending column order, then the four waves merge 0, 1, 2, 3: the order is
//    a function of the column alone, so a row's values are the same bits at any offset in a
//    tile and in any batch;
//  * rnnt_trie_gather_kernel   the LSTM state of a node's parent into the node's row, before
//    the predictor step of its depth (rnnt_linear / rnnt_cell, depth by depth);
//  * rnnt_lattice_kernel  one wave per hypothesis, anti-diagonal wavefront over (t, u) in fp64,
//    two columns of alpha in LDS (any U: lanes stride over u):
//      alpha(t, u) = log_add(alpha(t - 1, u) + lp_blank(t - 1, u), alpha(t, u - 1) + lp_label(t, u - 1))
//      score = alpha(T - 1, U) + lp_blank(T - 1, U).
#include "rnnt_joint_tile.h"

namespace wn {
namespace {

// wenet/utils/common.py:302-310 for two values, as transducer_beam.hip: two -inf give -inf
__device__ __forceinline__ double lat_log_add(double a, double b) {
  if (a != a || b != b) return __builtin_nan("");
  if (a == -INFINITY && b == -INFINITY) return -INFINITY;
  const double m = a > b ? a : b, n = a > b ? b : a;
  return m + log(1.0 + exp(n - m));
}

// (max, sum of exp(x - max)) of two column sets; an empty set is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& M, float& S, float m, float s) {
  const float n = fmaxf(M, m);
  const float a = M == -INFINITY ? 0.0f : S * expf(M - n);
  const float b = m == -INFINITY ? 0.0f : s * expf(m - n);
  M = n;
  S = a + b;
}

__global__ __launch_bounds__(256) void rnnt_gather_kernel(RnntGatherArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red_m[4][JT_ROWS], red_s[4][JT_ROWS];
  __shared__ float lse[JT_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * JT_ROWS;
  rnnt_joint_stage_a(smem, p.enc_proj, p.lde, p.pred_proj, p.ldp, p.row_enc, p.row_pred, p.M, p.J,
                     m0, tid);
  __syncthreads();

  const int e0 = p.col_off[m0], e1 = p.col_off[min(m0 + JT_ROWS, p.M)];
  // lane (lane & 31) = r < 16 keeps the running pair of tile row (r & 3) + 8 (r >> 2) +
  // 4 (lane >> 5) for this wave's column groups
  float st_m = -INFINITY, st_s = 0.0f;
  const int ncb = (p.V + JT_COLS - 1) / JT_COLS;
  for (int cb = 0; cb < ncb; ++cb) {
    const int n0 = cb * JT_COLS + wave * 32;
    f32x16 val = rnnt_joint_tile_sums(smem, p.W, p.J, p.V, n0, lane);
    const int col = n0 + (lane & 31);
    const float bias = col < p.V ? p.bias[col] : 0.0f;
    float gm = -INFINITY, gs = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      val[r] += bias;
      const float v = col < p.V ? val[r] : -INFINITY;
      float mx = v;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float sm = mx == -INFINITY ? 0.0f : expf(v - mx);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
      if ((lane & 31) == r) { gm = mx; gs = sm; }
    }
    lse_merge(st_m, st_s, gm, gs);
    // the listed columns of the tile's rows that fall into this wave's 32 columns
    for (int eb = e0; eb < e1; eb += 64) {
      const int e = eb + lane;
      int c = -1, rw = 0;
      if (e < e1) {
        rw = p.ent_row[e] - m0;
        if (p.row_enc[m0 + rw] >= 0) c = p.cols[e];
      }
      unsigned long long hits = __ballot(c >= n0 && c < n0 + 32);
      while (hits) {
        const int src = __ffsll(hits) - 1;
        hits &= hits - 1;
        const int cc = __shfl(c, src, 64), q = __shfl(rw, src, 64);
        const int r_w = (q & 3) + 4 * (q >> 3);
        float v = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (r == r_w) v = val[r];
        if (lane == (cc - n0) + 32 * ((q >> 2) & 1)) p.logp[eb + src] = v;
      }
    }
  }
  if ((lane & 31) < 16) {
    const int r = lane & 31;
    const int q = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    red_m[wave][q] = st_m;
    red_s[wave][q] = st_s;
  }
  __syncthreads();
  if (tid < JT_ROWS) {
    float M = red_m[0][tid], S = red_s[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) lse_merge(M, S, red_m[w][tid], red_s[w][tid]);
    lse[tid] = M + logf(S);
  }
  __syncthreads();      // (and this block's logit stores are visible to its threads)
  for (int e = e0 + tid; e < e1; e += 256) {
    const int rw = p.ent_row[e] - m0;
    if (p.row_enc[m0 + rw] >= 0) p.logp[e] = p.logp[e] - lse[rw];
  }
}

__global__ __launch_bounds__(256) void rnnt_trie_gather_kernel(const int* __restrict__ parent,
                                                               float* h, float* c, int r0, int L,
                                                               int64_t layer_stride, int H) {
  const int g = r0 + blockIdx.x;
  const int pg = parent[g];
  if (pg < 0) return;
  for (int l = 0; l < L; ++l) {
    const int64_t o = l * layer_stride + (int64_t)g * H, i = l * layer_stride + (int64_t)pg * H;
    for (int k = threadIdx.x; k < H; k += 256) { h[o + k] = h[i + k]; c[o + k] = c[i + k]; }
  }
}

__global__ __launch_bounds__(64) void rnnt_lattice_kernel(RnntLatticeArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* prev = reinterpret_cast<double*>(smem);
  double* cur = prev + (p.max_U + 1);
  const int n = blockIdx.x, lane = threadIdx.x;
  const int T = p.T[n], U = p.U[n];
  if (T <= 0) {
    if (lane == 0) p.score[n] = -INFINITY;
    return;
  }
  const float* eb = p.blank + p.blank_base[n];
  const float* el = p.label + p.label_base[n];
  const int64_t sb = p.blank_stride[n], sl = p.label_stride[n];
  const int* ub = p.ub + p.u_off[n];
  const int* ul = p.ul + p.u_off[n];
  for (int d = 0; d < T + U; ++d) {        // the anti-diagonal t + u = d
    const int ulo = max(0, d - T + 1), uhi = min(U, d);
    for (int u = ulo + lane; u <= uhi; u += 64) {
      const int t = d - u;
      double a = 0.0;                      // alpha(0, 0)
      if (d > 0) {
        const double x = t > 0 ? prev[u] + (double)eb[(t - 1) * sb + ub[u]] : -INFINITY;
        const double y = u > 0 ? prev[u - 1] + (double)el[t * sl + ul[u - 1]] : -INFINITY;
        a = lat_log_add(x, y);
      }
      cur[u] = a;
    }
    __syncthreads();
    double* sw = prev; prev = cur; cur = sw;
  }
  if (lane == 0) p.score[n] = prev[U] + (double)eb[(T - 1) * sb + ub[U]];
}

}  // namespace

int rnnt_joint_logp_gather(const RnntGatherArgs& a, hipStream_t s) {
  WN_CHECK(a.enc_proj && a.pred_proj && a.row_enc && a.row_pred && a.W && a.bias && a.col_off &&
           a.cols && a.ent_row && a.logp, "rnnt_joint_logp_gather: null operand");
  WN_CHECK(a.M >= 1 && a.V >= 1, "rnnt_joint_logp_gather: empty");
  WN_CHECK(a.J >= 32 && a.J % 32 == 0 && a.J <= 1024,
           "rnnt_joint_logp_gather: join_dim must be a multiple of 32 in [32, 1024]");
  WN_CHECK(a.lde % 4 == 0 && a.ldp % 4 == 0,
           "rnnt_joint_logp_gather: row pitches must be multiples of 4");
  const size_t lds = (size_t)JT_ROWS * (a.J * 4 + 16);
  WN_MAX_DYN_LDS(rnnt_gather_kernel, lds);
  hipLaunchKernelGGL(rnnt_gather_kernel, dim3(cdiv(a.M, JT_ROWS)), dim3(256), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_trie_gather(const int* parent, float* h, float* c, int r0, int n, int L,
                     int64_t layer_stride, int H, hipStream_t s) {
  WN_CHECK(parent && h && c && r0 >= 0 && n >= 1 && L >= 1 && H >= 1,
           "rnnt_trie_gather: null / empty operand");
  hipLaunchKernelGGL(rnnt_trie_gather_kernel, dim3(n), dim3(256), 0, s, parent, h, c, r0, L,
                     layer_stride, H);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_lattice(const RnntLatticeArgs& a, hipStream_t s) {
  WN_CHECK(a.blank && a.label && a.T && a.U && a.blank_base && a.label_base && a.blank_stride &&
           a.label_stride && a.u_off && a.ub && a.ul && a.score, "rnnt_lattice: null operand");
  WN_CHECK(a.N >= 1 && a.max_U >= 0, "rnnt_lattice: empty");
  const size_t lds = 2 * ((size_t)a.max_U + 1) * sizeof(double);
  WN_CHECK(lds <= 64 * 1024, "rnnt_lattice: a hypothesis is longer than 4095 tokens");
  hipLaunchKernelGGL(rnnt_lattice_kernel, dim3(a.N), dim3(64), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
