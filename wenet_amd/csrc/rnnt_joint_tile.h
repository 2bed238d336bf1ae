// The joint network's 32-row tile, shared by rnnt_joint_kernel (transducer.hip: arg-max and
// full-row epilogues) and rnnt_gather_kernel (transducer_score.hip: gathering log-softmax
// epilogue).  One text for the A tile and the k loop, so a logit is the same bits in all three.
#pragma once
#include "kernels.h"

namespace wn {

constexpr int JT_ROWS = 32;        // rows per block
constexpr int JT_COLS = 128;       // columns per block / per pass (four waves x 32)

// bytes per LDS row of the A tile: J / 4 + 1 sixteen-byte granules, odd for every J that is a
// multiple of 8, so the 32 rows of a ds_read_b128 fall into distinct granules mod 16
__device__ __forceinline__ int rnnt_joint_pitch(int J) { return J * 4 + 16; }

// A rows m0 .. m0 + 31 into LDS: tanh(enc_proj[row_enc[m]] + pred_proj[row_pred[m]]); rows past M
// and inert rows (row_enc[m] < 0) are zeros.  256 threads; the caller synchronises.
__device__ __forceinline__ void rnnt_joint_stage_a(char* smem, const float* __restrict__ enc_proj,
                                                   int lde, const float* __restrict__ pred_proj,
                                                   int ldp, const int* __restrict__ row_enc,
                                                   const int* __restrict__ row_pred, int M, int J,
                                                   int m0, int tid) {
  const int pitch = rnnt_joint_pitch(J);
  const int j4 = J / 4;
  for (int c = tid; c < JT_ROWS * j4; c += 256) {
    const int row = c / j4, kc = c - row * j4;
    const int m = m0 + row;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m < M) {
      const int re = row_enc[m];
      if (re >= 0) {
        const f32x4 e = *reinterpret_cast<const f32x4*>(enc_proj + (int64_t)re * lde + kc * 4);
        const f32x4 q = *reinterpret_cast<const f32x4*>(
            pred_proj + (int64_t)row_pred[m] * ldp + kc * 4);
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) v[e4] = tanhf(e[e4] + q[e4]);
      }
    }
    *reinterpret_cast<f32x4*>(smem + row * pitch + kc * 16) = v;
  }
}

// One wave: the 32 x 32 products of the A tile with W rows n0 .. n0 + 31 (columns past V: a copy
// of row V - 1, never kept), without the bias.  C / D layout: col = lane & 31,
// row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// Four accumulators, one per k mod 4 class (each an fmaf chain over J / 4 terms in ascending
// k -- the f32 MFMA is an fmaf chain per output element), summed as (0 + 1) + (2 + 3): a fixed
// order, shorter chains, less rounding error.
__device__ __forceinline__ f32x16 rnnt_joint_tile_sums(const char* smem,
                                                       const float* __restrict__ W, int J, int V,
                                                       int n0, int lane) {
  const int pitch = rnnt_joint_pitch(J);
  const int wrow = min(n0 + (lane & 31), V - 1);
  const float* w_ptr = W + (int64_t)wrow * J + (lane >> 5) * 4;
  const char* a_ptr = smem + (lane & 31) * pitch + (lane >> 5) * 16;
  f32x16 acc4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc4[e][r] = 0.0f;
  // 8 k per round: lanes 0..31 hold k0 + 0..3, lanes 32..63 k0 + 4..7 of their row / column
  const int nk8 = J / 8;
#pragma unroll 4
  for (int k8 = 0; k8 < nk8; ++k8) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(w_ptr + k8 * 8);
    const f32x4 a = *reinterpret_cast<const f32x4*>(a_ptr + k8 * 32);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      acc4[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], w[e], acc4[e], 0, 0, 0);
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = (acc4[0][r] + acc4[1][r]) + (acc4[2][r] + acc4[3][r]);
  return acc;
}

}  // namespace wn
