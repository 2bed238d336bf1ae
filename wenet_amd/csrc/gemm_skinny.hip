// Skinny GEMM for the autoregressive decoder step: C[M,N] = resid + act(A[M,K] * W[N,K]^T + bias)
// with M <= 256 rows (B x beam hypotheses) against d_model- / vocabulary-wide weights.
//
// At these shapes the tile rule of gemm.hip ends at 64 x 64 blocks: N = 1280 gives 60 blocks on
// 256 CUs and every weight slice is fetched by three M tiles.  The step is a weight stream (and,
// with fp32 operands, 64-cycle MFMAs on too few SIMDs), so this kernel turns the decomposition
// round:
//  * a block owns ALL M rows of a 128-column slice (four waves x 32 columns) and one K slice:
//    every byte of W is read from HBM exactly once;
//  * the grid is (N / 128) x S with the K split S chosen so that it covers about 3/4 of the CUs
//    (gemm_skinny_split);
//  * W goes global -> VGPR directly in the MFMA operand layout (lane = column, 16 B of k; no
//    other wave shares a W element, LDS staging would be pure overhead), one tile ahead of the
//    MFMAs that consume it;
//  * A (at most 256 x K fp32, L2-resident, re-read by every block) is the operand that goes
//    through LDS: whole 128-byte lines per 8 (fp32) / 16 (bf16) lanes, double-buffered, rows at
//    a 144-byte pitch (conflict-free ds_read_b128, the pitch gemm.hip uses);
//  * fp32 operands on v_mfma_f32_32x32x2_f32, or -- with the bf16 image of the weights -- A
//    rounded to bf16 on its way into LDS and v_mfma_f32_32x32x16_bf16; fp32 accumulation;
//  * split K is deterministic: slice partials to a workspace, summed in slice order by a second
//    launch that applies bias, activation and residual.  No float atomics: two runs give the
//    same bits (the beam search's token parity depends on it).  S = 1 writes C directly.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace wn {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int SK_COLS = 128;       // columns per block
constexpr int SK_PITCH = 144;      // bytes per LDS row: 32 floats / 64 bf16 + 16 B

__device__ __forceinline__ float skinny_act(float x, int act) {
  if (act == ACT_RELU) x = fmaxf(x, 0.0f);
  if (act == ACT_GELU) x = 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
  if (act == ACT_SILU) x = x * wn_rcp(1.0f + wn_exp(-x));
  return x;
}

template <int MT, bool BF>
__global__ __launch_bounds__(256) void skinny_kernel(SkinnyArgs p, int S) {
  constexpr int BK = BF ? 64 : 32;            // k per tile
  constexpr int ROWS = MT * 32;
  constexpr int CPR = BK / 4;                 // 16-byte fp32 chunks of A per tile row
  constexpr int ACH = ROWS * CPR / 256;       // ... per thread
  constexpr int TILE_B = ROWS * SK_PITCH;
  using WT = std::conditional_t<BF, bf16x8, f32x4>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * SK_COLS + wave * 32;
  const int nk = (p.K + BK - 1) / BK;
  const int slice = blockIdx.y;
  const int t0 = (int)((int64_t)slice * nk / S), t1 = (int)((int64_t)(slice + 1) * nk / S);

  const float* a_ptr[ACH];
  int a_lds[ACH], a_k[ACH];
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int c = tid + 256 * i;
    const int row = c / CPR, kc = c % CPR;
    const int grow = min(row, p.M - 1);       // rows past M: a copy of the last row, never stored
    a_ptr[i] = p.A + (int64_t)grow * p.lda + kc * 4;
    a_lds[i] = row * SK_PITCH + kc * (BF ? 8 : 16);
    a_k[i] = kc * 4;
  }
  const int wrow = min(n0 + (lane & 31), p.N - 1);   // columns past N: likewise
  const int wk = (lane >> 5) * (BF ? 8 : 4);
  const float* w_ptr = BF ? nullptr : p.W + (int64_t)wrow * p.K + wk;
  const __bf16* wh_ptr = BF ? reinterpret_cast<const __bf16*>(p.Wh) + (int64_t)wrow * p.K + wk
                            : nullptr;

  auto gload_a = [&](int t, f32x4 (&ra)[ACH]) {
    const int k0 = t * BK;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      if (!BF || k0 + a_k[i] < p.K)           // (bf16: K may end in the middle of a 64-k tile)
        ra[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
      else
        ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto lstore = [&](int buf, const f32x4 (&ra)[ACH]) {
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      char* dst = smem + buf * TILE_B + a_lds[i];
      if constexpr (BF) {
        bf16x4 h;
        h[0] = (__bf16)ra[i][0]; h[1] = (__bf16)ra[i][1];
        h[2] = (__bf16)ra[i][2]; h[3] = (__bf16)ra[i][3];
        *reinterpret_cast<bf16x4*>(dst) = h;
      } else {
        *reinterpret_cast<f32x4*>(dst) = ra[i];
      }
    }
  };
  auto gload_w = [&](int t, WT (&w)[4]) {
    const int k0 = t * BK;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if constexpr (BF) {
        if (k0 + 16 * kk + wk < p.K) {
          w[kk] = *reinterpret_cast<const bf16x8*>(wh_ptr + k0 + 16 * kk);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) w[kk][e] = (__bf16)0.f;
        }
      } else {
        w[kk] = *reinterpret_cast<const f32x4*>(w_ptr + k0 + 8 * kk);
      }
    }
  };

  f32x16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  // fragment of MFMA kk: row = lane & 31, 16 bytes of k at kk * 32 + (lane >> 5) * 16 -- the
  // same k the lane's W register holds (4 fp32 resp. 8 bf16)
  const int frag = (lane & 31) * SK_PITCH + (lane >> 5) * 16;
  auto compute = [&](int buf, const WT (&w)[4]) {
    const char* base = smem + buf * TILE_B + frag;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const char* fp = base + i * 32 * SK_PITCH + kk * 32;
        if constexpr (BF) {
          const bf16x8 fa = *reinterpret_cast<const bf16x8*>(fp);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, w[kk], acc[i], 0, 0, 0);
        } else {
          const f32x4 fa = *reinterpret_cast<const f32x4*>(fp);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], w[kk][e], acc[i], 0, 0, 0);
        }
      }
    }
  };

  // double-buffered: the loads of tile i + 1 (A to registers, W to its other register set) are
  // issued in front of the MFMAs of tile i and waited for behind them
  const int nt = t1 - t0;           // >= 1 (S <= nk), the same for the whole block
  {
    WT w0[4], w1[4];
    f32x4 ra[ACH];
    gload_a(t0, ra);
    gload_w(t0, w0);
    lstore(0, ra);
    __syncthreads();
    int i = 0;
    for (; i + 1 < nt; i += 2) {
      gload_a(t0 + i + 1, ra);
      gload_w(t0 + i + 1, w1);
      compute(0, w0);
      lstore(1, ra);
      __syncthreads();
      const bool more = i + 2 < nt;
      if (more) { gload_a(t0 + i + 2, ra); gload_w(t0 + i + 2, w0); }
      compute(1, w1);
      if (more) lstore(0, ra);
      __syncthreads();
    }
    if (i < nt) compute(0, w0);
  }

  // C / D layout of the 32 x 32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int col = n0 + (lane & 31);
  if (col >= p.N) return;
  const int row_hi = (lane >> 5) * 4;
  if (S == 1) {
    const float b = p.bias ? p.bias[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + row_hi + (r & 3) + 8 * (r >> 2);
        if (row < p.M) {
          float x = skinny_act(acc[i][r] + b, p.act);
          if (p.resid) x += p.resid[(int64_t)row * p.ldr + col];
          p.C[(int64_t)row * p.ldc + col] = x;
        }
      }
  } else {
    float* out = p.part + (int64_t)slice * p.M * p.N + col;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + row_hi + (r & 3) + 8 * (r >> 2);
        if (row < p.M) out[(int64_t)row * p.N] = acc[i][r];
      }
  }
}

// C = resid + act(sum_s part[s] + bias), the slices in ascending order
__global__ __launch_bounds__(256) void skinny_reduce_kernel(SkinnyArgs p, int S) {
  const int64_t mn = (int64_t)p.M * p.N;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= mn) return;
  const int row = (int)(idx / p.N), col = (int)(idx - (int64_t)row * p.N);
  float sum = p.part[idx];
  for (int s = 1; s < S; ++s) sum += p.part[(int64_t)s * mn + idx];
  float x = skinny_act(sum + (p.bias ? p.bias[col] : 0.0f), p.act);
  if (p.resid) x += p.resid[(int64_t)row * p.ldr + col];
  p.C[(int64_t)row * p.ldc + col] = x;
}

template <int MT, bool BF>
int launch_skinny(const SkinnyArgs& a, int S, hipStream_t s) {
  const size_t lds = (size_t)2 * MT * 32 * SK_PITCH;
  auto kern = skinny_kernel<MT, BF>;
  WN_MAX_DYN_LDS(kern, lds);
  hipLaunchKernelGGL(kern, dim3(cdiv(a.N, SK_COLS), S), dim3(256), lds, s, a, S);
  WN_HIP(hipGetLastError());
  return 0;
}

template <bool BF>
int dispatch_mt(const SkinnyArgs& a, int S, hipStream_t s) {
  switch (cdiv(a.M, 32)) {
    case 1: return launch_skinny<1, BF>(a, S, s);
    case 2: return launch_skinny<2, BF>(a, S, s);
    case 3: return launch_skinny<3, BF>(a, S, s);
    case 4: return launch_skinny<4, BF>(a, S, s);
    case 5: return launch_skinny<5, BF>(a, S, s);
    case 6: return launch_skinny<6, BF>(a, S, s);
    case 7: return launch_skinny<7, BF>(a, S, s);
    case 8: return launch_skinny<8, BF>(a, S, s);
  }
  set_error("gemm_skinny: M must be in [1, 256]");
  return -1;
}

}  // namespace

// K tiles of the kernel: 32 k with fp32 operands, 64 with the bf16 image
static int skinny_tiles(int K, bool bf16) { return bf16 ? cdiv(K, 64) : K / 32; }

// The K split: as many slices as bring the grid to ~192 blocks (3/4 of the CUs: every step GEMM
// of the decoder lands between 1/2 and 1 x the CU count), in whole K tiles of equal count.
int gemm_skinny_split(int N, int K, bool bf16) {
  const int nk = skinny_tiles(K, bf16);
  const int s0 = std::min(std::max(192 / cdiv(N, SK_COLS), 1), nk);
  const int per = std::max(nk / s0, 1);
  return cdiv(nk, per);
}

size_t gemm_skinny_ws_bytes(int M, int N, int S) {
  return S > 1 ? (size_t)S * M * N * sizeof(float) : 0;
}

int gemm_skinny(const SkinnyArgs& a, hipStream_t stream) {
  WN_CHECK(a.A && (a.W || a.Wh) && a.C, "gemm_skinny: null operand");
  WN_CHECK(a.M >= 1 && a.M <= 256, "gemm_skinny: M must be in [1, 256]");
  WN_CHECK(a.N > 0 && a.K > 0 && a.K % 32 == 0, "gemm_skinny: K must be a multiple of 32");
  WN_CHECK(a.lda % 4 == 0 && a.lda >= a.K, "gemm_skinny: lda must be a multiple of 4 floats");
  WN_CHECK(a.act == ACT_NONE || a.act == ACT_RELU || a.act == ACT_GELU || a.act == ACT_SILU,
           "gemm_skinny: unknown activation");
  const bool bf = a.Wh != nullptr;
  const int nk = skinny_tiles(a.K, bf);
  int S = a.split_k > 0 ? a.split_k : gemm_skinny_split(a.N, a.K, bf);
  S = std::min(S, nk);
  if (S > 1)
    WN_CHECK(a.part && a.part_bytes >= gemm_skinny_ws_bytes(a.M, a.N, S),
             "gemm_skinny: split-K workspace too small");
  WN_TRY(bf ? dispatch_mt<true>(a, S, stream) : dispatch_mt<false>(a, S, stream));
  if (S > 1) {
    const int64_t mn = (int64_t)a.M * a.N;
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)cdiv64(mn, 256)), dim3(256), 0,
                       stream, a, S);
    WN_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace wn
