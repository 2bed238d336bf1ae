// Conv2dSubsampling4's conv2 (3 x 3, stride 2, d_model = 256) as six bf16 plane products with
// conv1 computed INSIDE the block: no plane image of conv1's output exists (gemm_x6.hip's
// gathered-A form reads one that cmvn_conv1_x3_kernel wrote: 6 B per conv1 element, ~1 GB at
// config 2, written once and read 1.2 times).
//
// A block owns 128 consecutive GEMM rows (output frame g, position f2; f2 fastest) and all 256
// output channels; four waves side by side along N (wave tile 128 x 64, as the four-wave form of
// gemm_x6_kernel), two blocks per CU.  K is walked in chunks of 16 input channels with the nine
// taps inside -- the order gemm_x6_kernel's conv form walks it in (conv_taps = 9), so the fp32
// sums are the same bits.  Per chunk:
//   1. the block computes CMVN + conv1 + ReLU + split3 ONCE for the patch its rows read -- the
//      conv1 frames first .. last of the tile (2 per output frame + 1, + 1 per utterance
//      boundary inside the tile: packed conv1 frames are consecutive across utterances) x F1
//      positions x 16 channels -- from the features (L1 / L2: the tile's window is a few KB) into
//      three bf16 planes in LDS, 32 B per pixel and plane, the even f1 first so that the stride-2
//      taps of consecutive rows read consecutive pixels.  Same operation order as
//      cmvn_conv1_x3_kernel: the operand values are the same bits.
//   2. the nine taps read shifted windows of the patch as MFMA operand fragments; the weight
//      fragments come straight from the (L2-resident) weight image into registers, one k block
//      ahead, so the LDS holds the patch alone: 77 KB, two blocks per CU.
// The patch has ONE buffer (two barriers per chunk): while a block computes its patch, the other
// block of the CU multiplies.  The weight image's k blocks are in (chunk, tap) order
// (conv2_kperm_src), built once per model.
#include "common.h"
#include "kernels.h"
#include "x6.h"

namespace wn {

namespace {

constexpr int PF = CONV2P_FRAMES;          // conv1 frames the patch holds
constexpr int PF1 = 39;                    // F1 it is sized for (F = 80)
constexpr int PLANE = PF * PF1 * 32;       // bytes of one plane of the patch
constexpr int LDS_BYTES = 3 * PLANE + PF * 4;

__global__ __launch_bounds__(256, 2) void conv2_patch_kernel(Conv2PatchArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem_p[];
  int* featrow = reinterpret_cast<int*>(smem_p + 3 * PLANE);   // first feature row of a frame
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  const int F1 = p.F1, F2 = p.F2, ne = (F1 + 1) / 2;

  const int r0 = blockIdx.x * CONV2P_BM;
  const int r_last = min(r0 + CONV2P_BM - 1, p.rows - 1);
  const int g_first = r0 / F2, g_last = r_last / F2;
  int c1_first, nfr;
  {
    const int u0 = p.row_utt2[g_first], u1 = p.row_utt2[g_last];
    c1_first = p.off1[u0] + 2 * (g_first - p.off2[u0]);
    // (the launcher only takes batches whose tiles fit: the clamps keep a wrong call in bounds)
    nfr = min(p.off1[u1] + 2 * (g_last - p.off2[u1]) + 3 - c1_first, PF);
  }
  if (tid <= g_last - g_first) {
    const int g = g_first + tid;
    const int u = p.row_utt2[g], t2 = g - p.off2[u];
    const int c = p.off1[u] + 2 * t2 - c1_first;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
      if (c + ky < PF) featrow[c + ky] = u * p.T + 4 * t2 + 2 * ky;
  }
  // byte offset (inside a plane) of the base pixel of this lane's row in each of the four A tiles
  int pixb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = min(r0 + i * 32 + li, p.rows - 1);
    const int g = row / F2, f2 = row - g * F2;
    const int u = p.row_utt2[g];
    const int slot = min(p.off1[u] + 2 * (g - p.off2[u]) - c1_first, PF - 3);
    pixb[i] = (slot * F1 + f2) * 32 + hi * 16;
  }
  int delta[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    delta[ky * 3 + 0] = (ky * F1) * 32;            // f1 = 2 f2     (even, position f2)
    delta[ky * 3 + 1] = (ky * F1 + ne) * 32;       // f1 = 2 f2 + 1 (odd, position ne + f2)
    delta[ky * 3 + 2] = (ky * F1 + 1) * 32;        // f1 = 2 f2 + 2 (even, position f2 + 1)
  }
  __syncthreads();

  struct FA { bf16x8 p[3]; };
  struct FB { bf16x8 p[2][3]; };
  const char* wp = reinterpret_cast<const char*>(p.W3p) + (wn * 2) * X3_TILE + lane * 16;
  auto loadW = [&](int kb) {
    const char* q = wp + (int64_t)kb * (8 * X3_TILE);
    FB f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        f.p[j][pl] = *reinterpret_cast<const bf16x8*>(q + j * X3_TILE + pl * X3_REC);
    return f;
  };
  auto loadA = [&](int tap, int i) {
    const char* q = smem_p + pixb[i] + delta[tap];
    FA f;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) f.p[pl] = *reinterpret_cast<const bf16x8*>(q + pl * PLANE);
    return f;
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the patch of channel chunk c: wave w computes the channel half w & 1 (its 72 weights + 8
  // biases are wave-uniform) of the pixels (w >> 1) * 64 + lane + 128 j
  const int half = wn & 1;
  const int npix = nfr * F1;
  auto patch = [&](int c) {
    const int ch = c * 16 + half * 8;
    float w[9][8], bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = p.b1[ch + e];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) w[k][e] = p.w1[k * CONV2P_D + ch + e];
    for (int px = (wn >> 1) * 64 + lane; px < npix; px += 128) {
      const int slot = px / F1, pos = px - slot * F1;
      const int f1 = pos < ne ? 2 * pos : 2 * (pos - ne) + 1;
      const float* src = p.feats + (int64_t)featrow[slot] * p.F + 2 * f1;
      float x[3][3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) x[ky][kx] = src[ky * p.F + kx];
      if (p.mean) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float mu = p.mean[2 * f1 + kx], is = p.istd[2 * f1 + kx];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) x[ky][kx] = (x[ky][kx] - mu) * is;
        }
      }
      float a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = bias[e];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(w[ky * 3 + kx][e], x[ky][kx], a[e]);
      bf16x8 p0, p1, p2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const Split3 sp = split3(fmaxf(a[e], 0.f));
        p0[e] = sp.h0; p1[e] = sp.h1; p2[e] = sp.h2;
      }
      char* o = smem_p + px * 32 + half * 16;
      *reinterpret_cast<bf16x8*>(o) = p0;
      *reinterpret_cast<bf16x8*>(o + PLANE) = p1;
      *reinterpret_cast<bf16x8*>(o + 2 * PLANE) = p2;
    }
  };

  // six plane products in gemm_x6_kernel's order (the small ones first, the two accumulators of
  // the A tile alternating); W fragment = MFMA "A": a lane owns one row of C
  auto mma = [&](const FA& a, const FB& b, int i) {
    constexpr int PB[6] = {2, 0, 1, 1, 0, 0}, PA[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b.p[j][PB[q]], a.p[PA[q]], acc[i][j],
                                                            0, 0, 0);
  };

  constexpr int NCH = CONV2P_D / 16, NKB = 9 * NCH;
  FB fb = loadW(0);
  for (int c = 0; c < NCH; ++c) {
    if (c > 0) __syncthreads();          // everyone has read the patch of chunk c - 1
    patch(c);
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const FB nb = loadW(min(c * 9 + tap + 1, NKB - 1));
      FA fa = loadA(tap, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        FA na;
        if (i + 1 < 4) na = loadA(tap, i + 1);
        mma(fa, fb, i);
        if (i + 1 < 4) fa = na;
      }
      fb = nb;
    }
  }

  // epilogue (gemm_x6_kernel's EPI 0 with ReLU): lane = row of C, registers = columns
  // 8 g + 4 hi + e of the 32-column tile
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cb = (wn * 2 + j) * 32;
    f32x4 bias4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      bias4[g] = *reinterpret_cast<const f32x4*>(p.bias + cb + 8 * g + 4 * hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r0 + i * 32 + li;
      if (row >= p.rows) continue;
      float* crow = p.C + (int64_t)row * p.ldc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(acc[i][j][4 * g + e] + bias4[g][e], 0.0f);
        *reinterpret_cast<f32x4*>(crow + cb + 8 * g + 4 * hi) = o;
      }
    }
  }
}

}  // namespace

int conv2_kperm_src(int kb, int kbc, int taps) { return (kb % taps) * kbc + kb / taps; }

// the most conv1 frames a 128-row tile of the batch reads (off2 / len2: output frames per
// utterance; F2 positions per frame)
int conv2_patch_max_frames(const std::vector<int>& off2, const std::vector<int>& len2, int F2) {
  int M = 0;
  for (size_t b = 0; b < off2.size(); ++b) M = std::max(M, off2[b] + len2[b]);
  std::vector<int> c1((size_t)std::max(M, 1), 0);
  int o1 = 0;
  for (size_t b = 0; b < off2.size(); ++b) {
    for (int t = 0; t < len2[b]; ++t) c1[off2[b] + t] = o1 + 2 * t;
    if (len2[b] > 0) o1 += 2 * len2[b] + 1;
  }
  const int64_t rows = (int64_t)M * F2;
  int worst = 0;
  for (int64_t r0 = 0; r0 < rows; r0 += CONV2P_BM) {
    const int64_t r1 = std::min(r0 + CONV2P_BM - 1, rows - 1);
    worst = std::max(worst, c1[r1 / F2] + 3 - c1[r0 / F2]);
  }
  return worst;
}

int conv2_patch(const Conv2PatchArgs& a, hipStream_t s) {
  WN_CHECK(a.feats && a.w1 && a.b1 && a.W3p && a.bias && a.row_utt2 && a.off2 && a.off1 && a.C,
           "conv2_patch: null argument");
  WN_CHECK(a.F1 > 0 && a.F1 <= PF1 && a.F1 == (a.F - 1) / 2 && a.F2 == (a.F1 - 1) / 2 &&
               a.F2 > 0,
           "conv2_patch: feature width");
  WN_CHECK(a.rows > 0 && a.rows % a.F2 == 0 && a.ldc >= CONV2P_D && a.ldc % 4 == 0 &&
               a.rows < (1 << 24),
           "conv2_patch: rows / pitch");
  WN_CHECK(a.max_frames > 0 && a.max_frames <= PF, "conv2_patch: a tile reads too many frames");
  WN_CHECK((int64_t)a.B * a.T < ((int64_t)1 << 31), "conv2_patch: feature rows");
  WN_MAX_DYN_LDS(conv2_patch_kernel, LDS_BYTES);
  hipLaunchKernelGGL(conv2_patch_kernel, dim3(cdiv(a.rows, CONV2P_BM)), dim3(256), LDS_BYTES, s,
                     a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
