// Conv2dSubsampling6's front end in one launch (subsampling.py:231-280, F = 80): CMVN + conv1
// (3 x 3, stride 2) + ReLU + conv2 (5 x 5, stride 3) + bias + ReLU, fp32 semantics from six bf16
// plane products of exactly split operands (x6.h split3, v_mfma_f32_32x32x16_bf16, the plane
// order of conv2_patch.hip / gemm_x6.hip).  No conv1 tensor and no plane image exist in HBM.
//
// GEMM view: row = (output frame g, position f2), F2 = 12 rows per frame; K = 25 taps x d input
// channels; N = d.  At d = 512 that is 0.16 GFLOP per output frame.
//
// Tiles.  A block owns FT whole output frames of ONE utterance (host-built tile list: utterance,
// first frame t0, frame count n <= FT, packed first frame g0).  Output frame t2 reads the conv1
// frames 3 t2 .. 3 t2 + 4, so a tile's conv1 frames are one contiguous run of 3 n + 2 frames that
// starts at conv1 frame 3 t0, made from the 2 (3 n + 2) + 1 feature rows from 6 t0 on (the last
// is row 6 (t0 + n - 1) + 10 < L: no padding is ever read).  There is no boundary term and no
// "tile reads too many frames" fall-back: every batch takes this one route, a streaming chunk's
// few rows included.  Dead rows exist only in an utterance's last tile (n < FT) and behind row
// 12 FT of the last 32-row MFMA tile; they read patch slots inside the allocation that nobody
// wrote for this tile (a GEMM row never mixes with another row) and are not stored.
//
//   FT   GEMM rows    conv1 frames   LDS (patch + features)   blocks / CU
//    5   60 of 64     17              62.2 + 10.9 KB            2
//    8   96 of 96     26              95.1 + 16.6 KB            1
//   10   120 of 128   32             117.0 + 20.3 KB            1
// The weight image (25 d^2 x 6 B: 9.8 MB at d = 256, 39 MB at 512) is read once per tile from
// L2, so a larger FT reads proportionally less of it.
//
// K walk: chunks of 16 input channels with the 25 taps inside, the weight image's k blocks in
// that (chunk, tap) order (conv2_kperm_src(kb, d / 16, 25); staged so by wn_model_create, split
// by build_x6_images).  Per chunk the block computes conv1 + ReLU + split3 ONCE for its patch
// -- (3 n + 2) x 39 pixels x 16 channels -- into three bf16 planes in LDS; 25 taps then read it
// (9 in conv2_patch.hip), so the patch arithmetic is a small share.  The CMVN-normalised feature
// window of the tile is staged in LDS once per block: the per-chunk patch pass reads no global
// memory but conv1's 16 x 10 weights (wave-uniform).  Weight fragments go from L2 to registers
// one k block ahead; the LDS holds activations only.  One patch buffer, two barriers per chunk.
//
// Patch layout.  F1 = 39 = 3 x 13: pixel f1 sits at position (f1 % 3) * 13 + f1 / 3 of its frame,
// so tap kx of row f2 (f1 = 3 f2 + kx) reads position (kx % 3) * 13 + kx / 3 + f2: consecutive
// rows read consecutive positions (the stride-3 analogue of conv2_patch.hip's even-first order).
// A plane is two half planes, [channel half h][frame][position] x 16 B (8 bf16): an MFMA operand
// fragment is ONE ds_read_b128 per lane and plane, lane = (h, row).
// Banks (taking 64 banks x 4 B and a b128 access served per group of 16 lanes = 256 B): the 16
// lanes of a group have the same h and consecutive rows.  The 12 rows of a frame read 192
// contiguous bytes; the next frame's rows start 3 x 39 x 16 = 1872 B further, i.e. 80 B further
// modulo 256, so where a group spans a frame boundary at most 7 of its 16 pieces fall on banks
// the group already uses: 2-way on those, none inside a frame.
// With 32-B pixels (both halves together, as conv2_patch.hip stores them) every group would
// read at stride 32 B: 2-way throughout -- hence the half planes.  The patch pass writes 16-B
// pieces at consecutive positions per lane: conflict-free.  The feature window is read at a
// stride of 6 floats between neighbouring positions of a residue: 2-way on b32 reads.
//
// Column split at d = 512: WIDE = eight waves side by side (one block, one patch per tile), or
// two column halves per tile (grid.y = 2, four waves each; each half rebuilds the patch).
#include "common.h"
#include "kernels.h"
#include "x6.h"

namespace wn {

namespace {

constexpr int CF = CONV2D6_F, CF1 = 39, CF2 = 12, CP3 = 13;

template <int FT> struct Geo {
  static constexpr int NFR = 3 * FT + 2;            // conv1 frames of the patch
  static constexpr int HALF = NFR * CF1 * 16;       // bytes of one channel half of a plane
  static constexpr int PLANE = 2 * HALF;
  static constexpr int XROWS = 2 * NFR + 1;         // feature rows of the tile's window
  static constexpr int LDS = 3 * PLANE + XROWS * CF * 4;
  static constexpr int RT = (FT * CF2 + 31) / 32;   // 32-row MFMA tiles
};

template <int D, int FT, int NW>
__global__ __launch_bounds__(NW * 64, (FT <= 5 && NW == 4) ? 2 : 1)
void conv2d6_patch_kernel(Conv2d6Args p) {
  using G = Geo<FT>;
  constexpr int RT = G::RT, HALF = G::HALF, PLANE = G::PLANE, NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) char smem_6[];
  float* xs = reinterpret_cast<float*>(smem_6 + 3 * PLANE);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;

  const int4 tl = p.tiles[blockIdx.x];
  const int u = tl.x, t0 = tl.y, n = min(tl.z, FT);
  const int nfr = 3 * n + 2;
  const int col0 = blockIdx.y * (NW * 64);          // first output channel of this block

  // the tile's feature window, CMVN applied (GlobalCMVN: (x - mean) * istd)
  {
    const float* src = p.feats + ((int64_t)u * p.T + 6 * t0) * CF;
    const int nx = (2 * nfr + 1) * CF;
    for (int i = tid; i < nx; i += NT) {
      float v = src[i];
      if (p.mean) {
        const int f = i % CF;
        v = (v - p.mean[f]) * p.istd[f];
      }
      xs[i] = v;
    }
  }
  // byte offset (inside a plane) of the base piece of this lane's row in each A tile
  int pixb[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int row = i * 32 + li;
    const int fl = min(row / CF2, FT - 1), f2 = row % CF2;
    pixb[i] = hi * HALF + (3 * fl * CF1 + f2) * 16;
  }

  struct FA { bf16x8 p[3]; };
  struct FB { bf16x8 p[2][3]; };
  constexpr int NTILE = D / 32;                     // 32-column tiles of the weight image
  const char* wp = reinterpret_cast<const char*>(p.W3) +
                   (int64_t)(col0 / 32 + wn * 2) * X3_TILE + lane * 16;
  auto loadW = [&](int kb) {
    const char* q = wp + (int64_t)kb * (NTILE * X3_TILE);
    FB f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        f.p[j][pl] = *reinterpret_cast<const bf16x8*>(q + j * X3_TILE + pl * X3_REC);
    return f;
  };
  auto loadA = [&](int delta, int i) {
    const char* q = smem_6 + pixb[i] + delta;
    FA f;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) f.p[pl] = *reinterpret_cast<const bf16x8*>(q + pl * PLANE);
    return f;
  };

  f32x16 acc[RT][2];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the patch of channel chunk c: wave w computes the channel half w & 1 (its 72 weights + 8
  // biases are wave-uniform) of the pixels (w >> 1) * 64 + lane + (NW / 2) * 64 j
  const int half = wn & 1;
  const int npix = nfr * CF1;
  auto patch = [&](int c) {
    const int ch = c * 16 + half * 8;
    float w[9][8], bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = p.b1[ch + e];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) w[k][e] = p.w1[k * D + ch + e];
    for (int px = (wn >> 1) * 64 + lane; px < npix; px += (NW / 2) * 64) {
      const int slot = px / CF1, pos = px - slot * CF1;
      const int res = pos / CP3;
      const int f1 = 3 * (pos - res * CP3) + res;
      const float* src = xs + (2 * slot) * CF + 2 * f1;
      float a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = bias[e];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float x = src[ky * CF + kx];
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(w[ky * 3 + kx][e], x, a[e]);
        }
      bf16x8 p0, p1, p2;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const Split3 sp = split3(fmaxf(a[e], 0.f));
        p0[e] = sp.h0; p1[e] = sp.h1; p2[e] = sp.h2;
      }
      char* o = smem_6 + half * HALF + px * 16;
      *reinterpret_cast<bf16x8*>(o) = p0;
      *reinterpret_cast<bf16x8*>(o + PLANE) = p1;
      *reinterpret_cast<bf16x8*>(o + 2 * PLANE) = p2;
    }
  };

  // six plane products in gemm_x6_kernel's order (the small ones first); W fragment = MFMA "A":
  // a lane owns one row of C
  auto mma = [&](const FA& a, const FB& b, int i) {
    constexpr int PB[6] = {2, 0, 1, 1, 0, 0}, PA[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b.p[j][PB[q]], a.p[PA[q]], acc[i][j],
                                                            0, 0, 0);
  };

  constexpr int NCH = D / 16, NKB = 25 * NCH;
  FB fb = loadW(0);
  for (int c = 0; c < NCH; ++c) {
    __syncthreads();            // the feature window is there / chunk c - 1's patch has been read
    patch(c);
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 25; ++tap) {
      const int ky = tap / 5, kx = tap % 5;
      const int delta = (ky * CF1 + (kx % 3) * CP3 + kx / 3) * 16;
      const FB nb = loadW(min(c * 25 + tap + 1, NKB - 1));
      FA fa = loadA(delta, 0);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        FA na;
        if (i + 1 < RT) na = loadA(delta, i + 1);
        mma(fa, fb, i);
        if (i + 1 < RT) fa = na;
      }
      fb = nb;
    }
  }

  // epilogue: lane = row of C, registers = columns 8 g + 4 hi + e of the 32-column tile
  float* cbase = p.C + (int64_t)tl.w * CF2 * p.ldc;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cb = col0 + (wn * 2 + j) * 32;
    f32x4 bias4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      bias4[g] = *reinterpret_cast<const f32x4*>(p.bias + cb + 8 * g + 4 * hi);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int row = i * 32 + li;
      if (row >= n * CF2) continue;
      float* crow = cbase + (int64_t)row * p.ldc;
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

template <int D, int FT, int NW>
int launch(const Conv2d6Args& a, hipStream_t s) {
  auto kern = conv2d6_patch_kernel<D, FT, NW>;
  WN_MAX_DYN_LDS(kern, Geo<FT>::LDS);
  hipLaunchKernelGGL(kern, dim3(a.n_tiles, D / (NW * 64)), dim3(NW * 64), Geo<FT>::LDS, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int conv2d6_frames(int L) { return L >= 11 ? ((L - 1) / 2 - 2) / 3 : 0; }

int conv2d6_ft(int ft, int d) {
  if (ft == 5 || ft == 8 || ft == 10) return ft;
  return d == 256 ? CONV2D6_FT_256 : CONV2D6_FT;
}

// (utterance, first output frame, frame count, packed first frame) per tile of `ft` frames
void conv2d6_tiles(const std::vector<int>& off2, const std::vector<int>& len2, int ft,
                   std::vector<int>* tiles) {
  tiles->clear();
  for (size_t b = 0; b < len2.size(); ++b)
    for (int t0 = 0; t0 < len2[b]; t0 += ft) {
      tiles->push_back((int)b);
      tiles->push_back(t0);
      tiles->push_back(std::min(ft, len2[b] - t0));
      tiles->push_back(off2[b] + t0);
    }
}

int conv2d6_patch(const Conv2d6Args& a, hipStream_t s) {
  WN_CHECK(a.feats && a.w1 && a.b1 && a.W3 && a.bias && a.tiles && a.C,
           "conv2d6_patch: null argument");
  WN_CHECK(a.F == CF, "conv2d6_patch: feature width (F = 80)");
  WN_CHECK(a.d == 256 || a.d == 512, "conv2d6_patch: d (256 or 512)");
  WN_CHECK(a.ft == 5 || a.ft == 8 || a.ft == 10, "conv2d6_patch: ft (5, 8 or 10)");
  WN_CHECK(a.n_tiles > 0 && a.n_tiles < (1 << 24), "conv2d6_patch: n_tiles");
  WN_CHECK(a.ldc >= a.d && a.ldc % 4 == 0 && ((uintptr_t)a.C & 15) == 0,
           "conv2d6_patch: ldc / alignment of C");
  WN_CHECK(a.T >= 11 && (int64_t)a.B * a.T < ((int64_t)1 << 31), "conv2d6_patch: feature rows");
  // (at ft 10 the eight-wave form's 128 accumulators + two weight fragments do not fit 256
  // registers without spilling: not built, ft 10 runs as two column halves)
  const bool wide = a.d == 512 && (a.wide ? a.wide : CONV2D6_WIDE) == 2 && a.ft != 10;
  if (a.d == 256) {
    if (a.ft == 5) return launch<256, 5, 4>(a, s);
    if (a.ft == 8) return launch<256, 8, 4>(a, s);
    return launch<256, 10, 4>(a, s);
  }
  if (wide) {
    if (a.ft == 5) return launch<512, 5, 8>(a, s);
    return launch<512, 8, 8>(a, s);
  }
  if (a.ft == 5) return launch<512, 5, 4>(a, s);
  if (a.ft == 8) return launch<512, 8, 4>(a, s);
  return launch<512, 10, 4>(a, s);
}

}  // namespace wn
