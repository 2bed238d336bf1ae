// Efficient Conformer encoder kernels (wenet/models/efficient_conformer/), fp32, untuned:
//   attention_grouped      GroupedRelPositionMultiHeadedAttention (attention.py:83-126, 180-258):
//                          heads of W = group * d_k columns over GROUPS of `group` frames
//   stride_dwconv_ln_silu  the depthwise conv of a StrideConv module (convolution.py:64-72,
//                          141-146) with stride 2, its norm and swish
//   avgpool_residual_add   the stride layer's residual: AvgPool1d(2, 2, ceil_mode,
//                          count_include_pad=False) over time (encoder_layer.py:138-148)
#include <algorithm>

#include "kernels.h"

namespace wn {

namespace {

// ===========================================================================
// Grouped attention.  pad4group reads the (T, D) matrix of an utterance, zero frames appended up
// to a multiple of g, as (ceil(T / g), h, W): head hh of group row r is flat elements
// [hh W, (hh + 1) W) of the g D floats of frames g r .. g r + g - 1.  Element e of a group row is
// frame g r + e / D, column e % D; a float4 never straddles a frame (D % 4 == 0).  Every operand
// is read in place through that view, frames >= the utterance's own length as zeros (never the
// neighbour's rows of the packed buffer, never table rows the utterance alone would not have).
//
// The layout of attention_d128_kernel at W = 96 / 192: NW waves of 32 query groups, 32-key-group
// tiles, S^T = KP Q^T on v_mfma_f32_32x32x2_f32 (lane l holds, for ITS query l & 31, the 16 keys
// (r&3) + 8(r>>2) + 4(l>>5)), online softmax in the lane, the probabilities as the A operand of
// the P.V MFMAs.  No (T x T) tensor reaches HBM.
//
// The FOLDED form of the score: there is no rel-shift, so key s meets one table row, its own:
//     (q + u) . k_s + (q + v) . p_s = q . (k_s + p_s) + (u . k_s + v . p_s)
// One W-deep contraction per score tile instead of two, W / 8 Q quads per lane instead of W / 4
// (at W = 192 the unfolded form's 192 Q registers beside 96 accumulators leave no room for the
// staging loads of a second wave per SIMD).  k + p is formed while the tile is staged; the per-key
// term is summed in a FIXED order -- one partial per staged float4 in LDS, W / 8 of them per lane
// half, then the other half's -- so a result does not depend on the batch around it.
//
// LDS: KP and V tiles 32 x (W + 4) floats, the partials 32 x (W / 4 + 1): 56.4 KB at W = 192,
// 28.8 KB at W = 96, single buffered as attention_d128.  Row pitch W + 4: 196 = 4 (mod 64), one
// 16-byte slot per row like d128's 132; 100 = 36 (mod 64), slot 9 r (mod 16), a bijection over 16
// consecutive rows, so the ds_read_b128 of 16 key rows at one k offset meets 16 slots.  The
// partial rows' pitch is odd: 32 lanes, 32 banks.  Nothing here has been measured beyond one
// timing (tools/bench_efficonformer.py).
constexpr int GA_KT = 32;        // key groups per tile
constexpr int GA_NW = 2;         // waves = 32-query-group blocks per workgroup
constexpr int GA_NTHR = GA_NW * 64;

template <int W>
__global__ __launch_bounds__(GA_NTHR, 1) void attention_grouped_kernel(GroupedAttnArgs a) {
  constexpr int KSTR = W + 4;
  constexpr int W4 = W / 4;
  constexpr int CSTR = W4 + 1;
  constexpr int NT = W / 32;       // output column tiles
  const int s = blockIdx.z, hh = blockIdx.y;
  const int len = a.len[s];
  const int g = a.group, D = a.D;
  const int ng = (len + g - 1) / g;          // group rows: queries and keys alike
  const int q0 = blockIdx.x * (GA_NW * 32);
  if (q0 >= ng) return;
  const int off = a.off[s];
  const int poff = a.p_off ? a.p_off[s] : 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;

  __shared__ __attribute__((aligned(16))) float stile[2 * GA_KT * KSTR + GA_KT * CSTR];
  float* sKP = stile;
  float* sV = stile + GA_KT * KSTR;
  float* sC = stile + 2 * GA_KT * KSTR;

  // ---- this lane's query group row (frames >= len: zeros) --------------------------------
  const int qi = q0 + wave * 32 + li;
  f32x4 qu[W / 8];
#pragma unroll
  for (int kk = 0; kk < W / 8; ++kk) {
    const int e = hh * W + kk * 8 + hi * 4;
    const int fr = g * qi + e / D;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (fr < len) q = *reinterpret_cast<const f32x4*>(a.Q + (int64_t)(off + fr) * a.ldq + e % D);
    qu[kk] = q;
  }
  // the chunk window of this lane's query, in frames of the mask's own rate (mask_step frames per
  // group row): keys with lo <= m j < up
  const int m = a.mask_step;
  int up = 0x7fffffff, lo = -0x7fffffff;
  if (a.chunk_size > 0) {
    const int qc = (m * qi) / a.chunk_size;
    up = (qc + 1) * a.chunk_size;
    if (a.left_chunks >= 0) lo = (qc - a.left_chunks) * a.chunk_size;
  }
  // key groups any query of this workgroup may see (block-uniform)
  int n_key = ng;
  if (a.chunk_size > 0) {
    const int qmax = min(q0 + GA_NW * 32, ng) - 1;
    const int upmax = ((m * qmax) / a.chunk_size + 1) * a.chunk_size;
    n_key = min(ng, (upmax + m - 1) / m);
  }
  const int n_it = (n_key + GA_KT - 1) / GA_KT;

  f32x16 o[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[c][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const bool wave_live = q0 + wave * 32 < ng;   // (a dead wave only stages and meets barriers)

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * GA_KT;
    __syncthreads();   // every wave is done with the previous tile
    // ---- stage KP = K + P, V and the partials of u . k + v . p -----------------------------
#pragma unroll 2
    for (int c = tid; c < GA_KT * W4; c += GA_NTHR) {
      const int r = c / W4, c4 = c - r * W4;
      const int e = hh * W + c4 * 4;
      const int fr = g * (j0 + r) + e / D;
      const int col = e % D;
      f32x4 k = {0.f, 0.f, 0.f, 0.f}, p = k, v = k;
      if (fr < len) {
        k = *reinterpret_cast<const f32x4*>(a.K + (int64_t)(off + fr) * a.ldk + col);
        v = *reinterpret_cast<const f32x4*>(a.V + (int64_t)(off + fr) * a.ldv + col);
        p = *reinterpret_cast<const f32x4*>(a.P + (int64_t)(poff + fr) * a.ldp + col);
      }
      const f32x4 bu = *reinterpret_cast<const f32x4*>(a.bias_u + e);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias_v + e);
      float part = bu[0] * k[0];
      part = fmaf(bu[1], k[1], part);
      part = fmaf(bu[2], k[2], part);
      part = fmaf(bu[3], k[3], part);
      part = fmaf(bv[0], p[0], part);
      part = fmaf(bv[1], p[1], part);
      part = fmaf(bv[2], p[2], part);
      part = fmaf(bv[3], p[3], part);
      *reinterpret_cast<f32x4*>(sKP + r * KSTR + c4 * 4) = k + p;
      *reinterpret_cast<f32x4*>(sV + r * KSTR + c4 * 4) = v;
      sC[r * CSTR + c4] = part;
    }
    __syncthreads();   // the tile is visible

    if (wave_live) {
      // ---- the per-key term of key group li: this half's W / 8 partials, then the other's ----
      float ck = 0.f;
      {
        const float* cp = sC + li * CSTR + hi * (W4 / 2);
#pragma unroll
        for (int i = 0; i < W4 / 2; ++i) ck += cp[i];
        ck += __shfl_xor(ck, 32, 64);
      }
      // ---- S^T tile ------------------------------------------------------------------------
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
      const float* kf = sKP + li * KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < W / 8; ++kk) {
        const f32x4 fk = *reinterpret_cast<const f32x4*>(kf + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[t], qu[kk][t], sc, 0, 0, 0);
      }
      // ---- online softmax on this lane's query ---------------------------------------------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int j = j0 + kj;
        ok[r] = j < ng && m * j < up && m * j >= lo;
        sc[r] = (sc[r] + __shfl(ck, kj, 64)) * a.scale;
        if (ok[r]) tmax = fmaxf(tmax, sc[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __expf(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = ok[r] ? __expf(sc[r] - m_new) : 0.f;
        sc[r] = p;
        psum += p;
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
      // rescale the running output: its rows are queries (r&3)+8(r>>2)+4hi
      if (!__all(alpha == 1.0f)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
#pragma unroll
          for (int c = 0; c < NT; ++c) o[c][r] *= ar;
        }
      }
      // ---- O += P V ------------------------------------------------------------------------
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float* vr = sV + ((st & 3) + 8 * (st >> 2) + 4 * hi) * KSTR + li;
#pragma unroll
        for (int c = 0; c < NT; ++c)
          o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], vr[32 * c], o[c], 0, 0, 0);
      }
    }
  }
  if (!wave_live) return;
  // ---- normalise and store through the same view; frames >= len are not written -------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qr, 64);
    const int gq = q0 + wave * 32 + qr;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int e = hh * W + 32 * c + li;
      const int fr = g * gq + e / D;
      if (fr < len) a.O[(int64_t)(off + fr) * a.ldo + e % D] = o[c][r] * ir;
    }
  }
}

// ===========================================================================
// Strided depthwise conv + norm + SiLU.  Output frame t of utterance b reads input frames
// s t - pad + k, k < K, pad = (K - 1) / 2 or K - 1 (causal); frames >= len are zeros, frames < 0
// are zeros or, on a causal module with `cpad`, that vector (the reference pads the K - 1 causal
// frames in FRONT of pointwise_conv1 + GLU, convolution.py:117-119, so they reach the depthwise
// conv as the GLU of the bias).  A wave owns one output frame at a time, lane l the channels
// l + 64 i; the norm is a two-pass LayerNorm in registers (wave_sum), or the per-channel affine.
constexpr int SD_THREADS = 256;
constexpr int SD_FRAMES = 16;      // output frames per workgroup
constexpr int SD_MAXI = 8;         // D <= 512

__global__ __launch_bounds__(SD_THREADS) void stride_dwconv_kernel(StrideDwConvArgs a) {
  const int b = blockIdx.y;
  const int len = a.len[b];
  const int st = a.stride;
  const int len2 = (len + st - 1) / st;
  const int t0 = blockIdx.x * SD_FRAMES;
  if (t0 >= len2) return;
  const int row0 = a.off[b], orow0 = a.off2[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nI = a.D / 64;
  const int pad = a.causal ? a.K - 1 : (a.K - 1) / 2;
  const float invD = 1.0f / (float)a.D;
  for (int t = t0 + wave; t < min(t0 + SD_FRAMES, len2); t += SD_THREADS / 64) {
    float acc[SD_MAXI];
#pragma unroll
    for (int i = 0; i < SD_MAXI; ++i) acc[i] = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const int src = st * t - pad + k;
      if (src >= len) break;
      if (src < 0 && !(a.causal && a.cpad)) continue;
#pragma unroll
      for (int i = 0; i < SD_MAXI; ++i) {
        if (i < nI) {
          const int c = lane + 64 * i;
          const float v = src < 0 ? a.cpad[c] : a.x[(int64_t)(row0 + src) * a.ldx + c];
          acc[i] = fmaf(a.wt[(int64_t)k * a.D + c], v, acc[i]);
        }
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SD_MAXI; ++i)
      if (i < nI) { acc[i] += a.bias[lane + 64 * i]; sum += acc[i]; }
    float mean = 0.f, rstd = 1.f;
    if (a.norm_mode == 0) {
      mean = wave_sum(sum) * invD;
      float var = 0.f;
#pragma unroll
      for (int i = 0; i < SD_MAXI; ++i)
        if (i < nI) { const float dl = acc[i] - mean; var = fmaf(dl, dl, var); }
      rstd = rsqrtf(wave_sum(var) * invD + a.eps);
    }
#pragma unroll
    for (int i = 0; i < SD_MAXI; ++i) {
      if (i < nI) {
        const int c = lane + 64 * i;
        const float n = a.norm_mode == 0 ? (acc[i] - mean) * rstd * a.ln_w[c] + a.ln_b[c]
                                         : fmaf(acc[i], a.ln_w[c], a.ln_b[c]);
        a.y[(int64_t)(orow0 + t) * a.ldy + c] = silu_f(n);
      }
    }
  }
}

// y[off2[b] + t] = z[off2[b] + t] + mean(x[off[b] + s t .. min(s t + s, len) - 1]), s = 2: a full
// window is (a + b) * 0.5, the last window of an odd length the last frame itself.
__global__ __launch_bounds__(256) void avgpool_residual_kernel(AvgPoolResidArgs a) {
  const int b = blockIdx.y;
  const int len = a.len[b];
  const int len2 = (len + 1) / 2;
  const int C4 = a.C / 4;
  const int64_t n = (int64_t)len2 * C4;
  const int row0 = a.off[b], orow0 = a.off2[b];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / C4), c = (int)(i % C4) * 4;
    const float4 x0 = *reinterpret_cast<const float4*>(a.x + (int64_t)(row0 + 2 * t) * a.ldx + c);
    float4 p = x0;
    if (2 * t + 1 < len) {
      const float4 x1 =
          *reinterpret_cast<const float4*>(a.x + (int64_t)(row0 + 2 * t + 1) * a.ldx + c);
      p = make_float4((x0.x + x1.x) * 0.5f, (x0.y + x1.y) * 0.5f, (x0.z + x1.z) * 0.5f,
                      (x0.w + x1.w) * 0.5f);
    }
    const float4 z = *reinterpret_cast<const float4*>(a.z + (int64_t)(orow0 + t) * a.ldz + c);
    *reinterpret_cast<float4*>(a.y + (int64_t)(orow0 + t) * a.ldy + c) =
        make_float4(z.x + p.x, z.y + p.y, z.z + p.z, z.w + p.w);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int attention_grouped(const GroupedAttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.P && a.bias_u && a.bias_v && a.O && a.off && a.len,
           "attention_grouped: null argument");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 65536 && a.n_heads > 0 && a.n_heads < 65536 && a.max_len > 0,
           "attention_grouped: empty");
  WN_CHECK(a.group >= 1 && a.group <= 16, "attention_grouped: group must be in [1, 16]");
  WN_CHECK(a.width == 96 || a.width == 192,
           "attention_grouped: head width group * d_k = " + std::to_string(a.width) +
               " has no kernel (96 and 192 have)");
  WN_CHECK((a.n_heads * a.width) % a.group == 0 && a.D == a.n_heads * a.width / a.group &&
               a.D % 4 == 0,
           "attention_grouped: D must be n_heads * width / group, a multiple of 4");
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldp % 4 == 0,
           "attention_grouped: strides must be multiples of 4 floats");
  WN_CHECK(a.ldq >= a.D && a.ldk >= a.D && a.ldv >= a.D && a.ldp >= a.D && a.ldo >= a.D,
           "attention_grouped: a stride is smaller than D");
  WN_CHECK(aligned16(a.Q) && aligned16(a.K) && aligned16(a.V) && aligned16(a.P) &&
               aligned16(a.bias_u) && aligned16(a.bias_v),
           "attention_grouped: Q, K, V, P and the biases must be 16-byte aligned");
  WN_CHECK(a.mask_step >= 1 && a.chunk_size >= 0 && a.mask_step <= 4096 &&
               a.chunk_size <= (1 << 20) && a.max_len <= (1 << 18),
           "attention_grouped: mask_step / chunk_size / max_len");
  const int ng = cdiv(a.max_len, a.group);
  dim3 grid(cdiv(ng, GA_NW * 32), a.n_heads, a.n_seq), t(GA_NTHR);
  if (a.width == 96) hipLaunchKernelGGL(attention_grouped_kernel<96>, grid, t, 0, s, a);
  else hipLaunchKernelGGL(attention_grouped_kernel<192>, grid, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int stride_dwconv_ln_silu(const StrideDwConvArgs& a, hipStream_t s) {
  WN_CHECK(a.x && a.wt && a.bias && a.ln_w && a.ln_b && a.y && a.off && a.len && a.off2,
           "stride_dwconv_ln_silu: null argument");
  WN_CHECK(a.stride == 2, "stride_dwconv_ln_silu: stride = " + std::to_string(a.stride) +
                              " has no kernel (2 has)");
  WN_CHECK(a.D >= 64 && a.D % 64 == 0 && a.D <= 64 * SD_MAXI,
           "stride_dwconv_ln_silu: D must be a multiple of 64 up to 512");
  WN_CHECK(a.K >= 1 && a.K <= 63 && (a.causal || a.K % 2 == 1),
           "stride_dwconv_ln_silu: K must be in [1, 63], odd unless causal");
  WN_CHECK(a.norm_mode == 0 || a.norm_mode == 1, "stride_dwconv_ln_silu: norm_mode is 0 or 1");
  WN_CHECK(a.ldx >= a.D && a.ldy >= a.D, "stride_dwconv_ln_silu: a stride is smaller than D");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.max_len > 0, "stride_dwconv_ln_silu: empty batch");
  WN_CHECK(a.y != a.x, "stride_dwconv_ln_silu: not in place");
  const dim3 grid(cdiv(cdiv(a.max_len, a.stride), SD_FRAMES), a.B);
  hipLaunchKernelGGL(stride_dwconv_kernel, grid, dim3(SD_THREADS), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int avgpool_residual_add(const AvgPoolResidArgs& a, hipStream_t s) {
  WN_CHECK(a.x && a.z && a.y && a.off && a.len && a.off2, "avgpool_residual_add: null argument");
  WN_CHECK(a.stride == 2, "avgpool_residual_add: stride = " + std::to_string(a.stride) +
                              " has no kernel (2 has)");
  WN_CHECK(a.C >= 4 && a.C % 4 == 0, "avgpool_residual_add: channels must be a multiple of 4");
  WN_CHECK(a.ldx % 4 == 0 && a.ldz % 4 == 0 && a.ldy % 4 == 0 && a.ldx >= a.C && a.ldz >= a.C &&
               a.ldy >= a.C,
           "avgpool_residual_add: row strides must be multiples of 4 floats, at least C");
  WN_CHECK(aligned16(a.x) && aligned16(a.z) && aligned16(a.y),
           "avgpool_residual_add: buffers must be 16-byte aligned");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.max_len > 0, "avgpool_residual_add: empty batch");
  const int64_t n = (int64_t)((a.max_len + 1) / 2) * (a.C / 4);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 4096), a.B);
  hipLaunchKernelGGL(avgpool_residual_kernel, grid, dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
