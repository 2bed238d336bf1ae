// fp32 attention for heads of d_k = 128 (the Paraformer's SANM encoder and decoder: 4 heads at
// d_model 512).  The design of attention_kernel (encoder_kernels.hip) at twice the head width:
// per 32-key tile the TRANSPOSED score tile S^T = K Q^T on v_mfma_f32_32x32x2_f32, so that lane l
// holds, for ITS query (l & 31), the 16 keys (r&3)+8(r>>2)+4(l>>5); online softmax with 15 in-lane
// operations and one exchange with lane^32; the probabilities are already the A operand of the
// P.V MFMAs.  No (T x T) tensor reaches HBM.  A head of 128 cannot be run as two heads of 64: the
// softmax is over the whole dot product.
//
// What doubles: 16 Q quads per lane (64 VGPRs) and four 32-column output tiles (64 accumulator
// registers), 64 + 64 MFMAs per key tile.  A 32-key K + V tile pair is 2 x 32 x 132 floats =
// 33.8 KB, so double buffering would pass the 64 KB of static LDS.  This kernel SINGLE-buffers
// (two barriers per tile, as the key-split form of attention_kernel does) and leaves the latency
// to the other resident blocks: 33.8 KB lets four blocks of two waves share a CU, two waves per
// SIMD at <= 256 VGPRs.  The alternative, 67.6 KB of dynamic LDS, halves the blocks per CU for a
// prefetch whose 64 extra VGPRs this kernel does not have.
//
// Q and K / V have separate offsets and lengths: the encoder's self attention and the decoder's
// cross attention (q_len = tokens, kv_len = frames) are the same kernel.  mask_mode 0 only, no
// position term.  The score is (q . k) * scale; the reference's decoder scales q before the
// product (paraformer/attention.py, MultiHeadedAttentionCrossAtt) -- one rounding of each q
// element against one of the sum, inside the tolerance of the operator tests.
#include "kernels.h"

namespace wn {

namespace {

constexpr int KT = 32;          // keys per tile
constexpr int DK = 128;
constexpr int KSTR = DK + 4;    // LDS row stride (floats): consecutive rows one 16-byte slot apart
constexpr int NW = 2;           // waves = 32-query groups per block
constexpr int NTHR = NW * 64;
constexpr int NCH = KT * (DK / 4) / NTHR;   // float4 chunks per thread and matrix

__global__ __launch_bounds__(NTHR, 2) void attention_d128_kernel(AttnArgs a) {
  const int s = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (NW * 32);
  const int qlen = a.q_len[s];
  if (q0 >= qlen) return;
  const int kvlen = a.kv_len[s];
  const int qoff = a.q_off[s], kvoff = a.kv_off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;

  __shared__ __attribute__((aligned(16))) float stile[2 * KT * KSTR];
  float* sK = stile;
  float* sV = stile + KT * KSTR;

  // ---- this lane's query row ------------------------------------------------------------
  const int qi = q0 + wave * 32 + li;
  const int qc = qi < qlen ? qi : qlen - 1;
  f32x4 qu[DK / 8];
  {
    const float* qp = a.Q + (int64_t)(qoff + qc) * a.ldq + h * DK + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 8; ++kk) qu[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
  }
  const int n_it = (kvlen + KT - 1) / KT;    // kvlen <= 0: no tile, the rows are written as zeros

  f32x16 o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[c][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  // (a query group past the sequence's end only stages and meets the barriers)
  const bool wave_live = q0 + wave * 32 < qlen;

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * KT;
    // ---- stage the tile: global -> registers -> LDS; rows past the sequence's end repeat its
    // last row (never a neighbour's) and are masked below
    f32x4 rK[NCH], rV[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * NTHR;
      const int r = c >> 5, c4 = c & 31;
      int j = j0 + r;
      if (j > kvlen - 1) j = kvlen - 1;
      const int64_t grow = kvoff + j;
      rK[i] = *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * DK + c4 * 4);
      rV[i] = *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * DK + c4 * 4);
    }
    __syncthreads();   // every wave is done with the previous tile
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * NTHR;
      const int r = c >> 5, c4 = c & 31;
      *reinterpret_cast<f32x4*>(sK + r * KSTR + c4 * 4) = rK[i];
      *reinterpret_cast<f32x4*>(sV + r * KSTR + c4 * 4) = rV[i];
    }
    __syncthreads();   // the tile is visible

    if (wave_live) {
      // ---- S^T tile ---------------------------------------------------------------------
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
      const float* kf = sK + li * KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < DK / 8; ++kk) {
        const f32x4 fk = *reinterpret_cast<const f32x4*>(kf + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[t], qu[kk][t], sc, 0, 0, 0);
      }
      // ---- online softmax on this lane's query --------------------------------------------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        ok[r] = j < kvlen;
        sc[r] *= a.scale;
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
          for (int c = 0; c < 4; ++c) o[c][r] *= ar;
        }
      }
      // ---- O += P V -------------------------------------------------------------------------
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float* vr = sV + ((st & 3) + 8 * (st >> 2) + 4 * hi) * KSTR + li;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], vr[32 * c], o[c], 0, 0, 0);
      }
    }
  }
  if (!wave_live) return;
  // ---- normalise and store ------------------------------------------------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // no key -> 0
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qr, 64);
    const int qrow = q0 + wave * 32 + qr;
    if (qrow < qlen) {
      float* op = a.O + (int64_t)(qoff + qrow) * a.ldo + h * DK;
#pragma unroll
      for (int c = 0; c < 4; ++c) op[32 * c + li] = o[c][r] * ir;
    }
  }
}

}  // namespace

int attention_d128(const AttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.O && a.q_off && a.q_len && a.kv_off && a.kv_len,
           "attention_d128: null argument");
  WN_CHECK(a.mask_mode == 0 && !a.P && !a.kbias && !a.bias_u && !a.bias_v,
           "attention_d128: full context without a position term only");
  WN_CHECK(!a.o_bf16 && !a.qkv_bf16, "attention_d128: fp32 only");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 32768 && a.n_heads > 0 && a.n_heads < 256,
           "attention_d128: n_seq / n_heads");
  const int d = a.n_heads * DK;
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0, "attention_d128: strides % 4");
  WN_CHECK(a.ldq >= d && a.ldk >= d && a.ldv >= d && a.ldo >= d,
           "attention_d128: a stride is smaller than n_heads * 128");
  WN_CHECK(a.max_q_len > 0, "attention_d128: empty");
  WN_CHECK(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0,
           "attention_d128: Q, K and V must be 16-byte aligned");
  dim3 g(cdiv(a.max_q_len, NW * 32), a.n_heads, a.n_seq), t(NTHR);
  hipLaunchKernelGGL(attention_d128_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
