// fp32 rel-pos self attention for ENCODER heads of d_k = 32: the E-Branchformer recipe (8 heads at
// 256) and the plain layers of the Efficient Conformer recipes.  The score is the reference's
// rel-pos attention without the shift, as attention_kernel (encoder_kernels.hip) computes it at 64:
//     ((q_i + u) . k_j + (q_i + v) . p_j) * scale,   p_j = row j of P, u / v = bias_u / bias_v [h][32]
// in the FOLDED form of attention_grouped and ATTN_FOLD:
//     q_i . (k_j + p_j)  +  (u . k_j + v . p_j)  =  q_i . k'_j + kb_j
// The threads that stage a key tile write k' = k + p into the K tile and the per-key scalar kb
// into a 32-float strip behind the tile: eight consecutive lanes hold the eight float4 of one
// 32-wide row, three cross-lane steps finish the dot, the lane of column quad 0 stores it.  The
// score tile is then ONE contraction, S^T = K' Q^T, 16 steps of v_mfma_f32_32x32x2_f32 over the 32
// dimensions (two contractions would be 32), and the softmax input is (s + kb) * scale.  The fold
// holds the project's tolerance in every data regime of the operator test
// (tests/test_gpu_attention_d32_relpos.py); the two-contraction form is not built.
//
// Work split.  A block is NW waves (2, or 4 for long sequences: attention_d32_relpos picks by
// max_q_len against ATTN_D32_RELPOS_NW4_LEN); wave w owns the 32 query rows q0 + 32 w .. of one
// (sequence, head), and all waves share each 32-key tile K' | V | kb, staged global -> registers ->
// LDS one tile ahead: two buffers of 2 x 32 x 36 + 32 floats (18.7 KB), one barrier per tile, the
// next tile's loads in flight under this tile's 32 MFMAs.  A wave whose 32 rows lie past the
// sequence's end only stages and meets the barriers (attention_d128_kernel).  Softmax and output
// are attention_d32_kernel's: lane l holds, for ITS query (l & 31), the 16 keys
// (r&3)+8(r>>2)+4(l>>5); 15 in-lane operations and one exchange with lane^32 give the maximum and
// the sum; the probabilities are already the A operand of the P.V MFMAs, ONE 32 x 32 accumulator.
// No score tensor reaches HBM.
//
// Masks.  mask_mode 0: keys < kv_len.  mask_mode 2: the chunk window of attention_kernel's mode 2
// -- query i, c = i / chunk_size, sees keys [max((c - left_chunks) * chunk_size, 0) (left_chunks
// < 0: 0), min(kv_len, (c + 1) * chunk_size)).  A block visits only the key tiles its queries'
// windows touch: from the tile of its FIRST query row's window start to the tile of its last LIVE
// query row's window end; a lane masks inside the tile.  Rows past the sequence's end repeat the
// sequence's own last row while staging (never a neighbour's) and are masked.
//
// LDS banks (64 banks of 4 bytes; a wave's access is served in fixed lane groups, and only the
// lanes of one group can conflict), row stride KSTR = 36 floats -- the argument of attention_d32.hip
// carries over for the tiles, whatever NW (every wave reads the same tile at the same addresses):
//  * K' fragment, ds_read_b128 at dword li * 36 + hi * 4 + kk * 8: a group of 16 lanes holds one hi
//    and 16 values of li that cover every residue mod 16; 36 li mod 64 = 4 (9 li mod 16), 9 odd:
//    the 16 lanes start at the 16 different multiples of 4, their four-bank spans tile the 64 banks.
//  * V operand, ds_read_b32 at dword key * 36 + li: a group of 32 lanes is one hi, one key row, 32
//    consecutive dwords.
//  * staging stores, ds_write_b128: 8 consecutive threads hold the 8 float4 of ONE row, 32
//    consecutive dwords.
//  * kb strip (dwords 2304 .. 2335 of a buffer; 2304 mod 64 = 0).  Read: ds_read_b128 at dword
//    8 g + 4 hi, g = 0..3 -- every lane of a group has ONE hi, hence one address: a broadcast, no
//    conflict (the wave touches two addresses, banks 8 g .. 8 g + 3 and 8 g + 4 .. 8 g + 7).
//    Write: ds_write_b32 from the lanes of column quad 0, one lane in eight; a wave's eight writers
//    hold eight CONSECUTIVE rows (r = c >> 3), eight consecutive dwords: conflict free.
//
// mask_mode 1, kbias, p_off, block lists and the bf16 flags are refused by name.  scale is a
// multiplier (1 / sqrt(32) from the encoders; the reference divides by math.sqrt(d_k) -- one
// rounding apart, inside the tolerance of the operator tests).
#include "kernels.h"

namespace wn {

namespace {

constexpr int KT = 32;          // keys per tile
constexpr int DK = 32;
constexpr int KSTR = DK + 4;    // LDS row stride (floats)
constexpr int MAT = KT * KSTR;
constexpr int BUF = 2 * MAT + KT;   // K' | V | kb

template <int NW>
__global__ __launch_bounds__(NW * 64) void attention_d32_relpos_kernel(AttnArgs a) {
  constexpr int NTHR = NW * 64;
  constexpr int NCH = KT * (DK / 4) / NTHR;   // float4 chunks per thread and matrix
  const int s = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (NW * 32);
  const int len = a.q_len[s];
  if (q0 >= len) return;
  const int off = a.q_off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;

  __shared__ __attribute__((aligned(16))) float stile[2 * BUF];

  // ---- this lane's query row ------------------------------------------------------------
  const int qi = q0 + wave * 32 + li;
  const int qc = qi < len ? qi : len - 1;
  f32x4 qr[DK / 8];
  {
    const float* qp = a.Q + (int64_t)(off + qc) * a.ldq + h * DK + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 8; ++kk) qr[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
  }
  // key window of this query [jmin, jmax) and of the whole block [blo, bhi) (uniform)
  int jmin = 0, jmax = len, blo = 0, bhi = len;
  if (a.mask_mode == 2) {
    const int c = qi / a.chunk_size;
    const int qlast = min(q0 + NW * 32, len) - 1;
    jmax = min(len, (c + 1) * a.chunk_size);
    bhi = min(len, (qlast / a.chunk_size + 1) * a.chunk_size);
    if (a.left_chunks >= 0) {
      jmin = max((c - a.left_chunks) * a.chunk_size, 0);
      blo = max((q0 / a.chunk_size - a.left_chunks) * a.chunk_size, 0);
    }
  }
  const int t_lo = blo / KT, n_it = (bhi + KT - 1) / KT - t_lo;
  const bool wave_live = q0 + wave * 32 < len;

  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  // ---- tile staging with the fold.  NTHR is a multiple of 8: a thread's column quad never changes
  const int c4 = tid & 7;
  const f32x4 fu = *reinterpret_cast<const f32x4*>(a.bias_u + h * DK + c4 * 4);
  const f32x4 fv = *reinterpret_cast<const f32x4*>(a.bias_v + h * DK + c4 * 4);
  f32x4 rK[NCH], rV[NCH];
  float rC[NCH];
  auto gload = [&](int it) {
    f32x4 rP[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int j = (t_lo + it) * KT + ((tid + i * NTHR) >> 3);
      if (j > len - 1) j = len - 1;
      const int64_t grow = off + j;
      rK[i] = *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * DK + c4 * 4);
      rV[i] = *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * DK + c4 * 4);
      rP[i] = *reinterpret_cast<const f32x4*>(a.P + (int64_t)j * a.ldp + h * DK + c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const f32x4 k = rK[i], p = rP[i];
      float d = fu[0] * k[0] + fu[1] * k[1] + fu[2] * k[2] + fu[3] * k[3] +
                fv[0] * p[0] + fv[1] * p[1] + fv[2] * p[2] + fv[3] * p[3];
#pragma unroll
      for (int x = 4; x > 0; x >>= 1) d += __shfl_xor(d, x, 64);
      rC[i] = d;
      rK[i] = k + p;
    }
  };
  auto lstore = [&](int buf) {
    float* base = stile + buf * BUF;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int r = (tid + i * NTHR) >> 3;
      *reinterpret_cast<f32x4*>(base + r * KSTR + c4 * 4) = rK[i];
      *reinterpret_cast<f32x4*>(base + MAT + r * KSTR + c4 * 4) = rV[i];
      if (c4 == 0) base[2 * MAT + r] = rC[i];
    }
  };
  if (n_it > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();

  for (int it = 0; it < n_it; ++it) {
    const int j0 = (t_lo + it) * KT;
    const int cur = it & 1;
    const float* sK = stile + cur * BUF;
    const float* sV = sK + MAT;
    const float* sB = sK + 2 * MAT;
    if (it + 1 < n_it) gload(it + 1);

    if (wave_live) {
      // ---- S^T tile = K' Q^T ---------------------------------------------------------------
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
      const float* kf = sK + li * KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < DK / 8; ++kk) {
        const f32x4 fk = *reinterpret_cast<const f32x4*>(kf + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[t], qr[kk][t], sc, 0, 0, 0);
      }
      // ---- online softmax on this lane's query: keys 8 g + 4 hi + t, register 4 g + t ---------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 kb = *reinterpret_cast<const f32x4*>(sB + 8 * g + 4 * hi);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int r = 4 * g + t;
          const int j = j0 + 8 * g + 4 * hi + t;
          ok[r] = (j >= jmin) && (j < jmax);
          sc[r] = (sc[r] + kb[t]) * a.scale;
          if (ok[r]) tmax = fmaxf(tmax, sc[r]);
        }
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
        for (int r = 0; r < 16; ++r) o[r] *= __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
      }
      // ---- O += P V ---------------------------------------------------------------------------
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float v = sV[((st & 3) + 8 * (st >> 2) + 4 * hi) * KSTR + li];
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v, o, 0, 0, 0);
      }
    }
    if (it + 1 < n_it) lstore(cur ^ 1);
    __syncthreads();   // the next tile is visible, this buffer is free
  }
  if (!wave_live) return;
  // ---- normalise and store ------------------------------------------------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // no key -> 0
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qq, 64);
    const int qrow = q0 + wave * 32 + qq;
    if (qrow < len) a.O[(int64_t)(off + qrow) * a.ldo + h * DK + li] = o[r] * ir;
  }
}

}  // namespace

int attention_d32_relpos(const AttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.O && a.P && a.bias_u && a.bias_v && a.q_off && a.q_len,
           "attention_d32_relpos: null argument");
  WN_CHECK(a.kv_off == a.q_off && a.kv_len == a.q_len,
           "attention_d32_relpos: self attention only (kv_off / kv_len must be q_off / q_len)");
  WN_CHECK(a.mask_mode == 0 || a.mask_mode == 2,
           "attention_d32_relpos: mask_mode must be 0 (keys < kv_len) or 2 (chunk window), not 1 "
           "(causal)");
  WN_CHECK(a.mask_mode != 2 || a.chunk_size > 0,
           "attention_d32_relpos: chunk_size must be positive under mask_mode 2");
  WN_CHECK(!a.kbias && !a.fold, "attention_d32_relpos: no kbias (the fold is done while staging)");
  WN_CHECK(!a.p_off, "attention_d32_relpos: no p_off");
  WN_CHECK(!a.blk_tab && a.xcd_nqb == 0, "attention_d32_relpos: no block list");
  WN_CHECK(!a.o_bf16 && !a.qkv_bf16, "attention_d32_relpos: fp32 only, no bf16 flags");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 32768 && a.n_heads > 0 && a.n_heads < 256,
           "attention_d32_relpos: n_seq / n_heads");
  const int d = a.n_heads * DK;
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.ldp % 4 == 0,
           "attention_d32_relpos: strides % 4");
  WN_CHECK(a.ldq >= d && a.ldk >= d && a.ldv >= d && a.ldo >= d && a.ldp >= d,
           "attention_d32_relpos: a stride is smaller than n_heads * 32");
  WN_CHECK(a.max_q_len > 0, "attention_d32_relpos: empty");
  WN_CHECK(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0 &&
               ((uintptr_t)a.P & 15) == 0 && ((uintptr_t)a.bias_u & 15) == 0 &&
               ((uintptr_t)a.bias_v & 15) == 0,
           "attention_d32_relpos: Q, K, V, P, bias_u and bias_v must be 16-byte aligned");
  if (a.max_q_len >= ATTN_D32_RELPOS_NW4_LEN) {
    dim3 g(cdiv(a.max_q_len, 128), a.n_heads, a.n_seq), t(256);
    hipLaunchKernelGGL(attention_d32_relpos_kernel<4>, g, t, 0, s, a);
  } else {
    dim3 g(cdiv(a.max_q_len, 64), a.n_heads, a.n_seq), t(128);
    hipLaunchKernelGGL(attention_d32_relpos_kernel<2>, g, t, 0, s, a);
  }
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
