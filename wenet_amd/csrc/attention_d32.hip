// fp32 attention for heads of d_k = 32: the decoders of the shipped Efficient Conformer recipes
// (bitransformer, 8 heads at d_model 256).  The design of attention_kernel (encoder_kernels.hip)
// at half the head width: per 32-key tile the TRANSPOSED score tile S^T = K Q^T on
// v_mfma_f32_32x32x2_f32 (16 steps over the 32 dimensions), so that lane l holds, for ITS query
// (l & 31), the 16 keys (r&3)+8(r>>2)+4(l>>5); online softmax with 15 in-lane operations and one
// exchange with lane^32; the probabilities are already the A operand of the P.V MFMAs, ONE
// 32 x 32 accumulator, 16 steps over the tile's 32 keys.  No score tensor reaches HBM.
//
// The decoder's work is small and latency bound (<= ~40 token rows per hypothesis, B x beam
// sequences), so a block is ONE wave: the 32 query rows of a (sequence, head).  K and V are
// staged global -> registers -> LDS one tile ahead (two buffers, 2 x 2 x 32 x 36 floats =
// 18.4 KB): the next tile's loads are in flight under this tile's 32 MFMAs.
//
// LDS banks (64 banks of 4 bytes; a wave's access is served in fixed lane groups, and only the
// lanes of one group can conflict), row stride KSTR = 36 floats:
//  * K fragment, ds_read_b128 at dword li * 36 + hi * 4 + kk * 8, four groups of 16 lanes, bank
//    = dword mod 64.  A group holds one hi and 16 values of li that cover every residue mod 16
//    ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}); 36 li mod 64 = 4 (9 li mod 16) and 9 is
//    odd, so the 16 lanes start at the 16 different multiples of 4 and their four-bank spans
//    tile the 64 banks: conflict free.  (A stride of 32 would put the 16 lanes on two spans:
//    8-way.)
//  * V operand, ds_read_b32 at dword key * 36 + li, two groups of 32 lanes, bank = dword mod 32:
//    a group is one hi, hence one key row and 32 consecutive dwords: conflict free.
//  * staging stores, ds_write_b128, eight groups of 8 consecutive lanes, bank = dword mod 32:
//    8 consecutive threads hold the 8 float4 of ONE row, 32 consecutive dwords: conflict free.
//
// mask_mode 0: keys < kv_len (cross attention).  mask_mode 1: causal, key j <= query i AND
// j < kv_len -- with kv_len < q_len (the padded batches of wn_decoder_forward) the keys at or
// past kv_len are hidden from every query, padded query rows included.  No position term, no
// kbias, no chunk window, no block list: the encoder layers that need them stay on the 64 kernel.
// The score is (q . k) * scale with scale = 1 / sqrt(32) as a multiplier; the reference divides
// by math.sqrt(d_k) -- one rounding apart, inside the tolerance of the operator tests.
#include "kernels.h"

namespace wn {

namespace {

constexpr int KT = 32;          // keys per tile
constexpr int DK = 32;
constexpr int KSTR = DK + 4;    // LDS row stride (floats): consecutive rows one 16-byte slot apart
constexpr int NTHR = 64;        // one wave = one 32-query group per block
constexpr int NCH = KT * (DK / 4) / NTHR;   // float4 chunks per thread and matrix
constexpr int MAT = KT * KSTR;

__global__ __launch_bounds__(NTHR) void attention_d32_kernel(AttnArgs a) {
  const int s = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 32;
  const int qlen = a.q_len[s];
  if (q0 >= qlen) return;
  const int kvlen = a.kv_len[s];
  const int qoff = a.q_off[s], kvoff = a.kv_off[s];
  const int lane = threadIdx.x;
  const int hi = lane >> 5, li = lane & 31;

  __shared__ __attribute__((aligned(16))) float stile[2 * 2 * MAT];   // [buffer][K | V]

  // ---- this lane's query row ------------------------------------------------------------
  const int qi = q0 + li;
  const int qc = qi < qlen ? qi : qlen - 1;
  f32x4 qu[DK / 8];
  {
    const float* qp = a.Q + (int64_t)(qoff + qc) * a.ldq + h * DK + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 8; ++kk) qu[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
  }
  // keys of this query: [0, jmax); of the block: [0, bhi)  (kvlen <= 0: no tile, zeros)
  const int jmax = a.mask_mode == 1 ? min(kvlen, qi + 1) : kvlen;
  const int bhi = a.mask_mode == 1 ? min(kvlen, min(q0 + 32, qlen)) : kvlen;
  const int n_it = (bhi + KT - 1) / KT;

  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  // ---- tile staging: rows past the sequence's end repeat its last row (never a neighbour's)
  // and are masked below
  f32x4 rK[NCH], rV[NCH];
  auto gload = [&](int it) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * NTHR;
      const int r = c >> 3, c4 = c & 7;
      int j = it * KT + r;
      if (j > kvlen - 1) j = kvlen - 1;
      const int64_t grow = kvoff + j;
      rK[i] = *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * DK + c4 * 4);
      rV[i] = *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * DK + c4 * 4);
    }
  };
  auto lstore = [&](int buf) {
    float* base = stile + buf * 2 * MAT;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * NTHR;
      const int r = c >> 3, c4 = c & 7;
      *reinterpret_cast<f32x4*>(base + r * KSTR + c4 * 4) = rK[i];
      *reinterpret_cast<f32x4*>(base + MAT + r * KSTR + c4 * 4) = rV[i];
    }
  };
  if (n_it > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * KT;
    const int cur = it & 1;
    const float* sK = stile + cur * 2 * MAT;
    const float* sV = sK + MAT;
    if (it + 1 < n_it) gload(it + 1);

    // ---- S^T tile -------------------------------------------------------------------------
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
    // ---- online softmax on this lane's query ------------------------------------------------
    float tmax = -1e30f;
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ok[r] = j < jmax;
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
      for (int r = 0; r < 16; ++r) o[r] *= __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
    }
    // ---- O += P V -----------------------------------------------------------------------------
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const float v = sV[((st & 3) + 8 * (st >> 2) + 4 * hi) * KSTR + li];
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v, o, 0, 0, 0);
    }
    if (it + 1 < n_it) lstore(cur ^ 1);
    __syncthreads();   // the next tile is visible, this buffer is free
  }
  // ---- normalise and store ------------------------------------------------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // no key -> 0
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qr, 64);
    const int qrow = q0 + qr;
    if (qrow < qlen) a.O[(int64_t)(qoff + qrow) * a.ldo + h * DK + li] = o[r] * ir;
  }
}

}  // namespace

int attention_d32(const AttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.O && a.q_off && a.q_len && a.kv_off && a.kv_len,
           "attention_d32: null argument");
  WN_CHECK(!a.P && !a.bias_u && !a.bias_v && !a.fold, "attention_d32: no position term");
  WN_CHECK(!a.kbias, "attention_d32: no kbias");
  WN_CHECK(a.mask_mode == 0 || a.mask_mode == 1,
           "attention_d32: mask_mode must be 0 (keys < kv_len) or 1 (causal), not 2 (chunk window)");
  WN_CHECK(!a.blk_tab && a.xcd_nqb == 0, "attention_d32: no block list");
  WN_CHECK(!a.o_bf16 && !a.qkv_bf16, "attention_d32: fp32 only");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 32768 && a.n_heads > 0 && a.n_heads < 256,
           "attention_d32: n_seq / n_heads");
  const int d = a.n_heads * DK;
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0,
           "attention_d32: strides % 4");
  WN_CHECK(a.ldq >= d && a.ldk >= d && a.ldv >= d && a.ldo >= d,
           "attention_d32: a stride is smaller than n_heads * 32");
  WN_CHECK(a.max_q_len > 0, "attention_d32: empty");
  WN_CHECK(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0,
           "attention_d32: Q, K and V must be 16-byte aligned");
  dim3 g(cdiv(a.max_q_len, 32), a.n_heads, a.n_seq), t(NTHR);
  hipLaunchKernelGGL(attention_d32_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
