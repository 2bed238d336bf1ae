// fp32 self attention with rotary position embedding and grouped key / value heads, d_k = 64: the
// attention of the rotary Conformer encoders (RopeMultiHeadedAttention, attention.py:599-686, with
// the MQA / GQA head sharing of MultiHeadedAttention._update_kv_and_cache)
//     score(i, j) = rot(q_i, i) . rot(k_j, j) * scale,    V is not rotated,
//     rot(x, t) = [x1 c_t - x2 s_t | x1 s_t + x2 c_t],  x1 = x[0:32], x2 = x[32:64]
// (google_apply_rotary_emb, rope_utils.py:18-26), c_t | s_t the 64 floats of row t of the table
// a.P [max_pos][ldp >= 64] (cos[32] | sin[32]), t the frame index inside the row's own sequence.
// n_heads query heads read n_kv_heads key / value heads, G = n_heads / n_kv_heads; query head h
// reads K / V head h / G (the reference's expand + reshape).  The rotation is fused: no rotated Q
// or K in HBM, no pass over the QKV buffer.
//
// Work split.  A block is four waves = GB heads x 4 / GB groups of 32 query rows, GB the largest of
// 4, 2, 1 that divides G: wave w is head sub-index w % GB, row group w / GB.  All four waves
// belong to ONE K / V head, so its 32-key tile K' | V is staged -- and K rotated -- once per block,
// not once per query head: a block of GB = 4 moves a quarter of the K / V bytes per query row of a
// block of GB = 1.  blockIdx = (row group of 128 / GB rows, kv head x head sub-group, sequence).
//
// Q: each lane holds its query row (lane & 31) as attention_shaw does, dims hi * 4 + kk * 8 .. + 3 in
// qr[kk]; the partner of a dim < 32 is dim + 32 = register kk + 4 of the SAME lane, so the rotation
// is eight float4 pairs in registers, once per wave, with the row's cos / sin read from the table.
//
// K: a staging thread (256 threads = 32 rows x 8) owns, for ONE key row, float4 chunk c (dims 4 c ..)
// AND chunk c + 8 (dims 32 + 4 c ..) plus the cos and sin float4 of that row's position: the
// rotation is lane-local, applied between the global load (one tile ahead, in flight under the
// MFMAs) and the LDS store, as attention_d32_relpos folds k + p.  Two buffers, one barrier per tile.
// S^T = K' Q^T in 32 steps of v_mfma_f32_32x32x2_f32, online softmax, O += P V on two 32 x 32
// accumulators: attention_shaw's.  No score tensor reaches HBM.
//
// Masks and edges.  Keys >= len are masked; rows past the sequence's end repeat the sequence's own
// last row (and its position) while staging.  A wave whose 32 rows lie past the end only stages and
// meets the barriers; a block past the end, and every block of a len = 0 sequence, returns at once
// and writes nothing.  mask_mode 2 is the chunk window of attention(): query i, c = i / chunk_size,
// sees keys [max((c - left_chunks) * chunk_size, 0) (left_chunks < 0: 0), min(len, (c + 1) *
// chunk_size)); a block visits only the tiles from its first row's window start to its last live
// row's window end, a lane masks inside the tile.
//
// LDS (static): two buffers of K' | V, 2 x 32 x 68 floats each: 34.0 KB, four blocks per CU's
// 160 KB.  The table never passes through LDS: a key row's cos | sin is read from global memory
// (L2: 256 contiguous bytes per octet of threads, the same rows for every head) into the staging
// thread's registers, a query row's into the lane's.
// Banks (64 banks of 4 bytes; a b128 access is served 16 lanes at a time):
//  * K' fragment, ds_read_b128 at dword li * 68 + hi * 4 + kk * 8: 68 li mod 64 = 4 li, the 16
//    lanes of a group start at the 16 different multiples of 4 -- their spans tile the 64 banks.
//  * V operand, ds_read_b32 at key * 68 + li (+ 32): a half wave reads 32 consecutive dwords.
//  * staging stores, ds_write_b128 at row * 68 + 4 c (then + 32): consecutive octets of threads hold
//    rows r and r + 8 (stage_row), 8 * 68 mod 64 = 32, so 16 lanes write [4 r, 4 r + 32) and
//    [4 r + 32, 4 r + 64): all 64 banks once.  (Rows r and r + 1 would overlap on 28 banks.)
// The compiler reports, for each of GB = 1, 2, 4: 148 VGPRs, no scratch, 34816 bytes of LDS, an
// occupancy of two waves per SIMD -- two blocks per CU by registers, where the LDS would take four.
// Untuned: the block shape was chosen for the K / V traffic, not by measurement.
//
// mask_mode 1, kbias, p_off, block lists and the bf16 flags are refused by name, as are n_heads %
// n_kv_heads != 0 and a sequence longer than the table.  scale is a multiplier (0.125 from the
// encoder; the reference divides by math.sqrt(d_k)).
#include "kernels.h"

namespace wn {

namespace {

constexpr int KT = 32;            // keys per tile
constexpr int DK = 64;
constexpr int KSTR = DK + 4;      // LDS row stride of the K' / V tiles (floats)
constexpr int MAT = KT * KSTR;
constexpr int BUF = 2 * MAT;      // K' | V
constexpr int NTHR = 256;         // four waves

// tile row of thread octet o (0 .. 31): neighbouring octets are 8 rows apart (banks, above)
__device__ __forceinline__ int stage_row(int o) { return (o & 1) * 8 + ((o >> 1) & 7) + (o >> 4) * 16; }

template <int GB>
__global__ __launch_bounds__(NTHR) void attention_rope_kernel(AttnArgs a, int G) {
  constexpr int RB = (4 / GB) * 32;   // query rows per block
  const int s = blockIdx.z;
  const int q0 = blockIdx.x * RB;
  const int len = a.q_len[s];
  if (q0 >= len) return;
  const int off = a.q_off[s];
  const int nsub = G / GB;
  const int kvh = blockIdx.y / nsub, sub = blockIdx.y - kvh * nsub;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  const int h = kvh * G + sub * GB + wave % GB;   // this wave's query head
  const int i0 = q0 + (wave / GB) * 32;           // ... and its first query row

  __shared__ __attribute__((aligned(16))) float stile[2 * BUF];

  // ---- this lane's query row, rotated by its own position -----------------------------------
  const int qi = i0 + li;
  const int qc = min(qi, len - 1);
  f32x4 qr[DK / 8];
  {
    const float* qp = a.Q + (int64_t)(off + qc) * a.ldq + h * DK + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 8; ++kk) qr[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
    const float* tp = a.P + (int64_t)qc * a.ldp + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 16; ++kk) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(tp + kk * 8);
      const f32x4 sn = *reinterpret_cast<const f32x4*>(tp + 32 + kk * 8);
      const f32x4 x1 = qr[kk], x2 = qr[kk + 4];
      qr[kk] = x1 * c - x2 * sn;
      qr[kk + 4] = x1 * sn + x2 * c;
    }
  }
  // key window of this query [jmin, jmax) and of the whole block [blo, bhi) (uniform)
  int jmin = 0, jmax = len, blo = 0, bhi = len;
  if (a.mask_mode == 2) {
    const int c = qi / a.chunk_size;
    const int qlast = min(q0 + RB, len) - 1;
    jmax = min(len, (c + 1) * a.chunk_size);
    bhi = min(len, (qlast / a.chunk_size + 1) * a.chunk_size);
    if (a.left_chunks >= 0) {
      jmin = max((c - a.left_chunks) * a.chunk_size, 0);
      blo = max((q0 / a.chunk_size - a.left_chunks) * a.chunk_size, 0);
    }
  }
  const int t_lo = blo / KT, n_it = (bhi + KT - 1) / KT - t_lo;
  const bool wave_live = i0 < len;

  // ---- K | V staging: thread -> (row stage_row(tid >> 3), chunks c4 and c4 + 8) ------------------
  const int c4 = tid & 7, srow = stage_row(tid >> 3);
  f32x4 rK1, rK2, rV1, rV2, rC, rS;
  auto gload = [&](int it) {
    const int j = min((t_lo + it) * KT + srow, len - 1);
    const int64_t grow = off + j;
    const float* kp = a.K + grow * a.ldk + kvh * DK + c4 * 4;
    const float* vp = a.V + grow * a.ldv + kvh * DK + c4 * 4;
    const float* tp = a.P + (int64_t)j * a.ldp + c4 * 4;
    rK1 = *reinterpret_cast<const f32x4*>(kp);
    rK2 = *reinterpret_cast<const f32x4*>(kp + 32);
    rV1 = *reinterpret_cast<const f32x4*>(vp);
    rV2 = *reinterpret_cast<const f32x4*>(vp + 32);
    rC = *reinterpret_cast<const f32x4*>(tp);
    rS = *reinterpret_cast<const f32x4*>(tp + 32);
  };
  auto lstore = [&](int buf) {   // the rotation sits here: behind the MFMAs the loads ran under
    float* base = stile + buf * BUF + srow * KSTR + c4 * 4;
    *reinterpret_cast<f32x4*>(base) = rK1 * rC - rK2 * rS;
    *reinterpret_cast<f32x4*>(base + 32) = rK1 * rS + rK2 * rC;
    *reinterpret_cast<f32x4*>(base + MAT) = rV1;
    *reinterpret_cast<f32x4*>(base + MAT + 32) = rV2;
  };
  gload(0);
  lstore(0);
  __syncthreads();

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  for (int it = 0; it < n_it; ++it) {
    const int j0 = (t_lo + it) * KT;
    const int cur = it & 1;
    const float* sK = stile + cur * BUF;
    const float* sV = sK + MAT;
    if (it + 1 < n_it) gload(it + 1);

    if (wave_live) {
      // ---- S^T tile = K' Q^T -------------------------------------------------------------------
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
      // ---- online softmax on this lane's query: key (r&3)+8(r>>2)+4hi in register r -------------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        ok[r] = (j >= jmin) && (j < jmax);
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
          o0[r] *= ar;
          o1[r] *= ar;
        }
      }
      // ---- O += P V -------------------------------------------------------------------------------
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int key = (st & 3) + 8 * (st >> 2) + 4 * hi;
        const float v0 = sV[key * KSTR + li];
        const float v1 = sV[key * KSTR + 32 + li];
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v0, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v1, o1, 0, 0, 0);
      }
    }
    if (it + 1 < n_it) lstore(cur ^ 1);
    __syncthreads();   // the next tile is visible, this buffer is free
  }
  if (!wave_live) return;
  // ---- normalise and store --------------------------------------------------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // no key -> 0
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qq = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qq, 64);
    const int qrow = i0 + qq;
    if (qrow < len) {
      float* op = a.O + (int64_t)(off + qrow) * a.ldo + h * DK;
      op[li] = o0[r] * ir;
      op[32 + li] = o1[r] * ir;
    }
  }
}

}  // namespace

int attention_rope(const RopeAttnArgs& ra, hipStream_t s) {
  const AttnArgs& a = ra.a;
  const int Hkv = ra.n_kv_heads > 0 ? ra.n_kv_heads : a.n_heads;
  WN_CHECK(a.Q && a.K && a.V && a.O && a.P && a.q_off && a.q_len,
           "attention_rope: null argument");
  WN_CHECK(a.kv_off == a.q_off && a.kv_len == a.q_len,
           "attention_rope: self attention only (kv_off / kv_len must be q_off / q_len)");
  WN_CHECK(a.mask_mode == 0 || a.mask_mode == 2,
           "attention_rope: mask_mode must be 0 (keys < kv_len) or 2 (chunk window), not 1 "
           "(causal)");
  WN_CHECK(a.mask_mode != 2 || a.chunk_size > 0,
           "attention_rope: chunk_size must be positive under mask_mode 2");
  WN_CHECK(!a.kbias && !a.fold && !a.bias_u && !a.bias_v,
           "attention_rope: no kbias, no bias_u / bias_v (the position is in the rotation)");
  WN_CHECK(!a.p_off, "attention_rope: no p_off");
  WN_CHECK(!a.blk_tab && a.xcd_nqb == 0, "attention_rope: no block list");
  WN_CHECK(!a.o_bf16 && !a.qkv_bf16, "attention_rope: fp32 only, no bf16 flags");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 32768 && a.n_heads > 0 && a.n_heads < 256,
           "attention_rope: n_seq / n_heads");
  WN_CHECK(a.n_heads % Hkv == 0,
           "attention_rope: n_heads % n_kv_heads != 0 (n_kv_heads must divide n_heads)");
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.ldp % 4 == 0,
           "attention_rope: strides % 4");
  WN_CHECK(a.ldq >= a.n_heads * DK && a.ldo >= a.n_heads * DK,
           "attention_rope: the Q / O stride is smaller than n_heads * 64");
  WN_CHECK(a.ldk >= Hkv * DK && a.ldv >= Hkv * DK,
           "attention_rope: the K / V stride is smaller than n_kv_heads * 64");
  WN_CHECK(a.ldp >= DK, "attention_rope: the table stride is smaller than 64");
  WN_CHECK(a.max_q_len > 0, "attention_rope: empty");
  WN_CHECK(a.max_q_len <= ra.max_pos,
           "attention_rope: a sequence is longer than the table (max_pos rows)");
  WN_CHECK(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0 &&
               ((uintptr_t)a.P & 15) == 0,
           "attention_rope: Q, K, V and the table must be 16-byte aligned");
  const int G = a.n_heads / Hkv;
  const int GB = G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
  dim3 g(cdiv(a.max_q_len, (4 / GB) * 32), Hkv * (G / GB), a.n_seq), t(NTHR);
  if (GB == 4) hipLaunchKernelGGL(attention_rope_kernel<4>, g, t, 0, s, a, G);
  else if (GB == 2) hipLaunchKernelGGL(attention_rope_kernel<2>, g, t, 0, s, a, G);
  else hipLaunchKernelGGL(attention_rope_kernel<1>, g, t, 0, s, a, G);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
