// fp32 self attention with Shaw relative-position keys, d_k = 64, full context: the attention of the
// W2v-BERT 2.0 / conformer_shaw encoders (ShawRelPositionMultiHeadedAttention, attention.py:523-596)
//     score(i, j) = (q_i . k_j + q_i . E[clamp(j - i, -64, 8) + 64]) * scale
// with ONE 73-row table E [73][64] shared by all heads.  The position term of query i takes only 73
// values, G[c][i] = E[c] . q_i, and is the SAME value G[0][i] for every key 64 or more to the left
// and G[72][i] for every key 8 or more to the right: it is computed once per query, not per tile.
// stack_frames_ln, the front end of those encoders, sits at the end of the file.
//
// Work split.  A block is NW = 2 waves; wave w owns the 32 query rows i0 = q0 + 32 w .. of one
// (sequence, head), lane = query (l & 31), as in attention_kernel / attention_d32_relpos.
//
// Prologue, once per wave.  The block stages E into the (still unused) tile buffers at the tiles'
// row stride, rows 73 .. 95 as zeros; each live wave computes G = E Q^T as three 32 x 32 tiles of
// v_mfma_f32_32x32x2_f32 (table rows 0-31, 32-63, 64-95: 96 MFMAs) and writes rows 0 .. 72 to its
// own strip g[c][query], 73 x 32 floats at stride 32.  Each lane then keeps its two clamp values
// g_left = G[0][li] and g_right = G[72][li] in registers.
//
// Per 32-key tile j0 (K | V shared by the block's waves through LDS, staged global -> registers ->
// LDS one tile ahead, two buffers, one barrier per tile, as attention_d32_relpos): S^T = K Q^T in
// 32 MFMA steps; the lane holds the 16 keys (r&3)+8(r>>2)+4(l>>5) of its query.  The position
// term is added before the scale, by a WAVE-UNIFORM choice from dj = j0 - i0 alone:
//     dj <= -95 (every pair has j - i <= -64): + g_left          (a register)
//     dj >=  39 (every pair has j - i >=   8): + g_right         (a register)
//     otherwise:                               + g[clamp(j - i, -64, 8) + 64][li]   (the strip)
// i0 and j0 are multiples of 32, so only dj = -64, -32, 0, 32 -- at most four tiles per wave --
// read the strip; every other tile costs one add per score.  Online softmax and P.V (two 32 x 32
// accumulators) are attention_relshift's.  No score tensor reaches HBM.
//
// Masks and edges.  Keys >= len are masked; rows past the sequence's end repeat the sequence's own
// last row while staging (never a neighbour's).  A wave whose 32 rows lie past the end only stages
// and meets the barriers; a block past the end, and every block of a len = 0 sequence, returns at
// once and writes nothing.
//
// LDS (static): two buffers of K | V, 2 x 32 x 68 floats each (34.0 KB), and NW strips of 73 x 32
// floats (18.25 KB): 52.25 KB, so three blocks fit a CU's 160 KB.  NW = 4 with two buffers would
// need 70.5 KB; NW = 4 with one buffer (53.5 KB, two barriers per tile) is the other form that
// fits and has not been measured against this one.
// Banks (64 banks of 4 bytes; only lanes of one fixed lane group can conflict):
//  * K / E fragment, ds_read_b128 at dword li * 68 + hi * 4 + kk * 8: 68 li mod 64 = 4 li, the 16
//    lanes of a group start at the 16 different multiples of 4 -- their spans tile the 64 banks.
//  * V operand, ds_read_b32 at key * 68 + li (+ 32): a half wave reads 32 consecutive dwords.
//  * staging stores, ds_write_b128: 16 consecutive threads hold the 16 float4 of ONE row.
//  * strip write, ds_write_b32 at c * 32 + li: a half wave writes one row, 32 consecutive dwords.
//  * strip gather, ds_read_b32 at c * 32 + li with c = clamp(kj + dj - li, -64, 8) + 64: the
//    unclamped lanes of a half wave read dword (kj + dj + 64) * 32 - 31 li, and -31 is odd: distinct
//    banks; the clamped lanes share ONE c and read consecutive dwords.  A clamped and an unclamped
//    lane can meet on a bank (two-way at worst), on the at most four band tiles only.
// The compiler reports 164 VGPRs, no scratch, an occupancy of two waves per SIMD.  Untuned: NW and
// the buffering were chosen by the LDS budget above, not by measurement.
//
// mask_mode other than 0, kbias, p_off, block lists and the bf16 flags are refused by name.  scale
// is a multiplier (0.125 from the encoder; the reference divides by math.sqrt(d_k)).
#include "kernels.h"

namespace wn {

namespace {

constexpr int KT = 32;            // keys per tile
constexpr int DK = 64;
constexpr int KSTR = DK + 4;      // LDS row stride of the K / V / E tiles (floats)
constexpr int MAT = KT * KSTR;
constexpr int BUF = 2 * MAT;      // K | V
constexpr int NW = 2;             // waves per block
constexpr int NTHR = NW * 64;
constexpr int NCH = KT * (DK / 4) / NTHR;   // float4 chunks per thread and matrix
constexpr int GSTR = 32;          // strip row stride
static_assert(3 * KT * KSTR <= 2 * BUF, "the staged table must fit the tile buffers");

// the wave's own LDS traffic is in order; this keeps the compiler from moving it
#define SHAW_WAVE_LDS_ORDER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__global__ __launch_bounds__(NTHR) void attention_shaw_kernel(AttnArgs a) {
  const int s = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (NW * 32);
  const int len = a.q_len[s];
  if (q0 >= len) return;
  const int off = a.q_off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;

  __shared__ __attribute__((aligned(16))) float stile[2 * BUF];
  __shared__ float strips[NW][SHAW_ROWS * GSTR];
  float* g = strips[wave];

  // ---- this lane's query row ------------------------------------------------------------
  const int i0 = q0 + wave * 32;
  const int qc = min(i0 + li, len - 1);
  f32x4 qr[DK / 8];
  {
    const float* qp = a.Q + (int64_t)(off + qc) * a.ldq + h * DK + hi * 4;
#pragma unroll
    for (int kk = 0; kk < DK / 8; ++kk) qr[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
  }
  const int n_it = (len + KT - 1) / KT;
  const bool wave_live = i0 < len;

  // ---- K | V staging: thread -> (row c >> 4, column quad c & 15), c = tid + i * NTHR ----------
  f32x4 rK[NCH], rV[NCH];
  auto gload = [&](int it) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * NTHR;
      const int j = min(it * KT + (c >> 4), len - 1);
      const int64_t grow = off + j;
      rK[i] = *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * DK + (c & 15) * 4);
      rV[i] = *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * DK + (c & 15) * 4);
    }
  };
  auto lstore = [&](int buf) {
    float* base = stile + buf * BUF;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = tid + i * NTHR;
      *reinterpret_cast<f32x4*>(base + (c >> 4) * KSTR + (c & 15) * 4) = rK[i];
      *reinterpret_cast<f32x4*>(base + MAT + (c >> 4) * KSTR + (c & 15) * 4) = rV[i];
    }
  };
  gload(0);   // in flight under the prologue

  // ---- prologue: G = E Q^T into this wave's strip ---------------------------------------------
#pragma unroll
  for (int i = 0; i < 3 * NCH; ++i) {
    const int c = tid + i * NTHR;
    const int r = c >> 4;
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
    if (r < SHAW_ROWS) e = *reinterpret_cast<const f32x4*>(a.P + (int64_t)r * a.ldp + (c & 15) * 4);
    *reinterpret_cast<f32x4*>(stile + r * KSTR + (c & 15) * 4) = e;
  }
  __syncthreads();
  float g_left = 0.f, g_right = 0.f;
  if (wave_live) {
#pragma unroll
    for (int tile = 0; tile < 3; ++tile) {
      f32x16 gt;
#pragma unroll
      for (int r = 0; r < 16; ++r) gt[r] = 0.f;
      const float* ef = stile + (tile * 32 + li) * KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < DK / 8; ++kk) {
        const f32x4 fe = *reinterpret_cast<const f32x4*>(ef + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          gt = __builtin_amdgcn_mfma_f32_32x32x2f32(fe[t], qr[kk][t], gt, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (c < SHAW_ROWS) g[c * GSTR + li] = gt[r];
      }
    }
    SHAW_WAVE_LDS_ORDER();   // the whole wave's writes have landed (one wave: in order)
    g_left = g[li];
    g_right = g[(SHAW_ROWS - 1) * GSTR + li];
  }
  __syncthreads();   // every wave is done with the staged table
  lstore(0);
  __syncthreads();

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * KT;
    const int cur = it & 1;
    const float* sK = stile + cur * BUF;
    const float* sV = sK + MAT;
    if (it + 1 < n_it) gload(it + 1);

    if (wave_live) {
      // ---- S^T tile = K Q^T -------------------------------------------------------------------
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
      // ---- the position term (wave-uniform choice), the scale, the key mask ----------------------
      const int dj = j0 - i0;
      float tmax = -1e30f;
      bool ok[16];
      if (dj <= -(SHAW_LEFT + 31) || dj >= SHAW_RIGHT + 31) {
        const float gc = dj < 0 ? g_left : g_right;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = (sc[r] + gc) * a.scale;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const int c = min(max(dj + kj - li, -SHAW_LEFT), SHAW_RIGHT) + SHAW_LEFT;
          sc[r] = (sc[r] + g[c * GSTR + li]) * a.scale;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ok[r] = j0 + (r & 3) + 8 * (r >> 2) + 4 * hi < len;
        if (ok[r]) tmax = fmaxf(tmax, sc[r]);
      }
      // ---- online softmax on this lane's query ---------------------------------------------------
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
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
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

// ===========================================================================
// StackNFramesSubsampling up to its projection (subsampling.py:376-388, stride 2): output row t of
// an utterance is its frames 2 t and 2 t + 1 laid end to end -- 2 F consecutive floats of the
// padded (B, T, F) tensor -- after the optional per-frame CMVN, LayerNorm over the 2 F values.
// One wave per output row, up to four values per lane (F <= 128), two-pass statistics in
// registers.  A row reads its own utterance's frames only: 2 t + 1 < 2 * len[u] <= T.
__global__ __launch_bounds__(256) void stack_frames_ln_kernel(StackFramesArgs a) {
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.len[u]) return;
  const int n = 2 * a.F;
  const float* x = a.feats + ((int64_t)u * a.T + 2 * t) * a.F;
  float v[4];
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = lane + 64 * e;
    v[e] = 0.f;
    if (i < n) {
      v[e] = x[i];
      if (a.mean) {
        const int f = i < a.F ? i : i - a.F;
        v[e] = (v[e] - a.mean[f]) * a.istd[f];
      }
    }
    sum += v[e];
  }
#pragma unroll
  for (int x2 = 32; x2 > 0; x2 >>= 1) sum += __shfl_xor(sum, x2, 64);
  const float mu = sum / (float)n;
  float var = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dlt = lane + 64 * e < n ? v[e] - mu : 0.f;
    var += dlt * dlt;
  }
#pragma unroll
  for (int x2 = 32; x2 > 0; x2 >>= 1) var += __shfl_xor(var, x2, 64);
  const float rstd = rsqrtf(var / (float)n + a.eps);
  float* y = a.out + (int64_t)(a.off[u] + t) * a.ldo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = lane + 64 * e;
    if (i < n) y[i] = (v[e] - mu) * rstd * a.ln_w[i] + a.ln_b[i];
  }
}

}  // namespace

int attention_shaw(const AttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.O && a.P && a.q_off && a.q_len,
           "attention_shaw: null argument");
  WN_CHECK(a.kv_off == a.q_off && a.kv_len == a.q_len,
           "attention_shaw: self attention only (kv_off / kv_len must be q_off / q_len)");
  WN_CHECK(a.mask_mode == 0,
           "attention_shaw: mask_mode must be 0 (keys < kv_len): full context only");
  WN_CHECK(!a.kbias && !a.fold && !a.bias_u && !a.bias_v,
           "attention_shaw: no kbias, no bias_u / bias_v (the term is q . E[clamp(j - i)])");
  WN_CHECK(!a.p_off, "attention_shaw: no p_off");
  WN_CHECK(!a.blk_tab && a.xcd_nqb == 0, "attention_shaw: no block list");
  WN_CHECK(!a.o_bf16 && !a.qkv_bf16, "attention_shaw: fp32 only, no bf16 flags");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 32768 && a.n_heads > 0 && a.n_heads < 256,
           "attention_shaw: n_seq / n_heads");
  const int d = a.n_heads * DK;
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.ldp % 4 == 0,
           "attention_shaw: strides % 4");
  WN_CHECK(a.ldq >= d && a.ldk >= d && a.ldv >= d && a.ldo >= d && a.ldp >= DK,
           "attention_shaw: a stride is smaller than n_heads * 64");
  WN_CHECK(a.max_q_len > 0, "attention_shaw: empty");
  WN_CHECK(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0 &&
               ((uintptr_t)a.P & 15) == 0,
           "attention_shaw: Q, K, V and the table must be 16-byte aligned");
  dim3 g(cdiv(a.max_q_len, NW * 32), a.n_heads, a.n_seq), t(NTHR);
  hipLaunchKernelGGL(attention_shaw_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int stack_frames_ln(const StackFramesArgs& a, hipStream_t s) {
  WN_CHECK(a.feats && a.ln_w && a.ln_b && a.out && a.off && a.len,
           "stack_frames_ln: null argument");
  WN_CHECK((a.mean == nullptr) == (a.istd == nullptr),
           "stack_frames_ln: mean and istd come together");
  WN_CHECK(a.B > 0 && a.B < 65536 && a.T > 0 && a.F >= 1 && a.F <= 128,
           "stack_frames_ln: B / T / F (2 F values per row, F <= 128)");
  WN_CHECK(a.ldo >= 2 * a.F, "stack_frames_ln: output stride");
  if (a.max_len <= 0) return 0;
  WN_CHECK(2 * a.max_len <= a.T, "stack_frames_ln: a row would read past its utterance's frames");
  dim3 g(cdiv(a.max_len, 4), a.B), t(256);
  hipLaunchKernelGGL(stack_frames_ln_kernel, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
