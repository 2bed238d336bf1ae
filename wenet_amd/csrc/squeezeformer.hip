// Squeezeformer encoder kernels (wenet/models/squeezeformer/), fp32, untuned:
//   attention_sqshift    self attention with the reference's rel_shift on a T x T score matrix
//                        (squeezeformer/attention.py:75-99), which WRAPS
//   time_reduce_dwconv   the depthwise stride-2 conv of the time reduction layer
//   time_recover_add     skip + every half-rate row repeated twice
#include <algorithm>

#include "kernels.h"

namespace wn {

namespace {

// ===========================================================================
// Wrapped-shift attention.  The reference multiplies (q + v) with a T-row position table,
// bd[i][c] = (q_i + v) . p_c, and runs the Transformer-XL view trick on the SQUARE matrix.  In
// closed form (T = the sequence's own length):
//     j <= i     : shifted[i][j] = bd[i][T - 1 - (i - j)]
//     j == i + 1 : 0
//     j >= i + 2 : shifted[i][j] = bd[i + 1][j - i - 2]        -- the NEXT query row
// so score(i, j) = ((q_i + u) . k_j + shifted[i][j]) * scale.  Both branches read "table row =
// centre + (j - i')": the lower one with centre T - 1 and query i' = i, the upper one with centre
// -1 and query i' = i + 1.  That is the band of attention_relshift_kernel (firered.hip), whose
// layout this kernel keeps: NW waves of 32 query rows, 32-key tiles, S^T = K (Q+u)^T, the band
// product R = P_slab (Q'+v)^T on v_mfma_f32_32x32x2_f32 and the skew through a per-wave LDS
// buffer (lane li reads rbuf[kj - li + 31][li]).
//
// Per key tile the block runs up to two band passes, lower then upper, through the SAME band
// buffer.  A pass is run only where some (i, j) of the block needs it: tiles strictly below the
// block's diagonal run the lower pass alone, tiles strictly above it the upper pass alone, and
// only the NW tiles that straddle j in {i, i + 1, i + 2} run both (one more barrier pair each).
// Inside a pass a wave whose own 32 rows do not need it skips the MFMAs.  The branch of a pair is
// chosen by an explicit select on j - i, never by what a row outside the branch holds: table
// rows >= T exist for a shorter sequence (the table serves the longest one) and are wrong there.
// Band rows outside [0, p_rows) are staged as zeros; they only meet pairs of the other branch.
// The upper pass's query row i0 + 32 may lie behind the sequence: it is staged as zeros (it
// only meets pairs with j >= T), never read from the neighbour in the packed buffer.
//
// LDS as in firered.hip: K, V tiles 32 x 68 floats, the band (NW + 1) * 32 x 68, one skew
// buffer 64 x 32 per wave: 58.5 KB at NW = 2.  Skew buffer stride 32, unpadded: the write of a
// 32-lane half is one row of 32 consecutive dwords, the skewed read of a half is at
// (kj + 31) * 32 - 31 * li, and -31 = 1 (mod 32): 32 distinct banks (firered.hip:34-41).
// 59904 bytes in all.  The compiler reports 256 VGPRs + 89 AGPRs (345 registers), no scratch:
// one wave per SIMD.  Neither the occupancy nor LDS-bank counters have been measured; one timing
// beside attention_kernel and attention_relshift: tools/bench_squeezeformer.py.
constexpr int SQ_KT = 32;        // keys per tile
constexpr int SQ_KSTR = 68;      // LDS row stride of the K / V / band tiles (floats)
constexpr int SQ_RSTR = 32;      // skew buffer row stride

#define SQ_WAVE_LDS_ORDER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void attention_sqshift_kernel(SqShiftAttnArgs a) {
  const int s = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * (NW * 32);
  const int len = a.len[s];
  if (q0 >= len) return;
  const int off = a.off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  constexpr int NTHR = NW * 64;
  constexpr int BROWS = (NW + 1) * 32;
  constexpr int MAT = SQ_KT * SQ_KSTR;

  __shared__ __attribute__((aligned(16))) float stile[2 * MAT + BROWS * SQ_KSTR];
  __shared__ float rbuf_all[NW][64 * SQ_RSTR];
  float* sK = stile;
  float* sV = stile + MAT;
  float* sB = stile + 2 * MAT;
  float* rbuf = rbuf_all[wave];

  // ---- this lane's query row (+ u, + v) and the next one (+ v) ------------------
  const int i0 = q0 + wave * 32;
  const int qi = i0 + li;
  const int qc = qi < len ? qi : len - 1;
  const bool has_next = qi + 1 < len;
  f32x4 qu[8], qv[8], qn[8];
  {
    const float* qp = a.Q + (int64_t)(off + qc) * a.ldq + h * 64 + hi * 4;
    const float* np = a.Q + (int64_t)(off + (has_next ? qi + 1 : qc)) * a.ldq + h * 64 + hi * 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(qp + kk * 8);
      const f32x4 n = *reinterpret_cast<const f32x4*>(np + kk * 8);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias_v + h * 64 + kk * 8 + hi * 4);
      qu[kk] = q + *reinterpret_cast<const f32x4*>(a.bias_u + h * 64 + kk * 8 + hi * 4);
      qv[kk] = q + bv;
      const f32x4 nv = n + bv;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      qn[kk] = has_next ? nv : zero;
    }
  }
  const int n_it = (len + SQ_KT - 1) / SQ_KT;
  const bool wave_live = i0 < len;   // (a dead wave only stages and meets barriers)

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * SQ_KT;
    // ---- stage K, V ----------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < SQ_KT * 16 / NTHR; ++i) {
      const int c = tid + i * NTHR;
      const int r = c >> 4, c4 = c & 15;
      int j = j0 + r;
      if (j > len - 1) j = len - 1;
      const int64_t grow = off + j;
      *reinterpret_cast<f32x4*>(sK + r * SQ_KSTR + c4 * 4) =
          *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * 64 + c4 * 4);
      *reinterpret_cast<f32x4*>(sV + r * SQ_KSTR + c4 * 4) =
          *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * 64 + c4 * 4);
    }
    // the shift term of this lane's 16 (query, key) pairs; j == i + 1 keeps its zero
    float sft[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sft[r] = 0.f;
    // block-uniform: does any pair of the block take the lower (j <= i) / upper (j >= i + 2) branch
    const bool blk_lo = j0 <= q0 + NW * 32 - 1;
    const bool blk_up = j0 + SQ_KT - 1 >= q0 + 2;
    bool staged = false;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 0 ? !blk_lo : !blk_up) continue;
      // lower: centre len - 1, queries i; upper: centre -1, queries i + 1
      const int centre = pass == 0 ? len - 1 : -1;
      const int pb0 = centre - (q0 + pass + (NW - 1) * 32 - j0 + 31);
      if (staged) __syncthreads();   // every wave is done with the lower pass's band
#pragma unroll
      for (int i = 0; i < BROWS * 16 / NTHR; ++i) {
        const int c = tid + i * NTHR;
        const int r = c >> 4, c4 = c & 15;
        const int pr = pb0 + r;
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
        if (pr >= 0 && pr < a.p_rows)
          p = *reinterpret_cast<const f32x4*>(a.P + (int64_t)pr * a.ldp + h * 64 + c4 * 4);
        *reinterpret_cast<f32x4*>(sB + r * SQ_KSTR + c4 * 4) = p;
      }
      staged = true;
      __syncthreads();
      // wave-uniform: this wave's rows i0 .. i0 + 31 against keys j0 .. j0 + 31
      const bool wave_need = pass == 0 ? j0 <= i0 + 31 : j0 + SQ_KT - 1 >= i0 + 2;
      if (wave_live && wave_need) {
        f32x16 r0, r1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { r0[r] = 0.f; r1[r] = 0.f; }
        const float* bf = sB + ((NW - 1 - wave) * 32 + li) * SQ_KSTR + hi * 4;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const f32x4 f0 = *reinterpret_cast<const f32x4*>(bf + kk * 8);
          const f32x4 f1 = *reinterpret_cast<const f32x4*>(bf + 32 * SQ_KSTR + kk * 8);
          const f32x4 qq = pass == 0 ? qv[kk] : qn[kk];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            r0 = __builtin_amdgcn_mfma_f32_32x32x2f32(f0[t], qq[t], r0, 0, 0, 0);
            r1 = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[t], qq[t], r1, 0, 0, 0);
          }
        }
        SQ_WAVE_LDS_ORDER();   // the previous reads of rbuf are done
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2) + 4 * hi;
          rbuf[c * SQ_RSTR + li] = r0[r];
          rbuf[(32 + c) * SQ_RSTR + li] = r1[r];
        }
        SQ_WAVE_LDS_ORDER();   // the whole wave's writes have landed (one wave: in order)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
          const int dji = (j0 + kj) - (i0 + li);
          const float v = rbuf[(kj - li + 31) * SQ_RSTR + li];
          if (pass == 0 ? dji <= 0 : dji >= 2) sft[r] = v;
        }
      }
    }
    // (blk_lo || blk_up holds for every tile, so the K / V tiles are behind a barrier here)

    if (wave_live) {
      // ---- S^T = K (Q+u)^T ------------------------------------------------------
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = 0.f;
      const float* kf = sK + li * SQ_KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 fk = *reinterpret_cast<const f32x4*>(kf + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[t], qu[kk][t], sc, 0, 0, 0);
      }
      // ---- online softmax on this lane's query -----------------------------------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
        ok[r] = j0 + kj < len;
        sc[r] = (sc[r] + sft[r]) * a.scale;
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
      if (!__all(alpha == 1.0f)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
          o0[r] *= ar;
          o1[r] *= ar;
        }
      }
      // ---- O += P V ----------------------------------------------------------------
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int key = (st & 3) + 8 * (st >> 2) + 4 * hi;
        const float v0 = sV[key * SQ_KSTR + li];
        const float v1 = sV[key * SQ_KSTR + 32 + li];
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v0, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[st], v1, o1, 0, 0, 0);
      }
    }
    __syncthreads();   // every wave is done with the tiles
  }
  if (!wave_live) return;
  // ---- normalise and store -------------------------------------------------
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float ir = __shfl(inv, qr, 64);
    const int qrow = i0 + qr;
    if (qrow < len) {
      float* op = a.O + (int64_t)(off + qrow) * a.ldo + h * 64;
      op[li] = o0[r] * ir;
      op[32 + li] = o1[r] * ir;
    }
  }
}

// ===========================================================================
// Time reduction (squeezeformer/subsampling.py:97-179, 243-323): the depthwise stride-2 conv.
// A workgroup owns TR_TILE half-rate frames x 64 channels of ONE utterance and stages the
// full-rate frames they read once; frames outside the utterance's own [0, len) are zeros.
// grid (C / 64, tiles of the longest utterance, B); dynamic LDS: the staged frames, then the
// K x 64 taps.  K == 1 reads every second frame only, and stages only those.
constexpr int TR_CH = 64;
constexpr int TR_THREADS = 256;

__global__ __launch_bounds__(TR_THREADS) void time_reduce_kernel(TimeReduceArgs a) {
  extern __shared__ __align__(16) float tr_lds[];
  const int b = blockIdx.z;
  const int len = a.len[b];
  const int len2 = (len + 1) / 2;
  const int t0 = blockIdx.y * TR_TILE;
  if (t0 >= len2) return;
  const int row0 = a.off[b], orow0 = a.off2[b];
  const int c0 = blockIdx.x * TR_CH;
  const int K = a.K;
  const int step = K == 1 ? 2 : 1;                 // full-rate frames between staged frames
  const int n_in = K == 1 ? TR_TILE : 2 * TR_TILE + K - 2;
  const int ostr = K == 1 ? 1 : 2;                 // staged frames between output frames
  float* s_in = tr_lds;                            // [n_in][64]
  float* s_w = tr_lds + n_in * TR_CH;              // [K][64]
  const int tid = threadIdx.x;
  for (int i = tid; i < K * (TR_CH / 4); i += TR_THREADS) {
    const int k = i / (TR_CH / 4), q = i % (TR_CH / 4);
    *reinterpret_cast<float4*>(s_w + k * TR_CH + q * 4) =
        *reinterpret_cast<const float4*>(a.wt + (int64_t)k * a.C + c0 + q * 4);
  }
  for (int i = tid; i < n_in * (TR_CH / 4); i += TR_THREADS) {
    const int j = i / (TR_CH / 4), q = i % (TR_CH / 4);
    const int t = 2 * t0 - a.pad + j * step;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < len)
      v = *reinterpret_cast<const float4*>(a.x + (int64_t)(row0 + t) * a.ldx + c0 + q * 4);
    *reinterpret_cast<float4*>(s_in + j * TR_CH + q * 4) = v;
  }
  __syncthreads();
  constexpr int PER = TR_TILE / (TR_THREADS / 64);   // output frames per wave
  const int lane = tid & 63;
  const int o0 = (tid >> 6) * PER;
  float acc[PER];
#pragma unroll
  for (int o = 0; o < PER; ++o) acc[o] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float w = s_w[k * TR_CH + lane];
#pragma unroll
    for (int o = 0; o < PER; ++o)
      acc[o] = fmaf(w, s_in[((o0 + o) * ostr + k) * TR_CH + lane], acc[o]);
  }
  const int c = c0 + lane;
  const float bias = a.bias[c];
#pragma unroll
  for (int o = 0; o < PER; ++o) {
    const int t = t0 + o0 + o;
    if (t >= len2) break;
    a.y[(int64_t)(orow0 + t) * a.ldy + c] = acc[o] + bias;
  }
}

// y[off[b] + t] = skip[off[b] + t] + z[off2[b] + t / 2]; grid (blocks over the longest
// utterance's len * C / 4, B)
__global__ __launch_bounds__(256) void time_recover_kernel(TimeRecoverArgs a) {
  const int b = blockIdx.y;
  const int len = a.len[b];
  const int C4 = a.C / 4;
  const int64_t n = (int64_t)len * C4;
  const int row0 = a.off[b], zrow0 = a.off2[b];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i / C4), c = (int)(i % C4) * 4;
    const float4 sv = *reinterpret_cast<const float4*>(a.skip + (int64_t)(row0 + t) * a.lds + c);
    const float4 zv = *reinterpret_cast<const float4*>(a.z + (int64_t)(zrow0 + t / 2) * a.ldz + c);
    *reinterpret_cast<float4*>(a.y + (int64_t)(row0 + t) * a.ldy + c) =
        make_float4(sv.x + zv.x, sv.y + zv.y, sv.z + zv.z, sv.w + zv.w);
  }
}

}  // namespace

int attention_sqshift(const SqShiftAttnArgs& a, hipStream_t s) {
  WN_CHECK(a.Q && a.K && a.V && a.O && a.off && a.len, "attention_sqshift: null argument");
  WN_CHECK(a.n_seq > 0 && a.n_seq < 65536 && a.n_heads > 0 && a.n_heads < 65536 && a.max_len > 0,
           "attention_sqshift: empty");
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldp % 4 == 0,
           "attention_sqshift: strides must be multiples of 4 floats");
  WN_CHECK(a.P && a.bias_u && a.bias_v, "attention_sqshift: position table / biases");
  // the lower branch of the longest sequence reads rows 0 .. max_len - 1
  WN_CHECK(a.p_rows >= a.max_len,
           "attention_sqshift: a sequence is longer than the position table covers");
  constexpr int NW = 2;
  dim3 g(cdiv(a.max_len, NW * 32), a.n_heads, a.n_seq), t(NW * 64);
  hipLaunchKernelGGL(attention_sqshift_kernel<NW>, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

static int time_layout_check(const int* off, const int* len, const int* off2, int B, int C,
                             int max_len, const std::string& w) {
  WN_CHECK(off && len && off2, w + ": null argument");
  WN_CHECK(C >= 64 && C % 64 == 0, w + ": channels must be a multiple of 64");
  WN_CHECK(B > 0 && B < 65536 && max_len > 0, w + ": empty batch");
  return 0;
}

int time_reduce_dwconv(const TimeReduceArgs& a, hipStream_t s) {
  WN_TRY(time_layout_check(a.off, a.len, a.off2, a.B, a.C, a.max_len, "time_reduce_dwconv"));
  WN_CHECK(a.x && a.wt && a.bias && a.y, "time_reduce_dwconv: null argument");
  WN_CHECK((a.K == 5 && a.pad == 3) || (a.K == 1 && a.pad == 0),
           "time_reduce_dwconv: 5 taps with padding 3 (conv1d) or 1 tap without padding (stream)");
  WN_CHECK(a.ldx % 4 == 0 && a.ldx >= a.C && a.ldy >= a.C, "time_reduce_dwconv: row strides");
  WN_CHECK(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.wt & 15) == 0,
           "time_reduce_dwconv: x and the taps must be 16-byte aligned");
  WN_CHECK(a.y != a.x, "time_reduce_dwconv: not in place");
  const int n_in = a.K == 1 ? TR_TILE : 2 * TR_TILE + a.K - 2;
  const size_t lds = (size_t)(n_in + a.K) * TR_CH * sizeof(float);   // 18 KB at K = 5
  const dim3 grid(a.C / TR_CH, cdiv((a.max_len + 1) / 2, TR_TILE), a.B);
  hipLaunchKernelGGL(time_reduce_kernel, grid, dim3(TR_THREADS), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int time_recover_add(const TimeRecoverArgs& a, hipStream_t s) {
  WN_TRY(time_layout_check(a.off, a.len, a.off2, a.B, a.C, a.max_len, "time_recover_add"));
  WN_CHECK(a.skip && a.z && a.y, "time_recover_add: null argument");
  WN_CHECK(a.lds % 4 == 0 && a.ldz % 4 == 0 && a.ldy % 4 == 0 && a.lds >= a.C && a.ldz >= a.C &&
               a.ldy >= a.C,
           "time_recover_add: row strides must be multiples of 4 floats, at least C");
  WN_CHECK(((uintptr_t)a.skip & 15) == 0 && ((uintptr_t)a.z & 15) == 0 &&
               ((uintptr_t)a.y & 15) == 0,
           "time_recover_add: buffers must be 16-byte aligned");
  const int64_t n = (int64_t)a.max_len * (a.C / 4);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv64(n, 256), 4096), a.B);
  hipLaunchKernelGGL(time_recover_kernel, grid, dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
