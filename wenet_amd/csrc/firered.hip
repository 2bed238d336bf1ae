// FireRedASR-AED encoder kernels (wenet/models/firered/): the relative-position attention WITH
// the relative shift (Transformer-XL / ESPnet form, firered/attention.py:86-105, 134-165) and
// the 32-channel conv2d4 front end (firered/subsampling.py).  fp32, untuned.
#include <algorithm>

#include "kernels.h"

namespace wn {

namespace {

// ===========================================================================
// Rel-shift attention.  score(i, j) = ((q_i + u) . k_j + (q_i + v) . p_{i-j}) * scale: the
// position row is the one of the DISTANCE i - j, so the term cannot be folded into the keys
// (encoder_kernels.hip relpos_fold_kernel needs "row j for key j").  No (T x T) and no
// (T x (2T - 1)) tensor reaches HBM; both contractions of a score tile run on
// v_mfma_f32_32x32x2_f32.
//
// One block = NW waves, each wave owns 32 query rows i0 .. i0 + 31 of one (sequence, head), as
// in attention_kernel (same transposed score tile S^T = K (Q+u)^T, same online softmax and P.V).
// Per 32-key tile j0 .. j0 + 31 a wave needs the 63 distances i0 - j0 - 31 .. i0 - j0 + 31.  The
// table P holds distance r in row p_center - r (ascending row = descending distance, the order
// of the reference's pos_emb), so the block's band is the (NW + 1) * 32 consecutive rows from
//     pb0 = p_center - (q0 + (NW - 1) * 32 - j0 + 31)
// and wave w's 64-row slab of it starts at band row (NW - 1 - w) * 32: slab row c holds distance
// i0 - j0 + 31 - c.  Band rows outside [0, p_rows) are staged as zeros, never clamped into a
// wrong row (they only ever meet (query, key) pairs outside the sequence).
//
// R = P_slab (Q+v)^T is two more 32x32 MFMA tiles (slab rows 0-31 and 32-63; row 63 is never
// read).  The MFMA leaves lane l with R[c][l & 31] for the 16 rows c = (r&3)+8(r>>2)+4(l>>5) of
// each tile; the wave writes both tiles to its skew buffer rbuf[c][query] and every lane reads
// back, for its query li and its 16 keys kj, rbuf[kj - li + 31][li] -- the relative shift.
//
// LDS: K, V tiles 32 x 68 floats each, the band (NW + 1) * 32 x 68, one skew buffer 64 x 32 per
// wave: 58.5 KB at NW = 2 (two blocks fit a CU's 160 KB), single buffered, two barriers per
// tile.  The compiler reports 324 VGPRs with the fully unrolled staging, i.e. one wave per SIMD;
// neither the occupancy nor the overlap of two blocks' staging has been measured.
// Skew buffer stride 32, unpadded: ds_write_b32 / ds_read_b32 bank = dword address % 32 within
// a 32-lane half.  The write of a half is one row, 32 consecutive dwords; the skewed read of a
// half is at (kj + 31) * 32 - 31 * li, and -31 = 1 (mod 32): 32 distinct banks.  Any odd stride
// would put the whole half on ONE bank ((1 - stride) even).
constexpr int RS_KT = 32;        // keys per tile
constexpr int RS_KSTR = 68;      // LDS row stride of the K / V / band tiles (floats): 64 + 4 pad
constexpr int RS_RSTR = 32;      // skew buffer row stride

#define RS_WAVE_LDS_ORDER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

template <int NW>
__global__ __launch_bounds__(NW * 64, 1) void attention_relshift_kernel(RelShiftAttnArgs a) {
  const int s = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * (NW * 32);
  const int len = a.len[s];
  if (q0 >= len) return;
  const int off = a.off[s];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  constexpr int NTHR = NW * 64;
  constexpr int BROWS = (NW + 1) * 32;
  constexpr int MAT = RS_KT * RS_KSTR;

  __shared__ __attribute__((aligned(16))) float stile[2 * MAT + BROWS * RS_KSTR];
  __shared__ float rbuf_all[NW][64 * RS_RSTR];
  float* sK = stile;
  float* sV = stile + MAT;
  float* sB = stile + 2 * MAT;
  float* rbuf = rbuf_all[wave];

  // ---- this lane's query row (+ u, + v) ------------------------------------
  const int qi = q0 + wave * 32 + li;
  const int qc = qi < len ? qi : len - 1;
  f32x4 qu[8], qv[8];
  {
    const float* qp = a.Q + (int64_t)(off + qc) * a.ldq + h * 64 + hi * 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(qp + kk * 8);
      qu[kk] = q + *reinterpret_cast<const f32x4*>(a.bias_u + h * 64 + kk * 8 + hi * 4);
      qv[kk] = q + *reinterpret_cast<const f32x4*>(a.bias_v + h * 64 + kk * 8 + hi * 4);
    }
  }
  const int n_it = (len + RS_KT - 1) / RS_KT;
  const bool wave_live = q0 + wave * 32 < len;   // (a dead wave only stages and meets barriers)

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  for (int it = 0; it < n_it; ++it) {
    const int j0 = it * RS_KT;
    // ---- stage K, V and the band ----------------------------------------------
#pragma unroll
    for (int i = 0; i < RS_KT * 16 / NTHR; ++i) {
      const int c = tid + i * NTHR;
      const int r = c >> 4, c4 = c & 15;
      int j = j0 + r;
      if (j > len - 1) j = len - 1;
      const int64_t grow = off + j;
      *reinterpret_cast<f32x4*>(sK + r * RS_KSTR + c4 * 4) =
          *reinterpret_cast<const f32x4*>(a.K + grow * a.ldk + h * 64 + c4 * 4);
      *reinterpret_cast<f32x4*>(sV + r * RS_KSTR + c4 * 4) =
          *reinterpret_cast<const f32x4*>(a.V + grow * a.ldv + h * 64 + c4 * 4);
    }
    const int pb0 = a.p_center - (q0 + (NW - 1) * 32 - j0 + 31);
#pragma unroll
    for (int i = 0; i < BROWS * 16 / NTHR; ++i) {
      const int c = tid + i * NTHR;
      const int r = c >> 4, c4 = c & 15;
      const int pr = pb0 + r;
      f32x4 p = {0.f, 0.f, 0.f, 0.f};
      if (pr >= 0 && pr < a.p_rows)
        p = *reinterpret_cast<const f32x4*>(a.P + (int64_t)pr * a.ldp + h * 64 + c4 * 4);
      *reinterpret_cast<f32x4*>(sB + r * RS_KSTR + c4 * 4) = p;
    }
    __syncthreads();

    if (wave_live) {
      // ---- S^T = K (Q+u)^T ------------------------------------------------------
      f32x16 sc, r0, r1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sc[r] = 0.f; r0[r] = 0.f; r1[r] = 0.f; }
      const float* kf = sK + li * RS_KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 fk = *reinterpret_cast<const f32x4*>(kf + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          sc = __builtin_amdgcn_mfma_f32_32x32x2f32(fk[t], qu[kk][t], sc, 0, 0, 0);
      }
      // ---- R = P_slab (Q+v)^T, slab rows 0-31 and 32-63 ----------------------------
      const float* bf = sB + ((NW - 1 - wave) * 32 + li) * RS_KSTR + hi * 4;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 f0 = *reinterpret_cast<const f32x4*>(bf + kk * 8);
        const f32x4 f1 = *reinterpret_cast<const f32x4*>(bf + 32 * RS_KSTR + kk * 8);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          r0 = __builtin_amdgcn_mfma_f32_32x32x2f32(f0[t], qv[kk][t], r0, 0, 0, 0);
          r1 = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[t], qv[kk][t], r1, 0, 0, 0);
        }
      }
      // ---- the skew: through this wave's buffer -------------------------------------
      RS_WAVE_LDS_ORDER();   // the previous tile's reads of rbuf are done
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2) + 4 * hi;
        rbuf[c * RS_RSTR + li] = r0[r];
        rbuf[(32 + c) * RS_RSTR + li] = r1[r];
      }
      RS_WAVE_LDS_ORDER();   // the whole wave's writes have landed (one wave: in order)
      // ---- online softmax on this lane's query -----------------------------------
      float tmax = -1e30f;
      bool ok[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
        ok[r] = j0 + kj < len;
        sc[r] = (sc[r] + rbuf[(kj - li + 31) * RS_RSTR + li]) * a.scale;
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
        const float v0 = sV[key * RS_KSTR + li];
        const float v1 = sV[key * RS_KSTR + 32 + li];
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
    const int qrow = q0 + wave * 32 + qr;
    if (qrow < len) {
      float* op = a.O + (int64_t)(off + qrow) * a.ldo + h * 64;
      op[li] = o0[r] * ir;
      op[32 + li] = o1[r] * ir;
    }
  }
}

// ===========================================================================
// Front end (firered/subsampling.py): CMVN, six zero frames behind the utterance's OWN last
// frame, Conv2d(1->C,3,2) + ReLU, Conv2d(C->C,3,2) + ReLU; direct kernels (a few hundred MFLOP
// per batch).  h1 is packed channels-last [t1_off + t1][F1][C]; the output is packed
// [t2_off + t2][c * F2 + f2], the row layout of the reference's view(b, t, c * f) that the
// output projection takes.

// one thread per (frame t1, f1, c); c fastest
__global__ __launch_bounds__(256) void firered_conv1_kernel(FireRedFrontArgs a) {
  const int b = blockIdx.y;
  const int n1 = a.t1_len[b];
  const int64_t n = (int64_t)n1 * a.F1 * a.C;
  const int len = a.len[b];
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = i % a.C;
    const int f1 = (i / a.C) % a.F1;
    const int t1 = i / ((int64_t)a.C * a.F1);
    float acc = a.b1[c];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int t = 2 * t1 + dy;
      if (t >= len) continue;   // one of the six zero frames (appended AFTER CMVN)
      const float* x = a.feats + ((int64_t)b * a.T + t) * a.F;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int f = 2 * f1 + dx;
        float v = x[f];
        if (a.mean) v = (v - a.mean[f]) * a.istd[f];
        acc = fmaf(a.w1[(dy * 3 + dx) * a.C + c], v, acc);
      }
    }
    a.h1[((int64_t)(a.t1_off[b] + t1) * a.F1 + f1) * a.C + c] = fmaxf(acc, 0.f);
  }
}

// one thread per (frame t2, f2, c2); c2 fastest: the h1 reads of a wave are broadcasts, the
// weight reads [tap][c1][c2] are consecutive
__global__ __launch_bounds__(256) void firered_conv2_kernel(FireRedFrontArgs a) {
  const int b = blockIdx.y;
  const int n2 = a.t2_len[b];
  const int64_t n = (int64_t)n2 * a.F2 * a.C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c2 = i % a.C;
    const int f2 = (i / a.C) % a.F2;
    const int t2 = i / ((int64_t)a.C * a.F2);
    float acc = a.b2[c2];
    for (int dy = 0; dy < 3; ++dy) {
      for (int dx = 0; dx < 3; ++dx) {
        const float* hp =
            a.h1 + ((int64_t)(a.t1_off[b] + 2 * t2 + dy) * a.F1 + 2 * f2 + dx) * a.C;
        const float* wp = a.w2 + (int64_t)(dy * 3 + dx) * a.C * a.C + c2;
        for (int c1 = 0; c1 < a.C; ++c1) acc = fmaf(wp[c1 * a.C], hp[c1], acc);
      }
    }
    a.out[(int64_t)(a.t2_off[b] + t2) * a.ldo + c2 * a.F2 + f2] = fmaxf(acc, 0.f);
  }
}

}  // namespace

int attention_relshift(const RelShiftAttnArgs& a, hipStream_t s) {
  WN_CHECK(a.n_seq > 0 && a.n_heads > 0 && a.max_len > 0, "attention_relshift: empty");
  WN_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldp % 4 == 0,
           "attention_relshift: strides must be multiples of 4 floats");
  WN_CHECK(a.P && a.bias_u && a.bias_v, "attention_relshift: position table / biases");
  // every distance of the longest sequence has a row: p_center - (T - 1) .. p_center + (T - 1)
  WN_CHECK(a.p_center - (a.max_len - 1) >= 0 && a.p_center + (a.max_len - 1) < a.p_rows,
           "attention_relshift: a sequence is longer than the position table covers");
  constexpr int NW = 2;
  dim3 g(cdiv(a.max_len, NW * 32), a.n_heads, a.n_seq), t(NW * 64);
  hipLaunchKernelGGL(attention_relshift_kernel<NW>, g, t, 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int firered_frontend(const FireRedFrontArgs& a, hipStream_t s) {
  WN_CHECK(a.B > 0 && a.C > 0 && a.F >= 7, "firered_frontend: B / C / F");
  WN_CHECK(a.F1 == (a.F - 3) / 2 + 1 && a.F2 == (a.F1 - 3) / 2 + 1, "firered_frontend: F1 / F2");
  WN_CHECK(a.ldo >= a.C * a.F2, "firered_frontend: output stride");
  if (a.max_t2 <= 0) return 0;
  const int64_t n1 = (int64_t)(2 * a.max_t2 + 1) * a.F1 * a.C;
  const int64_t n2 = (int64_t)a.max_t2 * a.F2 * a.C;
  dim3 g1((unsigned)std::min<int64_t>(cdiv64(n1, 256), 4096), a.B);
  dim3 g2((unsigned)std::min<int64_t>(cdiv64(n2, 256), 4096), a.B);
  hipLaunchKernelGGL(firered_conv1_kernel, g1, dim3(256), 0, s, a);
  hipLaunchKernelGGL(firered_conv2_kernel, g2, dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
