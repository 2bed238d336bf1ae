// CTC forced alignment (wenet/utils/ctc_utils.py force_align, wenet/bin/alignment.py) on the
// GPU: the emission gather and the Viterbi trellis with its backtrace.
//
// The rule (fp32, ties to the earlier candidate: stay, step, skip; one add per state and frame)
// is stated in DESIGN.md section 3 and restated lane by lane in tests/align_formulation.py.
#include <math.h>

#include "kernels.h"

namespace wn {

namespace {

// ===========================================================================
// Emission gather: E[row][j] = logp[row][lab_b[j]], j = 0..L_b (lab_b[0] = blank), zeros behind.
// One wave per row.  normalize: the row holds logits and the log-softmax statistics are taken
// here, in the order of ctc_row_kernel (ctc.hip): its thread 64 w + lane sums the elements
// lane + 64 w + 256 j, j ascending; four wave sums added left to right -- so (x - mx) - lsum is
// bit for bit what that kernel writes into the full log-prob row, which is never written here.
// The row is read twice (maximum, sum); the second pass hits the cache, HBM sees it once.
__global__ __launch_bounds__(256) void align_gather_kernel(AlignGatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int b = a.row_utt ? a.row_utt[row] : row / a.Tp;
  if (b < 0) return;
  const int t = row - a.off[b];
  if (t < 0 || t >= a.len[b]) return;
  const float* x = a.x + (int64_t)row * a.ld;
  float mx = 0.f, lsum = 0.f;
  if (a.normalize) {
    mx = -INFINITY;
    for (int i = lane; i < a.V; i += 64) {
      float v = x[i];
      if (i == a.blank) v -= a.blank_penalty;
      mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    float sm4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < a.V; i0 += 256) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int i = i0 + w * 64 + lane;
        if (i < a.V) {
          float v = x[i];
          if (i == a.blank) v -= a.blank_penalty;
          sm4[w] += wn_exp(v - mx);
        }
      }
    }
    lsum = logf(wave_sum(sm4[0]) + wave_sum(sm4[1]) + wave_sum(sm4[2]) + wave_sum(sm4[3]));
  }
  const int L = a.lab_len[b];
  const int* lab = a.lab + (int64_t)b * a.lab_pitch;
  float* e = a.E + (int64_t)row * a.ldE;
  for (int j = lane; j < a.lab_pitch; j += 64) {
    float r = 0.f;
    if (j <= L) {
      const int id = lab[j];
      float v = x[id];
      if (a.normalize) {
        if (id == a.blank) v -= a.blank_penalty;
        v = (v - mx) - lsum;
      }
      r = v;
    }
    e[j] = r;
  }
}

// ===========================================================================
// Viterbi trellis + backtrace.  States s = 0..2L: even = blank (column 0 of E), odd s = label
// (s - 1) / 2 (column (s + 1) / 2 of E).
//
// Fast form, S = 2L + 1 <= 64 NS: ONE wave per utterance, no barrier per frame.  Lane l owns
// the states l NS .. l NS + NS - 1 in registers (static indices only); the two values it needs
// from its left neighbour come by wave shuffles; E rows are fetched four frames ahead; the back
// pointers of a frame are one byte per lane (2 bits per state), in LDS while the utterance has
// at most ALIGN_BPF frames, in the workspace otherwise (read back chunk-wise into LDS).  States
// >= S are computed like the others: nothing below them depends on them and the end picks
// S - 1 / S - 2 by index.  The backtrace is lane 0 walking bytes in LDS; it leaves state
// indices there, which the whole wave then turns into labels, the path and the two
// log-probs of each frame the time-stamp rule reads (blank, and the label of the token group
// the frame belongs to: the next label at or behind it).
constexpr int ALIGN_BPF = 640;       // frames of back pointers in LDS (40 KiB)

__device__ __forceinline__ void align_finish_chunk(const AlignArgs& a, int b, int t0, int t1,
                                                   const short* spath, const short* sgrp,
                                                   const int* lab, int lane, int nthr) {
  const int64_t row0 = a.off[b];
  for (int t = t0 + lane; t < t1; t += nthr) {
    const int s = spath[t - t0];
    const int col = (s & 1) ? (s + 1) >> 1 : 0;
    a.path[(int64_t)b * a.Tp + t] = lab[col];
    if (a.frame_logp) {
      const float* e = a.E + (row0 + t) * a.ldE;
      float* o = a.frame_logp + ((int64_t)b * a.Tp + t) * 2;
      o[0] = e[0];
      o[1] = e[sgrp[t - t0]];
    }
  }
}

// feasible iff T >= L + #{i : y[i] == y[i-1]}; the whole block calls this
template <int NT>
__device__ __forceinline__ int align_repeats(const int* lab, int L, int* red) {
  int r = 0;
  for (int i = 2 + threadIdx.x; i <= L; i += NT) r += lab[i] == lab[i - 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
  if (NT == 64) return r;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  r = 0;
  for (int w = 0; w < NT / 64; ++w) r += red[w];
  __syncthreads();
  return r;
}

template <int NS>
__global__ __launch_bounds__(64) void align_wave_kernel(AlignArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sbp[ALIGN_BPF * 64];
  __shared__ short spath[ALIGN_BPF], sgrp[ALIGN_BPF];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = a.len[b], L = a.lab_len[b], S = 2 * L + 1;
  if (S > a.fast_S) return;            // the general kernel's utterance
  const int* lab = a.lab + (int64_t)b * a.lab_pitch;
  const int rep = align_repeats<64>(lab, L, nullptr);
  if (T < L + rep || T == 0) {
    if (lane == 0) { a.status[b] = T < L + rep ? 1 : 0; a.score[b] = 0.f; }
    return;
  }
  if (lane == 0) a.status[b] = 0;
  const float NINF = -INFINITY;
  const float* E = a.E + (int64_t)a.off[b] * a.ldE;
  const int ldE = a.ldE;
  // per state: column of E, skip transition allowed
  int col[NS];
  bool skip[NS];
  float al[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int s = lane * NS + j;
    const int c = (s & 1) ? min((s + 1) >> 1, L) : 0;
    col[j] = c;
    skip[j] = (s & 1) && s >= 3 && s < S && lab[c] != lab[c - 1];
    al[j] = s == 0 ? E[0] : (s == 1 && L > 0) ? E[1] : NINF;
  }
  const bool in_lds = T <= ALIGN_BPF;
  unsigned char* gbp = a.bp + a.bp_off[b];
  if (in_lds) sbp[lane] = 0; else gbp[lane] = 0;

  auto fetch = [&](float (&e)[NS], int t) {
    const float* r = E + (int64_t)min(t, T - 1) * ldE;
    if (NS == 1) {
      e[0] = r[col[0]];
    } else {
      const float eb = r[0];
#pragma unroll
      for (int j = 0; j < NS; ++j) e[j] = (j & 1) ? r[col[j]] : eb;
    }
  };
  auto step = [&](const float (&e)[NS], int t) {
    float up1 = __shfl_up(al[NS - 1], 1, 64);
    float up2 = NS >= 2 ? __shfl_up(al[NS >= 2 ? NS - 2 : 0], 1, 64) : __shfl_up(al[0], 2, 64);
    if (lane < 1) up1 = NINF;
    if (lane < (NS >= 2 ? 1 : 2)) up2 = NINF;
    float nx[NS];
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const float x1 = j >= 1 ? al[j >= 1 ? j - 1 : 0] : up1;
      const float x2c = j >= 2 ? al[j >= 2 ? j - 2 : 0] : (j == 1 ? up1 : up2);
      const float x2 = skip[j] ? x2c : NINF;
      float best = al[j];
      unsigned k = 0;
      if (x1 > best) { best = x1; k = 1; }
      if (x2 > best) { best = x2; k = 2; }
      nx[j] = best + e[j];
      bits |= k << (2 * j);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) al[j] = nx[j];
    if (in_lds) sbp[t * 64 + lane] = (unsigned char)bits;
    else gbp[(int64_t)t * 64 + lane] = (unsigned char)bits;
  };

  float ec[4][NS], en[4][NS];
#pragma unroll
  for (int u = 0; u < 4; ++u) fetch(ec[u], 1 + u);
  for (int t = 1; t < T; t += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) fetch(en[u], t + 4 + u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (t + u < T) step(ec[u], t + u);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < NS; ++j) ec[u][j] = en[u][j];
  }

  // the end: the last label unless the trailing blank is strictly better
  float v1 = NINF, v2 = NINF;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if (lane * NS + j == S - 1) v1 = al[j];
    if (lane * NS + j == S - 2) v2 = al[j];
  }
  v1 = __shfl(v1, (S - 1) / NS, 64);
  v2 = __shfl(v2, max(S - 2, 0) / NS, 64);
  int s = (S == 1 || v1 > v2) ? S - 1 : S - 2;
  if (lane == 0) a.score[b] = s == S - 1 ? v1 : v2;

  __threadfence();
  __syncthreads();
  int grp = 0;     // column of the next label at or behind the frame (0: trailing blanks)
  for (int t1 = T; t1 > 0;) {
    const int t0 = max(0, t1 - ALIGN_BPF);
    if (!in_lds) {
      const uint4* src = reinterpret_cast<const uint4*>(gbp + (int64_t)t0 * 64);
      uint4* dst = reinterpret_cast<uint4*>(sbp);
      for (int i = lane; i < (t1 - t0) * 4; i += 64) dst[i] = src[i];
      __syncthreads();
    }
    if (lane == 0) {
      for (int t = t1 - 1; t >= t0; --t) {
        spath[t - t0] = (short)s;
        if (s & 1) grp = (s + 1) >> 1;
        sgrp[t - t0] = (short)grp;
        const unsigned byte = sbp[(t - t0) * 64 + s / NS];
        s -= (byte >> (2 * (s % NS))) & 3;
      }
    }
    s = __shfl(s, 0, 64);
    __syncthreads();
    align_finish_chunk(a, b, t0, t1, spath, sgrp, lab, lane, 64);
    __syncthreads();
    t1 = t0;
  }
}

// General form, any S the LDS holds: 256 threads per utterance, the alphas of two frames in
// LDS, one barrier per frame; a thread takes four consecutive states at a time (one byte of back
// pointers) and only the reachable band max(0, S - 2 (T - t)) <= s <= min(S - 1, 2 t + 1) is
// worked on (states above it still hold their initial -inf in both buffers; states below it are
// never read by a state inside it).  Back pointers go to the workspace and come back chunk-wise
// into LDS for the walk.
constexpr int ALIGN_STG = 16384;     // bytes of back pointers staged per chunk
constexpr int ALIGN_STG_FRAMES = 512;

__global__ __launch_bounds__(256) void align_block_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  __shared__ int red[4];
  __shared__ int s_cur, s_grp;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.len[b], L = a.lab_len[b], S = 2 * L + 1;
  if (S <= a.fast_S) return;           // the wave kernel's utterance
  const int* lab = a.lab + (int64_t)b * a.lab_pitch;
  const int rep = align_repeats<256>(lab, L, red);
  if (T < L + rep || T == 0) {
    if (tid == 0) { a.status[b] = T < L + rep ? 1 : 0; a.score[b] = 0.f; }
    return;
  }
  if (tid == 0) a.status[b] = 0;
  const int S16 = (S + 15) & ~15, rowb = S16 >> 2;
  float* A0 = reinterpret_cast<float*>(dyn);
  float* A1 = A0 + S16;
  int* slab = reinterpret_cast<int*>(A1 + S16);          // L + 1 labels
  int* ipath = slab + ((L + 1 + 3) & ~3);                // ALIGN_STG_FRAMES state indices
  int* igrp = ipath + ALIGN_STG_FRAMES;                  // ... and group label columns
  unsigned char* stg = reinterpret_cast<unsigned char*>(igrp + ALIGN_STG_FRAMES);
  const float NINF = -INFINITY;
  const float* E = a.E + (int64_t)a.off[b] * a.ldE;
  for (int i = tid; i < S16; i += 256) { A0[i] = NINF; A1[i] = NINF; }
  for (int i = tid; i <= L; i += 256) slab[i] = lab[i];
  __syncthreads();
  if (tid == 0) { A0[0] = E[0]; if (L > 0) A0[1] = E[1]; }
  unsigned char* gbp = a.bp + a.bp_off[b];
  __syncthreads();
  float* prev = A0;
  float* cur = A1;
  for (int t = 1; t < T; ++t) {
    const float* er = E + (int64_t)t * a.ldE;
    const float eb = er[0];
    const int lo = max(0, S - 2 * (T - t)) & ~3, hi = min(S - 1, 2 * t + 1);
    for (int g = (lo >> 2) + tid; 4 * g <= hi; g += 256) {
      const int s0 = 4 * g;
      float p[6];                      // prev[s0 - 2 .. s0 + 3]
      p[0] = s0 >= 2 ? prev[s0 - 2] : NINF;
      p[1] = s0 >= 1 ? prev[s0 - 1] : NINF;
#pragma unroll
      for (int j = 0; j < 4; ++j) p[2 + j] = prev[s0 + j];
      unsigned bits = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = s0 + j;
        const bool odd = j & 1;
        const int c = odd ? min((s + 1) >> 1, L) : 0;
        const bool sk = odd && s >= 3 && s < S && slab[c] != slab[c - 1];
        const float e = odd ? er[c] : eb;
        const float x1 = p[1 + j], x2 = sk ? p[j] : NINF;
        float best = p[2 + j];
        unsigned k = 0;
        if (x1 > best) { best = x1; k = 1; }
        if (x2 > best) { best = x2; k = 2; }
        cur[s] = best + e;
        bits |= k << (2 * j);
      }
      gbp[(int64_t)t * rowb + g] = (unsigned char)bits;
    }
    __syncthreads();
    float* sw = prev; prev = cur; cur = sw;
  }
  if (tid == 0) {
    const float v1 = prev[S - 1], v2 = S >= 2 ? prev[S - 2] : NINF;
    const int s = (S == 1 || v1 > v2) ? S - 1 : S - 2;
    a.score[b] = s == S - 1 ? v1 : v2;
    s_cur = s;
    s_grp = 0;
  }
  __threadfence();
  __syncthreads();
  const int cf = max(1, min(ALIGN_STG_FRAMES, ALIGN_STG / rowb));
  for (int t1 = T; t1 > 0;) {
    const int t0 = max(0, t1 - cf);
    {
      // frame 0 has no back pointers (never written): its bits are read and ignored
      const int tb = max(t0, 1);
      const unsigned* src = reinterpret_cast<const unsigned*>(gbp + (int64_t)tb * rowb);
      unsigned* dst = reinterpret_cast<unsigned*>(stg + (int64_t)(tb - t0) * rowb);
      for (int i = tid; i < (t1 - tb) * (rowb >> 2); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    if (tid == 0) {
      int s = s_cur, grp = s_grp;
      for (int t = t1 - 1; t >= t0; --t) {
        ipath[t - t0] = s;
        if (s & 1) grp = (s + 1) >> 1;
        igrp[t - t0] = grp;
        if (t > 0) s -= (stg[(t - t0) * rowb + (s >> 2)] >> (2 * (s & 3))) & 3;
      }
      s_cur = s;
      s_grp = grp;
    }
    __syncthreads();
    const int64_t row0 = a.off[b];
    for (int t = t0 + tid; t < t1; t += 256) {
      const int s = ipath[t - t0];
      const int col = (s & 1) ? (s + 1) >> 1 : 0;
      a.path[(int64_t)b * a.Tp + t] = slab[col];
      if (a.frame_logp) {
        const float* e = a.E + (row0 + t) * a.ldE;
        float* o = a.frame_logp + ((int64_t)b * a.Tp + t) * 2;
        o[0] = e[0];
        o[1] = e[igrp[t - t0]];
      }
    }
    __syncthreads();
    t1 = t0;
  }
}

}  // namespace

int ctc_align_gather(const AlignGatherArgs& a, hipStream_t s) {
  WN_CHECK(a.M > 0 && a.V > 0 && a.lab_pitch >= 1 && a.ldE >= a.lab_pitch, "align gather: empty");
  hipLaunchKernelGGL(align_gather_kernel, dim3(cdiv(a.M, 4)), dim3(256), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int64_t ctc_align_bp_bytes(int T, int L, int fast_S) {
  const int S = 2 * L + 1;
  const int64_t row = S <= fast_S ? 64 : ((S + 15) & ~15) >> 2;
  return ((int64_t)(T > 1 ? T : 1) * row + 15) / 16 * 16;
}

size_t ctc_align_block_lds(int max_L) {
  const size_t S16 = (size_t)((2 * max_L + 1 + 15) & ~15);
  return 2 * S16 * sizeof(float) + (size_t)((max_L + 1 + 3) & ~3) * sizeof(int) +
         2 * ALIGN_STG_FRAMES * sizeof(int) + ALIGN_STG;
}

int ctc_align_viterbi(const AlignArgs& a_in, int max_fast_L, int max_slow_L, hipStream_t s) {
  AlignArgs a = a_in;
  WN_CHECK(a.B > 0, "align: empty batch");
  WN_CHECK(a.fast_S == ALIGN_FAST_S, "align: fast_S must be ALIGN_FAST_S");
  if (max_fast_L >= 0) {
    const int S = 2 * max_fast_L + 1;
    if (S <= 64) hipLaunchKernelGGL(align_wave_kernel<1>, dim3(a.B), dim3(64), 0, s, a);
    else if (S <= 128) hipLaunchKernelGGL(align_wave_kernel<2>, dim3(a.B), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(align_wave_kernel<4>, dim3(a.B), dim3(64), 0, s, a);
    WN_HIP(hipGetLastError());
  }
  if (max_slow_L >= 0) {
    const size_t lds = ctc_align_block_lds(max_slow_L);
    WN_CHECK(lds <= 150 * 1024, "align: label sequence too long for the LDS trellis");
    WN_CHECK(((2 * max_slow_L + 1 + 15) & ~15) / 4 <= ALIGN_STG,
             "align: label sequence too long for the back pointer staging");
    WN_MAX_DYN_LDS(align_block_kernel, 150 * 1024);
    hipLaunchKernelGGL(align_block_kernel, dim3(a.B), dim3(256), lds, s, a);
    WN_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace wn
