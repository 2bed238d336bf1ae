// RNN-T prefix beam search (wenet/models/transducer/search/prefix_beam_search.py:66-148 for a
// whole batch in lock-step, one frame per step), fp32 rows and fp64 scores.
//
// Two facts make the batched form cheap:
//  * the predictor state and pred_out of a hypothesis are functions of its token sequence alone;
//  * rnnt_linear_kernel (transducer.hip) sums every row in one order whatever else the batch
//    holds.
// So a slot keeps the state reached after its WHOLE hypothesis together with its pred_proj row
// (the reference keeps the state after hyp[:-1] and runs the predictor on hyp[-1] for every
// hypothesis every frame): a blank-extended or fused-into-blank slot copies them, and only the
// slots that appended a token run the LSTM step (`advance`) -- the same bits as re-running the
// predictor every frame.  Kernels, per frame after the predictor step and rnnt_joint_rows:
//  * rnnt_fuse_topk_kernel   one block per live joint row, the row in LDS: log-sum-exp,
//    f[v] = log(tw exp(logp[v]) + cw exp(ctc[v])) with exp / log in fp64 and one rounding to fp32
//    (a fused value decides beam membership; the row's sum of exponentials is an fp32 sum of the
//    accurate expf) and the k largest (value, index): larger value first, the lower
//    index on equal values (the order of ctc_row_kernel).  A NaN ranks, and is returned, as -inf,
//    so the k indices are always distinct columns in [0, V): the next embedding read depends on it;
//  * rnnt_beam_step_kernel   one workgroup per utterance, one thread per candidate (at most
//    beam^2 = 256): candidate scores float32(score) + value held as doubles, the prefix fusion,
//    the stable rank and the cut, the new slots' token rows and the row map of the next frame.
//    Prefix identity is the token sequence, decided exactly on the flat token rows (compared in
//    full when length and last token match; no hash, no ids -- an id assigned at creation is not
//    an identity, ctc.hip explains why).  Live hypotheses are distinct, so the only possible
//    fusion is the blank candidate of slot j2 with the token candidate (j, k) where
//    hyp[j2] == hyp[j] + [k]: pairs, each summed once with log_add in fp64, the entry keeping
//    the earlier place in the j-major list.  The fused entry copies slot j2 (no LSTM step).
//    A NaN score ranks as -inf (the rule of beam_update_kernel): the rank is a permutation for
//    every input;
//  * rnnt_beam_gather_kernel h, c and pred_proj rows of the new slots from their source slots,
//    double buffered.
// No kernel waits for another workgroup; the host issues `longest T'` steps without looking at
// the device.  Rows of empty slots and finished utterances are inert (row_enc < 0).
// The resumable search (transducer_beam_stream.hip) runs the same kernels on a compact batch of
// sessions; rnnt_beam_step_kernel's carry mode (RnntBeamStepArgs::pending != nullptr, kernels.h)
// is what differs on a session's last frame of a call and behind it.  Without those pointers the
// kernel does what it did before they existed.
#include "kernels.h"

namespace wn {
namespace {

constexpr int BS_MAX_BEAM = 16;
constexpr int BS_THREADS = BS_MAX_BEAM * BS_MAX_BEAM;

struct VI { float v; int i; };
__device__ __forceinline__ VI vi_better(VI a, VI b) {
  // larger value first; on ties the lower index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ VI vi_wave(VI x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VI y;
    y.v = __shfl_xor(x.v, o, 64);
    y.i = __shfl_xor(x.i, o, 64);
    x = vi_better(x, y);
  }
  return x;
}

__global__ __launch_bounds__(256) void rnnt_fuse_topk_kernel(RnntFuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ float red[8];
  __shared__ VI redvi[4];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int re = a.row_enc[row];
  if (re < 0) {                      // an empty slot or a finished utterance
    if (tid < a.k) {
      a.val[(int64_t)row * a.k + tid] = -INFINITY;
      a.idx[(int64_t)row * a.k + tid] = -1;
    }
    return;
  }
  const float* x = a.logits + (int64_t)row * a.ldl;
  float mx = -INFINITY;
  for (int i = tid; i < a.V; i += 256) {
    const float v = x[i];
    srow[i] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sm = 0.f;
  for (int i = tid; i < a.V; i += 256) sm += expf(srow[i] - mx);
  sm = wave_sum(sm);
  if (lane == 0) red[4 + wave] = sm;
  __syncthreads();
  const double lsum = log((double)(((red[4] + red[5]) + red[6]) + red[7]));
  const float* c = a.cw != 0.f ? a.ctc + (int64_t)(a.row_ctc ? a.row_ctc[row] : re) * a.ldc : nullptr;
  float* fo = a.fused ? a.fused + (int64_t)row * a.ldf : nullptr;
  for (int i = tid; i < a.V; i += 256) {       // (each thread rewrites its own elements)
    // exp / log in fp64, rounded to fp32 once: log(exp(x)) through 1-ulp fp32 functions is off
    // by an ulp of x (2e-6 at x = -20), which is the size of the gaps that decide the beam
    const double lp = ((double)srow[i] - (double)mx) - lsum;
    double p = (double)a.tw * exp(lp);
    if (c) p += (double)a.cw * exp((double)c[i]);
    const float f = (float)log(p);
    if (fo) fo[i] = f;
    srow[i] = f == f ? f : -INFINITY;          // the ranking key; a taken element becomes NaN
  }
  // k rounds of one block arg-max; only the winner's owner rescans its elements
  auto local_best = [&]() {
    VI best;
    best.v = -INFINITY;
    best.i = 0x7fffffff;
    for (int i = tid; i < a.V; i += 256) {
      const float v = srow[i];
      if (v == v && (best.i == 0x7fffffff || v > best.v)) { best.v = v; best.i = i; }
    }
    return best;
  };
  VI mine = local_best();
  for (int r = 0; r < a.k; ++r) {
    const VI wb = vi_wave(mine);
    if (lane == 0) redvi[wave] = wb;
    __syncthreads();
    const VI b = vi_better(vi_better(redvi[0], redvi[1]), vi_better(redvi[2], redvi[3]));
    // k <= V: an element that was not taken always exists, so b.i is a column
    if (tid == 0) {
      a.val[(int64_t)row * a.k + r] = b.v;
      a.idx[(int64_t)row * a.k + r] = b.i;
    }
    if (b.i < a.V && (b.i & 255) == tid) {
      srow[b.i] = __builtin_nanf("");
      mine = local_best();
    }
    __syncthreads();
  }
}

// wenet/utils/common.py:302-310 for two values: max + log(exp(a - max) + exp(b - max)), where
// the term of the maximum is exp(0) = 1 exactly.  Two -inf give -inf; a NaN gives NaN.
__device__ __forceinline__ double log_add2(double a, double b) {
  if (a != a || b != b) return __builtin_nan("");
  if (a == -INFINITY && b == -INFINITY) return -INFINITY;
  const double m = a > b ? a : b, n = a > b ? b : a;
  return m + log(1.0 + exp(n - m));
}

__global__ __launch_bounds__(256) void rnnt_beam_init_kernel(RnntBeamSlots st, int* last_tok,
                                                             int* advance, int* row_enc,
                                                             int* row_pred,
                                                             const int* __restrict__ off,
                                                             const int* __restrict__ len, int B,
                                                             int beam, int blank) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * beam) return;
  const int b = g / beam, s = g - b * beam;
  const bool first = s == 0 && len[b] > 0;     // [blank], score 0.0, on a zero LSTM state
  st.score[g] = s == 0 ? 0.0 : -INFINITY;
  st.tok_len[g] = 0;
  last_tok[g] = blank;
  advance[g] = first;
  row_enc[g] = first ? off[b] : -1;
  row_pred[g] = g;
  if (s == 0) st.n_live[b] = 1;
}

__global__ __launch_bounds__(BS_THREADS) void rnnt_beam_step_kernel(RnntBeamStepArgs a) {
  __shared__ double c_sc[BS_THREADS];
  __shared__ int c_tok[BS_THREADS];     // the appended token; -1: the entry keeps its hypothesis
  __shared__ int c_src[BS_THREADS];     // slot (of this utterance) the entry copies
  __shared__ int c_alive[BS_THREADS];
  __shared__ int s_len[BS_MAX_BEAM], s_last[BS_MAX_BEAM], s_brank[BS_MAX_BEAM];
  __shared__ int w_cand[BS_MAX_BEAM];
  __shared__ int n_alive;
  const int b = blockIdx.x, tid = threadIdx.x, beam = a.beam;
  const int g0 = b * beam;
  const int n = min(max(a.in.n_live[b], 0), beam);
  const int len = a.len[b];
  const int64_t mt = a.max_tok;

  const bool carry = a.pending != nullptr;     // the resumable search (kernels.h)
  if (a.frame >= len) {      // finished (or empty): the slots move on as they are, inert
    if (tid < beam) {
      const int g = g0 + tid;
      a.out.score[g] = tid < n ? a.in.score[g] : -INFINITY;
      a.out.tok_len[g] = tid < n ? min(max(a.in.tok_len[g], 0), a.max_tok) : 0;
      a.advance[g] = 0; a.row_enc[g] = -1;
      if (carry) {           // the state goes along in both parities; last_tok / pending stay
        a.src[g] = tid < n ? g : -1;
        a.last_time_out[g] = tid < n ? a.last_time_in[g] : -1;
      } else {
        a.src[g] = -1; a.last_tok[g] = a.blank;
      }
    }
    if (tid == 0) a.out.n_live[b] = n;
    for (int s = 0; s < n; ++s) {
      const int l = min(max(a.in.tok_len[g0 + s], 0), a.max_tok);
      for (int t = tid; t < l; t += BS_THREADS)
        a.out.tokens[(g0 + s) * mt + t] = a.in.tokens[(g0 + s) * mt + t];
    }
    return;
  }

  if (tid < beam) {
    int l = 0, last = -1;
    if (tid < n) {
      l = min(max(a.in.tok_len[g0 + tid], 0), a.max_tok);
      if (l > 0) last = a.in.tokens[(g0 + tid) * mt + l - 1];
    }
    s_len[tid] = l; s_last[tid] = last; s_brank[tid] = 0x7fffffff;
  }
  if (tid == 0) n_alive = 0;
  c_alive[tid] = 0;
  __syncthreads();

  // ---- candidates, j-major and top-k-rank-minor (beam_A) --------------------------------------
  const int j = tid / beam, r = tid - j * beam;
  const bool have = tid < n * beam;
  int tok = -1;
  if (have) {
    const int ti = a.top_idx[(int64_t)(g0 + j) * beam + r];
    if ((unsigned)ti < (unsigned)a.V) {       // (anything else is no token: dropped)
      const float v = a.top_val[(int64_t)(g0 + j) * beam + r];
      // torch.add of the fp32 score row and the fp32 top-k value, then .item()
      c_sc[tid] = (double)((float)a.in.score[g0 + j] + v);
      c_src[tid] = j;
      c_alive[tid] = 1;
      if (ti == a.blank) atomicMin(&s_brank[j], r); else tok = ti;
      c_tok[tid] = tok;
    }
  }
  __syncthreads();

  // ---- prefix fusion: token candidate (j, tok) with the blank candidate of the slot j2 whose
  //      hypothesis is hyp[j] + [tok]; the pairs are disjoint, the token's thread sums ----------
  if (tok >= 0) {
    const int L = s_len[j];
    int partner = -1;
    for (int j2 = 0; j2 < n && partner < 0; ++j2) {
      if (j2 == j || s_len[j2] != L + 1 || s_last[j2] != tok || s_brank[j2] == 0x7fffffff) continue;
      const int* pa = a.in.tokens + (g0 + j) * mt;
      const int* pb = a.in.tokens + (g0 + j2) * mt;
      bool eq = true;
      for (int t = 0; t < L && eq; ++t) eq = pa[t] == pb[t];
      if (eq) partner = j2 * beam + s_brank[j2];
    }
    if (partner >= 0) {
      const int first = min(tid, partner), other = max(tid, partner);
      c_sc[first] = log_add2(c_sc[first], c_sc[other]);
      c_tok[first] = -1;
      c_src[first] = partner / beam;
      c_alive[other] = 0;
    }
  }
  __syncthreads();

  // ---- stable rank, descending; a NaN as -inf; equal scores keep list order --------------------
  if (c_alive[tid]) {
    const double mine = c_sc[tid] == c_sc[tid] ? c_sc[tid] : -INFINITY;
    int rank = 0;
    for (int c = 0; c < n * beam; ++c) {
      if (!c_alive[c]) continue;
      const double o = c_sc[c] == c_sc[c] ? c_sc[c] : -INFINITY;
      rank += (o > mine || (o == mine && c < tid)) ? 1 : 0;
    }
    if (rank < beam) w_cand[rank] = tid;
    atomicAdd(&n_alive, 1);
  }
  __syncthreads();

  // ---- the new slots --------------------------------------------------------------------------
  const int n_new = min(beam, n_alive);
  const bool more = a.frame + 1 < len;      // the utterance has another frame
  if (tid < beam) {
    const int g = g0 + tid;
    if (tid < n_new) {
      const int c = w_cand[tid], sj = c_src[c], t = c_tok[c];
      a.out.score[g] = c_sc[c];
      a.out.tok_len[g] = min(s_len[sj] + (t >= 0 ? 1 : 0), a.max_tok);
      a.src[g] = (more || carry) ? g0 + sj : -1;
      a.last_tok[g] = t >= 0 ? t : a.blank;
      const int adv = (t >= 0 && more) ? 1 : 0;
      a.advance[g] = adv;
      if (carry) {           // the step behind a token on the call's last frame is owed
        a.pending[g] = (t >= 0 && !more) ? 1 : 0;
        a.last_time_out[g] = t >= 0 ? a.frame0[b] + a.frame : a.last_time_in[g0 + sj];
      }
      if (adv && a.n_advance) atomicAdd(a.n_advance, 1);     // (a statistic: rows of LSTM steps)
      a.row_enc[g] = more ? a.off[b] + a.frame + 1 : -1;
      if (t >= 0 && s_len[sj] < a.max_tok) a.out.tokens[g * mt + s_len[sj]] = t;
    } else {
      a.out.score[g] = -INFINITY;
      a.out.tok_len[g] = 0;
      a.src[g] = -1; a.last_tok[g] = a.blank; a.advance[g] = 0; a.row_enc[g] = -1;
      if (carry) { a.pending[g] = 0; a.last_time_out[g] = -1; }
    }
  }
  if (tid == 0) a.out.n_live[b] = n_new;
  for (int s = 0; s < n_new; ++s) {
    const int sj = c_src[w_cand[s]], l = s_len[sj];
    for (int t = tid; t < l; t += BS_THREADS)
      a.out.tokens[(g0 + s) * mt + t] = a.in.tokens[(g0 + sj) * mt + t];
  }
}

__global__ __launch_bounds__(256) void rnnt_beam_gather_kernel(
    const int* __restrict__ src, const float* __restrict__ h_in, const float* __restrict__ c_in,
    const float* __restrict__ pp_in, float* __restrict__ h_out, float* __restrict__ c_out,
    float* __restrict__ pp_out, int M, int L, int H, int J) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int sj = src[g];
  if (sj < 0 || sj >= M) return;
  for (int l = 0; l < L; ++l) {
    const int64_t o = ((int64_t)l * M + g) * H, i = ((int64_t)l * M + sj) * H;
    for (int k = tid; k < H; k += 256) { h_out[o + k] = h_in[i + k]; c_out[o + k] = c_in[i + k]; }
  }
  for (int k = tid; k < J; k += 256) pp_out[(int64_t)g * J + k] = pp_in[(int64_t)sj * J + k];
}

}  // namespace

int rnnt_fuse_topk(const RnntFuseArgs& a, hipStream_t s) {
  WN_CHECK(a.logits && a.row_enc && a.val && a.idx, "rnnt_fuse_topk: null operand");
  WN_CHECK(a.M >= 1 && a.V >= 1 && a.ldl >= a.V, "rnnt_fuse_topk: empty, or a pitch below V");
  WN_CHECK(a.k >= 1 && a.k <= BS_MAX_BEAM && a.k <= a.V,
           "rnnt_fuse_topk: k must be in [1, 16] and at most the vocabulary");
  WN_CHECK(a.cw >= 0.f && a.tw >= 0.f && (a.cw > 0.f || a.tw > 0.f),
           "rnnt_fuse_topk: the weights must be >= 0 and not both 0");
  WN_CHECK(a.cw == 0.f || (a.ctc && a.ldc >= a.V), "rnnt_fuse_topk: ctc_weight without CTC rows");
  WN_CHECK(!a.fused || a.ldf >= a.V, "rnnt_fuse_topk: fused pitch below V");
  const size_t lds = (size_t)a.V * sizeof(float);
  WN_CHECK(lds <= 120 * 1024, "rnnt_fuse_topk: vocabulary too large for the LDS row buffer");
  WN_MAX_DYN_LDS(rnnt_fuse_topk_kernel, 120 * 1024);
  hipLaunchKernelGGL(rnnt_fuse_topk_kernel, dim3(a.M), dim3(256), lds, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_beam_init(const RnntBeamSlots& st, int* last_tok, int* advance, int* row_enc,
                   int* row_pred, const int* off, const int* len, int B, int beam, int blank, hipStream_t s) {
  WN_CHECK(B >= 1 && beam >= 1 && beam <= BS_MAX_BEAM, "rnnt_beam_init: beam must be in [1, 16]");
  hipLaunchKernelGGL(rnnt_beam_init_kernel, dim3(cdiv(B * beam, 256)), dim3(256), 0, s, st,
                     last_tok, advance, row_enc, row_pred, off, len, B, beam, blank);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_beam_step(const RnntBeamStepArgs& a, hipStream_t s) {
  WN_CHECK(a.in.n_live && a.in.score && a.in.tok_len && a.in.tokens && a.out.n_live &&
           a.out.score && a.out.tok_len && a.out.tokens && a.top_val && a.top_idx && a.off &&
           a.len && a.src && a.last_tok && a.advance && a.row_enc, "rnnt_beam_step: null operand");
  WN_CHECK(a.B >= 1 && a.beam >= 1 && a.beam <= BS_MAX_BEAM, "rnnt_beam_step: beam must be in [1, 16]");
  WN_CHECK(a.max_tok >= 1 && a.V >= 1 && a.frame >= 0, "rnnt_beam_step: empty");
  WN_CHECK(!a.pending || (a.last_time_in && a.last_time_out && a.frame0),
           "rnnt_beam_step: carry mode needs last_time_in / last_time_out / frame0");
  hipLaunchKernelGGL(rnnt_beam_step_kernel, dim3(a.B), dim3(BS_THREADS), 0, s, a);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_beam_gather(const int* src, const float* h_in, const float* c_in, const float* pp_in,
                     float* h_out, float* c_out, float* pp_out, int M, int L, int H, int J,
                     hipStream_t s) {
  hipLaunchKernelGGL(rnnt_beam_gather_kernel, dim3(M), dim3(256), 0, s, src, h_in, c_in, pp_in,
                     h_out, c_out, pp_out, M, L, H, J);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
