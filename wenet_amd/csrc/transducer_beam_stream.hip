// Resumable RNN-T prefix beam search: the lock-step search of transducer_beam.hip for sessions
// that receive their encoder frames in pieces (wn_rnnt_beam_stream_*,
// cabi_transducer_beam_stream.hip), fp32 rows and fp64 scores.
//
// A session's state -- per session n_live and frames, per slot the score, the token row, the last
// token, `pending`, last_time, the LSTM's h / c and the projected predictor output -- lives in
// HBM between calls (RnntBeamStreamSlots).  A call over n sessions gathers them into a compact
// batch of M = n x beam rows, runs the one-shot search's own per-frame kernels on it
// (predictor_step, rnnt_linear, rnnt_joint_rows, rnnt_fuse_topk, rnnt_beam_step in carry mode,
// rnnt_beam_gather: a row's sums keep their one fixed order, so a session's state depends neither
// on the pieces nor on its slot nor on the other sessions of the call) and scatters it back.
//  * rnnt_beam_stream_begin_kernel  slots -> compact batch, parity 0.  advance = pending &&
//    n_t > 0: the predictor step that the previous call owed (`pending` is the greedy search's
//    `stale`); off = i * chunk, len = n_t, the first row map;
//  * the carry mode of rnnt_beam_step_kernel (transducer_beam.hip): on a session's last frame of
//    the call the one-shot kernel hands no state on (src = -1, advance = 0: nothing follows).
//    Here a later call may follow: src is written as usual, the owed step of a token-appending
//    slot goes to `pending`, row_enc stays -1.  On the later steps of the call (sessions with a
//    smaller n_t, or n_t = 0) the session's slots move on with an IDENTITY src and advance = 0,
//    the slot arrays copied in to out: rnnt_beam_gather skips src < 0, so without it the rows of
//    the other parity would be two steps old.  Every session is therefore whole in the parity
//    the call ends in, whatever its own n_t;
//  * rnnt_beam_stream_end_kernel    that parity -> slots, frames += n_t, the call's results.
//    Dead slots (>= n_live) and token entries behind tok_len are stored in one canonical form,
//    so a session's stored state is a function of its frames alone, bit for bit;
//  * rnnt_beam_stream_reset_kernel  the state rnnt_beam_init gives an utterance.
// Plain stream-ordered launches; every store is a vector store.
#include "kernels.h"

namespace wn {
namespace {

__global__ __launch_bounds__(256) void rnnt_beam_stream_begin_kernel(RnntBeamStreamSlots sl,
                                                                     RnntBeamStreamCall c, int n,
                                                                     int chunk) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = c.slot[i], nt = c.n_t[i];
  const int beam = sl.beam, L = sl.L, H = sl.H, J = sl.J, M = n * beam;
  const int n_live = min(max(sl.n_live[slot], 0), beam);
  const bool go = nt > 0;
  for (int j = 0; j < beam; ++j) {
    const int q = slot * beam + j, g = i * beam + j;
    for (int e = tid; e < L * H; e += 256) {
      const int l = e / H, k = e - l * H;
      const int64_t src = ((int64_t)q * L + l) * H + k, dst = ((int64_t)l * M + g) * H + k;
      c.h[dst] = sl.h[src];
      c.c[dst] = sl.c[src];
    }
    for (int k = tid; k < J; k += 256) c.pred_proj[(int64_t)g * J + k] = sl.pred_proj[(int64_t)q * J + k];
    const int tl = j < n_live ? min(max(sl.tok_len[q], 0), sl.max_tok) : 0;   // <= c.max_tok
    for (int t = tid; t < tl; t += 256)
      c.st.tokens[(int64_t)g * c.max_tok + t] = sl.tokens[(int64_t)q * sl.max_tok + t];
    if (tid == 0) {
      const bool live = j < n_live;
      const int pend = live ? sl.pending[q] : 0;
      c.st.score[g] = live ? sl.score[q] : -INFINITY;
      c.st.tok_len[g] = tl;
      c.last_time[g] = live ? sl.last_time[q] : -1;
      c.last_tok[g] = sl.last_tok[q];
      c.advance[g] = (go && pend != 0) ? 1 : 0;
      c.pending[g] = go ? 0 : pend;           // the step runs in this call
      c.row_enc[g] = (go && live) ? i * chunk : -1;
      c.row_pred[g] = g;
    }
  }
  if (tid == 0) {
    c.st.n_live[i] = n_live;
    c.off[i] = i * chunk;
    c.len[i] = max(nt, 0);
    c.frame0[i] = sl.frames[slot];
  }
}

__global__ __launch_bounds__(256) void rnnt_beam_stream_end_kernel(RnntBeamStreamSlots sl,
                                                                   RnntBeamStreamCall c, int n,
                                                                   int blank) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = c.slot[i], nt = c.n_t[i];
  const int beam = sl.beam, L = sl.L, H = sl.H, J = sl.J, M = n * beam;
  const int n_live = min(max(c.st.n_live[i], 0), beam);
  const int frames = min(c.frame0[i] + max(nt, 0), sl.max_tok);   // (the host refuses more)
  for (int j = 0; j < beam; ++j) {
    const int q = slot * beam + j, g = i * beam + j;
    const bool live = j < n_live;
    for (int e = tid; e < L * H; e += 256) {
      const int l = e / H, k = e - l * H;
      const int64_t dst = ((int64_t)q * L + l) * H + k, src = ((int64_t)l * M + g) * H + k;
      sl.h[dst] = live ? c.h[src] : 0.f;
      sl.c[dst] = live ? c.c[src] : 0.f;
    }
    for (int k = tid; k < J; k += 256)
      sl.pred_proj[(int64_t)q * J + k] = live ? c.pred_proj[(int64_t)g * J + k] : 0.f;
    const int tl = live ? min(min(max(c.st.tok_len[g], 0), c.max_tok), frames) : 0;
    for (int t = tid; t < frames; t += 256) {
      const int v = t < tl ? c.st.tokens[(int64_t)g * c.max_tok + t] : -1;
      sl.tokens[(int64_t)q * sl.max_tok + t] = v;
      if (t < tl && t < c.ld_out) c.out_tok[(int64_t)g * c.ld_out + t] = v;
    }
    if (tid == 0) {
      const double sc = live ? c.st.score[g] : -INFINITY;
      sl.score[q] = sc;
      sl.tok_len[q] = tl;
      sl.last_tok[q] = live ? c.last_tok[g] : blank;
      sl.pending[q] = live ? c.pending[g] : 0;
      sl.last_time[q] = live ? c.last_time[g] : -1;
      c.out_len[g] = tl;
      c.out_score[g] = sc;
    }
  }
  if (tid == 0) {
    const int lt = n_live > 0 ? c.last_time[i * beam] : -1;     // of the best hypothesis
    sl.n_live[slot] = n_live;
    sl.frames[slot] = frames;
    c.out_stat[i] = n_live;
    c.out_stat[n + i] = frames;
    c.out_stat[2 * n + i] = frames - 1 - lt;
  }
}

__global__ __launch_bounds__(256) void rnnt_beam_stream_reset_kernel(RnntBeamStreamSlots sl,
                                                                     const int* __restrict__ slots,
                                                                     int blank) {
  const int slot = slots[blockIdx.x], tid = threadIdx.x;
  const int beam = sl.beam;
  const int64_t q0 = (int64_t)slot * beam;
  const int64_t n_state = (int64_t)beam * sl.L * sl.H, n_pp = (int64_t)beam * sl.J,
                n_tok = (int64_t)beam * sl.max_tok;
  for (int64_t e = tid; e < n_state; e += 256) {
    sl.h[q0 * sl.L * sl.H + e] = 0.f;
    sl.c[q0 * sl.L * sl.H + e] = 0.f;
  }
  for (int64_t e = tid; e < n_pp; e += 256) sl.pred_proj[q0 * sl.J + e] = 0.f;
  for (int64_t e = tid; e < n_tok; e += 256) sl.tokens[q0 * sl.max_tok + e] = -1;
  if (tid < beam) {
    const int64_t q = q0 + tid;
    sl.score[q] = tid == 0 ? 0.0 : -INFINITY;      // one live hypothesis [], score 0.0
    sl.tok_len[q] = 0;
    sl.last_tok[q] = blank;
    sl.pending[q] = tid == 0 ? 1 : 0;     // the predictor's first step: blank on a zero state
    sl.last_time[q] = -1;
  }
  if (tid == 0) { sl.n_live[slot] = 1; sl.frames[slot] = 0; }
}

bool beam_stream_dims_ok(const RnntBeamStreamSlots& sl) {
  return sl.beam >= 1 && sl.beam <= 16 && sl.L >= 0 && sl.H >= 0 && sl.J >= 1 && sl.max_tok >= 1;
}

}  // namespace

int rnnt_beam_stream_begin(const RnntBeamStreamSlots& sl, const RnntBeamStreamCall& c, int n,
                           int chunk, hipStream_t s) {
  WN_CHECK(n >= 1 && chunk >= 1 && beam_stream_dims_ok(sl) && c.max_tok >= sl.max_tok,
           "rnnt_beam_stream_begin: bad argument");
  hipLaunchKernelGGL(rnnt_beam_stream_begin_kernel, dim3(n), dim3(256), 0, s, sl, c, n, chunk);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_beam_stream_end(const RnntBeamStreamSlots& sl, const RnntBeamStreamCall& c, int n,
                         int blank, hipStream_t s) {
  WN_CHECK(n >= 1 && c.ld_out >= 1 && beam_stream_dims_ok(sl) && c.max_tok >= sl.max_tok,
           "rnnt_beam_stream_end: bad argument");
  hipLaunchKernelGGL(rnnt_beam_stream_end_kernel, dim3(n), dim3(256), 0, s, sl, c, n, blank);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_beam_stream_reset(const RnntBeamStreamSlots& sl, const int* slot, int n, int blank,
                           hipStream_t s) {
  WN_CHECK(n >= 1 && slot && beam_stream_dims_ok(sl), "rnnt_beam_stream_reset: bad argument");
  hipLaunchKernelGGL(rnnt_beam_stream_reset_kernel, dim3(n), dim3(256), 0, s, sl, slot, blank);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
