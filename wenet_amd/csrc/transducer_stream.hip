// Resumable RNN-T greedy search: the lock-step search of transducer.hip for sessions that
// receive their encoder frames in pieces (wn_rnnt_stream_*, cabi_transducer_stream.hip), fp32.
//
// A session's state -- the LSTM's h / c, the projected predictor output, the last token, the
// tokens with their frames, the frame counters -- lives in its slot in HBM between calls.  A call
// over n sessions gathers their predictor state into a compact [n] batch, runs the one-shot
// search's own kernels on it (rnnt_linear_kernel, rnnt_cell_kernel, rnnt_joint_kernel: a row's
// sums keep their one fixed order, so a session's state depends neither on the window nor on the
// other sessions of the call nor on its slot) and scatters the state back.  Kernels:
//  * rnnt_stream_begin_kernel    slot -> compact batch; advance = stale && n_t > 0 (the
//    predictor step that the previous call owed), done = n_t <= 0, first row map, n_active;
//  * rnnt_stream_advance_kernel  rnnt_advance_kernel's rule over the call's frames, a wave per
//    session; tokens and their absolute frames go to the slot's own buffers.  The one-shot kernel
//    drops the predictor step behind a token that the n_steps cap emits on the last frame
//    (`advance = adv && !done`: nothing follows); here a later call may follow, so the slot is
//    marked `stale` and the next call with frames runs the step first;
//  * rnnt_stream_end_kernel      compact batch -> slot, frames += n_t, the call's results;
//  * rnnt_stream_reset_kernel    zero state, last_tok = blank, stale = 1.
// A call ends only behind a blank or a cap, so the symbols-per-frame counter is 0 at every call
// boundary and has no place in the slot.  Plain stream-ordered launches.
#include "rnnt_argmax.h"

namespace wn {
namespace {

__global__ __launch_bounds__(256) void rnnt_stream_begin_kernel(RnntStreamSlots sl,
                                                                RnntStreamCall c, int n,
                                                                int chunk, int F) {
  __shared__ int live;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = c.slot[i], nt = c.n_t[i];
  const int L = sl.L, H = sl.H, J = sl.J;
  for (int e = tid; e < L * H; e += 256) {
    const int l = e / H, j = e - l * H;
    const int64_t src = ((int64_t)slot * L + l) * H + j, dst = ((int64_t)l * n + i) * H + j;
    c.h[dst] = sl.h[src];
    c.c[dst] = sl.c[src];
  }
  for (int j = tid; j < J; j += 256) c.pred_proj[(int64_t)i * J + j] = sl.pred_proj[(int64_t)slot * J + j];
  const bool done = nt <= 0;
  if (tid == 0) {
    c.last_tok[i] = sl.last_tok[slot];
    c.advance[i] = !done && sl.stale[slot] != 0;
    if (!done) sl.stale[slot] = 0;        // the step runs in this call
    c.done[i] = done;
    c.t[i] = 0;
    c.cnt[i] = 0;
  }
  for (int f = tid; f < F; f += 256) {
    c.row_enc[i * F + f] = (!done && f < nt) ? i * chunk + f : -1;
    c.row_pred[i * F + f] = i;
  }
  if (i == 0) {
    if (tid == 0) live = 0;
    __syncthreads();
    for (int k = tid; k < n; k += 256)
      if (c.n_t[k] > 0) atomicAdd(&live, 1);
    __syncthreads();
    if (tid == 0) { *c.n_active = live; *c.steps = 0; }
  }
}

__global__ __launch_bounds__(1024) void rnnt_stream_advance_kernel(
    const float* __restrict__ part_max, const int* __restrict__ part_idx, int ncb, int V,
    RnntStreamSlots sl, RnntStreamCall c, int n, int chunk, int F, int blank, int n_steps) {
  __shared__ int live;
  const int active_in = *c.n_active;
  if (active_in == 0) return;
  if (threadIdx.x == 0) live = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < n; b += 16) {
    if (c.done[b]) continue;       // (advance[b] is 0 and the row map inert since it finished)
    const int len = c.n_t[b], slot = c.slot[b];
    int t = c.t[b], cnt = c.cnt[b];
    const int nwin = min(F, len - t);
    int first = -1, tok = blank;
    for (int f = 0; f < nwin && first < 0; ++f) {     // frame order; F <= 16
      const int64_t base = (int64_t)(b * F + f) * ncb;
      float v;
      int i;
      rnnt_reduce_row(part_max, part_idx, base, ncb, lane, v, i);
      // a token is a row of the embedding table: anything outside [0, V) is read as blank
      if (i != blank && (unsigned)i < (unsigned)V) { first = f; tok = i; }
    }
    const int frame0 = sl.frames[slot];     // frames consumed before this call
    int last_time = sl.last_time[slot];
    bool adv = false;
    if (first < 0) {
      t += nwin; cnt = 0;
    } else {
      if (first > 0) cnt = 0;
      t += first;
      const int k = sl.n_tok[slot];
      last_time = frame0 + t;
      if (lane == 0) {
        if (k < sl.max_tok) {
          sl.tokens[(int64_t)slot * sl.max_tok + k] = tok;
          sl.times[(int64_t)slot * sl.max_tok + k] = last_time;
        }
        sl.n_tok[slot] = k + 1;
        sl.last_time[slot] = last_time;
        c.last_tok[b] = tok;
      }
      cnt += 1;
      if (cnt >= n_steps) { t += 1; cnt = 0; }
      adv = true;
    }
    const bool done = t >= len;
    if (lane == 0) {
      c.t[b] = t; c.cnt[b] = cnt;
      c.done[b] = done;
      c.advance[b] = adv && !done;
      if (adv && done) sl.stale[slot] = 1;      // the step is owed to the next call with frames
      sl.trailing_blank[slot] = frame0 + t - 1 - last_time;
      if (!done) atomicAdd(&live, 1);
    }
    for (int f = lane; f < F; f += 64) {
      c.row_enc[b * F + f] = (!done && t + f < len) ? b * chunk + t + f : -1;
      c.row_pred[b * F + f] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) { *c.n_active = live; *c.steps += 1; }
}

__global__ __launch_bounds__(256) void rnnt_stream_end_kernel(RnntStreamSlots sl, RnntStreamCall c,
                                                              int n) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int slot = c.slot[i], nt = c.n_t[i];
  const int L = sl.L, H = sl.H, J = sl.J;
  for (int e = tid; e < L * H; e += 256) {
    const int l = e / H, j = e - l * H;
    const int64_t dst = ((int64_t)slot * L + l) * H + j, src = ((int64_t)l * n + i) * H + j;
    sl.h[dst] = c.h[src];
    sl.c[dst] = c.c[src];
  }
  for (int j = tid; j < J; j += 256) sl.pred_proj[(int64_t)slot * J + j] = c.pred_proj[(int64_t)i * J + j];
  const int n_tok = sl.n_tok[slot];
  if (tid == 0) {
    const int frames = sl.frames[slot] + max(nt, 0);
    sl.last_tok[slot] = c.last_tok[i];
    sl.frames[slot] = frames;
    c.out_stat[i] = n_tok;
    c.out_stat[n + i] = frames;
    c.out_stat[2 * n + i] = sl.trailing_blank[slot];
  }
  const int keep = min(min(n_tok, sl.max_tok), c.ld_out);
  for (int k = tid; k < keep; k += 256) {
    c.out_tok[(int64_t)i * c.ld_out + k] = sl.tokens[(int64_t)slot * sl.max_tok + k];
    c.out_tok[(int64_t)(n + i) * c.ld_out + k] = sl.times[(int64_t)slot * sl.max_tok + k];
  }
}

__global__ __launch_bounds__(256) void rnnt_stream_reset_kernel(RnntStreamSlots sl,
                                                                const int* __restrict__ slots,
                                                                int blank) {
  const int slot = slots[blockIdx.x], tid = threadIdx.x;
  const int LH = sl.L * sl.H;
  for (int e = tid; e < LH; e += 256) {
    sl.h[(int64_t)slot * LH + e] = 0.f;
    sl.c[(int64_t)slot * LH + e] = 0.f;
  }
  for (int j = tid; j < sl.J; j += 256) sl.pred_proj[(int64_t)slot * sl.J + j] = 0.f;
  if (tid == 0) {
    sl.last_tok[slot] = blank;
    sl.stale[slot] = 1;            // the predictor's first step: the blank id on a zero state
    sl.n_tok[slot] = 0;
    sl.frames[slot] = 0;
    sl.trailing_blank[slot] = 0;
    sl.last_time[slot] = -1;
  }
}

}  // namespace

int rnnt_stream_begin(const RnntStreamSlots& sl, const RnntStreamCall& c, int n, int chunk, int F,
                      hipStream_t s) {
  WN_CHECK(n >= 1 && chunk >= 1 && F >= 1 && F <= 16, "rnnt_stream_begin: bad argument");
  hipLaunchKernelGGL(rnnt_stream_begin_kernel, dim3(n), dim3(256), 0, s, sl, c, n, chunk, F);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_stream_advance(const float* part_max, const int* part_idx, int ncb, int V,
                        const RnntStreamSlots& sl, const RnntStreamCall& c, int n, int chunk,
                        int F, int blank, int n_steps, hipStream_t s) {
  WN_CHECK(ncb >= 1 && ncb == rnnt_joint_col_blocks(V),
           "rnnt_stream_advance: ncb is not V's block count");
  hipLaunchKernelGGL(rnnt_stream_advance_kernel, dim3(1), dim3(1024), 0, s, part_max, part_idx,
                     ncb, V, sl, c, n, chunk, F, blank, n_steps);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_stream_end(const RnntStreamSlots& sl, const RnntStreamCall& c, int n, hipStream_t s) {
  WN_CHECK(n >= 1 && c.ld_out >= 0, "rnnt_stream_end: bad argument");
  hipLaunchKernelGGL(rnnt_stream_end_kernel, dim3(n), dim3(256), 0, s, sl, c, n);
  WN_HIP(hipGetLastError());
  return 0;
}

int rnnt_stream_reset(const RnntStreamSlots& sl, const int* slot, int n, int blank, hipStream_t s) {
  WN_CHECK(n >= 1 && slot, "rnnt_stream_reset: bad argument");
  hipLaunchKernelGGL(rnnt_stream_reset_kernel, dim3(n), dim3(256), 0, s, sl, slot, blank);
  WN_HIP(hipGetLastError());
  return 0;
}

}  // namespace wn
