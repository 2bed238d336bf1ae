// C ABI (include/wenet_amd.h), streaming transducer sessions: the resumable RNN-T greedy search
// (wn_rnnt_stream_*; kernels: transducer_stream.hip around the one-shot search's transducer.hip).
#include <algorithm>

#include "model_state.h"
#include "rnnt_host.h"

// Everything a set owns is allocated in wn_rnnt_stream_create or grows on the first call that
// needs it (the per-call workspace, whose size depends on n and the chunk): a steady stream of
// chunks allocates nothing.  The workspace is the set's own, so one-shot searches on the same
// handle between two calls leave a session as it was.
struct wn_rnnt_stream_set {
  wn_model* m = nullptr;
  int n_slots = 0, max_frames = 0, max_tokens = 0, n_steps = 0;
  DevBuf slot_f32, slot_i32, slot_tok;     // h | c | pred_proj, the counters, tokens | times
  RnntStreamSlots sl;
  std::vector<int> frames, n_tok;          // host mirrors of every slot's counters
  DevBuf desc;                             // slot | n_t of the call in flight
  Stager stage;
  DevBuf enc_proj, f32, i32, out_tok;      // the call's workspace
  PinnedBuf host;                          // n_active polls | the call's results
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~wn_rnnt_stream_set() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

extern "C" {

int wn_rnnt_stream_create(wn_model* m, int32_t n_slots, int32_t max_frames, int32_t max_tokens,
                          int32_t n_steps, wn_rnnt_stream_set** out, void* stream) {
  WN_CHECK(m && out, "wn_rnnt_stream_create: null argument");
  WN_CHECK(m->tr.on && m->data->j_out.w,
           "wn_rnnt_stream_create: this model has no transducer weights (predictor / joint); it "
           "was not built by wn_model_create_transducer");
  WN_CHECK(n_slots >= 1 && n_slots <= 256, "wn_rnnt_stream_create: n_slots must be in [1, 256]");
  WN_CHECK(max_frames >= 1, "wn_rnnt_stream_create: max_frames must be >= 1");
  WN_CHECK(max_tokens >= 1 && (int64_t)n_slots * max_tokens <= ((int64_t)1 << 28),
           "wn_rnnt_stream_create: max_tokens must be >= 1 and n_slots x max_tokens <= 2^28");
  WN_CHECK(n_steps >= 1, "wn_rnnt_stream_create: n_steps must be >= 1");
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_transducer_config& tc = m->tr.c;
  const int L = tc.pred_layers, H = tc.pred_hidden, J = tc.join_dim;
  std::unique_ptr<wn_rnnt_stream_set> S(new wn_rnnt_stream_set());
  S->m = m; S->n_slots = n_slots; S->max_frames = max_frames; S->max_tokens = max_tokens;
  S->n_steps = n_steps;
  S->frames.assign(n_slots, 0);
  S->n_tok.assign(n_slots, 0);
  const size_t n_state = up64((size_t)n_slots * L * H), n_pp = up64((size_t)n_slots * J);
  const size_t us = up64(n_slots);
  WN_TRY(S->slot_f32.ensure((2 * n_state + n_pp) * sizeof(float)));
  WN_TRY(S->slot_i32.ensure(6 * us * sizeof(int)));
  WN_TRY(S->slot_tok.ensure(2 * (size_t)n_slots * max_tokens * sizeof(int)));
  WN_TRY(S->desc.ensure(2 * us * sizeof(int)));
  for (hipEvent_t& e : S->ev) WN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  RnntStreamSlots& sl = S->sl;
  float* f = S->slot_f32.as<float>();
  int* ip = S->slot_i32.as<int>();
  sl.h = f; sl.c = f + n_state; sl.pred_proj = f + 2 * n_state;
  sl.last_tok = ip; sl.stale = ip + us; sl.n_tok = ip + 2 * us; sl.frames = ip + 3 * us;
  sl.trailing_blank = ip + 4 * us; sl.last_time = ip + 5 * us;
  sl.tokens = S->slot_tok.as<int>(); sl.times = sl.tokens + (size_t)n_slots * max_tokens;
  sl.max_tok = max_tokens; sl.L = L; sl.H = H; sl.J = J;
  WN_TRY(rnnt_stage_call(S->stage, S->desc, n_slots, n_slots, nullptr, nullptr, s));
  WN_TRY(rnnt_stream_reset(sl, S->desc.as<int>(), n_slots, tc.blank, s));
  WN_HIP(hipStreamSynchronize(s));
  *out = S.release();
  return 0;
}

int wn_rnnt_stream_destroy(wn_rnnt_stream_set* set) {
  delete set;
  return 0;
}

int wn_rnnt_stream_reset(wn_rnnt_stream_set* set, int32_t n, const int32_t* slot_ids,
                         void* stream) {
  WN_TRY(rnnt_reset_check("wn_rnnt_stream_reset", set && slot_ids, set ? set->n_slots : 0, n,
                          slot_ids));
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  WN_TRY(rnnt_stage_call(set->stage, set->desc, set->n_slots, n, slot_ids, nullptr, s));
  WN_TRY(rnnt_stream_reset(set->sl, set->desc.as<int>(), n, set->m->tr.c.blank, s));
  for (int i = 0; i < n; ++i) set->frames[slot_ids[i]] = set->n_tok[slot_ids[i]] = 0;
  return 0;
}

int wn_rnnt_stream_advance_encoded(wn_rnnt_stream_set* set, int32_t n, const int32_t* slot_ids,
                                   const float* enc_out_dev, const int32_t* n_t_host,
                                   int32_t chunk, const wn_rnnt_stream_result* out,
                                   void* stream) {
  WN_CHECK(set && slot_ids && enc_out_dev && n_t_host && out,
           "wn_rnnt_stream_advance_encoded: null argument");
  WN_CHECK(chunk >= 1 && chunk <= (1 << 20), "wn_rnnt_stream_advance_encoded: chunk must be >= 1");
  wn_rnnt_stream_set* S = set;
  int64_t need = 0;
  WN_TRY(rnnt_session_check(
      "wn_rnnt_stream_advance_encoded", S->n_slots, S->max_frames, S->frames, n, slot_ids,
      n_t_host, chunk,
      out->tok_lens && out->tokens && out->times && out->frames_decoded && out->trailing_blank &&
          out->max_len >= 0,
      [&](int sl, int n_t) {
        need = std::max(need, std::min<int64_t>((int64_t)S->n_tok[sl] + (int64_t)n_t * S->n_steps,
                                                S->max_tokens));
      }));
  WN_CHECK(out->max_len >= need,
           "wn_rnnt_stream_advance_encoded: max_len is smaller than a session's token count may "
           "become (" + std::to_string(need) + " tokens); no session was advanced");
  wn_model* m = S->m;
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const ModelData& W = *m->data;
  const wn_transducer_config& tc = m->tr.c;
  const int J = tc.join_dim, V = m->cfg.vocab, blank = tc.blank;
  const int F = std::min(std::max(tune().rnnt_lookahead, 1), 16);
  const int n_steps = S->n_steps;
  const int M = n * F, ncb = rnnt_joint_col_blocks(V), rows = n * chunk;
  int longest = 0;
  for (int i = 0; i < n; ++i) longest = std::max(longest, (int)n_t_host[i]);

  // ---- workspace ----------------------------------------------------------------------------
  const size_t n_stat = 2 + 3 * (size_t)n;       // n_active | steps | n_tok | frames | trailing
  WN_TRY(S->enc_proj.ensure((size_t)rows * J * sizeof(float)));
  RnntGreedyLayout w;
  WN_TRY(w.carve(tc, n, M, ncb, n_stat, S->f32, S->i32));
  const int ld = out->max_len;
  WN_TRY(S->out_tok.ensure(std::max<size_t>(2 * (size_t)n * ld, 1) * sizeof(int)));
  const size_t p_stat = 256, p_tok = p_stat + up64(n_stat) * sizeof(int);
  WN_TRY(S->host.ensure(p_tok + 2 * (size_t)n * ld * sizeof(int)));
  float* enc_proj = S->enc_proj.as<float>();
  RnntStreamCall cl;
  cl.slot = S->desc.as<int>(); cl.n_t = cl.slot + up64(S->n_slots);
  cl.h = w.h; cl.c = w.c; cl.pred_proj = w.pproj;
  cl.last_tok = w.last_tok; cl.advance = w.advance; cl.done = w.done; cl.t = w.t; cl.cnt = w.cnt;
  cl.row_enc = w.row_enc; cl.row_pred = w.row_pred;
  cl.n_active = w.stat; cl.steps = w.stat + 1; cl.out_stat = w.stat + 2;
  cl.out_tok = S->out_tok.as<int>(); cl.ld_out = ld;
  WN_TRY(rnnt_stage_call(S->stage, S->desc, S->n_slots, n, slot_ids, n_t_host, s));

  // ---- once per call: enc_proj = joint.enc_ffn(chunk), the sessions' state into the batch -------
  if (longest > 0) WN_TRY(rnnt_prepare(m, enc_out_dev, rows, enc_proj, s));
  WN_TRY(rnnt_stream_begin(S->sl, cl, n, chunk, F, s));

  // ---- the lock-step loop ---------------------------------------------------------------------
  StatelessWindow sw;     // the tail of the session's own token row up to n_tok
  sw.tokens = S->sl.tokens; sw.ld_tok = S->sl.max_tok; sw.tok_len = S->sl.n_tok;
  sw.tok_row = cl.slot;
  RnntJointArgs ja;
  ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = cl.pred_proj; ja.ldp = J;
  ja.row_enc = cl.row_enc; ja.row_pred = cl.row_pred;
  ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
  ja.part_max = w.pmax; ja.part_idx = w.pidx; ja.n_active = cl.n_active;
  const int64_t bound = longest > 0 ? (int64_t)longest * ((int64_t)n_steps + 1) + 1 : 0;
  WN_TRY(rnnt_poll_loop(bound, cl.n_active, S->host.p, S->ev, s, [&]() -> int {
    WN_TRY(pred_proj_step(m, sw, cl.last_tok, cl.h, cl.c, w.gates, w.pout, cl.pred_proj,
                          cl.advance, cl.n_active, n, s));
    WN_TRY(rnnt_joint_argmax(ja, s));
    return rnnt_stream_advance(w.pmax, w.pidx, ncb, V, S->sl, cl, n, chunk, F, blank, n_steps, s);
  }));
  WN_TRY(rnnt_stream_end(S->sl, cl, n, s));

  // ---- results: the counters first, then the token / time rows that were filled ----------------
  int* stat = reinterpret_cast<int*>(S->host.p + p_stat);
  WN_HIP(hipMemcpyAsync(stat, cl.n_active, n_stat * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  WN_CHECK(stat[0] == 0, "wn_rnnt_stream_advance_encoded: the search did not finish within its "
                         "step bound");
  if (out->steps) *out->steps = stat[1];
  const int *n_tok = stat + 2, *frames = n_tok + n, *trailing = frames + n;
  int most = 0;
  bool overflow = false;
  for (int i = 0; i < n; ++i) {
    S->n_tok[slot_ids[i]] = n_tok[i];
    S->frames[slot_ids[i]] = frames[i];
    overflow = overflow || n_tok[i] > S->max_tokens;
    most = std::max(most, std::min(n_tok[i], S->max_tokens));
  }
  WN_CHECK(!overflow, "wn_rnnt_stream_advance_encoded: token buffer overflow (a session emitted "
                      "more than max_tokens tokens; it keeps counting, stores no more and must "
                      "be reset)");
  WN_CHECK(most <= ld, "wn_rnnt_stream_advance_encoded: max_len is smaller than the longest result");
  const int* rows_pin = reinterpret_cast<const int*>(S->host.p + p_tok);
  if (most > 0) {
    WN_HIP(hipMemcpy2DAsync(S->host.p + p_tok, (size_t)most * sizeof(int), cl.out_tok,
                            (size_t)ld * sizeof(int), (size_t)most * sizeof(int), 2 * (size_t)n,
                            hipMemcpyDeviceToHost, s));
    WN_HIP(stream_wait(s));
  }
  for (int i = 0; i < n; ++i) {
    out->tok_lens[i] = n_tok[i];
    out->frames_decoded[i] = frames[i];
    out->trailing_blank[i] = trailing[i];
    std::copy(rows_pin + (size_t)i * most, rows_pin + (size_t)i * most + n_tok[i],
              out->tokens + (size_t)i * ld);
    std::copy(rows_pin + (size_t)(n + i) * most, rows_pin + (size_t)(n + i) * most + n_tok[i],
              out->times + (size_t)i * ld);
  }
  return 0;
}

int wn_rnnt_stream_state(wn_rnnt_stream_set* set, int32_t slot, float* h, float* c,
                         float* pred_proj, int32_t* scalars5, void* stream) {
  WN_CHECK(set && h && c && pred_proj && scalars5, "wn_rnnt_stream_state: null argument");
  WN_CHECK(slot >= 0 && slot < set->n_slots, "wn_rnnt_stream_state: slot id out of range");
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  const RnntStreamSlots& sl = set->sl;
  const size_t LH = (size_t)sl.L * sl.H;
  WN_HIP(hipMemcpyAsync(h, sl.h + slot * LH, LH * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(c, sl.c + slot * LH, LH * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(pred_proj, sl.pred_proj + (size_t)slot * sl.J, sl.J * sizeof(float),
                        hipMemcpyDeviceToHost, s));
  const int* fields[5] = {sl.last_tok, sl.stale, sl.n_tok, sl.frames, sl.trailing_blank};
  for (int i = 0; i < 5; ++i)
    WN_HIP(hipMemcpyAsync(scalars5 + i, fields[i] + slot, sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
