// C ABI (include/wenet_amd.h), streaming transducer sessions: the resumable RNN-T greedy search
// (wn_rnnt_stream_*; kernels: transducer_stream.hip around the one-shot search's transducer.hip).
#include <algorithm>

#include "model_state.h"
#include "rnnt_predictor.h"

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

namespace wn {
namespace {

// argument checks of an advance call: nothing here touches the device or a session
int rnnt_stream_check(const wn_rnnt_stream_set* S, int n, const int32_t* slot_ids,
                      const int32_t* n_t, int chunk, const wn_rnnt_stream_result* out) {
  WN_CHECK(n >= 1 && n <= S->n_slots, "wn_rnnt_stream_advance_encoded: n must be in [1, n_slots]");
  WN_CHECK(out->tok_lens && out->tokens && out->times && out->frames_decoded &&
               out->trailing_blank && out->max_len >= 0,
           "wn_rnnt_stream_advance_encoded: null output");
  std::vector<char> seen(S->n_slots, 0);
  int64_t need = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i];
    WN_CHECK(sl >= 0 && sl < S->n_slots,
             "wn_rnnt_stream_advance_encoded: slot_ids: slot id out of range");
    WN_CHECK(!seen[sl], "wn_rnnt_stream_advance_encoded: slot_ids: a slot is named twice in one "
                        "call (two rows would write one state)");
    seen[sl] = 1;
    WN_CHECK(n_t[i] >= 0 && n_t[i] <= chunk,
             "wn_rnnt_stream_advance_encoded: n_t: need 0 <= n_t <= chunk");
    if (S->frames[sl] + n_t[i] > S->max_frames) {
      set_error("wn_rnnt_stream_advance_encoded: the session in slot " + std::to_string(sl) +
                " has " + std::to_string(S->frames[sl]) + " frames and would pass max_frames = " +
                std::to_string(S->max_frames) + " with " + std::to_string(n_t[i]) +
                " more; no session was advanced");
      return -1;
    }
    need = std::max(need, std::min<int64_t>((int64_t)S->n_tok[sl] + (int64_t)n_t[i] * S->n_steps,
                                            S->max_tokens));
  }
  WN_CHECK(out->max_len >= need,
           "wn_rnnt_stream_advance_encoded: max_len is smaller than a session's token count may "
           "become (" + std::to_string(need) + " tokens); no session was advanced");
  return 0;
}

}  // namespace
}  // namespace wn

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
  std::vector<int> all(n_slots);
  for (int i = 0; i < n_slots; ++i) all[i] = i;
  WN_TRY(S->stage.begin(all.size() * sizeof(int) + 64));
  WN_TRY(S->stage.put_at(S->desc.p, all.data(), all.size() * sizeof(int), s));
  WN_TRY(S->stage.end(s));
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
  WN_CHECK(set && slot_ids, "wn_rnnt_stream_reset: null argument");
  WN_CHECK(n >= 1 && n <= set->n_slots, "wn_rnnt_stream_reset: n must be in [1, n_slots]");
  for (int i = 0; i < n; ++i)
    WN_CHECK(slot_ids[i] >= 0 && slot_ids[i] < set->n_slots,
             "wn_rnnt_stream_reset: slot_ids: slot id out of range");
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  WN_TRY(set->stage.begin((size_t)n * sizeof(int) + 64));
  WN_TRY(set->stage.put_at(set->desc.p, slot_ids, (size_t)n * sizeof(int), s));
  WN_TRY(set->stage.end(s));
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
  WN_TRY(rnnt_stream_check(set, n, slot_ids, n_t_host, chunk, out));
  wn_rnnt_stream_set* S = set;
  wn_model* m = S->m;
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_transducer_config& tc = m->tr.c;
  const int E = tc.pred_embed, H = tc.pred_hidden, L = tc.pred_layers, P = tc.pred_out;
  const int J = tc.join_dim, V = c.vocab, blank = tc.blank, d = c.d_model;
  const int F = std::min(std::max(tune().rnnt_lookahead, 1), 16);
  const int n_steps = S->n_steps;
  const bool stateless = m->tr.sp.kind != 0;
  const int M = n * F, ncb = rnnt_joint_col_blocks(V), rows = n * chunk;
  int longest = 0;
  for (int i = 0; i < n; ++i) longest = std::max(longest, (int)n_t_host[i]);

  // ---- workspace ----------------------------------------------------------------------------
  WN_TRY(S->enc_proj.ensure((size_t)rows * J * sizeof(float)));
  const size_t n_state = up64((size_t)L * n * H);
  const size_t o_h = 0, o_c = n_state, o_gates = o_c + n_state,
               o_pout = o_gates + up64((size_t)n * 4 * H), o_pproj = o_pout + up64((size_t)n * P),
               o_pmax = o_pproj + up64((size_t)n * J), n_f32 = o_pmax + up64((size_t)M * ncb);
  WN_TRY(S->f32.ensure(n_f32 * sizeof(float)));
  const size_t ub = up64(n), um = up64(M);
  const size_t n_stat = 2 + 3 * (size_t)n;       // n_active | steps | n_tok | frames | trailing
  const size_t n_i32 = 5 * ub + 2 * um + up64((size_t)M * ncb) + up64(n_stat);
  WN_TRY(S->i32.ensure(n_i32 * sizeof(int)));
  const int ld = out->max_len;
  WN_TRY(S->out_tok.ensure(std::max<size_t>(2 * (size_t)n * ld, 1) * sizeof(int)));
  const size_t p_stat = 256, p_tok = p_stat + up64(n_stat) * sizeof(int);
  WN_TRY(S->host.ensure(p_tok + 2 * (size_t)n * ld * sizeof(int)));
  float* f = S->f32.as<float>();
  float* enc_proj = S->enc_proj.as<float>();
  float *gates = f + o_gates, *pout = f + o_pout, *pmax = f + o_pmax;
  int* ip = S->i32.as<int>();
  RnntStreamCall cl;
  cl.slot = S->desc.as<int>(); cl.n_t = cl.slot + up64(S->n_slots);
  cl.h = f + o_h; cl.c = f + o_c; cl.pred_proj = f + o_pproj;
  cl.last_tok = ip; cl.advance = ip + ub; cl.done = ip + 2 * ub; cl.t = ip + 3 * ub;
  cl.cnt = ip + 4 * ub;
  cl.row_enc = ip + 5 * ub; cl.row_pred = cl.row_enc + um;
  int* pidx = cl.row_pred + um;
  cl.n_active = pidx + up64((size_t)M * ncb); cl.steps = cl.n_active + 1;
  cl.out_stat = cl.n_active + 2;
  cl.out_tok = S->out_tok.as<int>(); cl.ld_out = ld;

  WN_TRY(S->stage.begin(2 * ((size_t)n * sizeof(int) + 64)));
  WN_TRY(S->stage.put_at(S->desc.p, slot_ids, (size_t)n * sizeof(int), s));
  WN_TRY(S->stage.put_at(S->desc.as<int>() + up64(S->n_slots), n_t_host, (size_t)n * sizeof(int), s));
  WN_TRY(S->stage.end(s));

  // ---- once per call: enc_proj = joint.enc_ffn(chunk), the sessions' state into the batch -------
  if (longest > 0) {
    // always the fp32 GEMMs, whatever the handle's operand precision
    const int saved = t_gemm_prec;
    t_gemm_prec = PREC_F32;
    const int r = linear(W.j_enc, enc_out_dev, d, enc_proj, J, rows, s);
    t_gemm_prec = saved;
    WN_TRY(r);
  }
  WN_TRY(rnnt_stream_begin(S->sl, cl, n, chunk, F, s));

  // ---- the lock-step loop: groups of steps, n_active looked at one group late -----------------
  const int64_t bound = longest > 0 ? (int64_t)longest * ((int64_t)n_steps + 1) + 1 : 0;
  volatile int* pin = reinterpret_cast<volatile int*>(S->host.p);   // slots 0 / 1 (64 B apart)
  int64_t issued = 0;
  for (int g = 0; issued < bound; ++g) {
    const int k = (int)std::min<int64_t>(RNNT_GROUP, bound - issued);
    for (int i = 0; i < k; ++i) {
      if (stateless) {    // the window: the tail of the session's own token row up to n_tok
        StatelessWindow sw;
        sw.tokens = S->sl.tokens; sw.ld_tok = S->sl.max_tok; sw.tok_len = S->sl.n_tok;
        sw.tok_row = cl.slot;
        WN_TRY(stateless_step(m, sw, cl.pred_proj, cl.advance, cl.n_active, n, s));
      } else {
        WN_TRY(predictor_step(W.pred_embed, E, cl.last_tok, E, W.pred_rnn.data(), L, W.pred_proj,
                              cl.h, cl.c, gates, pout, cl.advance, cl.n_active, n, H, s));
        RnntLinearArgs q;   // joint.pred_ffn
        q.x1 = pout; q.ldx1 = P; q.K1 = P; q.W1 = W.j_pred.w; q.b1 = W.j_pred.b;
        q.y = cl.pred_proj; q.ldy = J; q.N = J; q.B = n;
        q.advance = cl.advance; q.n_active = cl.n_active;
        WN_TRY(rnnt_linear(q, s));
      }
      RnntJointArgs ja;
      ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = cl.pred_proj; ja.ldp = J;
      ja.row_enc = cl.row_enc; ja.row_pred = cl.row_pred;
      ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
      ja.part_max = pmax; ja.part_idx = pidx; ja.n_active = cl.n_active;
      WN_TRY(rnnt_joint_argmax(ja, s));
      WN_TRY(rnnt_stream_advance(pmax, pidx, ncb, V, S->sl, cl, n, chunk, F, blank, n_steps, s));
    }
    issued += k;
    WN_HIP(hipMemcpyAsync(S->host.p + 64 * (g & 1), cl.n_active, sizeof(int),
                          hipMemcpyDeviceToHost, s));
    WN_HIP(hipEventRecord(S->ev[g & 1], s));
    if (g >= 1) {
      WN_HIP(hipEventSynchronize(S->ev[(g - 1) & 1]));
      if (pin[16 * ((g - 1) & 1)] == 0) break;
    }
  }
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
