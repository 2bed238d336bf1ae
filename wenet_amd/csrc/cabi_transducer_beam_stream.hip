// C ABI (include/wenet_amd.h), streaming transducer sessions: the resumable RNN-T prefix beam
// search (wn_rnnt_beam_stream_*; kernels: transducer_beam_stream.hip around the one-shot search's
// transducer_beam.hip, whose beam step runs in carry mode).
#include <algorithm>
#include <cmath>

#include "model_state.h"
#include "rnnt_host.h"

// Everything a set owns is allocated in wn_rnnt_beam_stream_create or grows on the first call
// that needs it (the per-call workspace, whose size depends on n and the chunk): a steady stream
// of chunks allocates nothing.  The workspace is the set's own, so one-shot searches on the same
// handle between two calls leave a session as it was.
struct wn_rnnt_beam_stream_set {
  wn_model* m = nullptr;
  int n_slots = 0, beam = 0, max_frames = 0;
  float cw = 0.f, tw = 1.f;
  DevBuf slot_f32, slot_i32, slot_f64, slot_tok;
  RnntBeamStreamSlots sl;
  std::vector<int> frames;                 // host mirror of every slot's frame counter
  DevBuf desc;                             // slot | n_t of the call in flight
  Stager stage;
  DevBuf enc_proj, ctc, f32, i32, tok, out;   // the call's workspace and its compact results
  PinnedBuf host;
};

extern "C" {

int wn_rnnt_beam_stream_create(wn_model* m, int32_t n_slots, int32_t beam, int32_t max_frames,
                               float ctc_weight, float transducer_weight,
                               wn_rnnt_beam_stream_set** out, void* stream) {
  WN_CHECK(m && out, "wn_rnnt_beam_stream_create: null argument");
  WN_CHECK(m->tr.on && m->data->j_out.w,
           "wn_rnnt_beam_stream_create: this model has no transducer weights (predictor / joint); "
           "it was not built by wn_model_create_transducer");
  WN_CHECK(n_slots >= 1 && n_slots <= 256,
           "wn_rnnt_beam_stream_create: n_slots must be in [1, 256]");
  WN_CHECK(beam >= 1 && beam <= 16, "wn_rnnt_beam_stream_create: beam must be in [1, 16]");
  WN_CHECK(beam <= m->cfg.vocab, "wn_rnnt_beam_stream_create: beam is larger than the vocabulary");
  WN_CHECK(max_frames >= 1 && (int64_t)n_slots * beam * max_frames <= ((int64_t)1 << 28),
           "wn_rnnt_beam_stream_create: max_frames must be >= 1 and n_slots x beam x max_frames "
           "<= 2^28");
  WN_CHECK(ctc_weight >= 0.f && transducer_weight >= 0.f,
           "wn_rnnt_beam_stream_create: ctc_weight / transducer_weight must be >= 0");
  WN_CHECK(ctc_weight > 0.f || transducer_weight > 0.f,
           "wn_rnnt_beam_stream_create: ctc_weight and transducer_weight are both 0");
  WN_CHECK(ctc_weight == 0.f || m->data->ctc.w,
           "wn_rnnt_beam_stream_create: ctc_weight > 0 on a handle without a CTC head");
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_transducer_config& tc = m->tr.c;
  const int L = tc.pred_layers, H = tc.pred_hidden, J = tc.join_dim;
  std::unique_ptr<wn_rnnt_beam_stream_set> S(new wn_rnnt_beam_stream_set());
  S->m = m; S->n_slots = n_slots; S->beam = beam; S->max_frames = max_frames;
  S->cw = ctc_weight; S->tw = transducer_weight;
  S->frames.assign(n_slots, 0);
  const size_t Q = (size_t)n_slots * beam;
  const size_t n_state = up64(Q * L * H), n_pp = up64(Q * J), us = up64(n_slots), uq = up64(Q);
  WN_TRY(S->slot_f32.ensure((2 * n_state + n_pp) * sizeof(float)));
  WN_TRY(S->slot_i32.ensure((2 * us + 4 * uq) * sizeof(int)));
  WN_TRY(S->slot_f64.ensure(uq * sizeof(double)));
  WN_TRY(S->slot_tok.ensure(Q * max_frames * sizeof(int)));
  WN_TRY(S->desc.ensure(2 * us * sizeof(int)));
  RnntBeamStreamSlots& sl = S->sl;
  float* f = S->slot_f32.as<float>();
  int* ip = S->slot_i32.as<int>();
  sl.h = f; sl.c = f + n_state; sl.pred_proj = f + 2 * n_state;
  sl.n_live = ip; sl.frames = ip + us;
  sl.tok_len = ip + 2 * us; sl.last_tok = sl.tok_len + uq; sl.pending = sl.tok_len + 2 * uq;
  sl.last_time = sl.tok_len + 3 * uq;
  sl.score = S->slot_f64.as<double>();
  sl.tokens = S->slot_tok.as<int>(); sl.max_tok = max_frames;
  sl.beam = beam; sl.L = L; sl.H = H; sl.J = J;
  WN_TRY(rnnt_stage_call(S->stage, S->desc, n_slots, n_slots, nullptr, nullptr, s));
  WN_TRY(rnnt_beam_stream_reset(sl, S->desc.as<int>(), n_slots, tc.blank, s));
  WN_HIP(hipStreamSynchronize(s));
  *out = S.release();
  return 0;
}

int wn_rnnt_beam_stream_destroy(wn_rnnt_beam_stream_set* set) {
  delete set;
  return 0;
}

int wn_rnnt_beam_stream_reset(wn_rnnt_beam_stream_set* set, int32_t n, const int32_t* slot_ids,
                              void* stream) {
  WN_TRY(rnnt_reset_check("wn_rnnt_beam_stream_reset", set && slot_ids, set ? set->n_slots : 0,
                          n, slot_ids));
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  WN_TRY(rnnt_stage_call(set->stage, set->desc, set->n_slots, n, slot_ids, nullptr, s));
  WN_TRY(rnnt_beam_stream_reset(set->sl, set->desc.as<int>(), n, set->m->tr.c.blank, s));
  for (int i = 0; i < n; ++i) set->frames[slot_ids[i]] = 0;
  return 0;
}

int wn_rnnt_beam_stream_advance_encoded(wn_rnnt_beam_stream_set* set, int32_t n,
                                        const int32_t* slot_ids, const float* enc_out_dev,
                                        const int32_t* n_t_host, int32_t chunk,
                                        const wn_rnnt_beam_stream_result* out, void* stream) {
  WN_CHECK(set && slot_ids && enc_out_dev && n_t_host && out,
           "wn_rnnt_beam_stream_advance_encoded: null argument");
  WN_CHECK(chunk >= 1 && chunk <= (1 << 20),
           "wn_rnnt_beam_stream_advance_encoded: chunk must be >= 1");
  wn_rnnt_beam_stream_set* S = set;
  int ld = 1;       // the longest a hypothesis may become: one symbol per frame at most
  WN_TRY(rnnt_session_check(
      "wn_rnnt_beam_stream_advance_encoded", S->n_slots, S->max_frames, S->frames, n, slot_ids,
      n_t_host, chunk,
      out->n_hyps && out->hyp_lens && out->hyp_tokens && out->hyp_scores && out->frames_decoded &&
          out->trailing_blank && out->max_len >= 0,
      [&](int sl, int n_t) { ld = std::max(ld, S->frames[sl] + n_t); }));
  WN_CHECK(out->max_len >= ld,
           "wn_rnnt_beam_stream_advance_encoded: max_len is smaller than a hypothesis may become "
           "(" + std::to_string(ld) + " tokens); no session was advanced");
  wn_model* m = S->m;
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_transducer_config& tc = m->tr.c;
  const int J = tc.join_dim, V = m->cfg.vocab;
  const int beam = S->beam, max_tok = S->max_frames;
  const int M = n * beam, ldl = ctc_pitch(V);
  WN_CHECK((int64_t)n * chunk * std::max(J, ldl) <= ((int64_t)1 << 30) &&
               (int64_t)M * ldl <= ((int64_t)1 << 28),
           "wn_rnnt_beam_stream_advance_encoded: n x chunk rows do not fit the workspace");
  const int rows = n * chunk;
  int longest = 0;
  for (int i = 0; i < n; ++i) longest = std::max(longest, (int)n_t_host[i]);

  // ---- workspace, sized by n x beam: the one-shot search's layout + the carry fields ------------
  WN_TRY(S->enc_proj.ensure((size_t)rows * J * sizeof(float)));
  RnntBeamLayout w;
  WN_TRY(w.carve(tc, n, beam, V, max_tok, true, S->f32, S->i32, S->tok));
  float* enc_proj = S->enc_proj.as<float>();
  // results: score [M] | n_live, frames, trailing [3][n] | tok_len [M] | token rows [M][ld]
  const size_t um = up64(M);
  const size_t r_stat = um * sizeof(double), r_len = r_stat + up64(3 * (size_t)n) * sizeof(int),
               r_tok = r_len + um * sizeof(int), r_bytes = r_tok + (size_t)M * ld * sizeof(int);
  WN_TRY(S->out.ensure(r_bytes));
  WN_TRY(S->host.ensure(r_bytes));
  auto call_at = [&](int par) {
    RnntBeamStreamCall cl;
    cl.slot = S->desc.as<int>(); cl.n_t = cl.slot + up64(S->n_slots);
    cl.st = w.slots[par]; cl.max_tok = max_tok;
    cl.h = w.h_at(par); cl.c = w.c_at(par); cl.pred_proj = w.pp_at(par);
    cl.last_time = w.last_time[par];
    cl.last_tok = w.last_tok; cl.pending = w.pending; cl.advance = w.advance;
    cl.row_enc = w.row_enc; cl.row_pred = w.row_pred;
    cl.off = w.off; cl.len = w.len; cl.frame0 = w.frame0;
    char* o = S->out.as<char>();
    cl.out_score = reinterpret_cast<double*>(o);
    cl.out_stat = reinterpret_cast<int*>(o + r_stat);
    cl.out_len = reinterpret_cast<int*>(o + r_len);
    cl.out_tok = reinterpret_cast<int*>(o + r_tok);
    cl.ld_out = ld;
    return cl;
  };
  WN_TRY(rnnt_stage_call(S->stage, S->desc, S->n_slots, n, slot_ids, n_t_host, s));

  // ---- once per call: enc_proj and (cw > 0) the CTC log-prob rows of the n x chunk rows, as in
  //      wn_transducer_beam_search; the sessions' state into the batch -------------------------
  const float* ctc = nullptr;
  if (longest > 0) WN_TRY(rnnt_prepare(m, enc_out_dev, rows, enc_proj, s, S->cw, &S->ctc, &ctc));
  WN_TRY(rnnt_beam_stream_begin(S->sl, call_at(0), n, chunk, s));

  // ---- exactly max(n_t) steps, stream-ordered, no look at the device in between ----------------
  WN_TRY(rnnt_beam_steps(m, w, enc_proj, ctc, S->cw, S->tw, w.off, w.len, n, beam, max_tok,
                         longest, s));
  WN_TRY(rnnt_beam_stream_end(S->sl, call_at(longest & 1), n, tc.blank, s));

  // ---- results: one copy into pinned memory, one wait ------------------------------------------
  WN_HIP(hipMemcpyAsync(S->host.p, S->out.p, r_bytes, hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  const char* hp = S->host.p;
  const double* sc = reinterpret_cast<const double*>(hp);
  const int* stat = reinterpret_cast<const int*>(hp + r_stat);
  const int* tl = reinterpret_cast<const int*>(hp + r_len);
  const int* tk = reinterpret_cast<const int*>(hp + r_tok);
  for (int i = 0; i < n; ++i) S->frames[slot_ids[i]] += n_t_host[i];
  for (int i = 0; i < n; ++i) {
    WN_CHECK(stat[i] >= 1 && stat[i] <= beam && stat[n + i] == S->frames[slot_ids[i]],
             "wn_rnnt_beam_stream_advance_encoded: a session came back without a hypothesis or "
             "with a wrong frame count");
    out->frames_decoded[i] = stat[n + i];
    out->trailing_blank[i] = stat[2 * n + i];
    const size_t g = (size_t)i * beam;
    WN_TRY(rnnt_unpack_nbest("wn_rnnt_beam_stream_advance_encoded", stat[i], beam, tl + g, sc + g,
                             tk + g * ld, ld, out->n_hyps + i, out->hyp_lens + g,
                             out->hyp_scores + g, out->hyp_tokens + g * out->max_len,
                             out->max_len));
  }
  return 0;
}

int wn_rnnt_beam_stream_state(wn_rnnt_beam_stream_set* set, int32_t slot, int32_t* counters2,
                              double* scores, int32_t* slot_ints, int32_t* tokens, float* h,
                              float* c, float* pred_proj, void* stream) {
  WN_CHECK(set && counters2 && scores && slot_ints && tokens && h && c && pred_proj,
           "wn_rnnt_beam_stream_state: null argument");
  WN_CHECK(slot >= 0 && slot < set->n_slots, "wn_rnnt_beam_stream_state: slot id out of range");
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  const RnntBeamStreamSlots& sl = set->sl;
  const size_t beam = sl.beam, q0 = (size_t)slot * beam, LH = (size_t)sl.L * sl.H;
  auto down = [&](void* dst, const void* srcp, size_t bytes) {
    return hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, s);
  };
  WN_HIP(down(counters2, sl.n_live + slot, sizeof(int)));
  WN_HIP(down(counters2 + 1, sl.frames + slot, sizeof(int)));
  WN_HIP(down(scores, sl.score + q0, beam * sizeof(double)));
  const int* fields[4] = {sl.tok_len, sl.last_tok, sl.pending, sl.last_time};
  for (int i = 0; i < 4; ++i)
    WN_HIP(down(slot_ints + i * beam, fields[i] + q0, beam * sizeof(int)));
  WN_HIP(down(tokens, sl.tokens + q0 * sl.max_tok, beam * sl.max_tok * sizeof(int)));
  WN_HIP(down(h, sl.h + q0 * LH, beam * LH * sizeof(float)));
  WN_HIP(down(c, sl.c + q0 * LH, beam * LH * sizeof(float)));
  WN_HIP(down(pred_proj, sl.pred_proj + q0 * sl.J, beam * sl.J * sizeof(float)));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
