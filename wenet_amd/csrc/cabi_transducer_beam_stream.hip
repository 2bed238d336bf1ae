// C ABI (include/wenet_amd.h), streaming transducer sessions: the resumable RNN-T prefix beam
// search (wn_rnnt_beam_stream_*; kernels: transducer_beam_stream.hip around the one-shot search's
// transducer_beam.hip, whose beam step runs in carry mode).
#include <algorithm>
#include <cmath>

#include "model_state.h"
#include "rnnt_predictor.h"

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

namespace wn {
namespace {

// argument checks of an advance call: nothing here touches the device or a session
int rnnt_beam_stream_check(const wn_rnnt_beam_stream_set* S, int n, const int32_t* slot_ids,
                           const int32_t* n_t, int chunk, const wn_rnnt_beam_stream_result* out,
                           int* need_out) {
  WN_CHECK(n >= 1 && n <= S->n_slots,
           "wn_rnnt_beam_stream_advance_encoded: n must be in [1, n_slots]");
  WN_CHECK(out->n_hyps && out->hyp_lens && out->hyp_tokens && out->hyp_scores &&
               out->frames_decoded && out->trailing_blank && out->max_len >= 0,
           "wn_rnnt_beam_stream_advance_encoded: null output");
  std::vector<char> seen(S->n_slots, 0);
  int need = 1;
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i];
    WN_CHECK(sl >= 0 && sl < S->n_slots,
             "wn_rnnt_beam_stream_advance_encoded: slot_ids: slot id out of range");
    WN_CHECK(!seen[sl], "wn_rnnt_beam_stream_advance_encoded: slot_ids: a slot is named twice in "
                        "one call (two rows would write one state)");
    seen[sl] = 1;
    WN_CHECK(n_t[i] >= 0 && n_t[i] <= chunk,
             "wn_rnnt_beam_stream_advance_encoded: n_t: need 0 <= n_t <= chunk");
    if (S->frames[sl] + n_t[i] > S->max_frames) {
      set_error("wn_rnnt_beam_stream_advance_encoded: the session in slot " + std::to_string(sl) +
                " has " + std::to_string(S->frames[sl]) + " frames and would pass max_frames = " +
                std::to_string(S->max_frames) + " with " + std::to_string(n_t[i]) +
                " more; no session was advanced");
      return -1;
    }
    need = std::max(need, S->frames[sl] + n_t[i]);      // one symbol per frame at most
  }
  WN_CHECK(out->max_len >= need,
           "wn_rnnt_beam_stream_advance_encoded: max_len is smaller than a hypothesis may become "
           "(" + std::to_string(need) + " tokens); no session was advanced");
  *need_out = need;
  return 0;
}

}  // namespace
}  // namespace wn

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
  std::vector<int> all(n_slots);
  for (int i = 0; i < n_slots; ++i) all[i] = i;
  WN_TRY(S->stage.begin(all.size() * sizeof(int) + 64));
  WN_TRY(S->stage.put_at(S->desc.p, all.data(), all.size() * sizeof(int), s));
  WN_TRY(S->stage.end(s));
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
  WN_CHECK(set && slot_ids, "wn_rnnt_beam_stream_reset: null argument");
  WN_CHECK(n >= 1 && n <= set->n_slots, "wn_rnnt_beam_stream_reset: n must be in [1, n_slots]");
  for (int i = 0; i < n; ++i)
    WN_CHECK(slot_ids[i] >= 0 && slot_ids[i] < set->n_slots,
             "wn_rnnt_beam_stream_reset: slot_ids: slot id out of range");
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  WN_TRY(set->stage.begin((size_t)n * sizeof(int) + 64));
  WN_TRY(set->stage.put_at(set->desc.p, slot_ids, (size_t)n * sizeof(int), s));
  WN_TRY(set->stage.end(s));
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
  int ld = 1;
  WN_TRY(rnnt_beam_stream_check(set, n, slot_ids, n_t_host, chunk, out, &ld));
  wn_rnnt_beam_stream_set* S = set;
  wn_model* m = S->m;
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_transducer_config& tc = m->tr.c;
  const int E = tc.pred_embed, H = tc.pred_hidden, L = tc.pred_layers, P = tc.pred_out;
  const int J = tc.join_dim, V = c.vocab, blank = tc.blank, d = c.d_model;
  const int beam = S->beam, max_tok = S->max_frames;
  const float cw = S->cw, tw = S->tw;
  const bool stateless = m->tr.sp.kind != 0;
  const int M = n * beam, ldl = (V + 31) / 32 * 32;
  WN_CHECK((int64_t)n * chunk * std::max(J, ldl) <= ((int64_t)1 << 30) &&
               (int64_t)M * ldl <= ((int64_t)1 << 28),
           "wn_rnnt_beam_stream_advance_encoded: n x chunk rows do not fit the workspace");
  const int rows = n * chunk;
  int longest = 0;
  for (int i = 0; i < n; ++i) longest = std::max(longest, (int)n_t_host[i]);

  // ---- workspace, sized by n x beam: the one-shot search's layout + last_time, pending ----------
  WN_TRY(S->enc_proj.ensure((size_t)rows * J * sizeof(float)));
  const size_t n_state = up64((size_t)L * M * H), n_pp = up64((size_t)M * J), um = up64(M),
               ub = up64(n);
  const size_t o_h = 0, o_c = 2 * n_state, o_gates = 4 * n_state,
               o_pout = o_gates + up64((size_t)M * 4 * H), o_pp = o_pout + up64((size_t)M * P),
               o_logits = o_pp + 2 * n_pp, o_topv = o_logits + up64((size_t)M * ldl),
               o_score = o_topv + up64((size_t)M * beam), n_f32 = o_score + 4 * um;
  WN_TRY(S->f32.ensure(n_f32 * sizeof(float)));
  // n_live x 2 | off | len | frame0 | tok_len x 2 | last_time x 2 | src | last_tok | advance |
  // row_enc | row_pred | pending | top_idx
  const size_t o_topi = 5 * ub + 10 * um, n_i32 = o_topi + up64((size_t)M * beam);
  WN_TRY(S->i32.ensure(n_i32 * sizeof(int)));
  WN_TRY(S->tok.ensure((size_t)2 * M * max_tok * sizeof(int)));
  // results: score [M] | n_live, frames, trailing [3][n] | tok_len [M] | token rows [M][ld]
  const size_t r_stat = um * sizeof(double), r_len = r_stat + up64(3 * (size_t)n) * sizeof(int),
               r_tok = r_len + um * sizeof(int), r_bytes = r_tok + (size_t)M * ld * sizeof(int);
  WN_TRY(S->out.ensure(r_bytes));
  WN_TRY(S->host.ensure(r_bytes));
  float* f = S->f32.as<float>();
  int* ip = S->i32.as<int>();
  float* enc_proj = S->enc_proj.as<float>();
  float *gates = f + o_gates, *pout = f + o_pout, *logits = f + o_logits, *topv = f + o_topv;
  RnntBeamSlots slots[2];
  int* last_time[2];
  for (int i = 0; i < 2; ++i) {
    slots[i].n_live = ip + i * ub;
    slots[i].tok_len = ip + 5 * ub + i * um;
    slots[i].score = reinterpret_cast<double*>(f + o_score) + i * um;
    slots[i].tokens = S->tok.as<int>() + (size_t)i * M * max_tok;
    last_time[i] = ip + 5 * ub + (2 + i) * um;
  }
  int *off = ip + 2 * ub, *len = ip + 3 * ub, *frame0 = ip + 4 * ub;
  int* src = ip + 5 * ub + 4 * um;
  int *last_tok = src + um, *advance = src + 2 * um, *row_enc = src + 3 * um,
      *row_pred = src + 4 * um, *pending = src + 5 * um, *topi = ip + o_topi;
  auto call_at = [&](int par) {
    RnntBeamStreamCall cl;
    cl.slot = S->desc.as<int>(); cl.n_t = cl.slot + up64(S->n_slots);
    cl.st = slots[par]; cl.max_tok = max_tok;
    cl.h = f + o_h + par * n_state; cl.c = f + o_c + par * n_state;
    cl.pred_proj = f + o_pp + par * n_pp; cl.last_time = last_time[par];
    cl.last_tok = last_tok; cl.pending = pending; cl.advance = advance; cl.row_enc = row_enc;
    cl.row_pred = row_pred; cl.off = off; cl.len = len; cl.frame0 = frame0;
    char* o = S->out.as<char>();
    cl.out_score = reinterpret_cast<double*>(o);
    cl.out_stat = reinterpret_cast<int*>(o + r_stat);
    cl.out_len = reinterpret_cast<int*>(o + r_len);
    cl.out_tok = reinterpret_cast<int*>(o + r_tok);
    cl.ld_out = ld;
    return cl;
  };

  WN_TRY(S->stage.begin(2 * ((size_t)n * sizeof(int) + 64)));
  WN_TRY(S->stage.put_at(S->desc.p, slot_ids, (size_t)n * sizeof(int), s));
  WN_TRY(S->stage.put_at(S->desc.as<int>() + up64(S->n_slots), n_t_host, (size_t)n * sizeof(int), s));
  WN_TRY(S->stage.end(s));

  // ---- once per call: enc_proj and (cw > 0) the CTC log-prob rows of the n x chunk rows, as in
  //      wn_transducer_beam_search; the sessions' state into the batch -------------------------
  const float* ctc = nullptr;
  if (longest > 0) {
    const int saved = t_gemm_prec;      // always the fp32 GEMMs, whatever the handle's precision
    t_gemm_prec = PREC_F32;
    int r = linear(W.j_enc, enc_out_dev, d, enc_proj, J, rows, s);
    if (r == 0 && cw != 0.f) {
      r = S->ctc.ensure(((size_t)rows * ldl + 2 * (size_t)rows) * sizeof(float));
      if (r == 0) r = linear(W.ctc, enc_out_dev, d, S->ctc.as<float>(), ldl, rows, s);
    }
    t_gemm_prec = saved;
    WN_TRY(r);
    if (cw != 0.f) {
      CtcRowArgs r2;      // normalised in place; its top-1 is not used
      r2.logits = S->ctc.as<float>(); r2.ld = ldl; r2.M = rows; r2.V = V; r2.k = 1;
      r2.blank = blank; r2.blank_penalty = 0.f;
      r2.topk_val = S->ctc.as<float>() + (size_t)rows * ldl;
      r2.topk_idx = reinterpret_cast<int*>(r2.topk_val + rows);
      r2.logp = S->ctc.as<float>(); r2.ld_out = ldl;
      WN_TRY(ctc_logsoftmax_topk(r2, s));
      ctc = S->ctc.as<float>();
    }
  }
  WN_TRY(rnnt_beam_stream_begin(S->sl, call_at(0), n, chunk, s));

  // ---- exactly max(n_t) steps, stream-ordered, no look at the device in between ----------------
  for (int i = 0; i < longest; ++i) {
    const int cur = i & 1, nxt = cur ^ 1;
    float *h = f + o_h + cur * n_state, *cst = f + o_c + cur * n_state, *pp = f + o_pp + cur * n_pp;
    if (stateless) {    // the window: the tail of the slot's token row in the parity just written
      StatelessWindow sw;
      sw.tokens = slots[cur].tokens; sw.ld_tok = max_tok; sw.tok_len = slots[cur].tok_len;
      WN_TRY(stateless_step(m, sw, pp, advance, nullptr, M, s));
    } else {
      WN_TRY(predictor_step(W.pred_embed, E, last_tok, E, W.pred_rnn.data(), L, W.pred_proj, h, cst,
                            gates, pout, advance, nullptr, M, H, s));
      RnntLinearArgs q;   // joint.pred_ffn
      q.x1 = pout; q.ldx1 = P; q.K1 = P; q.W1 = W.j_pred.w; q.b1 = W.j_pred.b;
      q.y = pp; q.ldy = J; q.N = J; q.B = M; q.advance = advance;
      WN_TRY(rnnt_linear(q, s));
    }
    RnntJointArgs ja;
    ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = pp; ja.ldp = J;
    ja.row_enc = row_enc; ja.row_pred = row_pred;
    ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
    ja.logits = logits; ja.ldl = ldl;
    WN_TRY(rnnt_joint_rows(ja, s));
    RnntFuseArgs fa;
    fa.logits = logits; fa.ldl = ldl; fa.row_enc = row_enc; fa.ctc = ctc; fa.ldc = ldl;
    fa.cw = cw; fa.tw = tw; fa.M = M; fa.V = V; fa.k = beam;
    fa.val = topv; fa.idx = topi;
    WN_TRY(rnnt_fuse_topk(fa, s));
    RnntBeamStepArgs ba;
    ba.in = slots[cur]; ba.out = slots[nxt]; ba.max_tok = max_tok;
    ba.top_val = topv; ba.top_idx = topi; ba.off = off; ba.len = len;
    ba.frame = i; ba.B = n; ba.beam = beam; ba.blank = blank; ba.V = V;
    ba.src = src; ba.last_tok = last_tok; ba.advance = advance; ba.row_enc = row_enc;
    ba.pending = pending; ba.last_time_in = last_time[cur]; ba.last_time_out = last_time[nxt];
    ba.frame0 = frame0;
    WN_TRY(rnnt_beam_step(ba, s));
    WN_TRY(rnnt_beam_gather(src, h, cst, pp, f + o_h + nxt * n_state, f + o_c + nxt * n_state,
                            f + o_pp + nxt * n_pp, M, L, H, J, s));
  }
  WN_TRY(rnnt_beam_stream_end(S->sl, call_at(longest & 1), n, blank, s));

  // ---- results: one copy into pinned memory, one wait ------------------------------------------
  WN_HIP(hipMemcpyAsync(S->host.p, S->out.p, r_bytes, hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  const char* hp = S->host.p;
  const double* sc = reinterpret_cast<const double*>(hp);
  const int* stat = reinterpret_cast<const int*>(hp + r_stat);
  const int* tl = reinterpret_cast<const int*>(hp + r_len);
  const int* tk = reinterpret_cast<const int*>(hp + r_tok);
  const int max_len = out->max_len;
  for (int i = 0; i < n; ++i) S->frames[slot_ids[i]] += n_t_host[i];
  for (int i = 0; i < n; ++i) {
    const int nl = stat[i];
    WN_CHECK(nl >= 1 && nl <= beam && stat[n + i] == S->frames[slot_ids[i]],
             "wn_rnnt_beam_stream_advance_encoded: a session came back without a hypothesis or "
             "with a wrong frame count");
    out->n_hyps[i] = nl;
    out->frames_decoded[i] = stat[n + i];
    out->trailing_blank[i] = stat[2 * n + i];
    for (int k = 0; k < beam; ++k) {
      const int g = i * beam + k;
      const int len_k = k < nl ? tl[g] : 0;
      WN_CHECK(len_k >= 0 && len_k <= ld, "wn_rnnt_beam_stream_advance_encoded: token row overflow");
      out->hyp_lens[g] = len_k;
      out->hyp_scores[g] = k < nl ? sc[g] : -INFINITY;
      std::copy(tk + (size_t)g * ld, tk + (size_t)g * ld + len_k,
                out->hyp_tokens + (size_t)g * max_len);
    }
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
