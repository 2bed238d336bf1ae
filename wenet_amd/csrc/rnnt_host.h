// The host side of the transducer searches, written once: what cabi_transducer.hip (the one-shot
// greedy and beam searches, wn_op_lstm_step), cabi_transducer_stream.hip and
// cabi_transducer_beam_stream.hip (the resumable greedy and beam searches) and
// cabi_transducer_score.hip (the teacher-forced score) do around the kernels they share.  In the
// order an entry point uses it: the argument checks and the descriptor staging of the two session
// sets, the two workspace layouts, the once-per-call preparation (joint.enc_ffn, the CTC log-prob
// rows) under the fp32-GEMM guard, the predictor advance (the one place that chooses between the
// LSTM and a stateless predictor), the greedy poll loop and the beam step loop, the n-best unpack.
// No kernels here, and nothing that owns memory: the handle's tr_* buffers serve the one-shot
// searches, a session set's own buffers serve its sessions, and every function takes them.
#pragma once
#include <math.h>

#include <algorithm>

#include "model_state.h"

namespace wn {

constexpr int RNNT_GROUP = 8;     // steps issued between two looks at n_active

inline size_t up64(size_t n) { return (n + 63) / 64 * 64; }
// row pitch of the (rows, V) logits and CTC log-prob rows of the beam searches
inline int ctc_pitch(int V) { return (V + 31) / 32 * 32; }

// always the fp32 GEMMs inside the scope, whatever the handle's operand precision
struct Fp32GemmScope {
  const int saved;
  Fp32GemmScope() : saved(t_gemm_prec) { t_gemm_prec = PREC_F32; }
  ~Fp32GemmScope() { t_gemm_prec = saved; }
  Fp32GemmScope(const Fp32GemmScope&) = delete;
  Fp32GemmScope& operator=(const Fp32GemmScope&) = delete;
};

// ---- the session sets: checks and staging of a call ------------------------------------------

// Argument checks of an advance call of either session set, up to its own max_len rule: nothing
// here touches the device or a session.  `frames`: the set's host mirror of every slot's frame
// counter; per_slot(slot, n_t) is called for every row that passed, in order (the caller's
// `need`).
template <class PerSlot>
int rnnt_session_check(const char* who, int n_slots, int max_frames, const std::vector<int>& frames,
                       int n, const int32_t* slot_ids, const int32_t* n_t, int chunk,
                       bool outputs_ok, PerSlot&& per_slot) {
  const std::string w(who);
  WN_CHECK(n >= 1 && n <= n_slots, w + ": n must be in [1, n_slots]");
  WN_CHECK(outputs_ok, w + ": null output");
  std::vector<char> seen(n_slots, 0);
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i];
    WN_CHECK(sl >= 0 && sl < n_slots, w + ": slot_ids: slot id out of range");
    WN_CHECK(!seen[sl], w + ": slot_ids: a slot is named twice in one call (two rows would write "
                            "one state)");
    seen[sl] = 1;
    WN_CHECK(n_t[i] >= 0 && n_t[i] <= chunk, w + ": n_t: need 0 <= n_t <= chunk");
    if (frames[sl] + n_t[i] > max_frames) {
      set_error(w + ": the session in slot " + std::to_string(sl) + " has " +
                std::to_string(frames[sl]) + " frames and would pass max_frames = " +
                std::to_string(max_frames) + " with " + std::to_string(n_t[i]) +
                " more; no session was advanced");
      return -1;
    }
    per_slot(sl, n_t[i]);
  }
  return 0;
}

// argument checks of a reset call of either session set
inline int rnnt_reset_check(const char* who, bool args_ok, int n_slots, int n,
                            const int32_t* slot_ids) {
  const std::string w(who);
  WN_CHECK(args_ok, w + ": null argument");
  WN_CHECK(n >= 1 && n <= n_slots, w + ": n must be in [1, n_slots]");
  for (int i = 0; i < n; ++i)
    WN_CHECK(slot_ids[i] >= 0 && slot_ids[i] < n_slots, w + ": slot_ids: slot id out of range");
  return 0;
}

// The descriptor of the call in flight, desc = slot [up64(n_slots)] | n_t [up64(n_slots)]: stage
// the n slot ids (null: all of 0 .. n - 1) and, if given, n_t.
inline int rnnt_stage_call(Stager& stage, const DevBuf& desc, int n_slots, int n,
                           const int32_t* slot_ids, const int32_t* n_t, hipStream_t s) {
  std::vector<int> all;
  if (!slot_ids) {
    all.resize(n);
    for (int i = 0; i < n; ++i) all[i] = i;
    slot_ids = all.data();
  }
  const size_t bytes = (size_t)n * sizeof(int);
  WN_TRY(stage.begin((n_t ? 2 : 1) * (bytes + 64)));
  WN_TRY(stage.put_at(desc.p, slot_ids, bytes, s));
  if (n_t) WN_TRY(stage.put_at(desc.as<int>() + up64(n_slots), n_t, bytes, s));
  return stage.end(s);
}

// ---- workspace layouts -------------------------------------------------------------------------

// The greedy searches' workspace for a batch of B rows and M = B x F joint rows.  h | c are
// adjacent (one memset zeroes both); stat = n_active | steps | n_stat - 2 entries of the caller.
struct RnntGreedyLayout {
  size_t n_state = 0;               // entries of h, and of c
  float *h, *c, *gates, *pout, *pproj, *pmax;
  int *t, *cnt, *last_tok, *advance, *done, *n_tok;     // [B]
  int *row_enc, *row_pred;                              // [M]
  int *pidx, *stat;
  int carve(const wn_transducer_config& tc, int B, int M, int ncb, size_t n_stat, DevBuf& f32,
            DevBuf& i32) {
    const int H = tc.pred_hidden;
    n_state = up64((size_t)tc.pred_layers * B * H);
    const size_t n_part = up64((size_t)M * ncb), ub = up64(B), um = up64(M);
    size_t nf = 0, ni = 0;
    auto take = [](size_t& at, size_t n) { const size_t o = at; at += n; return o; };
    const size_t o_h = take(nf, n_state), o_c = take(nf, n_state),
                 o_gates = take(nf, up64((size_t)B * 4 * H)),
                 o_pout = take(nf, up64((size_t)B * tc.pred_out)),
                 o_pproj = take(nf, up64((size_t)B * tc.join_dim)), o_pmax = take(nf, n_part);
    WN_TRY(f32.ensure(nf * sizeof(float)));
    float* f = f32.as<float>();
    h = f + o_h; c = f + o_c; gates = f + o_gates; pout = f + o_pout; pproj = f + o_pproj;
    pmax = f + o_pmax;
    const size_t o_b = take(ni, 6 * ub), o_m = take(ni, 2 * um), o_pidx = take(ni, n_part),
                 o_stat = take(ni, up64(n_stat));
    WN_TRY(i32.ensure(ni * sizeof(int)));
    int* ip = i32.as<int>();
    t = ip + o_b; cnt = t + ub; last_tok = t + 2 * ub; advance = t + 3 * ub; done = t + 4 * ub;
    n_tok = t + 5 * ub;
    row_enc = ip + o_m; row_pred = row_enc + um;
    pidx = ip + o_pidx; stat = ip + o_stat;
    return 0;
  }
};

// The beam searches' workspace for B utterances and M = B x beam rows.  The predictor state and
// the slots exist in two parities (step i reads i & 1 and writes the other); h x 2 | c x 2 are
// adjacent.  `carry`: the fields of the beam step's carry mode and the call's own off / len (the
// resumable search); without it they are null and n_advance counts the advancing rows.
struct RnntBeamLayout {
  size_t n_state = 0, n_pp = 0;     // entries of one parity of h (and c), of pred_proj
  float *h, *c, *pp;                // parity p at + p * n_state / n_pp
  float *gates, *pout, *logits, *topv;
  RnntBeamSlots slots[2];
  int *src, *last_tok, *advance, *row_enc, *row_pred, *topi;
  int* n_advance = nullptr;
  int *last_time[2] = {nullptr, nullptr}, *pending = nullptr;
  int *off = nullptr, *len = nullptr, *frame0 = nullptr;
  float* h_at(int p) const { return h + p * n_state; }
  float* c_at(int p) const { return c + p * n_state; }
  float* pp_at(int p) const { return pp + p * n_pp; }
  int carve(const wn_transducer_config& tc, int B, int beam, int V, int max_tok, bool carry,
            DevBuf& f32, DevBuf& i32, DevBuf& tok) {
    const int H = tc.pred_hidden;
    const size_t M = (size_t)B * beam, um = up64(M), ub = up64(B);
    n_state = up64((size_t)tc.pred_layers * M * H);
    n_pp = up64(M * tc.join_dim);
    size_t nf = 0, ni = 0;
    auto take = [](size_t& at, size_t n) { const size_t o = at; at += n; return o; };
    const size_t o_h = take(nf, 2 * n_state), o_c = take(nf, 2 * n_state),
                 o_gates = take(nf, up64(M * 4 * H)), o_pout = take(nf, up64(M * tc.pred_out)),
                 o_pp = take(nf, 2 * n_pp), o_logits = take(nf, up64(M * ctc_pitch(V))),
                 o_topv = take(nf, up64(M * beam)), o_score = take(nf, 4 * um);
    WN_TRY(f32.ensure(nf * sizeof(float)));
    float* f = f32.as<float>();
    h = f + o_h; c = f + o_c; gates = f + o_gates; pout = f + o_pout; pp = f + o_pp;
    logits = f + o_logits; topv = f + o_topv;
    const size_t o_live = take(ni, 2 * ub), o_len = take(ni, 2 * um), o_m = take(ni, 5 * um),
                 o_topi = take(ni, up64(M * beam)), o_stat = take(ni, carry ? 0 : 64),
                 o_cb = take(ni, carry ? 3 * ub : 0), o_cm = take(ni, carry ? 3 * um : 0);
    WN_TRY(i32.ensure(ni * sizeof(int)));
    WN_TRY(tok.ensure(2 * M * max_tok * sizeof(int)));
    int* ip = i32.as<int>();
    for (int p = 0; p < 2; ++p) {
      slots[p].n_live = ip + o_live + p * ub;
      slots[p].tok_len = ip + o_len + p * um;
      slots[p].score = reinterpret_cast<double*>(f + o_score) + p * um;
      slots[p].tokens = tok.as<int>() + p * M * max_tok;
    }
    src = ip + o_m; last_tok = src + um; advance = src + 2 * um; row_enc = src + 3 * um;
    row_pred = src + 4 * um;
    topi = ip + o_topi;
    if (carry) {
      off = ip + o_cb; len = off + ub; frame0 = off + 2 * ub;
      last_time[0] = ip + o_cm; last_time[1] = last_time[0] + um; pending = last_time[0] + 2 * um;
    } else {
      n_advance = ip + o_stat;
    }
    return 0;
  }
};

// ---- once per call -----------------------------------------------------------------------------

// enc_proj [rows][J] = joint.enc_ffn(x [rows][d_model]) and, for ctc_weight != 0, the CTC
// log-prob rows [rows][ctc_pitch(V)] into `ctc` (*ctc_rows = them; for a weight of 0 neither is
// touched).  Each entry point keeps its own guard around the call.
inline int rnnt_prepare(const wn_model* m, const float* x, int rows, float* enc_proj,
                        hipStream_t s, float ctc_weight = 0.f, DevBuf* ctc = nullptr,
                        const float** ctc_rows = nullptr) {
  const ModelData& W = *m->data;
  const int d = m->cfg.d_model, V = m->cfg.vocab, ldl = ctc_pitch(V);
  Fp32GemmScope fp32;
  WN_TRY(linear(W.j_enc, x, d, enc_proj, m->tr.c.join_dim, rows, s));
  if (ctc_weight == 0.f) return 0;
  WN_TRY(ctc->ensure(((size_t)rows * ldl + 2 * (size_t)rows) * sizeof(float)));
  float* lp = ctc->as<float>();
  WN_TRY(linear(W.ctc, x, d, lp, ldl, rows, s));
  CtcRowArgs r;       // normalised in place; its top-1 is not used
  r.logits = lp; r.ld = ldl; r.M = rows; r.V = V; r.k = 1;
  r.blank = m->tr.c.blank; r.blank_penalty = 0.f;
  r.topk_val = lp + (size_t)rows * ldl;
  r.topk_idx = reinterpret_cast<int*>(r.topk_val + rows);
  r.logp = lp; r.ld_out = ldl;
  WN_TRY(ctc_logsoftmax_topk(r, s));
  *ctc_rows = lp;
  return 0;
}

// ---- the predictor -----------------------------------------------------------------------------

// one LSTM predictor step for the advancing rows: the layers in place on h / c, layer l of which
// is [B][H] at + l * layer_stride (a row offset into [L][n][H] state: layer_stride = n * H), then
// the projection into out [B][P] (proj.w == nullptr: none)
inline int predictor_step(const float* x, int ldx, const int* x_rows, int E,
                          const ModelData::LstmLayer* layers, int L, const Linear& proj, float* h,
                          float* c, int64_t layer_stride, float* gates, float* out,
                          const int* advance, const int* n_active, int B, int H, hipStream_t s) {
  for (int l = 0; l < L; ++l) {
    float* hl = h + l * layer_stride;
    RnntLinearArgs g;
    if (l == 0) { g.x1 = x; g.ldx1 = ldx; g.x1_rows = x_rows; g.K1 = E; }
    else { g.x1 = h + (l - 1) * layer_stride; g.ldx1 = H; g.K1 = H; }
    g.W1 = layers[l].w_ih; g.b1 = layers[l].b_ih;
    g.x2 = hl; g.ldx2 = H; g.W2 = layers[l].w_hh; g.K2 = H; g.b2 = layers[l].b_hh;
    g.y = gates; g.ldy = 4 * H; g.N = 4 * H; g.B = B;
    g.advance = advance; g.n_active = n_active;
    WN_TRY(rnnt_linear(g, s));
    WN_TRY(rnnt_cell(gates, hl, c + l * layer_stride, advance, B, H, n_active, s));
  }
  if (proj.w) {
    RnntLinearArgs g;
    g.x1 = h + (L - 1) * layer_stride; g.ldx1 = H; g.K1 = H;
    g.W1 = proj.w; g.b1 = proj.b;
    g.y = out; g.ldy = proj.out; g.N = proj.out; g.B = B;
    g.advance = advance; g.n_active = n_active;
    WN_TRY(rnnt_linear(g, s));
  }
  return 0;
}

// Where the window of a stateless predictor's row comes from: explicit ids [M][C], or the tail
// of a token row the search keeps (kernels.h, RnntStatelessArgs).
struct StatelessWindow {
  const int* ctx = nullptr;
  const int* tokens = nullptr; int ld_tok = 0;
  const int* tok_len = nullptr; const int* tok_row = nullptr;
};

// One advance of a stateless handle's predictor for the advancing rows, joint.pred_ffn included:
// pred_proj [M][J] in one launch.
inline int stateless_step(const wn_model* m, const StatelessWindow& w, float* pred_proj,
                          const int* advance, const int* n_active, int M, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_transducer_config& tc = m->tr.c;
  const wn_stateless_predictor_config& sc = m->tr.sp;
  RnntStatelessArgs a;
  a.kind = sc.kind; a.E = tc.pred_embed; a.C = sc.context; a.heads = sc.heads; a.J = tc.join_dim;
  a.V = m->cfg.vocab; a.act = sc.activation; a.eps = sc.norm_eps;
  a.embed = W.pred_embed; a.pos = W.pred_pos; a.ffn_w = W.pred_ffn.w; a.ffn_b = W.pred_ffn.b;
  a.conv_w = W.pred_conv_w; a.conv_b = W.pred_conv_b;
  a.norm_w = W.pred_norm.w; a.norm_b = W.pred_norm.b; a.pj_w = W.j_pred.w; a.pj_b = W.j_pred.b;
  a.ctx = w.ctx; a.tokens = w.tokens; a.ld_tok = w.ld_tok; a.tok_len = w.tok_len;
  a.tok_row = w.tok_row; a.blank = tc.blank;
  a.out = pred_proj; a.ldo = tc.join_dim; a.M = M; a.advance = advance; a.n_active = n_active;
  return rnnt_stateless_step(a, s);
}

// One advance of the handle's predictor, whichever kind it is, for the advancing rows of a search:
// pred_proj [M][J] = joint.pred_ffn(predictor(...)).  A stateless handle reads the window `w`;
// an LSTM handle steps h / c [L][M][H] on embed[last_tok] (gates [M][4H], pout [M][P] scratch).
inline int pred_proj_step(const wn_model* m, const StatelessWindow& w, const int* last_tok,
                          float* h, float* c, float* gates, float* pout, float* pred_proj,
                          const int* advance, const int* n_active, int M, hipStream_t s) {
  if (m->tr.sp.kind != 0) return stateless_step(m, w, pred_proj, advance, n_active, M, s);
  const ModelData& W = *m->data;
  const wn_transducer_config& tc = m->tr.c;
  const int E = tc.pred_embed, H = tc.pred_hidden, P = tc.pred_out, J = tc.join_dim;
  WN_TRY(predictor_step(W.pred_embed, E, last_tok, E, W.pred_rnn.data(), tc.pred_layers,
                        W.pred_proj, h, c, (int64_t)M * H, gates, pout, advance, n_active, M, H, s));
  RnntLinearArgs q;   // joint.pred_ffn
  q.x1 = pout; q.ldx1 = P; q.K1 = P; q.W1 = W.j_pred.w; q.b1 = W.j_pred.b;
  q.y = pred_proj; q.ldy = J; q.N = J; q.B = M;
  q.advance = advance; q.n_active = n_active;
  return rnnt_linear(q, s);
}

// ---- the search loops --------------------------------------------------------------------------

// The greedy searches' lock-step loop: at most `bound` calls of step() (which issues one step of
// the search on s) in groups of RNNT_GROUP; after each group the device's n_active goes to one
// of two pinned slots (pinned + 0 / + 64 bytes) and the host looks at it one group late, so the
// stream never runs dry; 0 there ends the loop.
template <class Step>
int rnnt_poll_loop(int64_t bound, const int* n_active, char* pinned, hipEvent_t* ev,
                   hipStream_t s, Step&& step) {
  volatile int* pin = reinterpret_cast<volatile int*>(pinned);
  int64_t issued = 0;
  for (int g = 0; issued < bound; ++g) {
    const int n = (int)std::min<int64_t>(RNNT_GROUP, bound - issued);
    for (int i = 0; i < n; ++i) WN_TRY(step());
    issued += n;
    WN_HIP(hipMemcpyAsync(pinned + 64 * (g & 1), n_active, sizeof(int), hipMemcpyDeviceToHost, s));
    WN_HIP(hipEventRecord(ev[g & 1], s));
    if (g >= 1) {
      WN_HIP(hipEventSynchronize(ev[(g - 1) & 1]));
      if (pin[16 * ((g - 1) & 1)] == 0) break;
    }
  }
  return 0;
}

// `steps` steps of the prefix beam search over the layout `w`, stream-ordered, no look at the
// device in between: the predictor advance, the joint rows, fusion + top-k, the beam step (in
// carry mode if the layout has the carry fields) and the state gather into the other parity.
// The result is in parity steps & 1.  off / len [B]: the encoder rows of each utterance.
inline int rnnt_beam_steps(const wn_model* m, const RnntBeamLayout& w, const float* enc_proj,
                           const float* ctc, float ctc_weight, float transducer_weight,
                           const int* off, const int* len, int B, int beam, int max_tok,
                           int steps, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_transducer_config& tc = m->tr.c;
  const int J = tc.join_dim, V = m->cfg.vocab, M = B * beam, ldl = ctc_pitch(V);
  for (int i = 0; i < steps; ++i) {
    const int cur = i & 1, nxt = cur ^ 1;
    StatelessWindow sw;   // the tail of the slot's token row in the parity just written
    sw.tokens = w.slots[cur].tokens; sw.ld_tok = max_tok; sw.tok_len = w.slots[cur].tok_len;
    WN_TRY(pred_proj_step(m, sw, w.last_tok, w.h_at(cur), w.c_at(cur), w.gates, w.pout,
                          w.pp_at(cur), w.advance, nullptr, M, s));
    RnntJointArgs ja;
    ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = w.pp_at(cur); ja.ldp = J;
    ja.row_enc = w.row_enc; ja.row_pred = w.row_pred;
    ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
    ja.logits = w.logits; ja.ldl = ldl;
    WN_TRY(rnnt_joint_rows(ja, s));
    RnntFuseArgs fa;
    fa.logits = w.logits; fa.ldl = ldl; fa.row_enc = w.row_enc; fa.ctc = ctc; fa.ldc = ldl;
    fa.cw = ctc_weight; fa.tw = transducer_weight; fa.M = M; fa.V = V; fa.k = beam;
    fa.val = w.topv; fa.idx = w.topi;
    WN_TRY(rnnt_fuse_topk(fa, s));
    RnntBeamStepArgs ba;
    ba.in = w.slots[cur]; ba.out = w.slots[nxt]; ba.max_tok = max_tok;
    ba.top_val = w.topv; ba.top_idx = w.topi; ba.off = off; ba.len = len;
    ba.frame = i; ba.B = B; ba.beam = beam; ba.blank = tc.blank; ba.V = V;
    ba.src = w.src; ba.last_tok = w.last_tok; ba.advance = w.advance; ba.row_enc = w.row_enc;
    ba.n_advance = w.n_advance;
    ba.pending = w.pending; ba.last_time_in = w.last_time[cur]; ba.last_time_out = w.last_time[nxt];
    ba.frame0 = w.frame0;
    WN_TRY(rnnt_beam_step(ba, s));
    WN_TRY(rnnt_beam_gather(w.src, w.h_at(cur), w.c_at(cur), w.pp_at(cur), w.h_at(nxt),
                            w.c_at(nxt), w.pp_at(nxt), M, tc.pred_layers, tc.pred_hidden, J, s));
  }
  return 0;
}

// ---- results -----------------------------------------------------------------------------------

// One utterance's n-best from the landing area of the result copy into the caller's arrays:
// hypothesis k < n_live with its length, score and the first `length` entries of its token row
// (pitch ld -> max_len), the others as (0, -inf).
inline int rnnt_unpack_nbest(const char* who, int n_live, int beam, const int* lens,
                             const double* scores, const int* tokens, int ld, int32_t* n_hyps_out,
                             int32_t* lens_out, double* scores_out, int32_t* tokens_out,
                             int max_len) {
  *n_hyps_out = n_live;
  for (int k = 0; k < beam; ++k) {
    const int n = k < n_live ? lens[k] : 0;
    WN_CHECK(n >= 0 && n <= ld, std::string(who) + ": token row overflow");
    WN_CHECK(n <= max_len, std::string(who) + ": max_len is smaller than the longest result (" +
                               std::to_string(n) + " tokens)");
    lens_out[k] = n;
    scores_out[k] = k < n_live ? scores[k] : -INFINITY;
    std::copy(tokens + (size_t)k * ld, tokens + (size_t)k * ld + n,
              tokens_out + (size_t)k * max_len);
  }
  return 0;
}

}  // namespace wn
