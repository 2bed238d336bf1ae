// C ABI (include/wenet_amd.h), hybrid transducer: the batched RNN-T greedy search with frame
// lookahead and the batched prefix beam search over the handle's current batch (kernels:
// transducer.hip, transducer_beam.hip) and the operator hooks of the predictor step, the joint +
// arg-max, the joint + fusion + top-k and the beam step (plain and in carry mode).
#include <algorithm>

#include "model_state.h"
#include "rnnt_host.h"

extern "C" {

int wn_transducer_greedy_search(wn_model* m, int32_t n_steps, int32_t* tokens_host,
                                int32_t* tok_lens_host, int32_t max_len, int32_t* steps_out,
                                void* stream) {
  WN_CHECK(m, "wn_transducer_greedy_search: null handle");
  WN_CHECK(m->tr.on && m->data->j_out.w,
           "wn_transducer_greedy_search: this model has no transducer weights (predictor / "
           "joint); it was not built by wn_model_create_transducer");
  WN_ENTER(m);
  WN_CHECK(m->B > 0 && m->enc.p,
           "wn_transducer_greedy_search: no current batch (call wn_encode / wn_set_encoder_out)");
  WN_CHECK(tokens_host && tok_lens_host && max_len >= 0, "wn_transducer_greedy_search: null output");
  WN_CHECK(n_steps >= 1, "wn_transducer_greedy_search: n_steps must be >= 1");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const ModelData& W = *m->data;
  const int B = m->B, rows = m->rows;
  const wn_transducer_config& tc = m->tr.c;
  const int J = tc.join_dim, V = m->cfg.vocab, blank = tc.blank;
  const int F = std::min(std::max(tune().rnnt_lookahead, 1), 16);
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = std::max(longest, m->len[b]);
  // an utterance emits at most n_steps symbols per frame
  const int64_t max_tok64 = (int64_t)std::max(longest, 1) * n_steps;
  WN_CHECK((int64_t)B * max_tok64 <= ((int64_t)1 << 28),
           "wn_transducer_greedy_search: B x T' x n_steps tokens do not fit the token buffer");
  const int max_tok = (int)max_tok64;
  const int M = B * F, ncb = rnnt_joint_col_blocks(V);

  // ---- workspace ----------------------------------------------------------------------------
  WN_TRY(m->tr_enc.ensure((size_t)std::max(rows, 1) * J * sizeof(float)));
  RnntGreedyLayout w;
  WN_TRY(w.carve(tc, B, M, ncb, 2, m->tr_f32, m->tr_i32));
  WN_TRY(m->tr_tok.ensure((size_t)B * max_tok * sizeof(int)));
  WN_TRY(m->tr_host.ensure(256 + (size_t)B * sizeof(int)));
  for (hipEvent_t& e : m->tr_ev)
    if (!e) WN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  float* enc_proj = m->tr_enc.as<float>();
  RnntState st;
  st.t = w.t; st.cnt = w.cnt; st.last_tok = w.last_tok; st.advance = w.advance;
  st.done = w.done; st.n_tok = w.n_tok;
  st.row_enc = w.row_enc; st.row_pred = w.row_pred;
  st.n_active = w.stat; st.steps = w.stat + 1;
  st.tokens = m->tr_tok.as<int>(); st.max_tok = max_tok;
  st.off = m->d_off.as<int>(); st.len = m->d_len.as<int>();

  // ---- once per batch: enc_proj = joint.enc_ffn(encoder_out), zero LSTM state -----------------
  if (rows > 0) WN_TRY(rnnt_prepare(m, m->enc.as<float>(), rows, enc_proj, s));
  if (w.n_state > 0) WN_HIP(hipMemsetAsync(w.h, 0, 2 * w.n_state * sizeof(float), s));
  WN_TRY(rnnt_init(st, B, F, blank, s));

  // ---- the lock-step loop ---------------------------------------------------------------------
  StatelessWindow sw;     // the tail of the utterance's token row up to n_tok
  sw.tokens = st.tokens; sw.ld_tok = max_tok; sw.tok_len = st.n_tok;
  RnntJointArgs ja;
  ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = w.pproj; ja.ldp = J;
  ja.row_enc = st.row_enc; ja.row_pred = st.row_pred;
  ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
  ja.part_max = w.pmax; ja.part_idx = w.pidx; ja.n_active = st.n_active;
  const int64_t bound = (int64_t)longest * ((int64_t)n_steps + 1) + 1;
  WN_TRY(rnnt_poll_loop(bound, st.n_active, m->tr_host.p, m->tr_ev, s, [&]() -> int {
    WN_TRY(pred_proj_step(m, sw, st.last_tok, w.h, w.c, w.gates, w.pout, w.pproj, st.advance,
                          st.n_active, B, s));
    WN_TRY(rnnt_joint_argmax(ja, s));
    return rnnt_advance(w.pmax, w.pidx, ncb, V, st, B, F, blank, n_steps, s);
  }));

  // ---- results: lengths and the step count first, then the token rows that were filled ---------
  int* lens_pin = reinterpret_cast<int*>(m->tr_host.p + 256);
  WN_HIP(hipMemcpyAsync(lens_pin, st.n_tok, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(m->tr_host.p + 128, st.n_active, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  const int* tail = reinterpret_cast<const int*>(m->tr_host.p + 128);
  WN_CHECK(tail[0] == 0, "wn_transducer_greedy_search: the search did not finish within its "
                         "step bound");
  if (steps_out) *steps_out = tail[1];
  int most = 0;
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens_pin[b] <= max_tok, "wn_transducer_greedy_search: token buffer overflow");
    tok_lens_host[b] = lens_pin[b];
    most = std::max(most, lens_pin[b]);
  }
  WN_CHECK(most <= max_len, "wn_transducer_greedy_search: max_len is smaller than the longest "
                            "result (" + std::to_string(most) + " tokens)");
  if (most > 0) {
    WN_HIP(hipMemcpy2DAsync(tokens_host, (size_t)max_len * sizeof(int), st.tokens,
                            (size_t)max_tok * sizeof(int), (size_t)most * sizeof(int), B,
                            hipMemcpyDeviceToHost, s));
    WN_HIP(stream_wait(s));
  }
  return 0;
}

int wn_transducer_beam_search(wn_model* m, int32_t beam, float ctc_weight,
                              float transducer_weight, int32_t* n_hyps_host,
                              int32_t* hyp_lens_host, int32_t* hyp_tokens_host,
                              double* hyp_scores_host, int32_t max_len, void* stream) {
  WN_CHECK(m, "wn_transducer_beam_search: null handle");
  WN_CHECK(m->tr.on && m->data->j_out.w,
           "wn_transducer_beam_search: this model has no transducer weights (predictor / "
           "joint); it was not built by wn_model_create_transducer");
  WN_ENTER(m);
  WN_CHECK(m->B > 0 && m->enc.p,
           "wn_transducer_beam_search: no current batch (call wn_encode / wn_set_encoder_out)");
  WN_CHECK(n_hyps_host && hyp_lens_host && hyp_tokens_host && hyp_scores_host && max_len >= 0,
           "wn_transducer_beam_search: null output");
  const int V = m->cfg.vocab;
  WN_CHECK(beam >= 1 && beam <= 16, "wn_transducer_beam_search: beam must be in [1, 16]");
  WN_CHECK(beam <= V, "wn_transducer_beam_search: beam is larger than the vocabulary");
  WN_CHECK(ctc_weight >= 0.f && transducer_weight >= 0.f,
           "wn_transducer_beam_search: the weights must be >= 0");
  WN_CHECK(ctc_weight > 0.f || transducer_weight > 0.f,
           "wn_transducer_beam_search: ctc_weight and transducer_weight are both 0");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  WN_CHECK(ctc_weight == 0.f || m->data->ctc.w, "wn_transducer_beam_search: ctc_weight > 0 on a "
                                                "handle without a CTC head");
  const int B = m->B, rows = m->rows;
  const wn_transducer_config& tc = m->tr.c;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = std::max(longest, m->len[b]);
  const int max_tok = std::max(longest, 1);     // one symbol per frame at most
  const int64_t M64 = (int64_t)B * beam;
  WN_CHECK(M64 * std::max(max_tok, ctc_pitch(V)) <= ((int64_t)1 << 28),
           "wn_transducer_beam_search: B x beam rows do not fit the workspace");
  const int M = (int)M64;

  // ---- workspace, sized by B x beam -----------------------------------------------------------
  WN_TRY(m->tr_enc.ensure((size_t)std::max(rows, 1) * tc.join_dim * sizeof(float)));
  RnntBeamLayout w;
  WN_TRY(w.carve(tc, B, beam, V, max_tok, false, m->tr_f32, m->tr_i32, m->tr_tok));
  float* enc_proj = m->tr_enc.as<float>();
  const int* off = m->d_off.as<int>();
  const int* len = m->d_len.as<int>();

  // ---- once per batch: enc_proj, the CTC log-prob rows (cw > 0 only), zero LSTM state ----------
  const float* ctc = nullptr;
  if (rows > 0)
    WN_TRY(rnnt_prepare(m, m->enc.as<float>(), rows, enc_proj, s, ctc_weight, &m->tr_ctc, &ctc));
  if (w.n_state > 0) WN_HIP(hipMemsetAsync(w.h, 0, 4 * w.n_state * sizeof(float), s));
  WN_HIP(hipMemsetAsync(w.n_advance, 0, sizeof(int), s));
  WN_TRY(rnnt_beam_init(w.slots[0], w.last_tok, w.advance, w.row_enc, w.row_pred, off, len, B,
                        beam, tc.blank, s));

  // ---- exactly `longest` steps, stream-ordered, no look at the device in between ---------------
  WN_TRY(rnnt_beam_steps(m, w, enc_proj, ctc, ctc_weight, transducer_weight, off, len, B, beam,
                         max_tok, longest, s));

  // ---- results: counts | lengths | scores | token rows into pinned memory, one wait ------------
  const RnntBeamSlots& fin = w.slots[longest & 1];
  const size_t um = up64(M);
  const size_t p_len = up64(B) * sizeof(int), p_sc = p_len + um * sizeof(int),
               p_tok = p_sc + um * sizeof(double),
               p_stat = p_tok + up64((size_t)M * max_tok) * sizeof(int);
  WN_TRY(m->tr_host.ensure(p_stat + 64));
  char* hp = m->tr_host.p;
  WN_HIP(hipMemcpyAsync(hp, fin.n_live, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(hp + p_len, fin.tok_len, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(hp + p_sc, fin.score, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(hp + p_tok, fin.tokens, (size_t)M * max_tok * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(hp + p_stat, w.n_advance, sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  m->tr_beam_steps = longest;
  m->tr_beam_advance = *reinterpret_cast<const int*>(hp + p_stat);
  for (int b = 0; b < B; ++b) m->tr_beam_advance += m->len[b] > 0;    // the first step's rows
  const int* nl = reinterpret_cast<const int*>(hp);
  const int* tl = reinterpret_cast<const int*>(hp + p_len);
  const double* sc = reinterpret_cast<const double*>(hp + p_sc);
  const int* tk = reinterpret_cast<const int*>(hp + p_tok);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(nl[b] >= 1 && nl[b] <= beam, "wn_transducer_beam_search: an utterance ended without "
                                          "a hypothesis");
    const size_t g = (size_t)b * beam;
    WN_TRY(rnnt_unpack_nbest("wn_transducer_beam_search", nl[b], beam, tl + g, sc + g,
                             tk + g * max_tok, max_tok, n_hyps_host + b, hyp_lens_host + g,
                             hyp_scores_host + g, hyp_tokens_host + g * max_len, max_len));
  }
  return 0;
}

int wn_transducer_beam_stats(wn_model* m, int32_t* steps_out, int64_t* advance_rows_out) {
  WN_CHECK(m, "wn_transducer_beam_stats: null handle");
  if (steps_out) *steps_out = m->tr_beam_steps;
  if (advance_rows_out) *advance_rows_out = m->tr_beam_advance;
  return 0;
}

int wn_op_lstm_step(const float* x_dev, const float* const* w_host, int32_t n_layers,
                    const float* proj_w_dev, const float* proj_b_dev, float* h_dev, float* c_dev,
                    const int32_t* advance_dev, float* out_dev, int32_t B, int32_t E, int32_t H,
                    int32_t P, void* stream) {
  WN_CHECK(x_dev && w_host && h_dev && c_dev, "wn_op_lstm_step: null argument");
  WN_CHECK(n_layers >= 1 && n_layers <= 8 && B >= 1 && E >= 1 && E <= 1024 && H >= 1 && H <= 1024,
           "wn_op_lstm_step: 1..8 layers, widths in [1, 1024]");
  WN_CHECK(!proj_w_dev || (out_dev && P >= 1), "wn_op_lstm_step: projection without an output");
  hipStream_t s = (hipStream_t)stream;
  std::vector<ModelData::LstmLayer> layers(n_layers);
  for (int l = 0; l < n_layers; ++l) {
    for (int i = 0; i < 4; ++i) WN_CHECK(w_host[4 * l + i], "wn_op_lstm_step: null weight");
    layers[l] = {w_host[4 * l], w_host[4 * l + 1], w_host[4 * l + 2], w_host[4 * l + 3]};
  }
  static thread_local DevBuf gates;
  WN_TRY(gates.ensure((size_t)B * 4 * H * sizeof(float)));
  Linear proj;
  proj.w = proj_w_dev; proj.b = proj_b_dev; proj.out = P; proj.in = H;
  return predictor_step(x_dev, E, nullptr, E, layers.data(), n_layers, proj, h_dev, c_dev,
                        (int64_t)B * H, gates.as<float>(), out_dev, advance_dev, nullptr, B, H,
                        s);
}

int wn_op_stateless_step(const wn_stateless_predictor_config* scfg, const int32_t* ctx_host,
                         const float* const* w_dev, const int32_t* advance_host, float* out_dev,
                         int32_t M, int32_t V, int32_t E, int32_t J, void* stream) {
  WN_CHECK(scfg && ctx_host && w_dev && out_dev, "wn_op_stateless_step: null argument");
  const wn_stateless_predictor_config& sc = *scfg;
  WN_CHECK(sc.kind == 1 || sc.kind == 2,
           "wn_op_stateless_step: kind must be 1 (embedding) or 2 (conv)");
  WN_CHECK(M >= 1 && M <= (1 << 20) && V >= 1, "wn_op_stateless_step: empty or too large");
  WN_CHECK(E >= 1 && E <= 1024 && J >= 1 && J <= 1024,
           "wn_op_stateless_step: widths must be in [1, 1024]");
  WN_CHECK(sc.context >= 1 && sc.context <= 16 && sc.heads >= 1 && sc.heads <= 16,
           "wn_op_stateless_step: context and heads must be in [1, 16]");
  WN_CHECK(sc.activation == 0 || sc.activation == 1,
           "wn_op_stateless_step: activation 0 (swish) or 1 (relu)");
  const int C = sc.context, nw = sc.kind == 1 ? 8 : 7;
  for (int i = 0; i < nw; ++i)
    WN_CHECK(w_dev[i] || (sc.kind == 2 && i == 2), "wn_op_stateless_step: null weight");
  for (int64_t i = 0; i < (int64_t)M * C; ++i)
    WN_CHECK(ctx_host[i] >= -1 && ctx_host[i] < V,
             "wn_op_stateless_step: context id outside [-1, vocabulary)");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf ids;
  const size_t n_ctx = up64((size_t)M * C);
  WN_TRY(ids.ensure((n_ctx + (size_t)M) * sizeof(int)));
  WN_HIP(hipMemcpyAsync(ids.p, ctx_host, (size_t)M * C * sizeof(int), hipMemcpyHostToDevice, s));
  if (advance_host)
    WN_HIP(hipMemcpyAsync(ids.as<int>() + n_ctx, advance_host, (size_t)M * sizeof(int),
                          hipMemcpyHostToDevice, s));
  RnntStatelessArgs a;
  a.kind = sc.kind; a.E = E; a.C = C; a.heads = sc.kind == 1 ? sc.heads : 1; a.J = J; a.V = V;
  a.act = sc.activation; a.eps = sc.norm_eps;
  a.embed = w_dev[0];
  if (sc.kind == 1) { a.pos = w_dev[1]; a.ffn_w = w_dev[2]; a.ffn_b = w_dev[3]; }
  else { a.conv_w = w_dev[1]; a.conv_b = w_dev[2]; }
  const float* const* r = w_dev + (sc.kind == 1 ? 4 : 3);
  a.norm_w = r[0]; a.norm_b = r[1]; a.pj_w = r[2]; a.pj_b = r[3];
  a.ctx = ids.as<int>();
  a.out = out_dev; a.ldo = J; a.M = M;
  a.advance = advance_host ? ids.as<int>() + n_ctx : nullptr;
  WN_TRY(rnnt_stateless_step(a, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_joint_argmax(const float* enc_proj_dev, int32_t enc_rows, const float* pred_proj_dev,
                       int32_t pred_rows, const int32_t* row_enc_host,
                       const int32_t* row_pred_host, const float* w_dev, const float* bias_dev,
                       int32_t M, int32_t J, int32_t V, int32_t* idx_host, float* max_host,
                       void* stream) {
  WN_CHECK(enc_proj_dev && pred_proj_dev && row_enc_host && row_pred_host && w_dev && bias_dev &&
           idx_host && max_host, "wn_op_joint_argmax: null argument");
  WN_CHECK(M >= 1 && V >= 1 && enc_rows >= 1 && pred_rows >= 1, "wn_op_joint_argmax: empty");
  for (int i = 0; i < M; ++i)
    WN_CHECK(row_enc_host[i] < enc_rows && row_pred_host[i] >= 0 && row_pred_host[i] < pred_rows,
             "wn_op_joint_argmax: row map outside its matrix");
  hipStream_t s = (hipStream_t)stream;
  const int ncb = rnnt_joint_col_blocks(V);
  static thread_local DevBuf map, part;
  WN_TRY(map.ensure((size_t)2 * M * sizeof(int)));
  WN_TRY(part.ensure(((size_t)2 * M * ncb + 2 * M) * sizeof(float)));
  WN_HIP(hipMemcpyAsync(map.p, row_enc_host, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipMemcpyAsync(map.as<int>() + M, row_pred_host, (size_t)M * sizeof(int),
                        hipMemcpyHostToDevice, s));
  RnntJointArgs ja;
  ja.enc_proj = enc_proj_dev; ja.lde = J; ja.pred_proj = pred_proj_dev; ja.ldp = J;
  ja.row_enc = map.as<int>(); ja.row_pred = map.as<int>() + M;
  ja.W = w_dev; ja.bias = bias_dev; ja.M = M; ja.J = J; ja.V = V;
  ja.part_max = part.as<float>(); ja.part_idx = part.as<int>() + (size_t)M * ncb;
  WN_TRY(rnnt_joint_argmax(ja, s));
  // the column-block partials through the device reduction of the search's advance kernel
  float* out_max = part.as<float>() + (size_t)2 * M * ncb;
  int* out_idx = part.as<int>() + (size_t)2 * M * ncb + M;
  WN_TRY(rnnt_reduce_partials(ja.part_max, ja.part_idx, ncb, M, out_max, out_idx, s));
  WN_HIP(hipMemcpyAsync(max_host, out_max, (size_t)M * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(idx_host, out_idx, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_joint_fuse_topk(const float* enc_proj_dev, int32_t enc_rows, const float* pred_proj_dev,
                          int32_t pred_rows, const int32_t* row_enc_host,
                          const int32_t* row_pred_host, const float* w_dev, const float* bias_dev,
                          int32_t M, int32_t J, int32_t V, const float* ctc_logp_dev,
                          int32_t ctc_rows, const int32_t* row_ctc_host, float ctc_weight,
                          float transducer_weight, int32_t k, float* val_host, int32_t* idx_host,
                          float* fused_host, void* stream) {
  WN_CHECK(enc_proj_dev && pred_proj_dev && row_enc_host && row_pred_host && w_dev && bias_dev &&
           val_host && idx_host, "wn_op_joint_fuse_topk: null argument");
  WN_CHECK(M >= 1 && V >= 1 && enc_rows >= 1 && pred_rows >= 1, "wn_op_joint_fuse_topk: empty");
  WN_CHECK(k >= 1 && k <= 16, "wn_op_joint_fuse_topk: k must be in [1, 16]");
  WN_CHECK(k <= V, "wn_op_joint_fuse_topk: k is larger than the vocabulary");
  WN_CHECK(ctc_weight >= 0.f && transducer_weight >= 0.f,
           "wn_op_joint_fuse_topk: the weights must be >= 0");
  WN_CHECK(ctc_weight > 0.f || transducer_weight > 0.f,
           "wn_op_joint_fuse_topk: ctc_weight and transducer_weight are both 0");
  WN_CHECK(ctc_weight == 0.f || (ctc_logp_dev && ctc_rows >= 1),
           "wn_op_joint_fuse_topk: ctc_weight > 0 without CTC log-probs");
  WN_CHECK((int64_t)M * V <= ((int64_t)1 << 28), "wn_op_joint_fuse_topk: M x V is too large");
  for (int i = 0; i < M; ++i) {
    WN_CHECK(row_enc_host[i] < enc_rows && row_pred_host[i] >= 0 && row_pred_host[i] < pred_rows,
             "wn_op_joint_fuse_topk: row map outside its matrix");
    if (ctc_weight != 0.f && row_enc_host[i] >= 0) {
      const int rc = row_ctc_host ? row_ctc_host[i] : row_enc_host[i];
      WN_CHECK(rc >= 0 && rc < ctc_rows, "wn_op_joint_fuse_topk: CTC row map outside its matrix");
    }
  }
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf map, rowsb, out;
  WN_TRY(map.ensure((size_t)3 * M * sizeof(int)));
  WN_TRY(rowsb.ensure((size_t)2 * M * V * sizeof(float)));
  WN_TRY(out.ensure((size_t)2 * M * k * sizeof(float)));
  int* mp = map.as<int>();
  WN_HIP(hipMemcpyAsync(mp, row_enc_host, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipMemcpyAsync(mp + M, row_pred_host, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  if (row_ctc_host)
    WN_HIP(hipMemcpyAsync(mp + 2 * M, row_ctc_host, (size_t)M * sizeof(int), hipMemcpyHostToDevice, s));
  float* logits = rowsb.as<float>();
  float* fused = logits + (size_t)M * V;
  if (fused_host) WN_HIP(hipMemsetAsync(fused, 0, (size_t)M * V * sizeof(float), s));
  RnntJointArgs ja;
  ja.enc_proj = enc_proj_dev; ja.lde = J; ja.pred_proj = pred_proj_dev; ja.ldp = J;
  ja.row_enc = mp; ja.row_pred = mp + M;
  ja.W = w_dev; ja.bias = bias_dev; ja.M = M; ja.J = J; ja.V = V;
  ja.logits = logits; ja.ldl = V;
  WN_TRY(rnnt_joint_rows(ja, s));
  RnntFuseArgs fa;
  fa.logits = logits; fa.ldl = V; fa.row_enc = mp;
  fa.ctc = ctc_weight != 0.f ? ctc_logp_dev : nullptr; fa.ldc = V;
  fa.row_ctc = row_ctc_host ? mp + 2 * M : nullptr;
  fa.cw = ctc_weight; fa.tw = transducer_weight; fa.M = M; fa.V = V; fa.k = k;
  fa.val = out.as<float>(); fa.idx = out.as<int>() + (size_t)M * k;
  if (fused_host) { fa.fused = fused; fa.ldf = V; }
  WN_TRY(rnnt_fuse_topk(fa, s));
  WN_HIP(hipMemcpyAsync(val_host, fa.val, (size_t)M * k * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(idx_host, fa.idx, (size_t)M * k * sizeof(int), hipMemcpyDeviceToHost, s));
  if (fused_host)
    WN_HIP(hipMemcpyAsync(fused_host, fused, (size_t)M * V * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

// the body of wn_op_rnnt_beam_step; `cy` non-null: the carry mode (wn_op_rnnt_beam_step_carry)
struct BeamStepCarry {
  const int32_t* frame0; const int32_t* last_time; const int32_t* pending; const int32_t* last_tok;
  int32_t* pending_out; int32_t* last_time_out;
};
static int beam_step_op(int32_t B, int32_t beam, int32_t blank, int32_t V, int32_t frame,
                        const int32_t* lens_host, int32_t max_tok, const int32_t* n_live_host,
                        const double* scores_host, const int32_t* tok_lens_host,
                        const int32_t* tokens_host, const float* top_val_host,
                        const int32_t* top_idx_host, int32_t* n_live_out, double* scores_out,
                        int32_t* tok_lens_out, int32_t* tokens_out, int32_t* src_out,
                        int32_t* tok_out, int32_t* advance_out, int32_t* row_enc_out,
                        const BeamStepCarry* cy, void* stream) {
  WN_CHECK(lens_host && n_live_host && scores_host && tok_lens_host && tokens_host &&
           top_val_host && top_idx_host && n_live_out && scores_out && tok_lens_out &&
           tokens_out && src_out && tok_out && advance_out && row_enc_out,
           "wn_op_rnnt_beam_step: null argument");
  WN_CHECK(beam >= 1 && beam <= 16, "wn_op_rnnt_beam_step: beam must be in [1, 16]");
  WN_CHECK(B >= 1 && V >= 1 && max_tok >= 1 && frame >= 0 && blank >= 0 && blank < V &&
           (int64_t)B * beam * max_tok <= ((int64_t)1 << 28),
           "wn_op_rnnt_beam_step: empty or too large, or a blank outside the vocabulary");
  std::vector<int> off(B);
  int rows = 0;
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens_host[b] >= 0, "wn_op_rnnt_beam_step: negative length");
    off[b] = rows;
    rows += lens_host[b];
    WN_CHECK(n_live_host[b] >= 0 && n_live_host[b] <= beam,
             "wn_op_rnnt_beam_step: live count outside [0, beam]");
    for (int j = 0; j < n_live_host[b]; ++j) {
      const int g = b * beam + j;
      // a live slot of an unfinished utterance may append one token
      const int room = frame < lens_host[b] ? max_tok - 1 : max_tok;
      WN_CHECK(tok_lens_host[g] >= 0 && tok_lens_host[g] <= room,
               "wn_op_rnnt_beam_step: token count outside its row");
      if (frame < lens_host[b])
        for (int r = 0; r < beam; ++r)
          WN_CHECK(top_idx_host[(size_t)g * beam + r] >= 0 && top_idx_host[(size_t)g * beam + r] < V,
                   "wn_op_rnnt_beam_step: top-k index outside the vocabulary");
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const int M = B * beam;
  const size_t um = up64(M), ub = up64(B);
  static thread_local DevBuf ibuf, fbuf, cbuf;
  const size_t o_tok = 4 * ub + 6 * um + 2 * up64((size_t)M * beam);
  if (cy) WN_TRY(cbuf.ensure((ub + 3 * um) * sizeof(int)));
  WN_TRY(ibuf.ensure((o_tok + 2 * (size_t)M * max_tok) * sizeof(int)));
  WN_TRY(fbuf.ensure(2 * um * sizeof(double)));
  int* ip = ibuf.as<int>();
  RnntBeamStepArgs a;
  int *d_off = ip, *d_len = ip + ub;
  a.in.n_live = ip + 2 * ub; a.out.n_live = ip + 3 * ub;
  int* q = ip + 4 * ub;
  a.in.tok_len = q; a.out.tok_len = q + um; a.src = q + 2 * um; a.last_tok = q + 3 * um;
  a.advance = q + 4 * um; a.row_enc = q + 5 * um;
  int* d_topi = q + 6 * um;
  float* d_topv = reinterpret_cast<float*>(d_topi + up64((size_t)M * beam));
  a.in.tokens = ip + o_tok; a.out.tokens = a.in.tokens + (size_t)M * max_tok;
  a.in.score = fbuf.as<double>(); a.out.score = a.in.score + um;
  auto up = [&](void* dst, const void* srcp, size_t bytes) {
    return hipMemcpyAsync(dst, srcp, bytes, hipMemcpyHostToDevice, s);
  };
  WN_HIP(up(d_off, off.data(), (size_t)B * sizeof(int)));
  WN_HIP(up(d_len, lens_host, (size_t)B * sizeof(int)));
  WN_HIP(up(a.in.n_live, n_live_host, (size_t)B * sizeof(int)));
  WN_HIP(up(a.in.tok_len, tok_lens_host, (size_t)M * sizeof(int)));
  WN_HIP(up(a.in.tokens, tokens_host, (size_t)M * max_tok * sizeof(int)));
  WN_HIP(up(a.in.score, scores_host, (size_t)M * sizeof(double)));
  WN_HIP(up(d_topi, top_idx_host, (size_t)M * beam * sizeof(int)));
  WN_HIP(up(d_topv, top_val_host, (size_t)M * beam * sizeof(float)));
  WN_HIP(hipMemsetAsync(a.out.tokens, 0xff, (size_t)M * max_tok * sizeof(int), s));   // -1
  a.max_tok = max_tok; a.top_val = d_topv; a.top_idx = d_topi; a.off = d_off; a.len = d_len;
  a.frame = frame; a.B = B; a.beam = beam; a.blank = blank; a.V = V;
  if (cy) {
    int* cp = cbuf.as<int>();
    int *d_f0 = cp, *d_lt_in = cp + ub, *d_lt_out = d_lt_in + um, *d_pend = d_lt_in + 2 * um;
    WN_HIP(up(d_f0, cy->frame0, (size_t)B * sizeof(int)));
    WN_HIP(up(d_lt_in, cy->last_time, (size_t)M * sizeof(int)));
    WN_HIP(up(d_pend, cy->pending, (size_t)M * sizeof(int)));
    WN_HIP(up(a.last_tok, cy->last_tok, (size_t)M * sizeof(int)));
    WN_HIP(hipMemsetAsync(d_lt_out, 0xff, (size_t)M * sizeof(int), s));
    a.frame0 = d_f0; a.last_time_in = d_lt_in; a.last_time_out = d_lt_out; a.pending = d_pend;
  }
  WN_TRY(rnnt_beam_step(a, s));
  auto down = [&](void* dst, const void* srcp, size_t bytes) {
    return hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, s);
  };
  if (cy) {
    WN_HIP(down(cy->pending_out, a.pending, (size_t)M * sizeof(int)));
    WN_HIP(down(cy->last_time_out, a.last_time_out, (size_t)M * sizeof(int)));
  }
  WN_HIP(down(n_live_out, a.out.n_live, (size_t)B * sizeof(int)));
  WN_HIP(down(scores_out, a.out.score, (size_t)M * sizeof(double)));
  WN_HIP(down(tok_lens_out, a.out.tok_len, (size_t)M * sizeof(int)));
  WN_HIP(down(tokens_out, a.out.tokens, (size_t)M * max_tok * sizeof(int)));
  WN_HIP(down(src_out, a.src, (size_t)M * sizeof(int)));
  WN_HIP(down(tok_out, a.last_tok, (size_t)M * sizeof(int)));
  WN_HIP(down(advance_out, a.advance, (size_t)M * sizeof(int)));
  WN_HIP(down(row_enc_out, a.row_enc, (size_t)M * sizeof(int)));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_rnnt_beam_step(int32_t B, int32_t beam, int32_t blank, int32_t V, int32_t frame,
                         const int32_t* lens_host, int32_t max_tok, const int32_t* n_live_host,
                         const double* scores_host, const int32_t* tok_lens_host,
                         const int32_t* tokens_host, const float* top_val_host,
                         const int32_t* top_idx_host, int32_t* n_live_out, double* scores_out,
                         int32_t* tok_lens_out, int32_t* tokens_out, int32_t* src_out,
                         int32_t* tok_out, int32_t* advance_out, int32_t* row_enc_out,
                         void* stream) {
  return beam_step_op(B, beam, blank, V, frame, lens_host, max_tok, n_live_host, scores_host,
                      tok_lens_host, tokens_host, top_val_host, top_idx_host, n_live_out,
                      scores_out, tok_lens_out, tokens_out, src_out, tok_out, advance_out,
                      row_enc_out, nullptr, stream);
}

int wn_op_rnnt_beam_step_carry(int32_t B, int32_t beam, int32_t blank, int32_t V, int32_t frame,
                               const int32_t* lens_host, int32_t max_tok,
                               const int32_t* n_live_host, const double* scores_host,
                               const int32_t* tok_lens_host, const int32_t* tokens_host,
                               const float* top_val_host, const int32_t* top_idx_host,
                               const int32_t* frame0_host, const int32_t* last_time_host,
                               const int32_t* pending_host, const int32_t* last_tok_host,
                               int32_t* n_live_out, double* scores_out, int32_t* tok_lens_out,
                               int32_t* tokens_out, int32_t* src_out, int32_t* tok_out,
                               int32_t* advance_out, int32_t* row_enc_out, int32_t* pending_out,
                               int32_t* last_time_out, void* stream) {
  WN_CHECK(frame0_host && last_time_host && pending_host && last_tok_host && pending_out &&
           last_time_out, "wn_op_rnnt_beam_step_carry: null argument");
  const BeamStepCarry cy = {frame0_host, last_time_host, pending_host, last_tok_host, pending_out,
                            last_time_out};
  if (beam_step_op(B, beam, blank, V, frame, lens_host, max_tok, n_live_host, scores_host,
                   tok_lens_host, tokens_host, top_val_host, top_idx_host, n_live_out, scores_out,
                   tok_lens_out, tokens_out, src_out, tok_out, advance_out, row_enc_out, &cy,
                   stream) != 0) {
    // the shared body names the plain hook in its refusals
    std::string e = wn_last_error();
    const std::string from = "wn_op_rnnt_beam_step:";
    const size_t at = e.find(from);
    if (at != std::string::npos) e.replace(at, from.size(), "wn_op_rnnt_beam_step_carry:");
    set_error(e);
    return -1;
  }
  return 0;
}

}  // extern "C"
