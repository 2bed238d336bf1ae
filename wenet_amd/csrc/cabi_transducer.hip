// C ABI (include/wenet_amd.h), hybrid transducer: the batched RNN-T greedy search with frame
// lookahead over the handle's current batch (kernels: transducer.hip) and the two operator hooks
// of its predictor step and joint + arg-max.
#include <algorithm>

#include "model_state.h"

namespace wn {
namespace {

constexpr int RNNT_GROUP = 8;     // steps issued between two looks at n_active

// one predictor step for the advancing rows: LSTM layers in place on h / c [L][B][H], then the
// projection into out [B][P] (proj.w == nullptr: none)
int predictor_step(const float* x, int ldx, const int* x_rows, int E,
                   const ModelData::LstmLayer* layers, int L, const Linear& proj, float* h,
                   float* c, float* gates, float* out, const int* advance, const int* n_active,
                   int B, int H, hipStream_t s) {
  for (int l = 0; l < L; ++l) {
    float* hl = h + (size_t)l * B * H;
    RnntLinearArgs g;
    if (l == 0) { g.x1 = x; g.ldx1 = ldx; g.x1_rows = x_rows; g.K1 = E; }
    else { g.x1 = h + (size_t)(l - 1) * B * H; g.ldx1 = H; g.K1 = H; }
    g.W1 = layers[l].w_ih; g.b1 = layers[l].b_ih;
    g.x2 = hl; g.ldx2 = H; g.W2 = layers[l].w_hh; g.K2 = H; g.b2 = layers[l].b_hh;
    g.y = gates; g.ldy = 4 * H; g.N = 4 * H; g.B = B;
    g.advance = advance; g.n_active = n_active;
    WN_TRY(rnnt_linear(g, s));
    WN_TRY(rnnt_cell(gates, hl, c + (size_t)l * B * H, advance, B, H, n_active, s));
  }
  if (proj.w) {
    RnntLinearArgs g;
    g.x1 = h + (size_t)(L - 1) * B * H; g.ldx1 = H; g.K1 = H;
    g.W1 = proj.w; g.b1 = proj.b;
    g.y = out; g.ldy = proj.out; g.N = proj.out; g.B = B;
    g.advance = advance; g.n_active = n_active;
    WN_TRY(rnnt_linear(g, s));
  }
  return 0;
}

size_t up64(size_t n) { return (n + 63) / 64 * 64; }

}  // namespace
}  // namespace wn

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
  const wn_config& c = m->cfg;
  const int B = m->B, rows = m->rows, d = c.d_model;
  const wn_transducer_config& tc = m->tr.c;
  const int E = tc.pred_embed, H = tc.pred_hidden, L = tc.pred_layers, P = tc.pred_out;
  const int J = tc.join_dim, V = c.vocab, blank = tc.blank;
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
  const size_t n_state = up64((size_t)L * B * H);
  const size_t o_h = 0, o_c = n_state, o_gates = o_c + n_state,
               o_pout = o_gates + up64((size_t)B * 4 * H), o_pproj = o_pout + up64((size_t)B * P),
               o_pmax = o_pproj + up64((size_t)B * J), n_f32 = o_pmax + up64((size_t)M * ncb);
  WN_TRY(m->tr_f32.ensure(n_f32 * sizeof(float)));
  const size_t ub = up64(B), um = up64(M);
  const size_t n_i32 = 6 * ub + 2 * um + up64((size_t)M * ncb) + 64;
  WN_TRY(m->tr_i32.ensure(n_i32 * sizeof(int)));
  WN_TRY(m->tr_tok.ensure((size_t)B * max_tok * sizeof(int)));
  WN_TRY(m->tr_host.ensure(256 + (size_t)B * sizeof(int)));
  for (hipEvent_t& e : m->tr_ev)
    if (!e) WN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  float* f = m->tr_f32.as<float>();
  float* enc_proj = m->tr_enc.as<float>();
  float *h = f + o_h, *cst = f + o_c, *gates = f + o_gates, *pout = f + o_pout,
        *pproj = f + o_pproj, *pmax = f + o_pmax;
  int* ip = m->tr_i32.as<int>();
  RnntState st;
  st.t = ip; st.cnt = ip + ub; st.last_tok = ip + 2 * ub; st.advance = ip + 3 * ub;
  st.done = ip + 4 * ub; st.n_tok = ip + 5 * ub;
  st.row_enc = ip + 6 * ub; st.row_pred = st.row_enc + um;
  int* pidx = st.row_pred + um;
  st.n_active = pidx + up64((size_t)M * ncb); st.steps = st.n_active + 1;
  st.tokens = m->tr_tok.as<int>(); st.max_tok = max_tok;
  st.off = m->d_off.as<int>(); st.len = m->d_len.as<int>();

  // ---- once per batch: enc_proj = joint.enc_ffn(encoder_out), zero LSTM state -----------------
  {
    // always the fp32 GEMMs, whatever the handle's operand precision
    const int saved = t_gemm_prec;
    t_gemm_prec = PREC_F32;
    const int r = rows > 0 ? linear(W.j_enc, m->enc.as<float>(), d, enc_proj, J, rows, s) : 0;
    t_gemm_prec = saved;
    WN_TRY(r);
  }
  WN_HIP(hipMemsetAsync(h, 0, 2 * n_state * sizeof(float), s));
  WN_TRY(rnnt_init(st, B, F, blank, s));

  // ---- the lock-step loop: groups of steps, n_active looked at one group late -----------------
  const int64_t bound = (int64_t)longest * ((int64_t)n_steps + 1) + 1;
  volatile int* pin = reinterpret_cast<volatile int*>(m->tr_host.p);   // slots 0 / 1 (64 B apart)
  int64_t issued = 0;
  for (int g = 0; issued < bound; ++g) {
    const int n = (int)std::min<int64_t>(RNNT_GROUP, bound - issued);
    for (int i = 0; i < n; ++i) {
      WN_TRY(predictor_step(W.pred_embed, E, st.last_tok, E, W.pred_rnn.data(), L, W.pred_proj, h,
                            cst, gates, pout, st.advance, st.n_active, B, H, s));
      RnntLinearArgs q;   // joint.pred_ffn
      q.x1 = pout; q.ldx1 = P; q.K1 = P; q.W1 = W.j_pred.w; q.b1 = W.j_pred.b;
      q.y = pproj; q.ldy = J; q.N = J; q.B = B;
      q.advance = st.advance; q.n_active = st.n_active;
      WN_TRY(rnnt_linear(q, s));
      RnntJointArgs ja;
      ja.enc_proj = enc_proj; ja.lde = J; ja.pred_proj = pproj; ja.ldp = J;
      ja.row_enc = st.row_enc; ja.row_pred = st.row_pred;
      ja.W = W.j_out.w; ja.bias = W.j_out.b; ja.M = M; ja.J = J; ja.V = V;
      ja.part_max = pmax; ja.part_idx = pidx; ja.n_active = st.n_active;
      WN_TRY(rnnt_joint_argmax(ja, s));
      WN_TRY(rnnt_advance(pmax, pidx, ncb, V, st, B, F, blank, n_steps, s));
    }
    issued += n;
    WN_HIP(hipMemcpyAsync(m->tr_host.p + 64 * (g & 1), st.n_active, sizeof(int),
                          hipMemcpyDeviceToHost, s));
    WN_HIP(hipEventRecord(m->tr_ev[g & 1], s));
    if (g >= 1) {
      WN_HIP(hipEventSynchronize(m->tr_ev[(g - 1) & 1]));
      if (pin[16 * ((g - 1) & 1)] == 0) break;
    }
  }

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
                        gates.as<float>(), out_dev, advance_dev, nullptr, B, H, s);
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

}  // extern "C"
