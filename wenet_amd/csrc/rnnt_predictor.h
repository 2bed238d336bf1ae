// The predictor step of the RNN-T searches on the host side, shared by cabi_transducer.hip (the
// one-shot greedy and beam searches, wn_op_lstm_step), cabi_transducer_stream.hip and
// cabi_transducer_beam_stream.hip (the resumable greedy and beam searches): the launches of one LSTM time step + projection for the advancing
// rows of a batch.
#pragma once
#include "model_state.h"

namespace wn {

constexpr int RNNT_GROUP = 8;     // steps issued between two looks at n_active

// one predictor step for the advancing rows: LSTM layers in place on h / c [L][B][H], then the
// projection into out [B][P] (proj.w == nullptr: none)
inline int predictor_step(const float* x, int ldx, const int* x_rows, int E,
                          const ModelData::LstmLayer* layers, int L, const Linear& proj, float* h,
                          float* c, float* gates, float* out, const int* advance,
                          const int* n_active, int B, int H, hipStream_t s) {
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

// Where the window of a stateless predictor's row comes from: explicit ids [M][C], or the tail
// of a token row the search keeps (kernels.h, RnntStatelessArgs).
struct StatelessWindow {
  const int* ctx = nullptr;
  const int* tokens = nullptr; int ld_tok = 0;
  const int* tok_len = nullptr; const int* tok_row = nullptr;
};

// One advance of a stateless handle's predictor for the advancing rows, joint.pred_ffn included:
// pred_proj [M][J] in one launch (the LSTM route: predictor_step + the joint.pred_ffn launch).
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

inline size_t up64(size_t n) { return (n + 63) / 64 * 64; }

}  // namespace wn
