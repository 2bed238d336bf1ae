// C ABI (include/wenet_amd.h), hybrid transducer: the teacher-forced transducer score of host
// n-bests over the handle's current batch (kernels: transducer_score.hip, trie: rnnt_trie.h) and
// the operator hooks of the trie, the joint log-prob gather and the lattice.
#include <algorithm>

#include "model_state.h"
#include "rnnt_host.h"
#include "rnnt_trie.h"

namespace wn {
namespace {

constexpr int TS_MAX_BEAM = 16;
constexpr int TS_MAX_LEN = 4095;      // rnnt_lattice: two alpha columns of U + 1 doubles in LDS

// sections of one int32 upload, each starting at a multiple of 64 entries
struct IntPack {
  std::vector<int> host;
  size_t add(size_t n) {
    const size_t o = host.size();
    host.resize(o + up64(std::max<size_t>(n, 1)), 0);
    return o;
  }
};

int ts_check_hyps(const char* who, int n, int beam, const int32_t* lens, const int32_t* tokens,
                  int max_len, int V) {
  WN_CHECK(n >= 1 && n <= beam, std::string(who) + ": n_hyps outside [1, beam]");
  for (int k = 0; k < n; ++k) {
    WN_CHECK(lens[k] >= 0 && lens[k] <= max_len,
             std::string(who) + ": a hypothesis length outside [0, max_len]");
    for (int j = 0; j < lens[k]; ++j) {
      const int v = tokens[(size_t)k * max_len + j];
      WN_CHECK(v >= 0 && v < V, std::string(who) + ": a token outside the vocabulary");
    }
  }
  return 0;
}

}  // namespace
}  // namespace wn

extern "C" {

int wn_transducer_score(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
                        const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
                        int32_t max_len, double* td_scores_host, void* stream) {
  WN_CHECK(m, "wn_transducer_score: null handle");
  WN_CHECK(m->tr.on && m->data->j_out.w,
           "wn_transducer_score: this model has no transducer weights (predictor / joint); it "
           "was not built by wn_model_create_transducer");
  WN_ENTER(m);
  WN_CHECK(m->B > 0 && m->enc.p,
           "wn_transducer_score: no current batch (call wn_encode / wn_set_encoder_out)");
  WN_CHECK(n_hyps_host && hyp_lens_host && hyp_tokens_host && td_scores_host,
           "wn_transducer_score: null argument");
  WN_CHECK(beam >= 1 && beam <= TS_MAX_BEAM, "wn_transducer_score: beam must be in [1, 16]");
  WN_CHECK(max_len >= 0 && max_len <= TS_MAX_LEN,
           "wn_transducer_score: max_len must be in [0, 4095]");
  const wn_config& c = m->cfg;
  const ModelData& W = *m->data;
  const wn_transducer_config& tc = m->tr.c;
  const int B = m->B, rows = m->rows, V = c.vocab;
  const int E = tc.pred_embed, H = tc.pred_hidden, L = tc.pred_layers, P = tc.pred_out;
  const int J = tc.join_dim, blank = tc.blank;
  for (int b = 0; b < B; ++b)
    WN_TRY(ts_check_hyps("wn_transducer_score", n_hyps_host[b], beam,
                         hyp_lens_host + (size_t)b * beam,
                         hyp_tokens_host + (size_t)b * beam * max_len, max_len, V));
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));

  // ---- host: one trie per utterance with frames, global node ids by depth ----------------------
  std::vector<RnntTrie> tries(B);
  int depth_max = 0;
  int64_t M64 = 0, ent64 = 0, unshared = 0;
  for (int b = 0; b < B; ++b) {
    if (m->len[b] <= 0) continue;
    rnnt_trie_build(hyp_tokens_host + (size_t)b * beam * max_len, hyp_lens_host + (size_t)b * beam,
                    n_hyps_host[b], max_len, blank, tries[b]);
    depth_max = std::max(depth_max, tries[b].depth.back());
    M64 += (int64_t)m->len[b] * tries[b].nodes();
    ent64 += (int64_t)m->len[b] * (int64_t)tries[b].cols.size();
    for (int k = 0; k < n_hyps_host[b]; ++k)
      unshared += (int64_t)m->len[b] * (hyp_lens_host[(size_t)b * beam + k] + 1);
  }
  const int NH = B * beam;
  m->tr_score_rows = M64;
  m->tr_score_unshared = unshared;
  m->tr_score_nodes = 0;
  if (M64 == 0) {       // nothing but utterances of zero frames
    std::fill(td_scores_host, td_scores_host + NH, -INFINITY);
    return 0;
  }
  WN_CHECK(ent64 <= ((int64_t)1 << 28),
           "wn_transducer_score: frames x trie nodes do not fit the workspace");
  const int M = (int)M64, n_ent = (int)ent64;
  std::vector<int> lvl_off(depth_max + 2, 0);
  std::vector<std::vector<int>> gid(B);       // global id of (utterance, node)
  int n_tot = 0;
  {
    std::vector<size_t> at(B, 0);
    for (int dd = 0; dd <= depth_max; ++dd) {
      lvl_off[dd] = n_tot;
      for (int b = 0; b < B; ++b) {
        const RnntTrie& t = tries[b];
        if (dd == 0) gid[b].resize(t.parent.size());
        while (at[b] < t.parent.size() && t.depth[at[b]] == dd) gid[b][at[b]++] = n_tot++;
      }
    }
    lvl_off[depth_max + 1] = n_tot;
  }
  m->tr_score_nodes = n_tot;

  IntPack ip;
  const size_t o_par = ip.add(n_tot), o_tok = ip.add(n_tot), o_renc = ip.add(M),
               o_rpred = ip.add(M), o_coff = ip.add((size_t)M + 1), o_cols = ip.add(n_ent),
               o_erow = ip.add(n_ent), o_T = ip.add(NH), o_U = ip.add(NH), o_str = ip.add(NH),
               o_uoff = ip.add(NH), o_base = ip.add(2 * (size_t)NH);
  // (only the validated entries are read: those of hypotheses k < n_hyps[b]; what a caller
  // leaves beyond them, as wn_rescore allows, is never looked at)
  size_t n_u = 0;
  for (int b = 0; b < B; ++b)
    if (m->len[b] > 0)
      for (int k = 0; k < n_hyps_host[b]; ++k) n_u += (size_t)hyp_lens_host[(size_t)b * beam + k] + 1;
  const size_t o_ub = ip.add(n_u), o_ul = ip.add(n_u);
  // a stateless predictor: the window of every node, (nodes, C), next to the trie
  const bool stateless = m->tr.sp.kind != 0;
  const int C = m->tr.sp.context;
  const size_t o_ctx = stateless ? ip.add((size_t)n_tot * C) : 0;
  std::vector<int>& hi = ip.host;
  std::vector<int64_t> base(NH, 0);
  int max_u = 0;
  {
    int row = 0, ent = 0, u_at = 0;
    for (int b = 0; b < B; ++b) {
      const RnntTrie& t = tries[b];
      const int Tb = m->len[b], Nb = t.nodes(), Eb = (int)t.cols.size();
      for (int i = 0; i < Nb; ++i) {
        hi[o_par + gid[b][i]] = t.parent[i] < 0 ? -1 : gid[b][t.parent[i]];
        hi[o_tok + gid[b][i]] = t.token[i];
      }
      if (stateless && Nb > 0) {
        std::vector<int> ctx((size_t)Nb * C);
        rnnt_trie_context(t, C, ctx.data());
        for (int i = 0; i < Nb; ++i)
          std::copy(ctx.begin() + (size_t)i * C, ctx.begin() + (size_t)(i + 1) * C,
                    hi.begin() + o_ctx + (size_t)gid[b][i] * C);
      }
      const int ent_base = ent;
      for (int f = 0; f < Tb; ++f)
        for (int i = 0; i < Nb; ++i, ++row) {
          hi[o_renc + row] = m->off[b] + f;
          hi[o_rpred + row] = gid[b][i];
          hi[o_coff + row] = ent;
          for (int e = t.col_off[i]; e < t.col_off[i + 1]; ++e, ++ent) {
            hi[o_cols + ent] = t.cols[e];
            hi[o_erow + ent] = row;
          }
        }
      for (int k = 0; k < beam; ++k) {
        const int g = b * beam + k;
        const bool live = Tb > 0 && k < n_hyps_host[b];
        hi[o_T + g] = live ? Tb : 0;
        hi[o_U + g] = live ? hyp_lens_host[g] : 0;
        hi[o_str + g] = Eb;
        hi[o_uoff + g] = u_at;
        base[g] = ent_base;
        if (!live) continue;
        const int U = hyp_lens_host[g];
        max_u = std::max(max_u, U);
        const int* path = t.path.data() + t.path_off[k];
        for (int u = 0; u <= U; ++u) {
          hi[o_ub + u_at + u] = t.col_off[path[u]];
          hi[o_ul + u_at + u] = u < U ? t.col_off[path[u]] + t.slot[path[u + 1]] : 0;
        }
        u_at += U + 1;
      }
    }
    hi[o_coff + M] = ent;
    memcpy(&hi[o_base], base.data(), (size_t)NH * sizeof(int64_t));
    WN_CHECK(row == M && ent == n_ent, "wn_transducer_score: row bookkeeping");
  }

  // ---- workspace ---------------------------------------------------------------------------------
  int n_lvl_max = 0;
  for (int dd = 0; dd <= depth_max; ++dd) n_lvl_max = std::max(n_lvl_max, lvl_off[dd + 1] - lvl_off[dd]);
  WN_TRY(m->tr_enc.ensure((size_t)std::max(rows, 1) * J * sizeof(float)));
  const size_t n_state = up64((size_t)L * n_tot * H);
  const size_t o_score = 0, o_h = up64(2 * (size_t)NH), o_c = o_h + n_state,
               o_gates = o_c + n_state, o_pout = o_gates + up64((size_t)n_lvl_max * 4 * H),
               o_pproj = o_pout + up64((size_t)n_tot * P),
               n_f32 = o_pproj + up64((size_t)n_tot * J);
  WN_TRY(m->tr_sc_f32.ensure(n_f32 * sizeof(float)));
  WN_TRY(m->tr_sc_i32.ensure(hi.size() * sizeof(int)));
  WN_TRY(m->tr_sc_logp.ensure((size_t)n_ent * sizeof(float)));
  WN_TRY(m->tr_host.ensure((size_t)NH * sizeof(double) + 64));
  float* f = m->tr_sc_f32.as<float>();
  int* di = m->tr_sc_i32.as<int>();
  float* enc_proj = m->tr_enc.as<float>();
  float *h = f + o_h, *cst = f + o_c, *gates = f + o_gates, *pout = f + o_pout,
        *pproj = f + o_pproj, *logp = m->tr_sc_logp.as<float>();
  double* score = reinterpret_cast<double*>(f + o_score);
  WN_HIP(hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, s));
  // stage marks for wn_transducer_score_times, under wn_profile_enable only
  const bool marks = m->prof_on;
  auto mark = [&](int i) { return marks ? hipEventRecord(m->tr_sc_ev[i], s) : hipSuccess; };
  if (marks)
    for (hipEvent_t& e : m->tr_sc_ev)
      if (!e) WN_HIP(hipEventCreate(&e));
  WN_HIP(mark(0));

  // ---- enc_proj = joint.enc_ffn(encoder_out), always the fp32 GEMM -------------------------------
  WN_TRY(rnnt_prepare(m, m->enc.as<float>(), rows, enc_proj, s));

  WN_HIP(mark(1));

  // ---- the predictor over the trie, depth by depth: a node starts from its parent's state --------
  if (n_state > 0) WN_HIP(hipMemsetAsync(h, 0, 2 * n_state * sizeof(float), s));
  const int64_t lstride = (int64_t)n_tot * H;
  if (stateless) {    // every node at once: its output is a function of its window alone
    StatelessWindow sw;
    sw.ctx = di + o_ctx;
    WN_TRY(stateless_step(m, sw, pproj, nullptr, nullptr, n_tot, s));
  }
  for (int dd = 0; !stateless && dd <= depth_max; ++dd) {
    const int r0 = lvl_off[dd], n = lvl_off[dd + 1] - r0;
    if (n <= 0) continue;
    if (dd > 0) WN_TRY(rnnt_trie_gather(di + o_par, h, cst, r0, n, L, lstride, H, s));
    // the LSTM layers on the depth's rows of the [L][n_tot][H] state, no projection yet
    WN_TRY(predictor_step(W.pred_embed, E, di + o_tok + r0, E, W.pred_rnn.data(), L, Linear(),
                          h + (size_t)r0 * H, cst + (size_t)r0 * H, lstride, gates, nullptr,
                          nullptr, nullptr, n, H, s));
  }
  const float* top = h + (L - 1) * lstride;
  int ld_top = H, k_top = H;
  if (!stateless && W.pred_proj.w) {
    RnntLinearArgs g;
    g.x1 = top; g.ldx1 = H; g.K1 = H; g.W1 = W.pred_proj.w; g.b1 = W.pred_proj.b;
    g.y = pout; g.ldy = P; g.N = P; g.B = n_tot;
    WN_TRY(rnnt_linear(g, s));
    top = pout; ld_top = P; k_top = P;
  }
  if (!stateless) {
    RnntLinearArgs q;   // joint.pred_ffn
    q.x1 = top; q.ldx1 = ld_top; q.K1 = k_top; q.W1 = W.j_pred.w; q.b1 = W.j_pred.b;
    q.y = pproj; q.ldy = J; q.N = J; q.B = n_tot;
    WN_TRY(rnnt_linear(q, s));
  }

  WN_HIP(mark(2));

  // ---- log-probs at the listed columns of every (frame, node), then the lattices ------------------
  RnntGatherArgs ga;
  ga.enc_proj = enc_proj; ga.lde = J; ga.pred_proj = pproj; ga.ldp = J;
  ga.row_enc = di + o_renc; ga.row_pred = di + o_rpred;
  ga.W = W.j_out.w; ga.bias = W.j_out.b; ga.M = M; ga.J = J; ga.V = V;
  ga.col_off = di + o_coff; ga.cols = di + o_cols; ga.ent_row = di + o_erow; ga.logp = logp;
  WN_TRY(rnnt_joint_logp_gather(ga, s));
  WN_HIP(mark(3));
  RnntLatticeArgs la;
  la.blank = logp; la.label = logp; la.T = di + o_T; la.U = di + o_U;
  la.blank_base = la.label_base = reinterpret_cast<const int64_t*>(di + o_base);
  la.blank_stride = la.label_stride = di + o_str;
  la.u_off = di + o_uoff; la.ub = di + o_ub; la.ul = di + o_ul;
  la.score = score; la.N = NH; la.max_U = max_u;
  WN_TRY(rnnt_lattice(la, s));
  WN_HIP(mark(4));
  WN_HIP(hipMemcpyAsync(m->tr_host.p, score, (size_t)NH * sizeof(double), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  for (int i = 0; i < 4; ++i) {
    m->tr_score_ms[i] = 0.f;
    if (marks) WN_HIP(hipEventElapsedTime(&m->tr_score_ms[i], m->tr_sc_ev[i], m->tr_sc_ev[i + 1]));
  }
  const double* sc = reinterpret_cast<const double*>(m->tr_host.p);
  std::copy(sc, sc + NH, td_scores_host);
  return 0;
}

int wn_transducer_score_stats(wn_model* m, int64_t* rows_out, int64_t* rows_unshared_out,
                              int32_t* nodes_out) {
  WN_CHECK(m, "wn_transducer_score_stats: null handle");
  if (rows_out) *rows_out = m->tr_score_rows;
  if (rows_unshared_out) *rows_unshared_out = m->tr_score_unshared;
  if (nodes_out) *nodes_out = m->tr_score_nodes;
  return 0;
}

int wn_transducer_score_times(wn_model* m, float* ms_out) {
  WN_CHECK(m && ms_out, "wn_transducer_score_times: null argument");
  std::copy(m->tr_score_ms, m->tr_score_ms + 4, ms_out);
  return 0;
}

int wn_op_rnnt_trie(int32_t n_hyps, const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
                    int32_t max_len, int32_t blank, int32_t* n_nodes_out, int32_t* parent_out,
                    int32_t* token_out, int32_t* depth_out, int32_t* path_out,
                    int32_t* col_off_out, int32_t* cols_out) {
  WN_CHECK(hyp_lens_host && hyp_tokens_host && n_nodes_out && parent_out && token_out &&
           depth_out && path_out && col_off_out && cols_out, "wn_op_rnnt_trie: null argument");
  WN_CHECK(max_len >= 0 && max_len <= wn::TS_MAX_LEN, "wn_op_rnnt_trie: max_len must be in [0, 4095]");
  WN_CHECK(blank >= 0, "wn_op_rnnt_trie: negative blank");
  WN_TRY(wn::ts_check_hyps("wn_op_rnnt_trie", n_hyps, wn::TS_MAX_BEAM, hyp_lens_host,
                           hyp_tokens_host, max_len, INT32_MAX));
  wn::RnntTrie t;
  wn::rnnt_trie_build(hyp_tokens_host, hyp_lens_host, n_hyps, max_len, blank, t);
  const int N = t.nodes();
  *n_nodes_out = N;
  std::copy(t.parent.begin(), t.parent.end(), parent_out);
  std::copy(t.token.begin(), t.token.end(), token_out);
  std::copy(t.depth.begin(), t.depth.end(), depth_out);
  std::copy(t.col_off.begin(), t.col_off.end(), col_off_out);
  std::copy(t.cols.begin(), t.cols.end(), cols_out);
  std::fill(path_out, path_out + (size_t)n_hyps * (max_len + 1), -1);
  for (int k = 0; k < n_hyps; ++k)
    std::copy(t.path.begin() + t.path_off[k], t.path.begin() + t.path_off[k + 1],
              path_out + (size_t)k * (max_len + 1));
  return 0;
}

int wn_op_joint_logp_gather(const float* enc_proj_dev, int32_t enc_rows,
                            const float* pred_proj_dev, int32_t pred_rows,
                            const int32_t* row_enc_host, const int32_t* row_pred_host,
                            const float* w_dev, const float* bias_dev, int32_t M, int32_t J,
                            int32_t V, const int32_t* col_off_host, const int32_t* cols_host,
                            float* logp_host, void* stream) {
  WN_CHECK(enc_proj_dev && pred_proj_dev && row_enc_host && row_pred_host && w_dev && bias_dev &&
           col_off_host && cols_host && logp_host, "wn_op_joint_logp_gather: null argument");
  WN_CHECK(M >= 1 && V >= 1 && enc_rows >= 1 && pred_rows >= 1, "wn_op_joint_logp_gather: empty");
  WN_CHECK(M <= (1 << 24), "wn_op_joint_logp_gather: too many rows");
  WN_CHECK(col_off_host[0] == 0, "wn_op_joint_logp_gather: col_off must start at 0");
  for (int i = 0; i < M; ++i) {
    WN_CHECK(row_enc_host[i] < enc_rows && row_pred_host[i] >= 0 && row_pred_host[i] < pred_rows,
             "wn_op_joint_logp_gather: row map outside its matrix");
    const int n = col_off_host[i + 1] - col_off_host[i];
    WN_CHECK(n >= 0 && n <= 17, "wn_op_joint_logp_gather: a column list of more than 17 entries");
    for (int e = col_off_host[i]; e < col_off_host[i + 1]; ++e)
      WN_CHECK(cols_host[e] >= 0 && cols_host[e] < V,
               "wn_op_joint_logp_gather: a column outside the vocabulary");
  }
  const int n_ent = col_off_host[M];
  if (n_ent == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> ent_row(n_ent);
  for (int i = 0; i < M; ++i)
    for (int e = col_off_host[i]; e < col_off_host[i + 1]; ++e) ent_row[e] = i;
  static thread_local wn::DevBuf ibuf, obuf;
  const size_t um = wn::up64((size_t)M + 1), ue = wn::up64(n_ent);
  WN_TRY(ibuf.ensure((3 * um + 2 * ue) * sizeof(int)));
  WN_TRY(obuf.ensure((size_t)n_ent * sizeof(float)));
  int* ip = ibuf.as<int>();
  auto up = [&](int* dst, const int* src, size_t n) {
    return hipMemcpyAsync(dst, src, n * sizeof(int), hipMemcpyHostToDevice, s);
  };
  WN_HIP(up(ip, row_enc_host, M));
  WN_HIP(up(ip + um, row_pred_host, M));
  WN_HIP(up(ip + 2 * um, col_off_host, (size_t)M + 1));
  WN_HIP(up(ip + 3 * um, cols_host, n_ent));
  WN_HIP(up(ip + 3 * um + ue, ent_row.data(), n_ent));
  WN_HIP(hipMemsetAsync(obuf.p, 0xff, (size_t)n_ent * sizeof(float), s));   // NaN: not written
  wn::RnntGatherArgs ga;
  ga.enc_proj = enc_proj_dev; ga.lde = J; ga.pred_proj = pred_proj_dev; ga.ldp = J;
  ga.row_enc = ip; ga.row_pred = ip + um; ga.W = w_dev; ga.bias = bias_dev;
  ga.M = M; ga.J = J; ga.V = V;
  ga.col_off = ip + 2 * um; ga.cols = ip + 3 * um; ga.ent_row = ip + 3 * um + ue;
  ga.logp = obuf.as<float>();
  WN_TRY(wn::rnnt_joint_logp_gather(ga, s));
  WN_HIP(hipMemcpyAsync(logp_host, obuf.p, (size_t)n_ent * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_rnnt_lattice(int32_t N, const int32_t* T_host, const int32_t* U_host,
                       const float* lp_blank_host, const float* lp_label_host,
                       double* scores_host, void* stream) {
  WN_CHECK(T_host && U_host && lp_blank_host && lp_label_host && scores_host,
           "wn_op_rnnt_lattice: null argument");
  WN_CHECK(N >= 1 && N <= (1 << 20), "wn_op_rnnt_lattice: N must be in [1, 2^20]");
  int64_t nb = 0, nl = 0, nu = 0;
  int max_u = 0;
  for (int n = 0; n < N; ++n) {
    WN_CHECK(T_host[n] >= 0 && U_host[n] >= 0 && U_host[n] <= wn::TS_MAX_LEN,
             "wn_op_rnnt_lattice: T must be >= 0 and U in [0, 4095]");
    nb += (int64_t)T_host[n] * (U_host[n] + 1);
    nl += (int64_t)T_host[n] * U_host[n];
    nu += U_host[n] + 1;
    max_u = std::max(max_u, U_host[n]);
  }
  WN_CHECK(nb <= ((int64_t)1 << 28), "wn_op_rnnt_lattice: the lattices are too large");
  hipStream_t s = (hipStream_t)stream;
  wn::IntPack ip;
  const size_t o_T = ip.add(N), o_U = ip.add(N), o_sb = ip.add(N), o_sl = ip.add(N),
               o_uoff = ip.add(N), o_bb = ip.add(2 * (size_t)N), o_lb = ip.add(2 * (size_t)N),
               o_u = ip.add(nu);
  std::vector<int64_t> bb(N), lb(N);
  int64_t ab = 0, al = 0;
  int au = 0;
  for (int n = 0; n < N; ++n) {
    const int U = U_host[n];
    ip.host[o_T + n] = T_host[n]; ip.host[o_U + n] = U;
    ip.host[o_sb + n] = U + 1; ip.host[o_sl + n] = U;
    ip.host[o_uoff + n] = au;
    bb[n] = ab; lb[n] = al;
    for (int u = 0; u <= U; ++u) ip.host[o_u + au + u] = u;
    au += U + 1;
    ab += (int64_t)T_host[n] * (U + 1);
    al += (int64_t)T_host[n] * U;
  }
  memcpy(&ip.host[o_bb], bb.data(), (size_t)N * sizeof(int64_t));
  memcpy(&ip.host[o_lb], lb.data(), (size_t)N * sizeof(int64_t));
  static thread_local wn::DevBuf ibuf, fbuf;
  const size_t ub = wn::up64(std::max<int64_t>(nb, 1)), ul = wn::up64(std::max<int64_t>(nl, 1));
  WN_TRY(ibuf.ensure(ip.host.size() * sizeof(int)));
  WN_TRY(fbuf.ensure((ub + ul) * sizeof(float) + (size_t)N * sizeof(double)));
  int* di = ibuf.as<int>();
  double* score = fbuf.as<double>();
  float* eb = reinterpret_cast<float*>(score + N);
  float* el = eb + ub;
  WN_HIP(hipMemcpyAsync(di, ip.host.data(), ip.host.size() * sizeof(int), hipMemcpyHostToDevice, s));
  if (nb > 0)
    WN_HIP(hipMemcpyAsync(eb, lp_blank_host, (size_t)nb * sizeof(float), hipMemcpyHostToDevice, s));
  if (nl > 0)
    WN_HIP(hipMemcpyAsync(el, lp_label_host, (size_t)nl * sizeof(float), hipMemcpyHostToDevice, s));
  wn::RnntLatticeArgs la;
  la.blank = eb; la.label = el; la.T = di + o_T; la.U = di + o_U;
  la.blank_base = reinterpret_cast<const int64_t*>(di + o_bb);
  la.label_base = reinterpret_cast<const int64_t*>(di + o_lb);
  la.blank_stride = di + o_sb; la.label_stride = di + o_sl;
  la.u_off = di + o_uoff; la.ub = di + o_u; la.ul = di + o_u;
  la.score = score; la.N = N; la.max_U = max_u;
  WN_TRY(wn::rnnt_lattice(la, s));
  WN_HIP(hipMemcpyAsync(scores_host, score, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
