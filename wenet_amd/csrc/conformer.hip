// The Conformer layer stack of libwenet_amd: which kernel form every launch of a layer takes
// (feed-forward modules: fused / six-product pair / v_mfma_f32 / MXFP8; projections: row-block
// six-product kernels / row-LN GEMM / linear()), for whole utterances (encoder_layers) and for
// one chunk of streaming sessions (encoder_layers_chunk).  linear(), ln() and the front ends
// that leave x for these layers are model.hip; the state is model_state.h.
#include <algorithm>
#include "model_state.h"

// ---- roofline sample (wn_profile_*) -----------------------------------------------------------
// HIP events around the first kernel of a feed-forward module (the kernel the roofline is quoted
// on).  Every hipEventRecord pair costs ~10 us of idle GPU around the launch (measured in the
// rocprofv3 trace), so only every prof_stride-th (6th) launch is bracketed: an unbiased sample
// of the average launch duration (4 per 12-layer pass).  Every module comes through begin()
// exactly once, whichever form it runs, and the count is the handle's.
namespace {
struct ProfBracket {
  wn_model* m;
  hipStream_t s;
  bool on = false;
  int record(int which) { WN_HIP(hipEventRecord(m->prof_ev[m->prof_used + which], s)); return 0; }
  int begin() {
    on = m->prof_on && (m->prof_seq++ % m->prof_stride) == 0;
    if (!on) return 0;
    if (m->prof_used + 2 > m->prof_ev.size())
      for (int i = 0; i < 64; ++i) {
        hipEvent_t e;
        WN_HIP(hipEventCreate(&e));
        m->prof_ev.push_back(e);
      }
    return record(0);
  }
  // `kernel`: what the bracketed launch was (null: leave the name)
  int end(double flops, const char* kernel) {
    if (!on) return 0;
    WN_TRY(record(1));
    m->prof_used += 2;
    m->prof_flops += flops;
    if (kernel) m->prof_kernel = kernel;
    return 0;
  }
};
}  // namespace

// FFN w_1 GEMM (SiLU epilogue), optionally bracketed by HIP events
static int ffn_w1(wn_model* m, const Linear& l, const float* A, float* C, int M, hipStream_t s,
                  int act, bool h16) {
  ProfBracket pb{m, s};
  WN_TRY(pb.begin());
  WN_TRY(linear(l, A, l.in, C, l.out, M, s, act, nullptr, 0, 1.0f, false, h16, h16));
  // (the bracket also holds the plane-split pass of A when linear() took the six-product route)
  return pb.end(2.0 * M * (double)l.out * l.in,
                t_linear_took_x6
                    ? "x6_split + gemm_x6_kernel (FFN w_1 + act through linear(), six bf16 plane products)"
                    : "gemm (FFN w_1)");
}

// x += alpha * w_2(act(w_1(LN(x)))) -- one feed-forward module
// (positionwise_feed_forward.py:50-58 inside encoder_layer.py:220-228 / :253-261 /
// encoder_layer.py:117-125).  `ln_done`: t1 already holds LN(x) (fused earlier).
// fp8 mode (WN_PREC_FP8) and shapes the pipelined kernel takes: the LayerNorm writes
// MXFP8, w_1 reads it and writes the hidden tensor as MXFP8 again (block scales from
// its epilogue), w_2 reads that and adds into the fp32 residual stream.
int ffn_module(wn_model* m, const Norm& nrm, const Linear& w1, const Linear& w2, int act,
               float alpha, bool ln_done, bool h16, hipStream_t s) {
  const wn_config& c = m->cfg;
  const int d = c.d_model, M = m->rows;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* hb = m->hbuf.as<float>();
  bool mx = false;
  const ModelData::MxW *q1 = nullptr, *q2 = nullptr;
  if (t_mx && h16 && !ln_done) {
    auto i1 = t_mx->find(w1.w), i2 = t_mx->find(w2.w);
    const int64_t t256 = (int64_t)cdiv(M, 256) * cdiv(std::min(w1.out, w2.out), 256);
    GemmArgs p1, p2;      // the two launches as gemm_mxfp8 will see them: supported shapes only
    p1.M = p2.M = M; p1.N = w1.out; p1.K = d; p1.lda = d; p1.ldc = w1.out;
    p1.fp8 = p2.fp8 = true; p1.c_mx = true;
    p2.N = d; p2.K = w1.out; p2.lda = w1.out; p2.ldc = d; p2.resid = x; p2.ldr = d;
    if (i1 != t_mx->end() && i2 != t_mx->end() && d % 256 == 0 && w1.out % 128 == 0 &&
        t256 >= tune().fp8_min_tiles && gemm_bf16p_supported(p1) && gemm_bf16p_supported(p2)) {
      mx = true; q1 = &i1->second; q2 = &i2->second;
    }
  }
  if (!mx) {
    if (!ln_done) WN_TRY(ln(nrm, x, t1, M, d, c.norm_eps, s, h16));
    WN_TRY(ffn_w1(m, w1, t1, hb, M, s, act, h16));
    return linear(w2, hb, w1.out, x, d, M, s, ACT_NONE, x, d, alpha, false, h16);
  }
  const int pitch = cdiv(M, 256) * 256;
  WN_TRY(m->mx_sa.ensure((size_t)(d / 128) * pitch * 4));
  WN_TRY(m->mx_sh.ensure((size_t)(w1.out / 128) * pitch * 4));
  WN_TRY(layernorm_mx(x, d, nrm.w, nrm.b, t1, m->mx_sa.as<unsigned>(), pitch, M, d,
                      c.norm_eps, s));
  GemmArgs g;
  g.A = t1; g.bias = w1.b; g.C = hb; g.M = M; g.N = w1.out; g.K = d;
  g.lda = d; g.ldc = w1.out; g.act = act; g.fp8 = true; g.c_mx = true;
  g.a_scale = m->mx_sa.as<unsigned>(); g.a_scale_pitch = pitch;
  g.w_scale = q1->scale; g.w_scale_pitch = w1.out;
  g.c_scale = m->mx_sh.as<unsigned>(); g.c_scale_pitch = pitch;
  ProfBracket pb{m, s};
  WN_TRY(pb.begin());
  WN_TRY(gemm_mxfp8(g, q1->q, s));
  WN_TRY(pb.end(2.0 * M * (double)w1.out * d, nullptr));
  GemmArgs h;
  h.A = hb; h.bias = w2.b; h.C = x; h.resid = x; h.M = M; h.N = d; h.K = w1.out;
  h.lda = w1.out; h.ldc = d; h.ldr = d; h.alpha = alpha; h.fp8 = true;
  h.a_scale = m->mx_sh.as<unsigned>(); h.a_scale_pitch = pitch;
  h.w_scale = q2->scale; h.w_scale_pitch = d;
  return gemm_mxfp8(h, q2->q, s);
}

// hidden split of the x6 FFN's second GEMM: K slices so that 128-row tiles x slices fill
// the CUs once
int ffn_x6_split(int M, int F) {
  int S = 1;
  while (S < 16 && cdiv(M, 128) * (S * 2) <= 256 && (F / 16) % (S * 2) == 0) S *= 2;
  return S;
}

// Which form will ffn_x6_try run for this module on the current batch?  0 = none (the caller's
// v_mfma_f32 paths), 1 = the fused kernel (ffn_x6f.hip, d_model 256), 2 = the six-product GEMM
// pair with the hidden tensor as a plane image.  Forms 1 and 2 (without tune().x6_af32) read
// LN(x) as an X3 plane image: the producers of LN(x) ask before they decide to write that image
// instead of fp32 rows (t1_image_for) -- ONE predicate, so producer and consumer cannot disagree.
static int ffn_x6_route(wn_model* m, const Linear& w1, const Linear& w2, int act) {
  const ModelData& W = *m->data;
  const int d = m->cfg.d_model, M = m->rows, F = w1.out;
  if (t_gemm_prec != PREC_F32 || tune().gemm_x6 == 0 || w1.out != w2.in ||
      !(d == 256 || d == 512) || F % 16 != 0)
    return 0;
  // batches under 512 rows: only the fused kernel (the tile-GEMM pair is all prologue and
  // epilogue there; 2 = tests force it)
  const bool small = M < 512 && tune().gemm_x6 != 2;
  const bool fused_ok = tune().ffn_x6f != 0 && tune().x6_af32 == 0 &&
                        ffn_x6f_supported(M, d, F, act) && !(small && tune().ffn_x6f == 3);
  if (W.x6_at.count(w1.w) == 0 || W.x6_at.count(w2.w) == 0) return 0;
  const bool fused = fused_ok && W.x6p_at.count(w2.w) != 0;
  // small batches never take the tile-GEMM pair: the fused kernel or the v_mfma_f32 paths
  if (small) return fused ? 1 : 0;
  return fused ? 1 : 2;
}

// the image buffer of t1 = LN(x) when the next feed-forward module will take it, else null
static void* t1_image_for(wn_model* m, const Linear& w1, const Linear& w2, int act) {
  if (tune().ffn_ximg == 0) return nullptr;
  const int r = ffn_x6_route(m, w1, w2, act);
  if (r == 0 || (r == 2 && tune().x6_af32 != 0)) return nullptr;
  if (m->t1_img.ensure(x6_bytes(m->rows, m->cfg.d_model)) != 0) return nullptr;
  return m->t1_img.p;
}

// fp32 feed-forward module on the bf16 matrix cores (ffn_x6_route): t1 = LN(x) is in place, as
// fp32 rows or (m->t1_img_ok) as its plane image; leaves the hidden-slice / K-slice partials in
// m->ffn_part.  Returns the slice count (0: not taken).
static int ffn_x6_try(wn_model* m, const Linear& w1, const Linear& w2, int act, hipStream_t s) {
  const ModelData& W = *m->data;
  const int d = m->cfg.d_model, M = m->rows, F = w1.out;
  const bool ximg = m->t1_img_ok;      // t1 exists ONLY as its plane image
  m->t1_img_ok = false;
  // (d: the widths ffn_reduce_ln takes)
  const int route = ffn_x6_route(m, w1, w2, act);
  WN_CHECK(route != 0 || !ximg,
           "ffn_x6_try: LN(x) was left as a plane image but no six-product form takes it");
  if (route == 0) return 0;
  auto i1 = W.x6_at.find(w1.w), i2 = W.x6_at.find(w2.w);
  ProfBracket pb{m, s};
  if (route == 1) {
    // hidden tensor on chip (ffn_x6f.hip)
    FfnX6Args a;
    a.S = ffn_x6f_split(M, F);
    if (m->ffn_part.ensure((size_t)a.S * M * d * sizeof(float)) != 0) return -1;
    a.X = m->t1.as<float>(); a.ldx = d; a.W13 = i1->second; a.W2p = W.x6p_at.find(w2.w)->second;
    a.b1 = w1.b;
    if (ximg) { a.X3 = m->t1_img.p; a.X = nullptr; }
    a.P = m->ffn_part.as<float>(); a.M = M; a.D = d; a.F = F; a.act = act;
    WN_TRY(pb.begin());
    if (ffn_x6f(a, s) != 0) return -1;
    // both contractions (x 6 MFMA products)
    WN_TRY(pb.end(4.0 * M * (double)F * d,
                  "ffn_x6f_kernel (FFN w_1 + act + w_2, six bf16 plane products)"));
    m->prof_split = a.S;
    return a.S;
  }
  const int S = ffn_x6_split(M, F);
  if (m->ffn_part.ensure((size_t)S * M * d * sizeof(float)) != 0) return -1;
  // plane images (x6_split of t1, w_1 writes the hidden planes); tune().x6_af32 (A/B knob): the A
  // operands stay plain fp32 (t1, the hidden tensor in hbuf) and are split in registers
  const bool af32 = tune().x6_af32 != 0 && (int64_t)M * F * 4 < ((int64_t)1 << 31);
  X6Args g1;
  g1.B3 = i1->second; g1.M = M; g1.N = F; g1.K = d; g1.bias = w1.b; g1.act = act;
  if (af32) {
    WN_CHECK(!ximg, "ffn_x6_try: LN(x) was left as a plane image, x6_af32 wants fp32 rows");
    if (m->hbuf.ensure((size_t)M * F * sizeof(float)) != 0) return -1;
    g1.A = m->t1.as<float>(); g1.lda = d; g1.a_bytes = (int64_t)M * d * 4;
    g1.epi = 0; g1.C = m->hbuf.as<float>(); g1.ldc = F;
  } else {
    // (ximg: the producer of LN(x) already wrote its plane image, round 5: no x6_split launch)
    if (m->x6_h.ensure(x6_bytes(M, F)) != 0 || (!ximg && m->x6_a.ensure(x6_bytes(M, d)) != 0)) return -1;
    if (!ximg && x6_split(m->t1.as<float>(), M, d, d, m->x6_a.as<char>(), s) != 0) return -1;
    g1.A3 = ximg ? m->t1_img.as<char>() : m->x6_a.as<char>(); g1.epi = 2; g1.C3 = m->x6_h.as<char>();
  }
  WN_TRY(pb.begin());
  if (gemm_x6(g1, s) != 0) return -1;
  // the contraction (x 6 MFMA products)
  WN_TRY(pb.end(2.0 * M * (double)F * d, "gemm_x6_kernel (FFN w_1 + act, six bf16 plane products)"));
  X6Args g2;
  g2.B3 = i2->second; g2.M = M; g2.N = d; g2.K = F;
  g2.epi = 1; g2.ksplit = S; g2.C = m->ffn_part.as<float>();
  if (af32) { g2.A = m->hbuf.as<float>(); g2.lda = F; g2.a_bytes = (int64_t)M * F * 4; }
  else g2.A3 = m->x6_h.as<char>();
  if (gemm_x6(g2, s) != 0) return -1;
  m->prof_split = S;
  return S;
}

// The six-product GEMM pair of a feed-forward module on ANY rows (the decoders' ReLU modules over
// the R hypothesis rows of a rescoring pass, decoder_layer.py:140-147): A = LN(x) [M][d] is split
// into planes, w_1 + activation writes the plane image of the hidden tensor from its epilogue
// (no fp32 hidden tensor, no separate split pass over it: 10 B per hidden element of HBM traffic
// less than linear() + linear()), w_2 leaves K-slice partials in m->ffn_part for ffn_reduce_ln.
// Returns the slice count, 0 if the shape stays on linear(), < 0 on error.
int ffn_x6_pair(wn_model* m, const Linear& w1, const Linear& w2, int act, const float* A, int M,
                hipStream_t s) {
  const ModelData& W = *m->data;
  const int d = w1.in, F = w1.out;
  if (t_gemm_prec != PREC_F32 || tune().gemm_x6 == 0 || tune().x6_linear == 0 ||
      w1.out != w2.in || w2.out != d || !(d == 256 || d == 512) || F % 16 != 0 || M < 512 ||
      2.0 * M * (double)F * d < 1e8 * g_x6_linear_min)
    return 0;
  auto i1 = W.x6_at.find(w1.w), i2 = W.x6_at.find(w2.w);
  if (i1 == W.x6_at.end() || i2 == W.x6_at.end()) return 0;
  const int S = ffn_x6_split(M, F);
  if (m->ffn_part.ensure((size_t)S * M * d * sizeof(float)) != 0 ||
      m->x6_a.ensure(x6_bytes(M, d)) != 0 || m->x6_h.ensure(x6_bytes(M, F)) != 0)
    return -1;
  if (x6_split(A, M, d, d, m->x6_a.as<char>(), s) != 0) return -1;
  X6Args g1;
  g1.A3 = m->x6_a.as<char>(); g1.B3 = i1->second; g1.M = M; g1.N = F; g1.K = d; g1.bias = w1.b;
  g1.act = act; g1.epi = 2; g1.C3 = m->x6_h.as<char>();
  if (gemm_x6(g1, s) != 0) return -1;
  X6Args g2;
  g2.A3 = m->x6_h.as<char>(); g2.B3 = i2->second; g2.M = M; g2.N = d; g2.K = F;
  g2.epi = 1; g2.ksplit = S; g2.C = m->ffn_part.as<float>();
  if (gemm_x6(g2, s) != 0) return -1;
  return S;
}

// fp32 fused feed-forward module (the six-product forms above, else ffn_fused.hip): t1 = LN(x)
// is in place; leaves the hidden-slice partials in m->ffn_part and returns S (0: shape not
// taken, caller runs the two-GEMM path).
static int ffn_fused_try(wn_model* m, const Linear& w1, const Linear& w2, int act, hipStream_t s) {
  const int d = m->cfg.d_model, M = m->rows;
  if (const int s6 = ffn_x6_try(m, w1, w2, act, s)) return s6;
  if (t_gemm_prec != PREC_F32 || tune().ffn_fused == 0 || w1.out != w2.in ||
      !ffn_fused_supported(M, d, w1.out, act))
    return 0;
  FfnArgs a;
  a.X = m->t1.as<float>(); a.W1 = w1.w; a.b1 = w1.b; a.W2 = w2.w;
  a.M = M; a.D = d; a.F = w1.out; a.S = ffn_fused_split(M, d, w1.out); a.act = act;
  if (m->ffn_part.ensure((size_t)a.S * M * d * sizeof(float)) != 0) return -1;
  a.P = m->ffn_part.as<float>();
  ProfBracket pb{m, s};
  WN_TRY(pb.begin());
  if (ffn_fused(a, s) != 0) return -1;
  WN_TRY(pb.end(4.0 * M * (double)w1.out * d, "ffn_fused_kernel (FFN w_1 + act + w_2)"));   // both contractions
  m->prof_split = a.S;
  return a.S;
}

// ---- one Conformer layer on the rows of whole utterances --------------------------------------
namespace {

// What encoder_layers decides once per call, for every layer of the batch.
struct LayerCtx {
  wn_model* m; hipStream_t s;
  int M, d; float eps;
  // bf16-storage mode: the LayerNorm outputs (t1), the FFN hidden (hbuf) and the attention
  // context (t2) hold bf16; the GLU output / depthwise-conv tensors stay fp32 (the depthwise
  // kernel is fp32)
  bool h16;
  bool f32;                      // fp32 operands in fp32 storage: what the fused forms below take
  float *x, *t1, *t2, *qkv;
  int max_len;                   // rows of the longest utterance
  int mask_mode = 0, cs = 0, lc = -1;   // chunk mask (mask.py:126-198, decode-time branches)
  bool rowln;                    // x += l(A) and LN(x) in one v_mfma_f32 launch (gemm_rowln.hip)
  // the same fusion as six bf16 plane products on the row-block kernels (gemm_x6r.hip: A rows
  // in registers, d = 256; gemm_x6r512.hip: A image in LDS, d = 512 -- no v_mfma_f32 row-LN
  // kernel exists at that width)
  bool rowx;
  bool x6r_on;                   // the row-block route is open for this batch (x6r_image)

  LayerCtx(wn_model* m_, int chunk, int left, hipStream_t s_)
      : m(m_), s(s_), M(m_->rows), d(m_->cfg.d_model), eps(m_->cfg.norm_eps),
        h16(bf16_store_active()), f32(!h16 && t_gemm_prec == PREC_F32), x(m_->x.as<float>()),
        t1(m_->t1.as<float>()), t2(m_->t2.as<float>()), qkv(m_->qkv.as<float>()), max_len(0) {
    const wn_config& c = m->cfg;
    for (int b = 0; b < m->B; ++b) max_len = std::max(max_len, m->len[b]);
    if (c.use_dynamic_chunk) {
      if (chunk > 0) { mask_mode = 2; cs = chunk; lc = left; }
    } else if (c.static_chunk_size > 0) {
      mask_mode = 2; cs = c.static_chunk_size; lc = left;
    }
    rowln = f32 && gemm_rowln_supported(M, d, d);
    rowx = rowln || (f32 && d == 512);
    x6r_on = f32 && tune().x6r != 0 && tune().gemm_x6 != 0 && t_x6 && M >= 512;
  }
};

// THE predicate of the row-block route (gemm_x6r.hip / gemm_x6r512.hip): the plane image of l's
// weights iff the launch (M x N, K = l.in, epilogue epi) will run there, else null.  Every
// decision that depends on such a launch -- a prologue folded into it, an operand it alone can
// write -- hangs off the pointer the launch itself takes, so none can be "taken" by a launch
// that then declines.
const void* x6_image(const Linear& l) {   // (callers stand behind c.x6r_on: t_x6 is set)
  auto it = t_x6->find(l.w);
  return it != t_x6->end() ? it->second : nullptr;
}
const void* x6r_image(const LayerCtx& c, const Linear& l, int N, int epi) {
  return c.x6r_on && gemm_x6r_supported(c.M, N, l.in, epi) ? x6_image(l) : nullptr;
}

// x += A l.w^T + l.b; LN(x): the fields the row-LN epilogues of the row-block kernel share
// (epi 1: y = LN(x) to t1; epi 3: LN(x) feeds the chained second GEMM)
X6RArgs x6r_rowln_args(const LayerCtx& c, const Linear& l, const void* w3, const float* A,
                       const Norm& nrm, int epi) {
  X6RArgs g;
  g.A = A; g.lda = c.d; g.K = c.d; g.W3 = w3; g.bias = l.b; g.M = c.M; g.N = c.d; g.epi = epi;
  g.resid = c.x; g.ldr = c.d; g.alpha = 1.0f; g.x_out = c.x; g.ldx = c.d;
  g.ln_w = nrm.w; g.ln_b = nrm.b; g.eps = c.eps; g.y = c.t1; g.ldy = c.d;
  return g;
}

// the same step on the v_mfma_f32 row-LN GEMM (gemm_rowln.hip)
int rowln_gemm(const LayerCtx& c, const Linear& l, const float* A, const Norm& nrm) {
  RowLnArgs g;
  g.A = A; g.lda = c.d; g.W = l.w; g.bias = l.b; g.resid = c.x; g.ldr = c.d;
  g.alpha = 1.0f; g.x_out = c.x; g.ldx = c.d; g.ln_w = nrm.w; g.ln_b = nrm.b;
  g.eps = c.eps; g.y = c.t1; g.ldy = c.d; g.M = c.M; g.N = c.d; g.K = c.d;
  return gemm_rowln(g, c.s);
}

// x += 0.5 * FFN_macaron(LN(x)); t1 = norm_mha(x)      encoder_layer.py:220-230
// (for li > 0 the previous layer's tail already left LN(x) in t1)
// fp32: fused FFN (hidden tensor stays on chip), its partial reduction carries the residual add
// and the NEXT LayerNorm (norm_mha).  `qkv_x6r`: the QKV projection runs on the row-block kernel,
// which can form LN(x + 0.5 FFN) itself from the slice partials (gemm_x6r.hip, PRO) -- no
// ffn_reduce_ln launch, no t1 round trip; then *pro_S is the slice count left for it, else 0.
int macaron_ffn(const LayerCtx& c, const EncLayer& L, int li, bool qkv_x6r, int* pro_S) {
  wn_model* m = c.m;
  *pro_S = 0;
  int fS = 0;
  if (c.f32) {
    if (li == 0 && !m->ln0_done) WN_TRY(ln(L.norm_ff_mac, c.x, c.t1, c.M, c.d, c.eps, c.s));
    m->ln0_done = false;
    fS = ffn_fused_try(m, L.ffm1, L.ffm2, ACT_SILU, c.s);
    if (fS < 0) return -2;
  }
  if (fS > 0) {
    if (qkv_x6r && tune().x6r_pro != 0 && c.d == 256) {   // (d = 512: measured slower)
      *pro_S = fS;
      return 0;
    }
    return ffn_reduce_ln(c.x, m->ffn_part.as<float>(), fS, L.ffm2.b, 0.5f, L.norm_mha.w,
                         L.norm_mha.b, nullptr, nullptr, c.t1, c.M, c.d, c.eps, 0, c.s);
  }
  // (fp8 mode: every feed-forward module normalises for itself -- layernorm_mx writes the
  // MXFP8 operand -- so that ALL of them take the same path; the bf16 / fp32 modes get
  // LN(x) from the previous layer's fused tail)
  WN_TRY(ffn_module(m, L.norm_ff_mac, L.ffm1, L.ffm2, ACT_SILU, 0.5f,
                    (li > 0 && !(t_mx && c.h16)) || c.f32, c.h16, c.s));
  return ln(L.norm_mha, c.x, c.t1, c.M, c.d, c.eps, c.s, c.h16);
}

// t2 = MHA(t1) (the residual add is the out-projection's, conv_module)
// encoder_layer.py:230-238.  `qkv_w6`: the QKV projection's row-block image (x6r_image) or
// null; `pro_S` > 0: it starts from the macaron FFN's slice partials (macaron_ffn).
int self_attention(const LayerCtx& c, const EncLayer& L, const void* qkv_w6, int pro_S) {
  wn_model* m = c.m;
  const ModelData& W = *m->data;
  const int d = c.d, M = c.M, H = m->cfg.n_heads;
  hipStream_t s = c.s;
  // The six-product attention over key tiles aligned to the global 32-row blocks (tune
  // attn_x6_galign): decided HERE, in front of the QKV projection, because with = 2 that
  // projection writes the tile images itself (epi 4) and leaves no K / V rows behind
  const bool ax6 = c.f32 && tune().attn_x6 != 0 && tune().attn_fold == 1 && c.mask_mode == 0 &&
                   M >= 512 && c.max_len >= 128 && L.pos_tab && L.bias_u && L.bias_v;
  const bool ax6_img = ax6 && m->attn_img.ensure(attention_x6_image_bytes(M, m->B, H)) == 0;
  const std::pair<const void*, const float*>* qkv_q = nullptr;
  if (ax6_img && pro_S > 0 && tune().attn_x6_galign == 2) {
    auto it = W.x6q_at.find(L.qkv.w);
    if (it != W.x6q_at.end()) qkv_q = &it->second;
  }
  if (qkv_w6) {
    X6RArgs g;
    g.A = c.t1; g.lda = d; g.K = d; g.W3 = qkv_w6; g.bias = L.qkv.b; g.M = M; g.N = 3 * d;
    g.epi = 0; g.C = c.qkv; g.ldc = 3 * d;
    if (qkv_q) {
      g.epi = 4; g.W3 = qkv_q->first; g.bias = qkv_q->second;
      g.at_img = m->attn_img.p; g.at_P = L.pos_tab; g.at_ldp = d;
      g.at_u = L.bias_u; g.at_v = L.bias_v;
      g.at_row_utt = m->d_row_utt.as<int>(); g.at_off = m->d_off.as<int>();
    }
    if (pro_S > 0) {
      g.pro_P = m->ffn_part.as<float>(); g.pro_S = pro_S; g.pro_b2 = L.ffm2.b; g.pro_alpha = 0.5f;
      g.pro_x = c.x; g.ln_w = L.norm_mha.w; g.ln_b = L.norm_mha.b; g.eps = c.eps;
    }
    WN_TRY(gemm_x6r(g, s));
  } else {
    WN_TRY(linear(L.qkv, c.t1, d, c.qkv, 3 * d, M, s, ACT_NONE, nullptr, 0, 1.0f, false, c.h16));
  }
  AttnArgs a;
  a.Q = c.qkv; a.K = c.qkv + d; a.V = c.qkv + 2 * d;
  a.ldq = a.ldk = a.ldv = 3 * d;
  a.P = L.pos_tab; a.ldp = d; a.bias_u = L.bias_u; a.bias_v = L.bias_v;
  if (c.f32 && tune().attn_fold == 2 && (d == 256 || d == 512) && d == H * 64) {
    // A/B form: the folding as a separate pass (k <- k + p in place, scalars in HBM)
    WN_TRY(m->attn_kbias.ensure((size_t)M * H * sizeof(float)));
    WN_TRY(relpos_fold(c.qkv + d, 3 * d, L.pos_tab, d, L.bias_u, L.bias_v,
                       m->d_row_utt.as<int>(), m->d_off.as<int>(), nullptr,
                       m->attn_kbias.as<float>(), H, M, d, s));
    a.kbias = m->attn_kbias.as<float>();
    a.P = nullptr; a.bias_u = a.bias_v = nullptr;
  } else if (c.f32 && tune().attn_fold != 0) {
    // rel-pos folded into the keys as the attention kernel stages them: ONE score
    // contraction (encoder_kernels.hip, attention_kernel FOLD / relpos_fold_kernel)
    a.fold = true;
  }
  a.O = c.t2; a.ldo = d; a.o_bf16 = c.h16;
  a.q_off = a.kv_off = m->d_off.as<int>();
  a.q_len = a.kv_len = m->d_len.as<int>();
  a.n_seq = m->B; a.n_heads = H; a.max_q_len = c.max_len;
  a.mask_mode = c.mask_mode; a.chunk_size = c.cs; a.left_chunks = c.lc;
  a.scale = 1.0f / sqrtf(64.0f);
  if (ax6_img) {
    a.x6_img = m->attn_img.p; a.x6_img_bytes = m->attn_img.cap; a.x6_rows = M;
    if (tune().attn_x6_galign != 0) {
      a.x6_galign = 1;
      a.row_utt = m->d_row_utt.as<int>();
    }
  } else if (a.fold && tune().attn_x6 != 0 && c.f32 && M >= 512) {
    // (chunk-masked batches with attn_x6 = 2: the sequence-aligned image)
    if (m->attn_img.ensure(attention_x6_image_bytes(M, m->B, H)) == 0) {
      a.x6_img = m->attn_img.p; a.x6_img_bytes = m->attn_img.cap; a.x6_rows = M;
    }
  }
  // the encoder's self attention is dispatched from the batch's block list (set_layout) --
  // both fp32 kernels decode it
  if (c.f32 && tune().attn_x6_order != 0 && m->attn_n_blk > 0) {
    a.blk_tab = m->d_row_utt.as<int>() + m->attn_blk_off;
    a.n_blk = m->attn_n_blk;
  }
  if (!qkv_q) return attention(a, s);
  // the tiles are in the image already and K / V exist nowhere else: this launch MUST be
  // the six-product kernel
  a.x6_img_ready = true;
  WN_CHECK(a.fold && attention_x6_supported(a),
           "encoder: QKV wrote the key-tile images but the six-product attention declines");
  return attention_x6(a, s);
}

// x += out_proj(t2); x += Conv(LN_conv(x)); *ln_ff_done: t1 = LN_ff(x) came out of
// pointwise_conv2's epilogue                          encoder_layer.py:236-251
int conv_module(const LayerCtx& c, const EncLayer& L, bool* ln_ff_done) {
  wn_model* m = c.m;
  const wn_config& cfg = m->cfg;
  const int d = c.d, M = c.M;
  hipStream_t s = c.s;
  float *x = c.x, *t1 = c.t1, *t2 = c.t2;
  // (the projections of this module need the row-LN epilogue's width on top of the route)
  auto image = [&](const Linear& l, int N, int epi) {
    return c.rowx ? x6r_image(c, l, N, epi) : nullptr;
  };
  // out-projection + residual + LN_conv chained with pointwise_conv1 + GLU in ONE launch
  // (gemm_x6r.hip epi 3): LN_conv(x) never reaches HBM.  The second GEMM has the shape rule of
  // the GLU launch at d = 256; at d = 512, where GLU alone has no kernel, none beyond epi 3's:
  // its image has to exist, that is all
  const void* out_ch = tune().x6r_chain != 0 ? image(L.out, d, 3) : nullptr;
  const void* pw1_ch = !out_ch ? nullptr : d == 512 ? x6_image(L.pw1) : image(L.pw1, 2 * d, 2);
  if (out_ch && pw1_ch) {
    X6RArgs g = x6r_rowln_args(c, L.out, out_ch, t2, L.norm_conv, 3);
    g.y = nullptr;
    g.W3b = pw1_ch; g.bias2 = L.pw1.b; g.C = t2; g.ldc = d;   // (C aliases A: a block reads its rows first)
    if (gemm_x6r(g, s) != 0) return -2;
  } else {
    // x += out_proj(context); t1 = LN_conv(x)       encoder_layer.py:236-240
    if (const void* w6 = image(L.out, d, 1)) {
      if (gemm_x6r(x6r_rowln_args(c, L.out, w6, t2, L.norm_conv, 1), s) != 0) return -2;
    } else if (c.rowln) {
      WN_TRY(rowln_gemm(c, L.out, t2, L.norm_conv));
    } else {
      WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d, 1.0f, false, c.h16));
      // x += Conv(LN(x))                              encoder_layer.py:240-251
      WN_TRY(ln(L.norm_conv, x, t1, M, d, c.eps, s, c.h16));
    }
    // pointwise_conv1 + GLU                        convolution.py:115-118
    if (const void* w6 = image(L.pw1, 2 * d, 2)) {
      X6RArgs g;
      g.A = t1; g.lda = d; g.K = d; g.W3 = w6; g.bias = L.pw1.b; g.M = M; g.N = 2 * d;
      g.epi = 2; g.C = t2; g.ldc = d;
      WN_TRY(gemm_x6r(g, s));
    } else {
      WN_TRY(linear(L.pw1, t1, d, t2, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true, c.h16));
    }
  }
  DwConvArgs dw;
  dw.x = t2; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
  dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = cfg.cnn_norm;
  dw.y = t1; dw.ldy = d;
  dw.row_utt = m->d_row_utt.as<int>(); dw.off = m->d_off.as<int>();
  dw.len = m->d_len.as<int>();
  dw.M = M; dw.D = d; dw.K = cfg.cnn_kernel; dw.causal = cfg.causal;
  dw.t_max = m->Tp; dw.eps = 1e-5f;
  // x += pointwise_conv2(.); t1 = LN_ff(x)        encoder_layer.py:251-255
  // Everything the row-block launch takes over hangs off ITS image pointer:
  const void* pw2_w6 = image(L.pw2, d, 1);
  // d = 256: the depthwise conv + norm + SiLU is its prologue (gemm_x6r.hip DWC) -- no launch,
  // no round trip of the conv module's middle tensor
  const bool dwc = pw2_w6 && tune().x6r_dwc != 0 && d == 256;
  if (!dwc) WN_TRY(dwconv_ln_silu(dw, s));
  *ln_ff_done = pw2_w6 || c.rowln;
  if (pw2_w6) {
    // (the feed-forward module behind it takes LN_ff(x) as a plane image where it runs fused:
    // asked BEFORE the launch, the row-block kernel is the only producer that can write one)
    void* ff_img = t1_image_for(m, L.ff1, L.ff2, ACT_SILU);
    X6RArgs g = x6r_rowln_args(c, L.pw2, pw2_w6, t1, L.norm_ff, 1);
    if (dwc) { g.dw = dw; g.dw_on = 1; }
    if (ff_img) { g.y3 = ff_img; g.y = nullptr; }     // LN(x) leaves as its plane image only
    if (gemm_x6r(g, s) != 0) return -2;
    m->t1_img_ok = ff_img != nullptr;
    return 0;
  }
  if (c.rowln) return rowln_gemm(c, L.pw2, t1, L.norm_ff);
  return linear(L.pw2, t1, d, x, d, M, s, ACT_NONE, x, d);
}

// x += 0.5 * FFN(LN(x)); x = norm_final(x)            encoder_layer.py:253-263
// `Ln`: the next layer (null behind the last): its norm_ff_macaron(x) goes to t1 in the same pass
int final_ffn(const LayerCtx& c, const EncLayer& L, const EncLayer* Ln, bool ln_ff_done) {
  wn_model* m = c.m;
  const int d = c.d, M = c.M;
  hipStream_t s = c.s;
  int fS = 0;
  if (c.f32) {
    if (!ln_ff_done) WN_TRY(ln(L.norm_ff, c.x, c.t1, M, d, c.eps, s));
    fS = ffn_fused_try(m, L.ff1, L.ff2, ACT_SILU, s);
    if (fS < 0) return -2;
  }
  if (fS > 0) {
    // partial reduction + residual + norm_final (+ the next layer's norm_ff_macaron)
    const float* P = m->ffn_part.as<float>();
    if (!Ln)
      return ffn_reduce_ln(c.x, P, fS, L.ff2.b, 0.5f, L.norm_final.w, L.norm_final.b, nullptr,
                           nullptr, nullptr, M, d, c.eps, 2, s);
    void* mac_img = t1_image_for(m, Ln->ffm1, Ln->ffm2, ACT_SILU);
    if (!mac_img)
      return ffn_reduce_ln(c.x, P, fS, L.ff2.b, 0.5f, L.norm_final.w, L.norm_final.b,
                           Ln->norm_ff_mac.w, Ln->norm_ff_mac.b, c.t1, M, d, c.eps, 1, s);
    WN_TRY(ffn_reduce_ln_img(c.x, P, fS, L.ff2.b, 0.5f, L.norm_final.w, L.norm_final.b,
                             Ln->norm_ff_mac.w, Ln->norm_ff_mac.b, mac_img, M, d, c.eps, s));
    m->t1_img_ok = true;
    return 0;
  }
  WN_TRY(ffn_module(m, L.norm_ff, L.ff1, L.ff2, ACT_SILU, 0.5f, c.f32, c.h16, s));
  if (Ln && !(t_mx && c.h16))
    return layernorm2(c.x, L.norm_final.w, L.norm_final.b, Ln->norm_ff_mac.w, Ln->norm_ff_mac.b,
                      c.x, c.t1, M, d, c.eps, s, c.h16);
  return ln(L.norm_final, c.x, c.x, M, d, c.eps, s);
}

}  // namespace

// The Conformer layers over the packed rows of the current batch (m->x), then after_norm into
// m->enc.  One layer = the four modules of ConformerEncoderLayer.forward, encoder_layer.py:
// 188-265.
int encoder_layers(wn_model* m, int chunk, int left, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& cfg = m->cfg;
  const LayerCtx c(m, chunk, left, s);
  const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, cfg.n_layers) : cfg.n_layers;
  m->t1_img_ok = false;
  for (int li = 0; li < n_run; ++li) {
    const EncLayer& L = W.layers[li];
    const void* qkv_w6 = x6r_image(c, L.qkv, 3 * c.d, 0);
    int pro_S = 0;
    bool ln_ff_done = false;
    WN_TRY(macaron_ffn(c, L, li, qkv_w6 != nullptr, &pro_S));
    WN_TRY(self_attention(c, L, qkv_w6, pro_S));
    WN_TRY(conv_module(c, L, &ln_ff_done));
    WN_TRY(final_ffn(c, L, li + 1 < n_run ? &W.layers[li + 1] : nullptr, ln_ff_done));
  }
  return after_norm_out(m, s);
}

// The Conformer layers over ONE chunk of R frames of n_sess streaming sessions with their
// caches (ConformerEncoderLayer.forward with att_cache / cnn_cache, encoder_layer.py:
// 188-265, driven by BaseEncoder.forward_chunk, encoder.py:246-285; batched formulation:
// wenet/bin/export_onnx_gpu.py:83-232).  Same kernels as encoder_layers on n_sess * R rows;
// session b's attention sees its [cache | chunk] keys (ragged: cache lengths differ) with
// the position rows offset_b - t1_b ..., its causal convolution sees its cached left
// context.  All masks are the all-ones fakes of forward_chunk.
int encoder_layers_chunk(wn_model* m, int n_sess, int R, const int* offsets,
                         std::vector<ChunkSess>& sess, float* out, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, M = n_sess * R;
  const int lorder = c.causal ? c.cnn_kernel - 1 : 0;
  const int LR = lorder + R;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();
  float* qkv = m->qkv.as<float>();
  const float eps = c.norm_eps;
  // descriptors: attention (queries R per session, ragged keys), conv (LR rows per session)
  std::vector<int> qoff(n_sess), qlen(n_sess, R), kvoff(n_sess), kvlen(n_sess), poff(n_sess),
      coff(n_sess), clen(n_sess, LR), rowutt((size_t)n_sess * LR);
  std::vector<int64_t> pw2_rows((size_t)M);
  int total_kv = 0, max_tk = 0;
  for (int b = 0; b < n_sess; ++b) {
    const int tk = sess[b].t1 + R;
    qoff[b] = b * R;
    kvoff[b] = total_kv; kvlen[b] = tk;
    sess[b].kv_off = total_kv;
    total_kv += tk; max_tk = std::max(max_tk, tk);
    // key j of this call sits at position offset - t1 + j   encoder.py:256-257
    poff[b] = offsets[b] - sess[b].t1;
    coff[b] = b * LR;
    for (int r = 0; r < LR; ++r) rowutt[(size_t)b * LR + r] = b;
    for (int r = 0; r < R; ++r) pw2_rows[(size_t)b * R + r] = ((int64_t)b * LR + lorder + r) * d;
  }
  WN_TRY(m->ck_kv.ensure((size_t)total_kv * 2 * d * sizeof(float)));
  WN_TRY(m->ck_xext.ensure((size_t)n_sess * LR * d * sizeof(float)));
  WN_TRY(m->ck_glu.ensure((size_t)n_sess * LR * d * sizeof(float)));
  WN_TRY(m->stage.begin((size_t)(n_sess * (LR + 8) + 64) * sizeof(int) +
                        (size_t)M * sizeof(int64_t) + n_sess * sizeof(ChunkSess) + 4096));
  WN_TRY(upload_desc(m, m->ck_desc, qoff, s));
  WN_TRY(upload_desc(m, m->r_qlen, qlen, s));
  WN_TRY(upload_desc(m, m->r_kvoff, kvoff, s));
  WN_TRY(upload_desc(m, m->r_kvlen, kvlen, s));
  WN_TRY(upload_desc(m, m->r_pos, poff, s));
  WN_TRY(upload_desc(m, m->r_qoff, coff, s));
  WN_TRY(upload_desc(m, m->r_tgt, clen, s));
  WN_TRY(upload_desc(m, m->ck_rowutt, rowutt, s));
  WN_TRY(m->stage.put(m->d_a_row_off, pw2_rows.data(), pw2_rows.size() * sizeof(int64_t), s));
  WN_TRY(m->stage.put(m->ck_sess, sess.data(), sess.size() * sizeof(ChunkSess), s));
  WN_TRY(m->stage.end(s));
  const ChunkSess* dsess = m->ck_sess.as<ChunkSess>();
  float* kv = m->ck_kv.as<float>();
  float* xext = m->ck_xext.as<float>();
  float* glu = m->ck_glu.as<float>();
  for (int li = 0; li < c.n_layers; ++li) {
    const EncLayer& L = W.layers[li];
    WN_TRY(ln(L.norm_ff_mac, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ffm1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ffm2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    // attention over [cached | new] keys             attention.py:180-245,364-438
    WN_TRY(ln(L.norm_mha, x, t1, M, d, eps, s));
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * d, M, s));
    WN_TRY(chunk_kv_assemble(dsess, n_sess, li, max_tk, qkv, R, H, kv, s));
    AttnArgs a;
    a.Q = qkv; a.ldq = 3 * d;
    a.K = kv; a.V = kv + d; a.ldk = a.ldv = 2 * d;
    a.P = L.pos_tab; a.ldp = d; a.p_off = m->r_pos.as<int>();
    a.bias_u = L.bias_u; a.bias_v = L.bias_v;
    a.O = t2; a.ldo = d;
    a.q_off = m->ck_desc.as<int>(); a.q_len = m->r_qlen.as<int>();
    a.kv_off = m->r_kvoff.as<int>(); a.kv_len = m->r_kvlen.as<int>();
    a.n_seq = n_sess; a.n_heads = H; a.max_q_len = R;
    a.mask_mode = 0;
    a.scale = 1.0f / sqrtf(64.0f);
    WN_TRY(attention(a, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
    // convolution module with its left-context cache  convolution.py:98-153
    WN_TRY(ln(L.norm_conv, x, t1, M, d, eps, s));
    if (lorder > 0) {
      WN_TRY(chunk_conv_input(dsess, n_sess, li, t1, R, d, lorder, xext, s));
      WN_TRY(linear(L.pw1, xext, d, glu, d, n_sess * LR, s, ACT_NONE, nullptr, 0, 1.0f, true));
    } else {
      WN_TRY(linear(L.pw1, t1, d, glu, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
    }
    DwConvArgs dw;
    dw.x = glu; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
    dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = c.cnn_norm;
    dw.y = xext; dw.ldy = d;
    dw.row_utt = m->ck_rowutt.as<int>(); dw.off = m->r_qoff.as<int>();
    dw.len = m->r_tgt.as<int>();
    dw.M = n_sess * LR; dw.D = d; dw.K = c.cnn_kernel; dw.causal = c.causal;
    dw.t_max = LR; dw.eps = 1e-5f;
    WN_TRY(dwconv_ln_silu(dw, s));
    {
      // pointwise_conv2 on the chunk rows of every session (rows lorder.. of its segment)
      GemmArgs g;
      g.A = xext; g.W = L.pw2.w; g.bias = L.pw2.b; g.C = x; g.resid = x;
      g.M = M; g.N = d; g.K = d; g.lda = d; g.ldc = d; g.ldr = d;
      g.a_row_off = m->d_a_row_off.as<int64_t>(); g.conv_C = d;
      WN_TRY(gemm_f32(g, s));
    }
    WN_TRY(ln(L.norm_ff, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ff1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  }
  WN_TRY(ln(W.after_norm, x, out, M, d, eps, s));
  return 0;
}
