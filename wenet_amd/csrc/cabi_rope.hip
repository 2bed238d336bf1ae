// C ABI (include/wenet_amd.h), rotary Conformer handles (`encoder: conformer` with
// selfattention_layer_type rope_abs_selfattn, pos_enc_layer_type rope_pos, optionally n_kv_head /
// head_dim): the entry point that creates one, its weights, and what wn_encode runs on it -- the
// Conformer front end (Conv2dSubsampling4; RopePositionalEncoding scales by sqrt(d) and adds
// nothing), then the Conformer layers over the packed rows of the batch with attention_rope.  A
// plain fp32 path built from the generic pieces (ln, linear with its SiLU / GLU / residual
// epilogues, dwconv_ln_silu) and the kernel of attention_rope.hip; the six-product, row-block and
// fused feed-forward routes of conformer.hip stay off: untuned.
#include "model_state.h"
#include "weight_stage.h"

int rope_config_check(const wn_config& c, const wn_rope_config& r, bool other_family) {
  WN_CHECK(!other_family, "rope: an asr_model head only, no other encoder family");
  WN_CHECK(r.head_dim == 64, "rope: head_dim must be 64 (attention_rope)");
  WN_CHECK(c.encoder_type == 0 && c.input_layer == 0 && c.activation == 0,
           "rope: conformer layers behind the conv2d front end, swish");
  WN_CHECK(c.cnn_norm == 0 || c.cnn_norm == 1, "rope: cnn_norm 0 (layer_norm) or 1 (batch_norm)");
  WN_CHECK(c.n_heads > 0 && c.n_heads < 256 && c.d_model == c.n_heads * 64 && c.d_model <= 1024,
           "rope: d_model must be n_heads * 64, at most 1024");
  WN_CHECK(r.n_kv_heads >= 1 && c.n_heads % r.n_kv_heads == 0,
           "rope: n_kv_heads must divide n_heads");
  WN_CHECK(r.max_pos >= 1 && r.max_pos <= 65536, "rope: max_pos must be in [1, 65536]");
  WN_CHECK(c.cnn_kernel >= 1 && c.cnn_kernel <= 63, "rope: cnn_module_kernel must be in [1, 63]");
  return 0;
}

// The Conformer's names without linear_pos / pos_bias_u / pos_bias_v; linear_k / linear_v are
// [64 n_kv_heads][d]; the checkpoint's encoder.embed.pos_enc.pe [1][max_pos][32][2], the rotation
// table, arrives as encoder.embed.pos_enc.rope_pe (the name `pe` is the sinusoid table of the
// other families, whose rows size the decoder's positions)
int rope_stage(const wn::Src& src, wn::HostStage& hs, const wn_config& c, const wn_rope_config& r) {
  using namespace wn;
  const int d = c.d_model, F = c.ffn_dim, K = c.cnn_kernel, dkv = 64 * r.n_kv_heads;
  {  // (cos, sin) pairs -> cos[32] | sin[32] per position, the values untouched
    WN_GET(pe, "encoder.embed.pos_enc.rope_pe", (int64_t)r.max_pos * 64);
    float* t = hs.alloc("rope.tab", (size_t)r.max_pos * 64);
    for (int p = 0; p < r.max_pos; ++p)
      for (int i = 0; i < 32; ++i) {
        t[(size_t)p * 64 + i] = pe[((size_t)p * 32 + i) * 2];
        t[(size_t)p * 64 + 32 + i] = pe[((size_t)p * 32 + i) * 2 + 1];
      }
  }
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    for (const char* n : {"norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    if (c.cnn_norm == 0) {
      WN_TRY(stage_norm(src, hs, p + ".conv_module.norm", d));
    } else {
      // eval-mode BatchNorm1d as a per-channel affine (dwconv_ln_silu's norm_mode 1)
      const std::string q = p + ".conv_module.norm";
      WN_GET(bw, q + ".weight", d);
      WN_GET(bb, q + ".bias", d);
      WN_GET(bm, q + ".running_mean", d);
      WN_GET(bv, q + ".running_var", d);
      std::vector<float> sc(d), sh(d);
      for (int ch = 0; ch < d; ++ch) {
        const double g = (double)bw[ch] / sqrt((double)bv[ch] + 1e-5);
        sc[ch] = (float)g;
        sh[ch] = (float)((double)bb[ch] - (double)bm[ch] * g);
      }
      hs.add(q + ".weight", sc.data(), sc.size());
      hs.add(q + ".bias", sh.data(), sh.size());
    }
    for (const char* ff : {"feed_forward_macaron", "feed_forward"}) {
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_1", F, d));
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
    }
    {  // fused Q | K | V: d + 2 * 64 n_kv_heads rows
      std::vector<float> w((size_t)(d + 2 * dkv) * d), b((size_t)d + 2 * dkv);
      const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
      size_t row = 0;
      for (int j = 0; j < 3; ++j) {
        const int n = j == 0 ? d : dkv;
        WN_GET(pw, p + ".self_attn." + parts[j] + ".weight", (int64_t)n * d);
        WN_GET(pb, p + ".self_attn." + parts[j] + ".bias", n);
        memcpy(&w[row * d], pw, sizeof(float) * n * d);
        memcpy(&b[row], pb, sizeof(float) * n);
        row += n;
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
    }
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    {  // pointwise_conv1 (2d, d, 1): rows permuted per 64 as [32 a | 32 gate]
      WN_GET(w1, p + ".conv_module.pointwise_conv1.weight", (int64_t)2 * d * d);
      WN_GET(b1, p + ".conv_module.pointwise_conv1.bias", 2 * d);
      std::vector<float> w((size_t)2 * d * d), b(2 * d), cp(d);
      for (int g = 0; g < d / 32; ++g)
        for (int j = 0; j < 32; ++j) {
          const int ch = g * 32 + j;
          memcpy(&w[(size_t)(g * 64 + j) * d], &w1[(size_t)ch * d], sizeof(float) * d);
          memcpy(&w[(size_t)(g * 64 + 32 + j) * d], &w1[(size_t)(d + ch) * d], sizeof(float) * d);
          b[g * 64 + j] = b1[ch];
          b[g * 64 + 32 + j] = b1[d + ch];
          // GLU of a zero input frame: bias_a * sigmoid(bias_gate)
          cp[ch] = b1[ch] * (1.0f / (1.0f + expf(-b1[d + ch])));
        }
      hs.add(p + ".pw1.weight", w.data(), w.size());
      hs.add(p + ".pw1.bias", b.data(), b.size());
      hs.add(p + ".cpad", cp.data(), cp.size());
    }
    {  // depthwise (d,1,K) -> [K][d]
      WN_GET(wd, p + ".conv_module.depthwise_conv.weight", (int64_t)d * K);
      WN_GET(bd, p + ".conv_module.depthwise_conv.bias", d);
      std::vector<float> w((size_t)K * d);
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < K; ++k) w[(size_t)k * d + ch] = wd[(size_t)ch * K + k];
      hs.add(p + ".dw.weight", w.data(), w.size());
      hs.add(p + ".dw.bias", bd, d);
    }
    WN_TRY(stage_linear(src, hs, p + ".conv_module.pointwise_conv2", d, d));
  }
  return 0;
}

int rope_bind(ModelData& W, const wn_config& c, const wn_rope_config& r) {
  const int d = c.d_model, F = c.ffn_dim;
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& p, int o, int i) {
    Linear l; l.w = P(p + ".weight"); l.b = P(p + ".bias"); l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& p) {
    Norm n; n.w = P(p + ".weight"); n.b = P(p + ".bias"); return n;
  };
  W.rope_tab = P("rope.tab");
  W.layers.resize(c.n_layers);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    EncLayer& L = W.layers[i];
    L.norm_ff_mac = NORM(p + ".norm_ff_macaron");
    L.norm_mha = NORM(p + ".norm_mha");
    L.norm_conv = NORM(p + ".norm_conv");
    L.norm_ff = NORM(p + ".norm_ff");
    L.norm_final = NORM(p + ".norm_final");
    L.conv_norm = NORM(p + ".conv_module.norm");
    L.ffm1 = LIN(p + ".feed_forward_macaron.w_1", F, d);
    L.ffm2 = LIN(p + ".feed_forward_macaron.w_2", d, F);
    L.ff1 = LIN(p + ".feed_forward.w_1", F, d);
    L.ff2 = LIN(p + ".feed_forward.w_2", d, F);
    L.qkv = LIN(p + ".qkv", d + 128 * r.n_kv_heads, d);
    L.out = LIN(p + ".self_attn.linear_out", d, d);
    L.pw1 = LIN(p + ".pw1", 2 * d, d);
    L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, d);
    L.dw_wt = P(p + ".dw.weight");
    L.dw_b = P(p + ".dw.bias");
    L.cpad = P(p + ".cpad");
  }
  return 0;
}

// One layer = ConformerEncoderLayer.forward (encoder_layer.py):
// x += 0.5 FFN_mac(LN(x)); x += MHA_rope(LN(x)); x += Conv(LN(x)); x += 0.5 FFN(LN(x));
// x = norm_final(x).  after_norm behind the last layer.
static int encoder_layers_rope(wn_model* m, int chunk, int left, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_rope_config& r = m->rp.c;
  const int d = c.d_model, H = c.n_heads, dkv = 64 * r.n_kv_heads, wq = d + 2 * dkv, M = m->rows;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();     // M x max(ffn_dim, 2 d): FFN hidden, then GLU | conv
  float* qkv = m->qkv.as<float>();     // M x (d + 2 dkv): Q | K | V
  const float eps = c.norm_eps;
  int max_len = 0;
  for (int b = 0; b < m->B; ++b) max_len = std::max(max_len, m->len[b]);
  // the chunk mask of the decode-time branches of mask.py:126-198, as the Conformer path
  int mask_mode = 0, cs = 0, lc = -1;
  if (c.use_dynamic_chunk) {
    if (chunk > 0) { mask_mode = 2; cs = chunk; lc = left; }
  } else if (c.static_chunk_size > 0) {
    mask_mode = 2; cs = c.static_chunk_size; lc = left;
  }
  const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers) : c.n_layers;
  for (int li = 0; li < n_run; ++li) {
    const EncLayer& L = W.layers[li];
    WN_TRY(ln(L.norm_ff_mac, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ffm1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ffm2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_mha, x, t1, M, d, eps, s));
    WN_TRY(linear(L.qkv, t1, d, qkv, wq, M, s));
    wn::RopeAttnArgs ra;
    ra.n_kv_heads = r.n_kv_heads; ra.max_pos = r.max_pos;
    AttnArgs& a = ra.a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + d + dkv;
    a.ldq = a.ldk = a.ldv = wq;
    a.P = W.rope_tab; a.ldp = 64;
    a.O = t2; a.ldo = d;
    a.q_off = a.kv_off = m->d_off.as<int>(); a.q_len = a.kv_len = m->d_len.as<int>();
    a.n_seq = m->B; a.n_heads = H; a.max_q_len = max_len;
    a.mask_mode = mask_mode; a.chunk_size = cs; a.left_chunks = lc;
    a.scale = 1.0f / sqrtf(64.0f);
    WN_TRY(attention_rope(ra, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
    // convolution module                               convolution.py:36-89, 98-153
    WN_TRY(ln(L.norm_conv, x, t1, M, d, eps, s));
    float* glu = hb;
    float* cv = hb + (size_t)M * d;
    WN_TRY(linear(L.pw1, t1, d, glu, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
    DwConvArgs dw;
    dw.x = glu; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
    dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = c.cnn_norm;
    dw.y = cv; dw.ldy = d;
    dw.row_utt = m->d_row_utt.as<int>(); dw.off = m->d_off.as<int>(); dw.len = m->d_len.as<int>();
    dw.M = M; dw.D = d; dw.K = c.cnn_kernel; dw.causal = c.causal;
    // t_max 0: no frame behind an utterance's end is a masked frame of a longer batch (cpad); the
    // conv sees what it sees when the reference encodes the utterance ALONE -- zeros
    dw.t_max = 0; dw.eps = 1e-5f;
    WN_TRY(dwconv_ln_silu(dw, s));
    WN_TRY(linear(L.pw2, cv, d, x, d, M, s, ACT_NONE, x, d));
    WN_TRY(ln(L.norm_ff, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ff1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  }
  return after_norm_out(m, s);
}

// wn_encode on a rotary Conformer handle.  The front end is the classic Conformer's: utterance b
// gets the (len - 7) / 4 + 1 frames the reference gives it alone, and a row's position is its
// frame index in its own utterance, so alone and batched results are the same bits.
int encode_rope(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B, int T,
                int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const wn_config& c = m->cfg;
  const int d = c.d_model;
  const int Tp = ((T - 1) / 2 - 1) / 2;
  // the hidden buffer the front end sizes for the feed-forward alone is sized for the conv module
  // FIRST: its own ensure() calls then find room and move nothing
  size_t M = 0;
  for (int i = 0; i < B; ++i) {
    const int L = feat_lens_host[i];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    const int l2 = L > 6 ? (L - 7) / 4 + 1 : 0;
    // (RopePositionalEncoding.position_encoding asserts offset + size <= max_len)
    WN_CHECK(l2 <= m->rp.c.max_pos,
             "wn_encode: feat_lens: an utterance has more encoder frames than the rotation table "
             "(max_pos) has rows");
    M += l2;
  }
  if (M > 0) WN_TRY(m->hbuf.ensure(M * std::max(c.ffn_dim, 2 * d) * sizeof(float)));
  WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, enc_lens_host, 0, s));
  WN_TRY(encode_gate_wait(m, s));     // (paths that did not consume the gate behind conv1)
  WN_CHECK((size_t)m->rows == M, "wn_encode: internal row count");
  if (M > 0) WN_TRY(encoder_layers_rope(m, chunk, left, s));
  if (enc_out_dev) {
    if (M > 0) {
      WN_TRY(scatter_padded(m->enc.as<float>(), d, m->d_off.as<int>(), m->d_len.as<int>(), B, Tp,
                            d, enc_out_dev, s));
    } else if (Tp > 0) {
      WN_HIP(hipMemsetAsync(enc_out_dev, 0, (size_t)B * Tp * d * sizeof(float), s));
    }
  }
  return 0;
}

extern "C" {

int wn_model_create_rope(const wn_config* cfg, const wn_rope_config* rcfg,
                         const wn_tensor* weights, int32_t n_weights, int32_t device,
                         wn_model** out) {
  WN_CHECK(rcfg, "wn_model_create_rope: null argument");
  return create_model_impl(cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, weights,
                           n_weights, device, out, nullptr, rcfg);
}

}  // extern "C"
