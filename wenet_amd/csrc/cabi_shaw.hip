// C ABI (include/wenet_amd.h), W2v-BERT 2.0 / conformer_shaw handles (`encoder: conformer` with
// input_layer stack_n_frames, pos_enc_layer_type no_pos, selfattention_layer_type
// shaw_rel_selfattn; the recipe of wenet/models/ssl/w2vbert/convert_w2vbert_to_wenet_config_and_ckpt.py):
// the entry point that creates one, its weights, and what wn_encode runs on it -- the stacked-frame
// front end and the Conformer layers over the packed rows of the batch.  A plain fp32 path built
// from the generic pieces (ln, linear with its SiLU / GLU / residual epilogues, dwconv_ln_silu)
// and the two kernels of attention_shaw.hip; the six-product, row-block and fused feed-forward
// routes of conformer.hip stay off: untuned.
#include "model_state.h"
#include "weight_stage.h"

int shaw_config_check(const wn_config& c, const wn_shaw_config& h, bool other_family) {
  WN_CHECK(!other_family, "shaw: an asr_model head only, no other encoder family");
  WN_CHECK(h.max_left == SHAW_LEFT, "shaw: max_left must be 64 (attention_shaw)");
  WN_CHECK(h.max_right == SHAW_RIGHT, "shaw: max_right must be 8 (attention_shaw)");
  WN_CHECK(h.stack == 2, "shaw: stack must be 2 (stack_frames_ln)");
  WN_CHECK(c.encoder_type == 0 && c.input_layer == 0 && c.cnn_norm == 0 && c.activation == 0 &&
               c.use_dynamic_chunk == 0 && c.static_chunk_size <= 0,
           "shaw: conformer layers, layer_norm conv module, full context, swish");
  WN_CHECK(c.d_model >= 64 && c.d_model <= 1024 && c.d_model % 64 == 0,
           "shaw: d_model must be a multiple of 64 up to 1024");
  WN_CHECK(c.cnn_kernel >= 1 && c.cnn_kernel <= 63, "shaw: cnn_module_kernel must be in [1, 63]");
  return 0;
}

// StackNFramesSubsampling (norm, out) and the layers: the Conformer's names without linear_pos /
// pos_bias_u / pos_bias_v and without the conv module's biases (conv_bias false), plus
// self_attn.rel_k_embed.weight [73][64]
int shaw_stage(const wn::Src& src, wn::HostStage& hs, const wn_config& c) {
  using namespace wn;
  const int d = c.d_model, F = c.ffn_dim, K = c.cnn_kernel;
  WN_TRY(stage_norm(src, hs, "encoder.embed.norm", 2 * c.feat_dim));
  WN_TRY(stage_linear(src, hs, "encoder.embed.out", d, 2 * c.feat_dim));
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    for (const char* n : {"norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    WN_TRY(stage_norm(src, hs, p + ".conv_module.norm", d));
    for (const char* ff : {"feed_forward_macaron", "feed_forward"}) {
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_1", F, d));
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
    }
    {  // fused Q | K | V
      std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d);
      const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
      for (int j = 0; j < 3; ++j) {
        WN_GET(pw, p + ".self_attn." + parts[j] + ".weight", (int64_t)d * d);
        WN_GET(pb, p + ".self_attn." + parts[j] + ".bias", d);
        memcpy(&w[(size_t)j * d * d], pw, sizeof(float) * d * d);
        memcpy(&b[(size_t)j * d], pb, sizeof(float) * d);
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
    }
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    WN_GET(tab, p + ".self_attn.rel_k_embed.weight", (int64_t)SHAW_ROWS * 64);
    hs.add(p + ".shaw_tab", tab, (size_t)SHAW_ROWS * 64);
    {  // pointwise_conv1 (2d, d, 1), no bias: rows permuted per 64 as [32 a | 32 gate]; the GLU of
       // a zero frame is 0 (cpad)
      WN_GET(w1, p + ".conv_module.pointwise_conv1.weight", (int64_t)2 * d * d);
      std::vector<float> w((size_t)2 * d * d);
      for (int g = 0; g < d / 32; ++g)
        for (int j = 0; j < 32; ++j) {
          const int ch = g * 32 + j;
          memcpy(&w[(size_t)(g * 64 + j) * d], &w1[(size_t)ch * d], sizeof(float) * d);
          memcpy(&w[(size_t)(g * 64 + 32 + j) * d], &w1[(size_t)(d + ch) * d], sizeof(float) * d);
        }
      hs.add(p + ".pw1.weight", w.data(), w.size());
      hs.alloc(p + ".pw1.bias", 2 * d);
      hs.alloc(p + ".cpad", d);
    }
    {  // depthwise (d,1,K), no bias -> [K][d]; dwconv_ln_silu reads a bias row: zeros
      WN_GET(wd, p + ".conv_module.depthwise_conv.weight", (int64_t)d * K);
      std::vector<float> w((size_t)K * d);
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < K; ++k) w[(size_t)k * d + ch] = wd[(size_t)ch * K + k];
      hs.add(p + ".dw.weight", w.data(), w.size());
      hs.alloc(p + ".dw.bias", d);
    }
    WN_TRY(stage_linear(src, hs, p + ".conv_module.pointwise_conv2", d, d, false));
  }
  return 0;
}

int shaw_bind(ModelData& W, const wn_config& c) {
  const int d = c.d_model, F = c.ffn_dim;
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& p, int o, int i, bool bias = true) {
    Linear l; l.w = P(p + ".weight"); l.b = bias ? P(p + ".bias") : nullptr;
    l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& p) {
    Norm n; n.w = P(p + ".weight"); n.b = P(p + ".bias"); return n;
  };
  W.stack_norm = NORM("encoder.embed.norm");
  W.sub_out = LIN("encoder.embed.out", d, 2 * c.feat_dim);
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
    L.qkv = LIN(p + ".qkv", 3 * d, d);
    L.out = LIN(p + ".self_attn.linear_out", d, d);
    L.pw1 = LIN(p + ".pw1", 2 * d, d);
    L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, d, false);
    L.shaw_tab = P(p + ".shaw_tab");
    L.dw_wt = P(p + ".dw.weight");
    L.dw_b = P(p + ".dw.bias");
    L.cpad = P(p + ".cpad");
  }
  return 0;
}

// One layer = ConformerEncoderLayer.forward (encoder_layer.py) as the recipe configures it:
// x += 0.5 FFN_mac(LN(x)); x += MHA_shaw(LN(x)); x += Conv(LN(x)), causal, no biases;
// x += 0.5 FFN(LN(x)); x = norm_final(x).  after_norm behind the last layer (final_norm true).
static int encoder_layers_shaw(wn_model* m, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, M = m->rows;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();     // M x max(ffn_dim, 2 d): FFN hidden, then GLU | conv
  float* qkv = m->qkv.as<float>();
  const float eps = c.norm_eps;
  int max_len = 0;
  for (int b = 0; b < m->B; ++b) max_len = std::max(max_len, m->len[b]);
  const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers) : c.n_layers;
  for (int li = 0; li < n_run; ++li) {
    const EncLayer& L = W.layers[li];
    WN_TRY(ln(L.norm_ff_mac, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ffm1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ffm2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_mha, x, t1, M, d, eps, s));
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * d, M, s));
    AttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.P = L.shaw_tab; a.ldp = 64;
    a.O = t2; a.ldo = d;
    a.q_off = a.kv_off = m->d_off.as<int>(); a.q_len = a.kv_len = m->d_len.as<int>();
    a.n_seq = m->B; a.n_heads = H; a.max_q_len = max_len;
    a.scale = 1.0f / sqrtf(64.0f);
    WN_TRY(attention_shaw(a, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
    // convolution module                               convolution.py:36-89, 98-153
    WN_TRY(ln(L.norm_conv, x, t1, M, d, eps, s));
    float* glu = hb;
    float* cv = hb + (size_t)M * d;
    WN_TRY(linear(L.pw1, t1, d, glu, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
    DwConvArgs dw;
    dw.x = glu; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
    dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = 0;
    dw.y = cv; dw.ldy = d;
    dw.row_utt = m->d_row_utt.as<int>(); dw.off = m->d_off.as<int>(); dw.len = m->d_len.as<int>();
    dw.M = M; dw.D = d; dw.K = c.cnn_kernel; dw.causal = c.causal;
    dw.t_max = m->Tp; dw.eps = 1e-5f;
    WN_TRY(dwconv_ln_silu(dw, s));
    WN_TRY(linear(L.pw2, cv, d, x, d, M, s, ACT_NONE, x, d));
    WN_TRY(ln(L.norm_ff, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ff1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  }
  return after_norm_out(m, s);
}

// wn_encode on a shaw handle.  An utterance of L frames gives L / 2 rows, each from its own frames
// 2 t and 2 t + 1 < 2 (L / 2): the same rows alone or batched (the reference's mask keeps a
// shorter utterance's padding out of the attention, and the causal conv has no right context).
int encode_shaw(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B, int T,
                float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, F = c.feat_dim, Tp = T / 2;
  WN_CHECK(B < 65536, "wn_encode: more than 65535 utterances");
  m->ln0_done = false;
  m->front_route = 0;
  std::vector<int> off(B), len(B);
  int M = 0, max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    off[b] = M; len[b] = L / 2; M += len[b];
    max_len = std::max(max_len, len[b]);
    if (enc_lens_host) enc_lens_host[b] = len[b];
  }
  // raw fbank in (wn_model_set_utt_norm_input): the frame counts travel with the layout
  const bool utt = m->sh.utt_input;
  WN_TRY(set_layout(m, B, Tp, off, len, M, s, utt ? B + 16 : 0));
  if (utt) WN_TRY(m->stage.put(m->utt_len, feat_lens_host, (size_t)B * sizeof(int32_t), s));
  WN_TRY(m->stage.end(s));
  if (M > 0) {
    const int hid = std::max(c.ffn_dim, 2 * d);
    WN_TRY(m->c2.ensure((size_t)M * 2 * F * sizeof(float)));
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * hid * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    StackFramesArgs a;
    a.feats = feats_dev; a.mean = W.cmvn_mean; a.istd = W.cmvn_istd;
    a.ln_w = W.stack_norm.w; a.ln_b = W.stack_norm.b;
    a.out = m->c2.as<float>(); a.ldo = 2 * F;
    a.off = m->d_off.as<int>(); a.len = m->d_len.as<int>();
    a.B = B; a.T = T; a.F = F; a.max_len = max_len; a.eps = 1e-5f;
    if (utt) {
      // statistics over every frame of the utterance (the one an odd length drops included), the
      // division inside the front end: no normalised tensor in HBM
      int max_frames = 0;
      for (int b = 0; b < B; ++b) max_frames = std::max(max_frames, (int)feat_lens_host[b]);
      WN_TRY(utt_stats_handle(m, feats_dev, max_frames, B, T, F, s));
      StackFramesUttArgs ua;
      ua.k = a; ua.umean = m->utt_mean.as<float>(); ua.ustd = m->utt_std.as<float>();
      WN_TRY(stack_frames_ln_utt(ua, s));
    } else {
      WN_TRY(stack_frames_ln(a, s));
    }
    // Linear(2 F -> d); NoPositionalEncoding: no xscale, x unchanged
    WN_TRY(linear(W.sub_out, m->c2.as<float>(), 2 * F, m->x.as<float>(), d, M, s));
    WN_TRY(encoder_layers_shaw(m, s));
  }
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

int wn_model_create_shaw(const wn_config* cfg, const wn_shaw_config* hcfg,
                         const wn_tensor* weights, int32_t n_weights, int32_t device,
                         wn_model** out) {
  WN_CHECK(hcfg, "wn_model_create_shaw: null argument");
  return create_model_impl(cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, weights,
                           n_weights, device, out, hcfg);
}

}  // extern "C"
