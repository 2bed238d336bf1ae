// C ABI (include/wenet_amd.h), FireRedASR-AED handles (`model: firered`): the entry point that
// creates one, and what wn_encode runs on it -- the 32-channel front end and the layer stack of
// FireRedConformerEncoder (wenet/models/firered/encoder.py) over the packed rows of the batch.
// A plain fp32 path built from the generic pieces (ln, linear with its SiLU / GLU / residual
// epilogues, dwconv_ln_silu over 2 d_model channels) and the rel-shift attention of firered.hip;
// the six-product, row-block and fused feed-forward routes of conformer.hip stay off: untuned.
#include "model_state.h"

// One layer = FireRedConformerEncoderLayer.forward: x += 0.5 FFN_mac(LN(x)); x += MHA(x) with the
// three LayerNorms of the attention folded into the QKV projection (norm_mha is Identity);
// x += Conv(LN(x)) at conv_inner_factor 4; x += 0.5 FFN(LN(x)); x = norm_final(x).  No
// after_norm behind the last layer (final_norm false).
static int encoder_layers_firered(wn_model* m, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, d2 = 2 * d, H = c.n_heads, M = m->rows;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();     // M x max(ffn_dim, 4 d): FFN hidden, then GLU | conv
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
    // attention: one plain normalisation (eps of layer_norm_q/k/v) feeds the folded QKV
    WN_TRY(ln(L.norm_mha, x, t1, M, d, m->fr.c.attn_norm_eps, s));
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * d, M, s));
    RelShiftAttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.P = L.pos_tab; a.ldp = d;
    a.p_center = m->fr.c.max_frames - 1; a.p_rows = 2 * m->fr.c.max_frames - 1;
    a.bias_u = L.bias_u; a.bias_v = L.bias_v;
    a.O = t2; a.ldo = d;
    a.off = m->d_off.as<int>(); a.len = m->d_len.as<int>();
    a.n_seq = m->B; a.n_heads = H; a.max_len = max_len;
    a.scale = 1.0f / sqrtf(64.0f);
    WN_TRY(attention_relshift(a, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
    // convolution module, inner factor 4               convolution.py:36-89, 98-153
    WN_TRY(ln(L.norm_conv, x, t1, M, d, eps, s));
    float* glu = hb;
    float* cv = hb + (size_t)M * d2;
    WN_TRY(linear(L.pw1, t1, d, glu, d2, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
    DwConvArgs dw;
    dw.x = glu; dw.ldx = d2; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
    dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = 0;
    dw.y = cv; dw.ldy = d2;
    dw.row_utt = m->d_row_utt.as<int>(); dw.off = m->d_off.as<int>(); dw.len = m->d_len.as<int>();
    dw.M = M; dw.D = d2; dw.K = c.cnn_kernel; dw.causal = 0;
    dw.t_max = m->Tp; dw.eps = 1e-5f;
    WN_TRY(dwconv_ln_silu(dw, s));
    WN_TRY(linear(L.pw2, cv, d2, x, d, M, s, ACT_NONE, x, d));
    WN_TRY(ln(L.norm_ff, x, t1, M, d, eps, s));
    WN_TRY(linear(L.ff1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
    WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  }
  WN_TRY(m->enc.ensure((size_t)std::max(M, 1) * d * sizeof(float)));
  WN_HIP(hipMemcpyAsync(m->enc.p, m->x.p, (size_t)M * d * sizeof(float), hipMemcpyDeviceToDevice,
                        s));
  return 0;
}

// wn_encode on a FireRed handle.  Every utterance is encoded as the reference encodes it ALONE:
// six zero frames behind its own last frame (after CMVN), T' = ((len + 6 - 3) / 2 + 1 - 3) / 2 + 1
// -- the reference's batched mask would give a shorter utterance frames that read the batch's
// padding (deviations).  The padded output has the T' of a T-frame utterance.
int encode_firered(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B, int T,
                   float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, F1 = m->F1(), F2 = m->F2(), C = m->fr.c.sub_channels;
  auto out_len = [](int n) { return n > 0 ? ((n + 6 - 3) / 2 + 1 - 3) / 2 + 1 : 0; };
  const int Tp = out_len(T);
  WN_CHECK(B < 65536, "wn_encode: more than 65535 utterances");
  WN_CHECK(Tp <= m->fr.c.max_frames,
           "wn_encode: an utterance of " + std::to_string(T) + " frames gives " +
               std::to_string(Tp) + " encoder frames, more than the " +
               std::to_string(m->fr.c.max_frames) + " the position rows of this handle cover");
  m->ln0_done = false;
  m->front_route = 0;
  std::vector<int> off2(B), len2(B), off1(B), len1(B), flen(B);
  int M = 0, M1 = 0, max_t2 = 0;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    const int l2 = out_len(L), l1 = l2 > 0 ? 2 * l2 + 1 : 0;
    flen[b] = L;
    off2[b] = M; len2[b] = l2; M += l2;
    off1[b] = M1; len1[b] = l1; M1 += l1;
    max_t2 = std::max(max_t2, l2);
    if (enc_lens_host) enc_lens_host[b] = l2;
  }
  WN_TRY(set_layout(m, B, Tp, off2, len2, M, s));
  if (M > 0) {
    WN_TRY(upload_desc(m, m->d_off1, off1, s));
    WN_TRY(upload_desc(m, m->d_len1, len1, s));
    WN_TRY(upload_desc(m, m->ck_desc, flen, s));
  }
  WN_TRY(m->stage.end(s));
  if (M > 0) {
    const int hid = std::max(c.ffn_dim, 4 * d);
    WN_TRY(m->c1.ensure((size_t)M1 * F1 * C * sizeof(float)));
    WN_TRY(m->c2.ensure((size_t)M * F2 * C * sizeof(float)));
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * hid * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    FireRedFrontArgs a;
    a.feats = feats_dev; a.mean = W.cmvn_mean; a.istd = W.cmvn_istd;
    a.w1 = W.conv1_w; a.b1 = W.conv1_b; a.w2 = W.conv2.w; a.b2 = W.conv2.b;
    a.h1 = m->c1.as<float>(); a.out = m->c2.as<float>(); a.ldo = C * F2;
    a.len = m->ck_desc.as<int>();
    a.t1_off = m->d_off1.as<int>(); a.t1_len = m->d_len1.as<int>();
    a.t2_off = m->d_off.as<int>(); a.t2_len = m->d_len.as<int>();
    a.B = B; a.T = T; a.F = c.feat_dim; a.F1 = F1; a.F2 = F2; a.C = C; a.max_t2 = max_t2;
    WN_TRY(firered_frontend(a, s));
    // Linear(C * F2 -> d); no xscale, the positional encoding returns x unchanged
    WN_TRY(linear(W.sub_out, m->c2.as<float>(), C * F2, m->x.as<float>(), d, M, s));
    WN_TRY(encoder_layers_firered(m, s));
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

int wn_model_create_firered(const wn_config* cfg, const wn_firered_config* fcfg,
                            const wn_tensor* weights, int32_t n_weights, int32_t device,
                            wn_model** out) {
  WN_CHECK(fcfg, "wn_model_create_firered: null argument");
  return create_model_impl(cfg, nullptr, nullptr, fcfg, nullptr, nullptr, nullptr, weights, n_weights, device, out);
}

}  // extern "C"
