// C ABI (include/wenet_amd.h), Branchformer / E-Branchformer handles (`encoder: branchformer`,
// `encoder: e_branchformer` under an asr_model head): the entry point that creates one, and what
// wn_encode runs on it -- the Conformer front end (Conv2dSubsampling4, rel-pos encoding), then the
// layer stack of wenet/models/branchformer/encoder_layer.py or e_branchformer/encoder_layer.py
// over the packed rows of the batch, then after_norm.  A plain fp32 path built from the generic
// pieces (ln, linear with its GELU / SiLU / residual / alpha epilogues, attention with the
// rel-pos term) and the two kernels of branchformer.hip; the six-product, row-block and fused
// feed-forward routes of conformer.hip stay off: untuned.
#include "model_state.h"

// One layer.  Branchformer (kind 1): x1 = MHA(norm_mha(x)); x2 = cgMLP(norm_mlp(x));
// x += merge_proj([x1 | x2]); x = norm_final(x).  E-Branchformer (kind 2): x += 0.5 FFN_mac(LN x)
// in front, c = [x1 | x2], x += merge_proj(c + depthwise_conv_fusion(c)), x += 0.5 FFN(LN x),
// x = norm_final(x).  The attention's output projection and channel_proj2 write their halves of
// [x1 | x2] directly (ldc = 2 d): the concat is never a copy.
static int encoder_layers_branchformer(wn_model* m, int chunk, int left, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_branchformer_config& b = m->bf.c;
  const int d = c.d_model, d2 = 2 * d, H = c.n_heads, dq = H * 64, M = m->rows;
  const int U = b.cgmlp_units, C = U / 2;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* ctx = m->t2.as<float>();      // M x dq: the attention context
  float* hb = m->hbuf.as<float>();     // M x max(ffn_dim, U): FFN hidden / channel_proj1's output
  float* qkv = m->qkv.as<float>();     // M x 3 dq
  float* cat = m->bf_cat.as<float>();  // M x 2d: [x1 | x2]
  float* mrg = m->bf_mrg.as<float>();  // M x 2d: c + conv(c)
  float* gate = m->bf_gate.as<float>();   // M x C (+ M x C behind it with linear_after_conv)
  const float eps = c.norm_eps;
  int max_len = 0;
  for (int i = 0; i < m->B; ++i) max_len = std::max(max_len, m->len[i]);
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
    if (b.kind == 2) {
      WN_TRY(ln(L.norm_ff_mac, x, t1, M, d, eps, s));
      WN_TRY(linear(L.ffm1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
      WN_TRY(linear(L.ffm2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    }
    // branch 1: rel-pos attention without the shift; heads of bf.c.head_dim = 32 are laid out as
    // 64 columns with the upper 32 zero, so the d_k = 64 kernel adds exact zeros
    WN_TRY(ln(L.norm_mha, x, t1, M, d, eps, s));
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * dq, M, s));
    AttnArgs a;
    a.Q = qkv; a.K = qkv + dq; a.V = qkv + 2 * dq;
    a.ldq = a.ldk = a.ldv = 3 * dq;
    a.P = L.pos_tab; a.ldp = dq; a.bias_u = L.bias_u; a.bias_v = L.bias_v;
    a.O = ctx; a.ldo = dq;
    a.q_off = a.kv_off = m->d_off.as<int>();
    a.q_len = a.kv_len = m->d_len.as<int>();
    a.n_seq = m->B; a.n_heads = H; a.max_q_len = max_len;
    a.mask_mode = mask_mode; a.chunk_size = cs; a.left_chunks = lc;
    a.scale = 1.0f / sqrtf((float)b.head_dim);
    WN_TRY(attention(a, s));
    WN_TRY(linear(L.out, ctx, dq, cat, d2, M, s));
    // branch 2: cgMLP                                   branchformer/cgmlp.py:86-131, 161-194
    WN_TRY(ln(L.norm_mlp, x, t1, M, d, eps, s));
    WN_TRY(linear(L.proj1, t1, d, hb, U, M, s, ACT_GELU));
    DwTileArgs g;
    g.x = hb + C; g.ldx = U;         // h.chunk(2): r = columns [0, C), the gate half behind it
    g.wt = L.csgu_wt; g.bias = L.csgu_b;
    g.off = m->d_off.as<int>(); g.len = m->d_len.as<int>();
    g.B = m->B; g.C = C; g.K = b.cgmlp_kernel; g.causal = c.causal; g.max_len = max_len;
    g.ln_w = L.csgu_norm.w; g.ln_b = L.csgu_norm.b;
    g.stats = m->bf_stats.as<float2>(); g.M = M; g.eps = 1e-5f;   // nn.LayerNorm's default
    g.y = gate; g.ldy = C;
    if (b.linear_after_conv) {
      float* lin = gate + (size_t)M * C;
      WN_TRY(csgu_gate(g, s));                                    // the conv alone
      WN_TRY(linear(L.csgu_lin, gate, C, lin, C, M, s));
      WN_TRY(csgu_mul(hb, U, lin, C, gate, C, M, C, s));
    } else {
      g.r = hb; g.ldr = U;
      WN_TRY(csgu_gate(g, s));
    }
    WN_TRY(linear(L.proj2, gate, C, cat + d, d2, M, s));
    // merge
    if (b.kind == 2) {
      DwTileArgs mg;
      mg.x = cat; mg.ldx = d2; mg.wt = L.merge_wt; mg.bias = L.merge_b;
      mg.y = mrg; mg.ldy = d2;
      mg.off = g.off; mg.len = g.len;
      mg.B = m->B; mg.C = d2; mg.K = b.merge_kernel; mg.causal = c.causal; mg.max_len = max_len;
      WN_TRY(merge_dwconv(mg, s));
      WN_TRY(linear(L.merge_proj, mrg, d2, x, d, M, s, ACT_NONE, x, d));
      WN_TRY(ln(L.norm_ff, x, t1, M, d, eps, s));
      WN_TRY(linear(L.ff1, t1, d, hb, c.ffn_dim, M, s, ACT_SILU));
      WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d, 0.5f));
    } else {
      WN_TRY(linear(L.merge_proj, cat, d2, x, d, M, s, ACT_NONE, x, d));
    }
    WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  }
  return after_norm_out(m, s);
}

// wn_encode on a Branchformer handle.  The front end is the Conformer's: its row layout gives
// utterance b the (len - 7) / 4 + 1 frames the reference gives it alone.  The reference's cgMLP
// and merge convs ignore the padding mask, so in a reference batch a shorter utterance of a
// non-causal model reads the batch's subsampled padding; here the convs see the utterance's own
// frames only (deviations): alone and batched results are the same bits.
int encode_branchformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                        int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                        hipStream_t s) {
  const wn_config& c = m->cfg;
  const wn_branchformer_config& b = m->bf.c;
  const int d = c.d_model, dq = c.n_heads * 64, U = b.cgmlp_units, C = U / 2;
  const int Tp = ((T - 1) / 2 - 1) / 2;
  // the workspace the front end sizes for a Conformer (d-wide heads, ffn_dim hidden units) is
  // sized for this encoder FIRST: its own ensure() calls then find room and move nothing
  size_t M = 0;
  for (int i = 0; i < B; ++i) {
    const int L = feat_lens_host[i];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    M += L > 6 ? (size_t)((L - 7) / 4 + 1) : 0;
  }
  if (M > 0) {
    const size_t hid = (size_t)std::max(b.kind == 2 ? c.ffn_dim : 0, U);
    WN_TRY(m->t2.ensure(M * std::max(d, dq) * sizeof(float)));
    WN_TRY(m->hbuf.ensure(M * std::max(hid, (size_t)c.ffn_dim) * sizeof(float)));
    WN_TRY(m->qkv.ensure(M * 3 * dq * sizeof(float)));
    WN_TRY(m->bf_cat.ensure(M * 2 * d * sizeof(float)));
    if (b.kind == 2) WN_TRY(m->bf_mrg.ensure(M * 2 * d * sizeof(float)));
    WN_TRY(m->bf_gate.ensure(M * C * (b.linear_after_conv ? 2 : 1) * sizeof(float)));
    WN_TRY(m->bf_stats.ensure(M * sizeof(float2)));
  }
  WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, enc_lens_host, 0, s));
  WN_TRY(encode_gate_wait(m, s));     // (paths that did not consume the gate behind conv1)
  WN_CHECK((size_t)m->rows == M, "wn_encode: internal row count");
  if (M > 0) WN_TRY(encoder_layers_branchformer(m, chunk, left, s));
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

int wn_model_create_branchformer(const wn_config* cfg, const wn_branchformer_config* bcfg,
                                 const wn_tensor* weights, int32_t n_weights, int32_t device,
                                 wn_model** out) {
  WN_CHECK(bcfg, "wn_model_create_branchformer: null argument");
  return create_model_impl(cfg, nullptr, nullptr, nullptr, bcfg, nullptr, nullptr, weights, n_weights, device, out);
}

int32_t wn_csgu_time_tile(void) { return CSGU_TILE; }

}  // extern "C"
