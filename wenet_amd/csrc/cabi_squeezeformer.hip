// C ABI (include/wenet_amd.h), Squeezeformer handles (`encoder: squeezeformer` under an asr_model
// head): the entry point that creates one, and what wn_encode runs on it -- the Conformer's
// conv2d front end (the sqrt(d) scale folded behind input_proj), preln, then the blocks of
// wenet/models/squeezeformer/encoder.py over the packed rows of the batch, with the time
// reduction in front of block reduce_idx and the recovery in front of block recover_idx.  A
// plain fp32 path built from the generic pieces (ln, linear with its SiLU / GLU / residual
// epilogues, attention with the rel-pos term and chunk masks, dwconv_ln_silu) and the three
// kernels of squeezeformer.hip; the six-product, row-block and fused feed-forward routes of
// conformer.hip stay off: untuned.
#include "model_state.h"

namespace {

// a packed row layout: the full rate (the handle's own) or the half rate between the time
// reduction and the recovery
struct SqLayout {
  int M = 0, max_len = 0;
  const int* off = nullptr; const int* len = nullptr; const int* row_utt = nullptr;
};

}  // namespace

// One block = SqueezeformerEncoderLayer.forward, post-LN: x = LN1(x + MHA(x)); x = LN2(x +
// FFN1(x)); x = LN3(x + Conv(x)); x = LN4(x + FFN2(x)).  The `ada_scale * x + ada_bias` in front
// of every module is folded into the module's first Linear (cabi_model.hip).
static int squeezeformer_layer(wn_model* m, const EncLayer& L, float* x, const SqLayout& lay,
                               bool shift, int mask_mode, int cs, int lc, hipStream_t s) {
  const wn_config& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, M = lay.M;
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();
  float* qkv = m->qkv.as<float>();
  const float eps = c.norm_eps;
  // ---- attention ------------------------------------------------------------------
  WN_TRY(linear(L.qkv, x, d, qkv, 3 * d, M, s));
  if (shift) {
    SqShiftAttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.P = L.pos_tab; a.ldp = d; a.p_rows = lay.max_len;
    a.bias_u = L.bias_u; a.bias_v = L.bias_v;
    a.O = t2; a.ldo = d;
    a.off = lay.off; a.len = lay.len;
    a.n_seq = m->B; a.n_heads = H; a.max_len = lay.max_len;
    a.scale = 0.125f;
    WN_TRY(attention_sqshift(a, s));
  } else {
    AttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.P = L.pos_tab; a.ldp = d; a.bias_u = L.bias_u; a.bias_v = L.bias_v;
    a.O = t2; a.ldo = d;
    a.q_off = a.kv_off = lay.off;
    a.q_len = a.kv_len = lay.len;
    a.n_seq = m->B; a.n_heads = H; a.max_q_len = lay.max_len;
    a.mask_mode = mask_mode; a.chunk_size = cs; a.left_chunks = lc;
    a.scale = 0.125f;
    WN_TRY(attention(a, s));
  }
  WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
  WN_TRY(ln(L.norm_mha, x, x, M, d, eps, s));
  // ---- ffn1 -------------------------------------------------------------------------
  WN_TRY(linear(L.ffm1, x, d, hb, c.ffn_dim, M, s, ACT_SILU));
  WN_TRY(linear(L.ffm2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d));
  WN_TRY(ln(L.norm_ff_mac, x, x, M, d, eps, s));
  // ---- conv module                                   squeezeformer/convolution.py:121-177
  // frames behind an utterance's own last one are the depthwise conv's zero padding (t_max 0:
  // every utterance as alone); the K - 1 frames in front of a causal conv are L.cpad
  WN_TRY(linear(L.pw1, x, d, t1, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
  DwConvArgs dw;
  dw.x = t1; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
  dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = c.cnn_norm;
  dw.y = t2; dw.ldy = d;
  dw.row_utt = lay.row_utt; dw.off = lay.off; dw.len = lay.len;
  dw.M = M; dw.D = d; dw.K = c.cnn_kernel; dw.causal = c.causal;
  dw.t_max = 0; dw.eps = 1e-5f;
  WN_TRY(dwconv_ln_silu(dw, s));
  WN_TRY(linear(L.pw2, t2, d, x, d, M, s, ACT_NONE, x, d));
  WN_TRY(ln(L.norm_conv, x, x, M, d, eps, s));
  // ---- ffn2 -------------------------------------------------------------------------
  WN_TRY(linear(L.ff1, x, d, hb, c.ffn_dim, M, s, ACT_SILU));
  WN_TRY(linear(L.ff2, hb, c.ffn_dim, x, d, M, s, ACT_NONE, x, d));
  WN_TRY(ln(L.norm_final, x, x, M, d, eps, s));
  return 0;
}

static int encoder_layers_squeezeformer(wn_model* m, int mask_mode, int cs, int lc,
                                        const SqLayout& full, const SqLayout& half,
                                        hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_squeezeformer_config& q = m->sq.c;
  const int d = c.d_model;
  float* x = m->x.as<float>();
  float* xh = m->sq_xh.as<float>();
  float* t1 = m->t1.as<float>();
  const bool shift = q.do_rel_shift != 0;
  WN_TRY(ln(W.sq_preln, x, x, full.M, d, 1e-5f, s));
  const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers) : c.n_layers;
  bool reduced = false;
  for (int li = 0; li < n_run; ++li) {
    if (li == q.reduce_idx) {
      // x stays as it is until the recovery (the skip tensor); the blocks in between run on xh
      TimeReduceArgs r;
      r.x = x; r.ldx = d; r.wt = W.sq_red_wt; r.bias = W.sq_red_b; r.y = t1; r.ldy = d;
      r.off = full.off; r.len = full.len; r.off2 = half.off;
      r.B = m->B; r.C = d; r.K = q.reduce_kernel; r.pad = q.reduce_kernel == 5 ? 3 : 0;
      r.max_len = full.max_len;
      WN_TRY(time_reduce_dwconv(r, s));
      WN_TRY(linear(W.sq_red_pw, t1, d, xh, d, half.M, s));
      reduced = true;
    }
    if (li == q.recover_idx) {
      WN_TRY(linear(W.sq_recover, xh, d, t1, d, half.M, s));
      TimeRecoverArgs r;
      r.skip = x; r.lds = d; r.z = t1; r.ldz = d; r.y = x; r.ldy = d;
      r.off = full.off; r.len = full.len; r.off2 = half.off;
      r.B = m->B; r.C = d; r.max_len = full.max_len;
      WN_TRY(time_recover_add(r, s));
      reduced = false;
    }
    // mask[:, ::2, ::2] of a chunk mask of even size cs is the chunk mask of size cs / 2 at the
    // half rate, with the same number of left chunks
    if (reduced)
      WN_TRY(squeezeformer_layer(m, W.layers[li], xh, half, shift, mask_mode, cs / 2, lc, s));
    else
      WN_TRY(squeezeformer_layer(m, W.layers[li], x, full, shift, mask_mode, cs, lc, s));
  }
  // (no after_norm; a debug run cut between the reduction and the recovery returns the skip)
  WN_TRY(m->enc.ensure((size_t)std::max(full.M, 1) * d * sizeof(float)));
  WN_HIP(hipMemcpyAsync(m->enc.p, m->x.p, (size_t)full.M * d * sizeof(float),
                        hipMemcpyDeviceToDevice, s));
  return 0;
}

// wn_encode on a Squeezeformer handle.  The front end's row layout gives utterance b the
// (len - 7) / 4 + 1 frames the reference gives it ALONE; the reference's batched mask
// x_mask[:, :, :-2:2][:, :, :-2:2] counts one frame more for every utterance shorter than the
// batch's longest, and its shift wraps at the padded length (deviations).
int encode_squeezeformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                         int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                         hipStream_t s) {
  const wn_config& c = m->cfg;
  const wn_squeezeformer_config& q = m->sq.c;
  const int d = c.d_model;
  const int Tp = ((T - 1) / 2 - 1) / 2;
  // the chunk mask of the decode-time branches of mask.py:126-198, as the Conformer path
  int mask_mode = 0, cs = 0, lc = -1;
  if (c.use_dynamic_chunk) {
    if (chunk > 0) { mask_mode = 2; cs = chunk; lc = left; }
  } else if (c.static_chunk_size > 0) {
    mask_mode = 2; cs = c.static_chunk_size; lc = left;
  }
  WN_CHECK(!(mask_mode == 2 && q.do_rel_shift),
           "wn_encode: decoding_chunk_size > 0 on a Squeezeformer with do_rel_shift (the shift "
           "kernel is full context only)");
  WN_CHECK(!(mask_mode == 2 && q.reduce_idx >= 0 && cs % 2 != 0),
           "wn_encode: an odd decoding_chunk_size on a Squeezeformer with a time reduction (its "
           "mask at the half rate is no chunk window)");
  WN_CHECK(Tp <= c.max_pos, "wn_encode: more encoder frames than position rows");
  size_t M = 0;
  for (int i = 0; i < B; ++i) {
    const int L = feat_lens_host[i];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    M += L > 6 ? (size_t)((L - 7) / 4 + 1) : 0;
  }
  if (M > 0) {
    // sized FIRST, so that the front end's own ensure() calls find room and move nothing
    WN_TRY(m->t2.ensure(M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure(M * (size_t)c.ffn_dim * sizeof(float)));
    WN_TRY(m->qkv.ensure(M * 3 * d * sizeof(float)));
    WN_TRY(m->sq_xh.ensure(M * d * sizeof(float)));
  }
  WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, enc_lens_host, 0, s));
  WN_TRY(encode_gate_wait(m, s));     // (paths that did not consume the gate behind conv1)
  WN_CHECK((size_t)m->rows == M, "wn_encode: internal row count");
  if (M > 0) {
    SqLayout full, half;
    full.M = m->rows;
    full.off = m->d_off.as<int>(); full.len = m->d_len.as<int>();
    full.row_utt = m->d_row_utt.as<int>();
    for (int i = 0; i < B; ++i) full.max_len = std::max(full.max_len, m->len[i]);
    if (q.reduce_idx >= 0) {
      // the half-rate layout: off | len | row_utt in one block
      std::vector<int> h((size_t)2 * B);
      int M2 = 0;
      for (int i = 0; i < B; ++i) {
        const int l2 = (m->len[i] + 1) / 2;
        h[i] = M2; h[B + i] = l2; M2 += l2;
      }
      h.resize((size_t)2 * B + M2, -1);
      for (int i = 0; i < B; ++i)
        for (int t = 0; t < h[B + i]; ++t) h[(size_t)2 * B + h[i] + t] = i;
      WN_TRY(m->sq_desc.ensure(h.size() * sizeof(int)));
      WN_TRY(m->sq_stage.begin(h.size() * sizeof(int) + 256));
      WN_TRY(m->sq_stage.put_at(m->sq_desc.p, h.data(), h.size() * sizeof(int), s));
      WN_TRY(m->sq_stage.end(s));
      half.M = M2; half.max_len = (full.max_len + 1) / 2;
      half.off = m->sq_desc.as<int>(); half.len = half.off + B; half.row_utt = half.off + 2 * B;
    }
    WN_TRY(encoder_layers_squeezeformer(m, mask_mode, cs, lc, full, half, s));
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

int wn_model_create_squeezeformer(const wn_config* cfg, const wn_squeezeformer_config* qcfg,
                                  const wn_tensor* weights, int32_t n_weights, int32_t device,
                                  wn_model** out) {
  WN_CHECK(qcfg, "wn_model_create_squeezeformer: null argument");
  return create_model_impl(cfg, nullptr, nullptr, nullptr, nullptr, qcfg, nullptr, weights,
                           n_weights, device, out);
}

}  // extern "C"
