// C ABI (include/wenet_amd.h), Efficient Conformer handles (`encoder: efficientConformer` under an
// asr_model head): the entry point that creates one, its weights, and what wn_encode runs on it
// -- the conv2d or conv2d2 front end, then the layers of
// wenet/models/efficient_conformer/encoder.py over the packed rows of the batch, with one packed
// row layout per frame rate: a stride layer maps the rows of its rate to the rows of the next.
// A plain fp32 path built from the generic pieces (ln, linear with its SiLU / GLU / residual
// epilogues, attention with the rel-pos term and chunk masks, dwconv_ln_silu) and the three
// kernels of efficonformer.hip; the six-product, row-block and fused feed-forward routes of
// conformer.hip stay off: untuned.
#include "model_state.h"
#include "weight_stage.h"

namespace {

constexpr int EF_MAX_STRIDE = 4;

// a packed row layout of one frame rate
struct EfLayout {
  int M = 0, max_len = 0;
  const int* off = nullptr; const int* len = nullptr; const int* row_utt = nullptr;
};

// stride layers in front of layer i
int ef_strides_before(const wn_efficonformer_config& e, int i) {
  int n = 0;
  for (int j = 0; j < e.n_stride; ++j) n += e.stride_layers[j] < i;
  return n;
}
bool ef_is_stride(const wn_efficonformer_config& e, int i) {
  for (int j = 0; j < e.n_stride; ++j)
    if (e.stride_layers[j] == i) return true;
  return false;
}
// cnn_module_kernels[index] of encoder.py:125-132
int ef_kernel_at(const wn_config& c, const wn_efficonformer_config& e, int index) {
  int K = c.cnn_kernel;
  for (int j = 0; j < index; ++j) K = e.stride_kernel ? K / 2 : K;
  return K;
}

}  // namespace

int efficonformer_config_check(const wn_config& c, const wn_efficonformer_config& e,
                               bool other_family) {
  WN_CHECK(!other_family, "efficonformer: an asr_model head only, no other encoder family");
  WN_CHECK(c.encoder_type == 0 && c.input_layer == 0 && c.activation == 0,
           "efficonformer: encoder_type 0, input_layer 0 (front_rate picks the front end), swish");
  WN_CHECK(e.front_rate == 4 || e.front_rate == 2,
           "efficonformer: front_rate must be 4 (conv2d) or 2 (conv2d2)");
  WN_CHECK(c.d_model == 64 || c.d_model == 128 || c.d_model == 256 || c.d_model == 512,
           "efficonformer: output_size must be 64, 128, 256 or 512");
  WN_CHECK(c.n_layers >= 1 && c.n_layers <= 31, "efficonformer: num_blocks must be in [1, 31]");
  WN_CHECK(e.head_dim == 32 || e.head_dim == 64,
           "efficonformer: output_size / attention_heads must be 32 or 64 (other head widths have "
           "no attention kernel)");
  WN_CHECK(c.n_heads > 0 && c.n_heads < 256 && c.d_model == c.n_heads * e.head_dim,
           "efficonformer: output_size must be attention_heads * head_dim");
  WN_CHECK(e.group_mask >= 0 && (c.n_layers >= 31 || e.group_mask < (1 << c.n_layers)),
           "efficonformer: group_mask names a layer behind the last one");
  WN_CHECK(e.group_mask == 0 || e.group_size * e.head_dim == 96 || e.group_size * e.head_dim == 192,
           "efficonformer: group_size * head_dim must be 96 or 192 (attention_grouped)");
  WN_CHECK(e.n_stride >= 0 && e.n_stride <= EF_MAX_STRIDE,
           "efficonformer: at most 4 stride layers");
  for (int j = 0; j < e.n_stride; ++j)
    WN_CHECK(e.stride_layers[j] >= 0 && e.stride_layers[j] < c.n_layers &&
                 (j == 0 || e.stride_layers[j] > e.stride_layers[j - 1]),
             "efficonformer: stride_layers must be ascending layer indices");
  WN_CHECK(e.stride_kernel == 0 || e.stride_kernel == 1, "efficonformer: stride_kernel is 0 or 1");
  for (int j = 0; j <= e.n_stride; ++j) {
    const int K = ef_kernel_at(c, e, j);
    WN_CHECK(K >= 1 && K <= 63 && (c.causal || K % 2 == 1),
             "efficonformer: every layer's conv kernel must be in [1, 63], odd unless causal");
  }
  WN_CHECK(c.static_chunk_size <= 0 || c.static_chunk_size % (1 << e.n_stride) == 0,
           "efficonformer: static_chunk_size must be divisible by the product of the strides");
  return 0;
}

// conv2d2 (efficient_conformer/subsampling.py:25-75): Conv2d(1, d, 3, 2) + ReLU, then
// Linear(d * F1 -> d) over the (c, f)-flattened pixels.  conv1 (d,1,3,3) -> [tap][c]; the
// projection's columns c * F1 + f -> f * d + c, the channels-last pixel order cmvn_conv1_relu writes
int efficonformer_stage_front2(const Src& src, HostStage& hs, const wn_config& c, int F1) {
  const int d = c.d_model;
  WN_GET(w0, "encoder.embed.conv.0.weight", (int64_t)d * 9);
  WN_GET(b0, "encoder.embed.conv.0.bias", d);
  float* t = hs.alloc("conv1.w", (size_t)9 * d);
  for (int ch = 0; ch < d; ++ch)
    for (int k = 0; k < 9; ++k) t[k * d + ch] = w0[ch * 9 + k];
  hs.add("conv1.b", b0, d);
  WN_GET(wo, "encoder.embed.out.0.weight", (int64_t)d * d * F1);
  WN_GET(bo, "encoder.embed.out.0.bias", d);
  t = hs.alloc("sub_out.w", (size_t)d * d * F1);
  for (int n = 0; n < d; ++n)
    for (int ch = 0; ch < d; ++ch)
      for (int f = 0; f < F1; ++f)
        t[(size_t)n * d * F1 + (size_t)f * d + ch] = wo[(size_t)n * d * F1 + (size_t)ch * F1 + f];
  hs.add("sub_out.b", bo, d);
  return 0;
}

// ConformerEncoderLayer / StrideConformerEncoderLayer (efficient_conformer/encoder_layer.py); a
// stride layer's concat_linear.* is never used by the reference's forward and is not read
int efficonformer_stage_layers(const Src& src, HostStage& hs, const wn_config& c,
                               const wn_efficonformer_config& e) {
  const int d = c.d_model, F = c.ffn_dim, H = c.n_heads, hd = e.head_dim, dq = H * 64;
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    const bool grouped = (e.group_mask >> i) & 1;
    const int K = ef_kernel_at(c, e, ef_strides_before(e, i));
    for (const char* n : {"norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    if (c.cnn_norm == 0) {
      WN_TRY(stage_norm(src, hs, p + ".conv_module.norm", d));
    } else {  // eval-mode BatchNorm1d (eps 1e-5) as a per-channel affine, in fp64
      const std::string q = p + ".conv_module.norm";
      WN_GET(bw, q + ".weight", d);
      WN_GET(bb, q + ".bias", d);
      WN_GET(bm, q + ".running_mean", d);
      WN_GET(bvar, q + ".running_var", d);
      std::vector<float> sc(d), sh(d);
      for (int ch = 0; ch < d; ++ch) {
        const double g = (double)bw[ch] / sqrt((double)bvar[ch] + 1e-5);
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
    const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
    if (grouped) {
      // Q | K | V, the table and linear_out as the reference has them: the kernel reads them
      // through pad4group's flat view; pos_bias_u / v are (h, group * d_k)
      std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d);
      for (int j = 0; j < 3; ++j) {
        WN_GET(pw, p + ".self_attn." + parts[j] + ".weight", (int64_t)d * d);
        WN_GET(pb, p + ".self_attn." + parts[j] + ".bias", d);
        memcpy(&w[(size_t)j * d * d], pw, sizeof(float) * d * d);
        memcpy(&b[(size_t)j * d], pb, sizeof(float) * d);
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
      WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
      WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_pos", d, d, false));
      WN_GET(bu, p + ".self_attn.pos_bias_u", (int64_t)e.group_size * d);
      WN_GET(bv, p + ".self_attn.pos_bias_v", (int64_t)e.group_size * d);
      hs.add(p + ".pos_bias_u", bu, (size_t)e.group_size * d);
      hs.add(p + ".pos_bias_v", bv, (size_t)e.group_size * d);
    } else {
      // H heads of 64 columns: head h's hd rows, then 64 - hd zero rows (head_dim 32: every
      // added product of the d_k = 64 attention is an exact zero, as for an E-Branchformer)
      std::vector<float> w((size_t)3 * dq * d, 0.f), bq((size_t)3 * dq, 0.f);
      for (int j = 0; j < 3; ++j) {
        WN_GET(pw, p + ".self_attn." + parts[j] + ".weight", (int64_t)d * d);
        WN_GET(pb, p + ".self_attn." + parts[j] + ".bias", d);
        for (int h = 0; h < H; ++h)
          for (int r = 0; r < hd; ++r) {
            memcpy(&w[((size_t)j * dq + h * 64 + r) * d], &pw[(size_t)(h * hd + r) * d],
                   sizeof(float) * d);
            bq[(size_t)j * dq + h * 64 + r] = pb[h * hd + r];
          }
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", bq.data(), bq.size());
      WN_GET(pp, p + ".self_attn.linear_pos.weight", (int64_t)d * d);
      WN_GET(bu, p + ".self_attn.pos_bias_u", d);
      WN_GET(bv, p + ".self_attn.pos_bias_v", d);
      std::vector<float> wp((size_t)dq * d, 0.f), u(dq, 0.f), v(dq, 0.f);
      for (int h = 0; h < H; ++h)
        for (int r = 0; r < hd; ++r) {
          memcpy(&wp[((size_t)h * 64 + r) * d], &pp[(size_t)(h * hd + r) * d], sizeof(float) * d);
          u[h * 64 + r] = bu[h * hd + r];
          v[h * 64 + r] = bv[h * hd + r];
        }
      hs.add(p + ".self_attn.linear_pos.weight", wp.data(), wp.size());
      hs.add(p + ".pos_bias_u", u.data(), u.size());
      hs.add(p + ".pos_bias_v", v.data(), v.size());
      WN_GET(po, p + ".self_attn.linear_out.weight", (int64_t)d * d);
      WN_GET(pob, p + ".self_attn.linear_out.bias", d);
      std::vector<float> wo((size_t)d * dq, 0.f);
      for (int n = 0; n < d; ++n)
        for (int h = 0; h < H; ++h)
          memcpy(&wo[(size_t)n * dq + h * 64], &po[(size_t)n * d + h * hd], sizeof(float) * hd);
      hs.add(p + ".self_attn.linear_out.weight", wo.data(), wo.size());
      hs.add(p + ".self_attn.linear_out.bias", pob, d);
    }
    {  // pointwise_conv1 (2d, d, 1): rows permuted per 64 as [32 a | 32 gate]; cpad = the GLU of
       // the bias, the frame a causal module's left padding becomes (convolution.py:117-138)
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
          cp[ch] = (float)((double)b1[ch] / (1.0 + exp(-(double)b1[d + ch])));
        }
      hs.add(p + ".pw1.weight", w.data(), w.size());
      hs.add(p + ".pw1.bias", b.data(), b.size());
      hs.add(p + ".cpad", cp.data(), cp.size());
    }
    {  // depthwise (d,1,K) -> [K][d], K this layer's own kernel
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

int efficonformer_bind(ModelData& W, const wn_config& c, const wn_efficonformer_config& e) {
  const int d = c.d_model, F = c.ffn_dim, dq = c.n_heads * 64, wmax = std::max(d, dq);
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& p, int o, int i) {
    Linear l; l.w = P(p + ".weight"); l.b = P(p + ".bias"); l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& p) {
    Norm n; n.w = P(p + ".weight"); n.b = P(p + ".bias"); return n;
  };
  W.layers.resize(c.n_layers);
  WN_TRY(W.pos_tabs.ensure((size_t)c.n_layers * c.max_pos * wmax * sizeof(float)));
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    EncLayer& L = W.layers[i];
    const int nb = ef_strides_before(e, i);
    L.ef_grouped = (e.group_mask >> i) & 1;
    L.ef_stride = ef_is_stride(e, i);
    L.ef_rate = 1 << nb;
    L.ef_kernel = ef_kernel_at(c, e, nb);
    const int wq = L.ef_grouped ? d : dq;
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
    L.qkv = LIN(p + ".qkv", 3 * wq, d);
    L.out = LIN(p + ".self_attn.linear_out", d, wq);
    L.pw1 = LIN(p + ".pw1", 2 * d, d);
    L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, d);
    L.bias_u = P(p + ".pos_bias_u");
    L.bias_v = P(p + ".pos_bias_v");
    L.pos_w = P(p + ".self_attn.linear_pos.weight");
    L.dw_wt = P(p + ".dw.weight");
    L.dw_b = P(p + ".dw.bias");
    L.cpad = P(p + ".cpad");
    // p = linear_pos(pos_emb) depends on weights only; behind stride layers pos_emb is
    // pe[0::rate] (encoder.py:287): ceil(max_pos / rate) rows of pe with a row stride of rate * d
    L.pos_tab = W.pos_tabs.as<float>() + (size_t)i * c.max_pos * wmax;
    Linear lp; lp.w = L.pos_w; lp.b = nullptr; lp.out = wq; lp.in = d;
    WN_TRY(linear(lp, W.pe, L.ef_rate * d, L.pos_tab, wq, cdiv(c.max_pos, L.ef_rate), 0));
  }
  return 0;
}

namespace {

int ef_ffn(wn_model* m, const Norm& n, const Linear& w1, const Linear& w2, float* x, int M,
           hipStream_t s) {
  const wn_config& c = m->cfg;
  float* t1 = m->t1.as<float>();
  float* hb = m->hbuf.as<float>();
  WN_TRY(ln(n, x, t1, M, c.d_model, c.norm_eps, s));
  WN_TRY(linear(w1, t1, c.d_model, hb, c.ffn_dim, M, s, ACT_SILU));
  return linear(w2, hb, c.ffn_dim, x, c.d_model, M, s, ACT_NONE, x, c.d_model, 0.5f);
}

// One layer.  `a` is the layout of the rate the layer runs at, `b` the next one (a stride layer
// only).  Pre-LN, macaron: x += FFN(LN x) / 2; x += MHA(LN x); x = R(x) + Conv(LN x), R the
// identity or the average pool; x += FFN(LN x) / 2; x = norm_final(x).  cs is the chunk size in
// frames of the front end's rate (0: full context).
int efficonformer_layer(wn_model* m, const EncLayer& L, const EfLayout& a, const EfLayout& b,
                        int cs, int lc, hipStream_t s) {
  const wn_config& c = m->cfg;
  const wn_efficonformer_config& e = m->ef.c;
  const int d = c.d_model, H = c.n_heads, dq = H * 64, M = a.M;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* qkv = m->qkv.as<float>();
  const float eps = c.norm_eps;
  WN_TRY(ef_ffn(m, L.norm_ff_mac, L.ffm1, L.ffm2, x, M, s));
  // ---- attention ----------------------------------------------------------------------
  WN_TRY(ln(L.norm_mha, x, t1, M, d, eps, s));
  if (L.ef_grouped) {
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * d, M, s));
    GroupedAttnArgs g;
    g.Q = qkv; g.K = qkv + d; g.V = qkv + 2 * d;
    g.ldq = g.ldk = g.ldv = 3 * d;
    g.P = L.pos_tab; g.ldp = d;
    g.bias_u = L.bias_u; g.bias_v = L.bias_v;
    g.O = t2; g.ldo = d;
    g.off = a.off; g.len = a.len;
    g.n_seq = m->B; g.n_heads = H; g.group = e.group_size; g.width = e.group_size * e.head_dim;
    g.D = d; g.max_len = a.max_len;
    // mask[:, ::group, ::group] of the chunk mask this rate has: every group * rate-th frame
    g.mask_step = e.group_size * L.ef_rate; g.chunk_size = cs; g.left_chunks = lc;
    g.scale = 1.0f / sqrtf((float)g.width);
    WN_TRY(attention_grouped(g, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d));
  } else {
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * dq, M, s));
    AttnArgs at;
    at.Q = qkv; at.K = qkv + dq; at.V = qkv + 2 * dq;
    at.ldq = at.ldk = at.ldv = 3 * dq;
    at.P = L.pos_tab; at.ldp = dq; at.bias_u = L.bias_u; at.bias_v = L.bias_v;
    at.O = t2; at.ldo = dq;
    at.q_off = at.kv_off = a.off;
    at.q_len = at.kv_len = a.len;
    at.n_seq = m->B; at.n_heads = H; at.max_q_len = a.max_len;
    // chunk_masks[:, ::rate, ::rate] of a chunk mask whose size the rate divides is the chunk
    // mask of size cs / rate at this rate, with the same number of left chunks
    at.mask_mode = cs > 0 ? 2 : 0; at.chunk_size = cs / L.ef_rate; at.left_chunks = lc;
    at.scale = 1.0f / sqrtf((float)e.head_dim);
    WN_TRY(attention(at, s));
    WN_TRY(linear(L.out, t2, dq, x, d, M, s, ACT_NONE, x, d));
  }
  // ---- conv module                             efficient_conformer/convolution.py:93-154
  WN_TRY(ln(L.norm_conv, x, t1, M, d, eps, s));
  WN_TRY(linear(L.pw1, t1, d, t2, d, M, s, ACT_NONE, nullptr, 0, 1.0f, true));
  int Mo = M;
  if (!L.ef_stride) {
    DwConvArgs dw;
    dw.x = t2; dw.ldx = d; dw.wt = L.dw_wt; dw.bias = L.dw_b; dw.cpad = L.cpad;
    dw.ln_w = L.conv_norm.w; dw.ln_b = L.conv_norm.b; dw.norm_mode = c.cnn_norm;
    dw.y = t1; dw.ldy = d;
    dw.row_utt = a.row_utt; dw.off = a.off; dw.len = a.len;
    dw.M = M; dw.D = d; dw.K = L.ef_kernel; dw.causal = c.causal;
    dw.t_max = 0; dw.eps = 1e-5f;
    WN_TRY(dwconv_ln_silu(dw, s));
    WN_TRY(linear(L.pw2, t1, d, x, d, M, s, ACT_NONE, x, d));
  } else {
    Mo = b.M;
    float* x2 = m->ef_x2.as<float>();
    StrideDwConvArgs sd;
    sd.x = t2; sd.ldx = d; sd.wt = L.dw_wt; sd.bias = L.dw_b;
    sd.cpad = c.causal ? L.cpad : nullptr;
    sd.ln_w = L.conv_norm.w; sd.ln_b = L.conv_norm.b; sd.norm_mode = c.cnn_norm;
    sd.y = t1; sd.ldy = d;
    sd.off = a.off; sd.len = a.len; sd.off2 = b.off;
    sd.B = m->B; sd.D = d; sd.K = L.ef_kernel; sd.causal = c.causal; sd.stride = 2;
    sd.max_len = a.max_len; sd.eps = 1e-5f;
    WN_TRY(stride_dwconv_ln_silu(sd, s));
    WN_TRY(linear(L.pw2, t1, d, x2, d, Mo, s));
    AvgPoolResidArgs ap;
    ap.x = x; ap.ldx = d; ap.z = x2; ap.ldz = d; ap.y = x2; ap.ldy = d;
    ap.off = a.off; ap.len = a.len; ap.off2 = b.off;
    ap.B = m->B; ap.C = d; ap.stride = 2; ap.max_len = a.max_len;
    WN_TRY(avgpool_residual_add(ap, s));
    // the rows of the next rate become x
    WN_HIP(hipMemcpyAsync(x, x2, (size_t)Mo * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  WN_TRY(ef_ffn(m, L.norm_ff, L.ff1, L.ff2, x, Mo, s));
  return ln(L.norm_final, x, x, Mo, d, eps, s);
}

}  // namespace

// wn_encode on an Efficient Conformer handle.  Every utterance gets the frames the reference
// gives it ALONE at every rate: the front end's own count, then ceil(len / 2) behind every stride
// layer.  In a padded reference batch the last key group of a shorter utterance mixes in the
// padding frames and the average pool folds one into an odd length's last frame (DESIGN.md,
// deviations); here alone and batched results are the same bits.
int encode_efficonformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                         int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                         hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_efficonformer_config& e = m->ef.c;
  const int d = c.d_model, dq = c.n_heads * 64, nS = e.n_stride;
  const int Tp0 = e.front_rate == 4 ? ((T - 1) / 2 - 1) / 2 : (T - 1) / 2;
  // the chunk mask of the decode-time branches of mask.py:126-198, as the Conformer path
  int cs = 0, lc = -1;
  if (c.use_dynamic_chunk) {
    if (chunk > 0) { cs = chunk; lc = left; }
  } else if (c.static_chunk_size > 0) {
    cs = c.static_chunk_size; lc = left;
  }
  WN_CHECK(cs % (1 << nS) == 0,
           "wn_encode: decoding_chunk_size (a chunk mask of size " + std::to_string(cs) +
               ") must be divisible by the product of the strides, " + std::to_string(1 << nS) +
               ": its mask behind a stride layer is no chunk window otherwise");
  WN_CHECK(Tp0 <= c.max_pos, "wn_encode: more encoder frames than position rows");
  // ---- the layouts of every rate --------------------------------------------------------
  std::vector<std::vector<int>> off(nS + 1, std::vector<int>(B)), len(nS + 1, std::vector<int>(B));
  std::vector<int> Mr(nS + 1, 0), maxl(nS + 1, 0);
  for (int i = 0; i < B; ++i) {
    const int L = feat_lens_host[i];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    int l = e.front_rate == 4 ? (L > 6 ? (L - 7) / 4 + 1 : 0) : (L > 2 ? (L - 1) / 2 : 0);
    for (int r = 0; r <= nS; ++r) {
      off[r][i] = Mr[r]; len[r][i] = l; Mr[r] += l;
      maxl[r] = std::max(maxl[r], l);
      l = (l + 1) / 2;
    }
  }
  const size_t M = (size_t)Mr[0];
  if (M > 0) {
    // sized FIRST, so that the front end's own ensure() calls find room and move nothing
    WN_TRY(m->t2.ensure(M * std::max(d, dq) * sizeof(float)));
    WN_TRY(m->hbuf.ensure(M * (size_t)c.ffn_dim * sizeof(float)));
    WN_TRY(m->qkv.ensure(M * 3 * std::max(d, dq) * sizeof(float)));
    WN_TRY(m->ef_x2.ensure(M * d * sizeof(float)));
  }
  if (e.front_rate == 4) {
    WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, nullptr, 0, s));
    WN_TRY(encode_gate_wait(m, s));     // (paths that did not consume the gate behind conv1)
  } else {
    const int F1 = m->F1();
    m->ln0_done = false;
    m->front_route = 0;
    WN_TRY(set_layout(m, B, Tp0, off[0], len[0], Mr[0], s));
    WN_TRY(m->stage.end(s));
    WN_TRY(encode_gate_wait(m, s));
    if (M > 0) {
      WN_TRY(m->c1.ensure(M * F1 * d * sizeof(float)));
      WN_TRY(m->x.ensure(M * d * sizeof(float)));
      WN_TRY(m->t1.ensure(M * d * sizeof(float)));
      Conv1Args c1;
      c1.feats = feats_dev; c1.mean = W.cmvn_mean; c1.istd = W.cmvn_istd;
      c1.w = W.conv1_w; c1.bias = W.conv1_b; c1.out = m->c1.as<float>();
      c1.t1_off = m->d_off.as<int>(); c1.t1_len = m->d_len.as<int>();
      c1.B = B; c1.T = T; c1.F = c.feat_dim; c1.F1 = F1; c1.C = d; c1.max_t1 = maxl[0];
      WN_TRY(cmvn_conv1_relu(c1, s));
      // Linear(d * F1 -> d) * sqrt(d)      efficient_conformer/subsampling.py:73, embedding.py:144
      WN_TRY(linear(W.sub_out, m->c1.as<float>(), F1 * d, m->x.as<float>(), d, (int)M, s, ACT_NONE,
                    nullptr, 0, sqrtf((float)d)));
    }
  }
  WN_CHECK((size_t)m->rows == M, "wn_encode: internal row count");
  int rate = 0;
  if (M > 0) {
    // off | len | row_utt of every rate in one block
    std::vector<int> h;
    std::vector<size_t> at(nS + 1);
    for (int r = 0; r <= nS; ++r) {
      at[r] = h.size();
      h.insert(h.end(), off[r].begin(), off[r].end());
      h.insert(h.end(), len[r].begin(), len[r].end());
      const size_t ru = h.size();
      h.resize(ru + Mr[r], -1);
      for (int i = 0; i < B; ++i)
        for (int t = 0; t < len[r][i]; ++t) h[ru + off[r][i] + t] = i;
    }
    WN_TRY(m->ef_desc.ensure(h.size() * sizeof(int)));
    WN_TRY(m->ef_stage.begin(h.size() * sizeof(int) + 256));
    WN_TRY(m->ef_stage.put_at(m->ef_desc.p, h.data(), h.size() * sizeof(int), s));
    WN_TRY(m->ef_stage.end(s));
    std::vector<EfLayout> lay(nS + 2);
    for (int r = 0; r <= nS; ++r) {
      lay[r].M = Mr[r]; lay[r].max_len = maxl[r];
      lay[r].off = m->ef_desc.as<int>() + at[r]; lay[r].len = lay[r].off + B;
      lay[r].row_utt = lay[r].off + 2 * B;
    }
    const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers) : c.n_layers;
    for (int li = 0; li < n_run; ++li) {
      const EncLayer& L = W.layers[li];
      WN_TRY(efficonformer_layer(m, L, lay[rate], lay[rate + 1], cs, lc, s));
      if (L.ef_stride) ++rate;
    }
  }
  // the handle's current batch is the rows of the rate the stack ended at
  int TpF = Tp0;
  for (int r = 0; r < rate; ++r) TpF = (TpF + 1) / 2;
  if (rate > 0 || M == 0) {
    WN_TRY(set_layout(m, B, TpF, off[rate], len[rate], Mr[rate], s));
    WN_TRY(m->stage.end(s));
  }
  if (M > 0) WN_TRY(after_norm_out(m, s));
  if (enc_lens_host)
    for (int i = 0; i < B; ++i) enc_lens_host[i] = len[rate][i];
  if (enc_out_dev) {
    if (M > 0) {
      WN_TRY(scatter_padded(m->enc.as<float>(), d, m->d_off.as<int>(), m->d_len.as<int>(), B, TpF,
                            d, enc_out_dev, s));
    } else if (TpF > 0) {
      WN_HIP(hipMemsetAsync(enc_out_dev, 0, (size_t)B * TpF * d * sizeof(float), s));
    }
  }
  return 0;
}

extern "C" {

int wn_model_create_efficonformer(const wn_config* cfg, const wn_efficonformer_config* ecfg,
                                  const wn_tensor* weights, int32_t n_weights, int32_t device,
                                  wn_model** out) {
  WN_CHECK(ecfg, "wn_model_create_efficonformer: null argument");
  return create_model_impl(cfg, nullptr, nullptr, nullptr, nullptr, nullptr, ecfg, weights,
                           n_weights, device, out);
}

}  // extern "C"
