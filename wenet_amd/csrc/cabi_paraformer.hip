// C ABI (include/wenet_amd.h), Paraformer handles (`model: paraformer`, wenet/models/paraformer/):
// the entry point that creates one, what wn_encode runs on it (the LFR front end and the SANM
// encoder stack), wn_paraformer_decode (CIF predictor + SANM decoder stack on the handle's
// current batch), and the operator hooks of the kernels (attention_d128.hip, paraformer.hip).  A
// plain fp32 path built from the generic pieces (ln, linear with its ReLU / residual epilogues,
// merge_dwconv as the FSMN block); the six-product, row-block and fused-FFN routes stay off.
// In the hooks offsets and lengths are HOST arrays, checked against the caller's buffers BEFORE
// anything is launched: every loop bound of a kernel comes from a length validated on the host.
#include "model_state.h"
#include "weight_stage.h"

namespace wn {
namespace {

int pf_upload_ints(DevBuf& buf, const std::vector<int>& v, hipStream_t s) {
  WN_TRY(buf.ensure(std::max<size_t>(v.size(), 4) * sizeof(int)));
  WN_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

// offsets / lengths of a packed ragged batch: inside [0, rows), ascending, disjoint
bool pf_packed_ok(const int32_t* off, const int32_t* len, int n, int rows) {
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {
    if (len[i] < 0 || off[i] < end || (int64_t)off[i] + len[i] > rows) return false;
    end = (int64_t)off[i] + len[i];
  }
  return true;
}

// off | len | row_utt of a packed batch on the device
int pf_layout(const int32_t* off, const int32_t* len, int n, int rows, DevBuf& desc,
              hipStream_t s) {
  std::vector<int> h((size_t)2 * n + rows, -1);
  for (int i = 0; i < n; ++i) {
    h[i] = off[i]; h[n + i] = len[i];
    for (int t = 0; t < len[i]; ++t) h[2 * n + off[i] + t] = i;
  }
  return pf_upload_ints(desc, h, s);
}

// fsmn_block.weight (d, 1, K) -> [K][d] tap-major (merge_dwconv)
int pf_stage_fsmn(const Src& src, HostStage& hs, const std::string& p, int d, int K) {
  WN_GET(w, p + ".fsmn_block.weight", (int64_t)d * K);
  float* t = hs.alloc(p + ".fsmn", (size_t)K * d);
  for (int ch = 0; ch < d; ++ch)
    for (int k = 0; k < K; ++k) t[(size_t)k * d + ch] = w[(size_t)ch * K + k];
  return 0;
}

// attention of either head width: d_k = 128 on attention_d128, d_k = 64 on the existing kernel
int pf_attention(const wn_model* m, AttnArgs& a, hipStream_t s) {
  const int dk = m->cfg.d_model / a.n_heads;
  a.mask_mode = 0;
  a.scale = 1.0f / sqrtf((float)dk);   // (the decoder scales q by d_k^-0.5 before the product:
                                       // one rounding placed differently, inside the tolerance)
  return dk == 128 ? attention_d128(a, s) : attention(a, s);
}

// y = x + conv_K(x) [+ r]: the FSMN memory block over the C channels at x (zero padding, no bias)
int pf_fsmn(const wn_model* m, int K, const float* x, int ldx, const float* wt, const float* r,
            int ldr, float* y, const int* off, const int* len, int B, int max_len, hipStream_t s) {
  DwTileArgs a;
  a.x = x; a.ldx = ldx; a.wt = wt; a.bias = m->data->pf.zero_bias; a.y = y;
  a.ldy = m->cfg.d_model; a.off = off; a.len = len; a.B = B; a.C = m->cfg.d_model;
  a.K = K; a.causal = 0; a.max_len = max_len;
  a.r = r; a.ldr = ldr;
  return merge_dwconv(a, s);
}

// w_2(LayerNorm_F(relu(w_1 x))): PositionwiseFeedForwardDecoderSANM (layers.py:95-123)
int pf_dec_ffn(wn_model* m, const Linear& w1, const Norm& nrm, const Linear& w2, const float* x,
               float* y, int M, hipStream_t s) {
  const int d = m->cfg.d_model, F = m->cfg.dec_ffn_dim;
  float* h = m->pf_h.as<float>();
  WN_TRY(linear(w1, x, d, h, F, M, s, ACT_RELU));
  WN_TRY(layernorm_wide(h, F, nrm.w, nrm.b, h, F, M, F, F, 1e-5f, s));
  return linear(w2, h, F, y, d, M, s);
}

}  // namespace
}  // namespace wn

// The layer loop of both SANM stacks (the Paraformer's encoder, SenseVoice's two stacks): the
// workspace rows m->x / t1 / t2 / hbuf / qkv are sized by the caller.
int pf_encoder_layers(wn_model* m, const std::vector<PfEncLayer>& layers, int n_run,
                      bool first_wide, int ld0, int K, int B, int M, int max_len, hipStream_t s) {
  const wn_config& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, F = c.ffn_dim;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();
  float* qkv = m->qkv.as<float>();
  const int* d_off = m->d_off.as<int>();
  const int* d_len = m->d_len.as<int>();
  for (int li = 0; li < n_run; ++li) {
    // AliParaformerEncoderLayer.forward (layers.py:144-180): x1 = [x +] linear_out(attention)
    // + fsmn(v); out = x1 + w_2(relu(w_1(LN(x1)))).  A wide first layer reads the 560 (576)
    // columns the front end normalised and has no residual around the attention.
    const PfEncLayer& L = layers[li];
    const bool wide = first_wide && li == 0;
    if (!wide) WN_TRY(ln(L.n1, x, t1, M, d, c.norm_eps, s));
    WN_TRY(linear(L.qkv, t1, wide ? ld0 : d, qkv, 3 * d, M, s));
    AttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.O = t2; a.ldo = d;
    a.q_off = a.kv_off = d_off; a.q_len = a.kv_len = d_len;
    a.n_seq = B; a.n_heads = H; a.max_q_len = max_len;
    WN_TRY(pf_attention(m, a, s));
    // t1 = v + conv(v) [+ x], then x = t1 + linear_out(t2)
    WN_TRY(pf_fsmn(m, K, qkv + 2 * d, 3 * d, L.fsmn_wt, wide ? nullptr : x, d, t1, d_off, d_len,
                   B, max_len, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, t1, d));
    WN_TRY(ln(L.n2, x, t1, M, d, c.norm_eps, s));
    WN_TRY(linear(L.ff1, t1, d, hb, F, M, s, ACT_RELU));
    WN_TRY(linear(L.ff2, hb, F, x, d, M, s, ACT_NONE, x, d));
  }
  return 0;
}

// wn_encode on a Paraformer handle.  Every utterance is encoded as the reference encodes it
// ALONE: T' = ceil(len / 6) rows whose frame indices clamp to the utterance's own last frame --
// the reference's batched LFR pads a shorter utterance from the batch's zero padding when the
// longest one needs no right padding (deviations).
int encode_paraformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                      int T, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_paraformer_config& p = m->pf.c;
  const int d = c.d_model, F = c.ffn_dim, D0 = p.lfr_m * c.feat_dim;
  const int ld0 = cdiv(D0, 32) * 32;
  auto out_len = [&](int n) { return n > 0 ? (n + p.lfr_n - 1) / p.lfr_n : 0; };
  const int Tp = out_len(T);
  WN_CHECK(B < 32768, "wn_encode: more than 32767 utterances");
  WN_CHECK(Tp <= p.max_frames,
           "wn_encode: an utterance of " + std::to_string(T) + " frames gives " +
               std::to_string(Tp) + " encoder frames, more than the " +
               std::to_string(p.max_frames) + " the position rows of this handle cover");
  std::vector<int> off(B), len(B), flen(B);
  int M = 0, max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    flen[b] = L;
    off[b] = M; len[b] = out_len(L); M += len[b];
    max_len = std::max(max_len, len[b]);
    if (enc_lens_host) enc_lens_host[b] = len[b];
  }
  WN_TRY(set_layout(m, B, Tp, off, len, M, s));
  if (M > 0) WN_TRY(upload_desc(m, m->ck_desc, flen, s));
  WN_TRY(m->stage.end(s));
  if (M > 0) {
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * std::max(d, ld0) * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * F * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    float* t1 = m->t1.as<float>();
    const int* d_off = m->d_off.as<int>();
    LfrFrontArgs fa;
    fa.feats = feats_dev; fa.mean = W.cmvn_mean; fa.istd = W.cmvn_istd; fa.pe = W.pf.pe;
    fa.ln_w = W.pf.enc[0].n1.w; fa.ln_b = W.pf.enc[0].n1.b;
    fa.out = t1; fa.ldo = ld0; fa.len = m->ck_desc.as<int>(); fa.off = d_off;
    fa.B = B; fa.T = T; fa.F = c.feat_dim; fa.m = p.lfr_m; fa.n = p.lfr_n; fa.max_rows = max_len;
    fa.xscale = sqrtf((float)d); fa.eps = c.norm_eps;
    WN_TRY(lfr_front(fa, s));
    const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers) : c.n_layers;
    WN_TRY(pf_encoder_layers(m, W.pf.enc, n_run, true, ld0, p.kernel_size, B, M, max_len, s));
    WN_TRY(after_norm_out(m, s));
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

int wn_model_create_paraformer(const wn_config* cfg, const wn_paraformer_config* pcfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out) {
  WN_CHECK(cfg && pcfg && weights && out, "wn_model_create_paraformer: null argument");
  const wn_config& c = *cfg;
  const wn_paraformer_config& p = *pcfg;
  const int d = c.d_model, H = c.n_heads, F = c.ffn_dim, V = c.vocab, K = p.kernel_size;
  WN_CHECK(H > 0 && H < 256 && (d == H * 64 || d == H * 128),
           "paraformer: d_model / attention_heads must be 64 or 128");
  WN_CHECK(c.dec_heads == H, "paraformer: the decoder has the encoder's attention_heads");
  WN_CHECK(d % 64 == 0 && d <= CIF_MAX_D && d <= 1280, "paraformer: d_model % 64, at most 1024");
  WN_CHECK(F > 0 && F % 32 == 0 && c.dec_ffn_dim > 0 && c.dec_ffn_dim % 32 == 0 &&
               c.dec_ffn_dim <= 2048,
           "paraformer: linear_units % 32, the decoder's at most 2048");
  WN_CHECK(c.n_layers >= 1 && p.dec_blocks >= 1, "paraformer: num_blocks");
  WN_CHECK(p.lfr_m >= 1 && p.lfr_n >= 1 && c.feat_dim >= 1 && p.lfr_m * c.feat_dim <= LFR_MAX_D &&
               (p.lfr_m * c.feat_dim) % 4 == 0,
           "paraformer: lfr_m * input_dim at most 576");
  WN_CHECK(K >= 1 && K <= CSGU_MAX_K && K % 2 == 1, "paraformer: kernel_size odd, in [1, 63]");
  WN_CHECK(p.max_frames >= 1 && p.max_frames <= 8192, "paraformer: max_frames in [1, 8192]");
  WN_CHECK(p.threshold == 1.0f, "paraformer: predictor_conf.threshold must be 1.0");
  WN_CHECK(p.tail_threshold > 0.f && p.tail_threshold < 1.0f,
           "paraformer: predictor_conf.tail_threshold must be in (0, 1)");
  WN_CHECK(p.smooth_factor > 0.f && p.smooth_factor <= 1.0f && p.noise_threshold >= 0.f,
           "paraformer: smooth_factor in (0, 1] and noise_threshold >= 0 (every alpha <= 1: at "
           "most one fire per frame)");
  WN_CHECK(V >= 1 && c.norm_eps > 0.f, "paraformer: vocab / norm_eps");
  WN_HIP(hipSetDevice(device));
  std::unique_ptr<wn_model> m(new wn_model());
  m->cfg = c;
  m->device = device;
  m->pf.on = true; m->pf.c = p;
  const std::shared_ptr<ModelData> data = std::make_shared<ModelData>();
  m->data = data;
  ModelData& W = *data;
  Src src;
  for (int i = 0; i < n_weights; ++i) src.t[weights[i].name] = {weights[i].data, weights[i].numel};
  const int D0 = p.lfr_m * c.feat_dim, ld0 = cdiv(D0, 32) * 32;
  HostStage hs;
  if (c.has_cmvn) {
    WN_GET(mean, "encoder.global_cmvn.mean", D0);
    WN_GET(istd, "encoder.global_cmvn.istd", D0);
    hs.add("cmvn.mean", mean, D0);
    hs.add("cmvn.istd", istd, D0);
  }
  const FbankTables fbt = make_fbank_tables(c.feat_dim);
  stage_fbank_tables(fbt, hs, W);
  {  // WhisperPositionalEncoding of depth D0 (transformer/embedding.py:150-164), rebuilt in fp64:
     // [sin | cos] halves over D0 / 2 timescales; row p = position p
    float* t = hs.alloc("pf.pe", (size_t)(p.max_frames + 1) * D0);
    const int half = D0 / 2;
    const double inc = log(10000.0) / (double)(half - 1);
    for (int pos = 0; pos <= p.max_frames; ++pos)
      for (int i = 0; i < half; ++i) {
        const double st = (double)pos * exp(-inc * (double)i);
        t[(size_t)pos * D0 + i] = (float)sin(st);
        t[(size_t)pos * D0 + half + i] = (float)cos(st);
      }
  }
  hs.alloc("pf.zero_bias", d);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string q = i == 0 ? "encoder.encoders0.0" : "encoder.encoders." + std::to_string(i - 1);
    const int in = i == 0 ? D0 : d;
    WN_TRY(stage_norm(src, hs, q + ".norm1", in));
    WN_TRY(stage_norm(src, hs, q + ".norm2", d));
    if (i == 0) {   // K = 560 -> 576 with zero columns: the fp32 GEMM needs K % 32 == 0
      WN_GET(w, q + ".self_attn.linear_q_k_v.weight", (int64_t)3 * d * D0);
      WN_GET(b, q + ".self_attn.linear_q_k_v.bias", 3 * d);
      float* t = hs.alloc(q + ".self_attn.linear_q_k_v.weight", (size_t)3 * d * ld0);
      for (int o = 0; o < 3 * d; ++o) memcpy(t + (size_t)o * ld0, w + (size_t)o * D0, sizeof(float) * D0);
      hs.add(q + ".self_attn.linear_q_k_v.bias", b, 3 * d);
    } else {
      WN_TRY(stage_linear(src, hs, q + ".self_attn.linear_q_k_v", 3 * d, d));
    }
    WN_TRY(pf_stage_fsmn(src, hs, q + ".self_attn", d, K));
    WN_TRY(stage_linear(src, hs, q + ".self_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_1", F, d));
    WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_2", d, F));
  }
  WN_TRY(stage_norm(src, hs, "encoder.after_norm", d));
  const bool has_ctc = src.has("ctc.ctc_lo.weight");
  if (has_ctc) WN_TRY(stage_linear(src, hs, "ctc.ctc_lo", V, d));
  {  // Cif (cif.py:41-47): Conv1d(d, d, 3) dense -> [d][tap * d + c_in]; Linear(d, 1)
    WN_GET(w, "predictor.predictor.cif_conv1d.weight", (int64_t)d * d * 3);
    WN_GET(b, "predictor.predictor.cif_conv1d.bias", d);
    float* t = hs.alloc("pf.cif_conv.weight", (size_t)d * 3 * d);
    for (int o = 0; o < d; ++o)
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < 3; ++k)
          t[(size_t)o * 3 * d + (size_t)k * d + ch] = w[((size_t)o * d + ch) * 3 + k];
    hs.add("pf.cif_conv.bias", b, d);
    WN_TRY(stage_linear(src, hs, "predictor.predictor.cif_output", 1, d));
  }
  const int Fd = c.dec_ffn_dim;
  for (int j = 0; j <= p.dec_blocks; ++j) {     // the last round: decoders3.0
    const bool d3 = j == p.dec_blocks;
    const std::string q = d3 ? "decoder.decoders3.0" : "decoder.decoders." + std::to_string(j);
    WN_TRY(stage_norm(src, hs, q + ".norm1", d));
    WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_1", Fd, d));
    WN_TRY(stage_norm(src, hs, q + ".feed_forward.norm", Fd));
    WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_2", d, Fd, false));
    if (d3) break;
    WN_TRY(stage_norm(src, hs, q + ".norm2", d));
    WN_TRY(stage_norm(src, hs, q + ".norm3", d));
    WN_TRY(pf_stage_fsmn(src, hs, q + ".self_attn", d, K));
    WN_TRY(stage_linear(src, hs, q + ".src_attn.linear_q", d, d));
    WN_TRY(stage_linear(src, hs, q + ".src_attn.linear_k_v", 2 * d, d));
    WN_TRY(stage_linear(src, hs, q + ".src_attn.linear_out", d, d));
  }
  WN_TRY(stage_norm(src, hs, "decoder.after_norm", d));
  {  // output_layer with its bias padded to a multiple of 4 columns (vocab_linear's pitch)
    WN_GET(w, "decoder.output_layer.weight", (int64_t)V * d);
    WN_GET(b, "decoder.output_layer.bias", V);
    hs.add("decoder.output_layer.weight", w, (size_t)V * d);
    memcpy(hs.alloc("decoder.output_layer.bias", (size_t)(V + 3) / 4 * 4), b, sizeof(float) * V);
  }
  // ---- upload -------------------------------------------------------------------------------
  WN_TRY(W.weights.ensure(hs.data.size() * sizeof(float)));
  W.n_weight_elems = (int64_t)hs.data.size();
  WN_HIP(hipMemcpy(W.weights.p, hs.data.data(), hs.data.size() * sizeof(float),
                   hipMemcpyHostToDevice));
  const float* base = W.weights.as<float>();
  for (auto& kv : hs.at) W.w[kv.first] = base + kv.second.first;
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& q, int o, int i, bool bias = true) {
    Linear l; l.w = P(q + ".weight"); l.b = bias ? P(q + ".bias") : nullptr;
    l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& q) {
    Norm n; n.w = P(q + ".weight"); n.b = P(q + ".bias"); return n;
  };
  if (c.has_cmvn) { W.cmvn_mean = P("cmvn.mean"); W.cmvn_istd = P("cmvn.istd"); }
  WN_TRY(bind_fbank_tables(fbt, W));
  W.after_norm = NORM("encoder.after_norm");
  if (has_ctc) W.ctc = LIN("ctc.ctc_lo", V, d);
  PfData& pf = W.pf;
  pf.pe = P("pf.pe");
  pf.zero_bias = P("pf.zero_bias");
  pf.enc.resize(c.n_layers);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string q = i == 0 ? "encoder.encoders0.0" : "encoder.encoders." + std::to_string(i - 1);
    PfEncLayer& L = pf.enc[i];
    L.n1 = NORM(q + ".norm1"); L.n2 = NORM(q + ".norm2");
    L.qkv = LIN(q + ".self_attn.linear_q_k_v", 3 * d, i == 0 ? ld0 : d);
    L.out = LIN(q + ".self_attn.linear_out", d, d);
    L.ff1 = LIN(q + ".feed_forward.w_1", F, d);
    L.ff2 = LIN(q + ".feed_forward.w_2", d, F);
    L.fsmn_wt = P(q + ".self_attn.fsmn");
  }
  pf.cif_conv = LIN("pf.cif_conv", d, 3 * d);
  pf.cif_out_w = P("predictor.predictor.cif_output.weight");
  pf.cif_out_b = P("predictor.predictor.cif_output.bias");
  pf.dec.resize(p.dec_blocks);
  for (int j = 0; j < p.dec_blocks; ++j) {
    const std::string q = "decoder.decoders." + std::to_string(j);
    PfDecLayer& L = pf.dec[j];
    L.n1 = NORM(q + ".norm1"); L.n2 = NORM(q + ".norm2"); L.n3 = NORM(q + ".norm3");
    L.ffn_norm = NORM(q + ".feed_forward.norm");
    L.ff1 = LIN(q + ".feed_forward.w_1", Fd, d);
    L.ff2 = LIN(q + ".feed_forward.w_2", d, Fd, false);
    L.src_q = LIN(q + ".src_attn.linear_q", d, d);
    L.src_kv = LIN(q + ".src_attn.linear_k_v", 2 * d, d);
    L.src_out = LIN(q + ".src_attn.linear_out", d, d);
    L.fsmn_wt = P(q + ".self_attn.fsmn");
  }
  pf.dec3_n1 = NORM("decoder.decoders3.0.norm1");
  pf.dec3_ffn_norm = NORM("decoder.decoders3.0.feed_forward.norm");
  pf.dec3_ff1 = LIN("decoder.decoders3.0.feed_forward.w_1", Fd, d);
  pf.dec3_ff2 = LIN("decoder.decoders3.0.feed_forward.w_2", d, Fd, false);
  pf.dec_after = NORM("decoder.after_norm");
  pf.dec_out = LIN("decoder.output_layer", V, d);
  // (the plain fp32 path: no six-product / row-block images, as for FireRed and the Branchformers)
  WN_HIP(hipDeviceSynchronize());
  *out = m.release();
  return 0;
}

int wn_paraformer_decode(wn_model* m, int32_t* tokens, int32_t* tok_lens, float* logp,
                         int32_t* fire_frames, int32_t* n_fire, int32_t max_tok, void* stream) {
  WN_CHECK(m && tokens && tok_lens && logp, "wn_paraformer_decode: null argument");
  WN_ENTER(m);
  WN_CHECK(m->pf.on, "wn_paraformer_decode: not a Paraformer handle");
  PrecisionScope prec_scope(m);
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_paraformer_config& p = m->pf.c;
  const int B = m->B, M = m->rows, d = c.d_model, H = c.n_heads, V = c.vocab;
  WN_CHECK(B > 0, "wn_paraformer_decode: no current batch (wn_encode first)");
  // (max_tok is the pitch of the caller's arrays: any value that holds the token numbers)
  WN_CHECK(max_tok >= 1, "wn_paraformer_decode: max_tok must be at least 1");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  for (int b = 0; b < B; ++b) tok_lens[b] = 0;
  if (n_fire) for (int b = 0; b < B; ++b) n_fire[b] = 0;
  if (M == 0) return 0;
  const float* enc = m->enc.as<float>();
  const int* d_off = m->d_off.as<int>();
  const int* d_len = m->d_len.as<int>();
  // ---- predictor: alphas, then the scan with room for len + 1 embeddings per utterance -------
  std::vector<int> emb_off(B), emb_cap(B);
  int E = 0;
  for (int b = 0; b < B; ++b) {
    emb_off[b] = E;
    emb_cap[b] = m->len[b] > 0 ? m->len[b] + 1 : 0;
    E += emb_cap[b];
  }
  WN_TRY(m->pf_alpha.ensure((size_t)M * sizeof(float)));
  WN_TRY(m->pf_img.ensure((size_t)M * 3 * d * sizeof(float)));
  WN_TRY(m->pf_emb.ensure((size_t)E * d * sizeof(float)));
  WN_TRY(m->pf_int.ensure(((size_t)E + 6 * B) * sizeof(int)));
  WN_TRY(m->t1.ensure((size_t)M * d * sizeof(float)));
  int* ints = m->pf_int.as<int>();
  int* dev_emb_off = ints; int* dev_emb_cap = ints + B;
  int* dev_n_fire = ints + 2 * B; int* dev_tok = ints + 3 * B;
  int* dev_fire_t = ints + 6 * B;
  WN_TRY(m->stage.begin((size_t)16 * B * sizeof(int) + 65536));
  WN_TRY(m->stage.put_at(dev_emb_off, emb_off.data(), B * sizeof(int), s));
  WN_TRY(m->stage.put_at(dev_emb_cap, emb_cap.data(), B * sizeof(int), s));
  WN_TRY(m->stage.end(s));
  WN_TRY(cif_stage3(enc, d, m->pf_img.as<float>(), m->d_row_utt.as<int>(), d_off, d_len, M, d, s));
  WN_TRY(linear(W.pf.cif_conv, m->pf_img.as<float>(), 3 * d, m->t1.as<float>(), d, M, s, ACT_RELU));
  WN_TRY(cif_alpha_rows(m->t1.as<float>(), d, W.pf.cif_out_w, W.pf.cif_out_b, p.smooth_factor,
                        p.noise_threshold, m->pf_alpha.as<float>(), m->d_row_utt.as<int>(), M, d,
                        s));
  CifFireArgs fa;
  fa.h = enc; fa.ldh = d; fa.alpha = m->pf_alpha.as<float>();
  fa.off = d_off; fa.len = d_len; fa.emb_off = dev_emb_off; fa.emb_cap = dev_emb_cap;
  fa.emb = m->pf_emb.as<float>(); fa.lde = d;
  fa.fire_t = dev_fire_t; fa.n_fire = dev_n_fire; fa.token_num = dev_tok;
  fa.B = B; fa.d = d; fa.tail = p.tail_threshold;
  WN_TRY(cif_fire(fa, s));
  // the decoder's row layout depends on the token numbers: one small copy back
  WN_TRY(m->pf_host.ensure(((size_t)2 * B + E) * sizeof(int) + (size_t)E * 2 * sizeof(float)));
  int* h_nfire = reinterpret_cast<int*>(m->pf_host.p);
  int* h_tok = h_nfire + B;
  int* h_fire_t = h_tok + B;
  WN_HIP(hipMemcpyAsync(h_nfire, dev_n_fire, (size_t)2 * B * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(h_fire_t, dev_fire_t, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  std::vector<int> t_off(B), t_len(B);
  int Mt = 0, max_t = 0;
  for (int b = 0; b < B; ++b) {
    const int n = m->len[b] > 0 ? std::max(0, std::min(h_tok[b], emb_cap[b])) : 0;
    WN_CHECK(n <= max_tok, "wn_paraformer_decode: max_tok is smaller than a token number");
    t_off[b] = Mt; t_len[b] = n; Mt += n;
    max_t = std::max(max_t, n);
    tok_lens[b] = n;
    if (n_fire) n_fire[b] = m->len[b] > 0 ? h_nfire[b] : 0;
    if (fire_frames)
      for (int i = 0; i < n; ++i) fire_frames[(size_t)b * max_tok + i] = h_fire_t[emb_off[b] + i];
  }
  if (Mt == 0) return 0;
  // ---- decoder over the packed token rows -------------------------------------------------------
  const int Fd = c.dec_ffn_dim, V4 = (V + 3) / 4 * 4;
  WN_TRY(m->pf_x.ensure((size_t)Mt * d * sizeof(float)));
  WN_TRY(m->pf_y.ensure((size_t)Mt * d * sizeof(float)));
  WN_TRY(m->pf_t.ensure((size_t)Mt * d * sizeof(float)));
  WN_TRY(m->pf_o.ensure((size_t)Mt * d * sizeof(float)));
  WN_TRY(m->pf_q.ensure((size_t)Mt * d * sizeof(float)));
  WN_TRY(m->pf_h.ensure((size_t)Mt * Fd * sizeof(float)));
  WN_TRY(m->pf_kv.ensure((size_t)M * 2 * d * sizeof(float)));
  WN_TRY(m->pf_out.ensure((size_t)Mt * (V4 + 2) * sizeof(float)));
  int* dev_t_off = ints + 4 * B; int* dev_t_len = ints + 5 * B;
  WN_TRY(m->stage.begin((size_t)16 * B * sizeof(int) + 65536));
  WN_TRY(m->stage.put_at(dev_t_off, t_off.data(), B * sizeof(int), s));
  WN_TRY(m->stage.put_at(dev_t_len, t_len.data(), B * sizeof(int), s));
  WN_TRY(m->stage.end(s));
  float* x = m->pf_x.as<float>();
  float* y = m->pf_y.as<float>();
  float* t = m->pf_t.as<float>();
  float* o = m->pf_o.as<float>();
  float* q = m->pf_q.as<float>();
  float* kv = m->pf_kv.as<float>();
  // the first token_num embeddings of every utterance, packed
  for (int b = 0; b < B; ++b)
    if (t_len[b] > 0)
      WN_HIP(hipMemcpyAsync(x + (size_t)t_off[b] * d, m->pf_emb.as<float>() + (size_t)emb_off[b] * d,
                            (size_t)t_len[b] * d * sizeof(float), hipMemcpyDeviceToDevice, s));
  for (const PfDecLayer& L : W.pf.dec) {
    // SanmDecoderLayer.forward (layers.py:331-379): t = ffn(LN1(x)); y = x + fsmn(LN2(t)) -- the
    // residual is the layer INPUT; out = y + linear_out(cross attention(LN3(y), encoder_out))
    WN_TRY(ln(L.n1, x, t, Mt, d, 1e-12f, s));
    WN_TRY(pf_dec_ffn(m, L.ff1, L.ffn_norm, L.ff2, t, o, Mt, s));
    WN_TRY(ln(L.n2, o, t, Mt, d, 1e-12f, s));
    WN_TRY(pf_fsmn(m, p.kernel_size, t, d, L.fsmn_wt, x, d, y, dev_t_off, dev_t_len, B, max_t, s));
    WN_TRY(ln(L.n3, y, t, Mt, d, 1e-12f, s));
    WN_TRY(linear(L.src_q, t, d, q, d, Mt, s));
    WN_TRY(linear(L.src_kv, enc, d, kv, 2 * d, M, s));     // once per layer for the batch
    AttnArgs a;
    a.Q = q; a.K = kv; a.V = kv + d;
    a.ldq = d; a.ldk = a.ldv = 2 * d;
    a.O = o; a.ldo = d;
    a.q_off = dev_t_off; a.q_len = dev_t_len; a.kv_off = d_off; a.kv_len = d_len;
    a.n_seq = B; a.n_heads = H; a.max_q_len = max_t;
    WN_TRY(pf_attention(m, a, s));
    WN_TRY(linear(L.src_out, o, d, y, d, Mt, s, ACT_NONE, y, d));
    std::swap(x, y);
  }
  // decoders3 (ffn(LN(x)), no residual), after_norm, output_layer, log-softmax + arg-max
  WN_TRY(ln(W.pf.dec3_n1, x, t, Mt, d, 1e-5f, s));
  WN_TRY(pf_dec_ffn(m, W.pf.dec3_ff1, W.pf.dec3_ffn_norm, W.pf.dec3_ff2, t, y, Mt, s));
  WN_TRY(ln(W.pf.dec_after, y, t, Mt, d, 1e-5f, s));
  float* logits = m->pf_out.as<float>();
  float* top_v = logits + (size_t)Mt * V4;
  int* top_i = reinterpret_cast<int*>(top_v + Mt);
  WN_TRY(linear(W.pf.dec_out, t, d, logits, V4, Mt, s));
  CtcRowArgs ra;
  ra.logits = logits; ra.ld = V4; ra.M = Mt; ra.V = V; ra.k = 1;
  ra.blank = 0; ra.blank_penalty = 0.f;
  ra.topk_val = top_v; ra.topk_idx = top_i; ra.logp = nullptr; ra.ld_out = 0;
  WN_TRY(ctc_logsoftmax_topk(ra, s));
  float* h_val = reinterpret_cast<float*>(h_fire_t + E);
  int* h_idx = reinterpret_cast<int*>(h_val + Mt);
  WN_HIP(hipMemcpyAsync(h_val, top_v, (size_t)Mt * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < t_len[b]; ++i) {
      tokens[(size_t)b * max_tok + i] = h_idx[t_off[b] + i];
      logp[(size_t)b * max_tok + i] = h_val[t_off[b] + i];
    }
  return 0;
}

int wn_op_attention_d128(const float* Q, const float* K, const float* V, int32_t ldq,
                         int32_t ldk, int32_t ldv, int32_t q_rows, int32_t kv_rows, float* O,
                         int32_t ldo, const int32_t* q_off, const int32_t* q_len,
                         const int32_t* kv_off, const int32_t* kv_len, int32_t n_seq,
                         int32_t n_heads, float scale, void* stream) {
  WN_CHECK(Q && K && V && O && q_off && q_len && kv_off && kv_len,
           "attention_d128: null argument");
  WN_CHECK(n_seq > 0 && n_seq < 32768 && n_heads > 0 && n_heads < 256,
           "attention_d128: n_seq / n_heads");
  const int d = n_heads * 128;
  WN_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0,
           "attention_d128: strides must be multiples of 4 elements");
  WN_CHECK(ldq >= d && ldk >= d && ldv >= d && ldo >= d,
           "attention_d128: a stride is smaller than n_heads * 128");
  WN_CHECK(q_rows > 0 && kv_rows > 0, "attention_d128: empty buffers");
  WN_CHECK(((uintptr_t)Q & 15) == 0 && ((uintptr_t)K & 15) == 0 && ((uintptr_t)V & 15) == 0,
           "attention_d128: Q, K and V must be 16-byte aligned");
  WN_CHECK(pf_packed_ok(q_off, q_len, n_seq, q_rows),
           "attention_d128: query rows outside the buffer, unordered or overlapping");
  int max_q = 0;
  for (int i = 0; i < n_seq; ++i) {
    WN_CHECK(kv_len[i] >= 0 && kv_off[i] >= 0 && (int64_t)kv_off[i] + kv_len[i] <= kv_rows,
             "attention_d128: key rows outside the buffer");
    WN_CHECK(q_len[i] == 0 || kv_len[i] > 0, "attention_d128: queries without keys");
    max_q = std::max(max_q, q_len[i]);
  }
  WN_CHECK(max_q > 0, "attention_d128: empty");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  std::vector<int> h((size_t)4 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    h[i] = q_off[i]; h[n_seq + i] = q_len[i];
    h[2 * n_seq + i] = kv_off[i]; h[3 * n_seq + i] = kv_len[i];
  }
  WN_TRY(pf_upload_ints(desc, h, s));
  const int* dd = desc.as<int>();
  AttnArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.O = O; a.ldo = ldo;
  a.q_off = dd; a.q_len = dd + n_seq; a.kv_off = dd + 2 * n_seq; a.kv_len = dd + 3 * n_seq;
  a.n_seq = n_seq; a.n_heads = n_heads; a.max_q_len = max_q;
  a.mask_mode = 0; a.scale = scale;
  return attention_d128(a, s);
}

int wn_op_lfr_front(const float* feats, const float* mean, const float* istd, const float* pe,
                    int32_t pe_rows, const float* ln_w, const float* ln_b, float* out,
                    int32_t ldo, int32_t out_rows, const int32_t* lens, const int32_t* out_off,
                    int32_t* out_len, int32_t B, int32_t T, int32_t F, int32_t m, int32_t n,
                    float xscale, float eps, void* stream) {
  WN_CHECK(feats && pe && ln_w && ln_b && out && lens && out_off && out_len,
           "lfr_front: null argument");
  WN_CHECK((mean == nullptr) == (istd == nullptr), "lfr_front: mean and istd come together");
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F > 0 && m > 0 && n > 0, "lfr_front: B / T / F / m / n");
  WN_CHECK(m * F <= LFR_MAX_D && ldo >= m * F && ldo <= LFR_MAX_D,
           "lfr_front: m * F <= ldo <= 576");
  int max_rows = 0;
  std::vector<int> h((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens[b] >= 0 && lens[b] <= T, "lfr_front: a length outside [0, T]");
    out_len[b] = (lens[b] + n - 1) / n;
    max_rows = std::max(max_rows, out_len[b]);
    h[b] = lens[b]; h[B + b] = out_off[b];
  }
  WN_CHECK(pf_packed_ok(out_off, out_len, B, out_rows),
           "lfr_front: rows outside the buffer, unordered or overlapping");
  WN_CHECK(max_rows > 0, "lfr_front: empty");
  WN_CHECK(max_rows + 1 <= pe_rows, "lfr_front: position rows outside the table");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(pf_upload_ints(desc, h, s));
  LfrFrontArgs a;
  a.feats = feats; a.mean = mean; a.istd = istd; a.pe = pe; a.ln_w = ln_w; a.ln_b = ln_b;
  a.out = out; a.ldo = ldo; a.len = desc.as<int>(); a.off = a.len + B;
  a.B = B; a.T = T; a.F = F; a.m = m; a.n = n; a.max_rows = max_rows;
  a.xscale = xscale; a.eps = eps;
  return lfr_front(a, s);
}

int wn_op_layernorm_wide(const float* x, int32_t ldx, const float* w, const float* b, float* y,
                         int32_t ldy, int32_t M, int32_t D, int32_t Dpad, float eps,
                         void* stream) {
  return layernorm_wide(x, ldx, w, b, y, ldy, M, D, Dpad, eps, (hipStream_t)stream);
}

int wn_op_cif_alpha(const float* h, int32_t ldh, int32_t rows, int32_t d, const float* conv_w,
                    const float* conv_b, const float* out_w, const float* out_b, float smooth,
                    float noise, float* alpha, const int32_t* off, const int32_t* len,
                    int32_t n_seq, void* stream) {
  WN_CHECK(h && conv_w && conv_b && out_w && out_b && alpha && off && len,
           "cif_alpha: null argument");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && rows > 0, "cif_alpha: n_seq / rows");
  WN_CHECK(d > 0 && d % 32 == 0 && ldh % 4 == 0 && ldh >= d, "cif_alpha: d % 32, strides");
  WN_CHECK(pf_packed_ok(off, len, n_seq, rows),
           "cif_alpha: rows outside the buffer, unordered or overlapping");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, img, y;
  WN_TRY(pf_layout(off, len, n_seq, rows, desc, s));
  const int* dd = desc.as<int>();
  WN_TRY(img.ensure((size_t)rows * 3 * d * sizeof(float)));
  WN_TRY(y.ensure((size_t)rows * d * sizeof(float)));
  WN_TRY(cif_stage3(h, ldh, img.as<float>(), dd + 2 * n_seq, dd, dd + n_seq, rows, d, s));
  GemmArgs g;
  g.A = img.as<float>(); g.W = conv_w; g.bias = conv_b; g.C = y.as<float>();
  g.M = rows; g.N = d; g.K = 3 * d; g.lda = 3 * d; g.ldc = d; g.act = ACT_RELU;
  const int saved = t_gemm_prec;
  t_gemm_prec = PREC_F32;
  const int r = gemm_f32(g, s);
  t_gemm_prec = saved;
  WN_TRY(r);
  return cif_alpha_rows(y.as<float>(), d, out_w, out_b, smooth, noise, alpha, dd + 2 * n_seq,
                        rows, d, s);
}

int wn_op_cif_fire(const float* h, int32_t ldh, int32_t rows, int32_t d, const float* alpha,
                   const int32_t* off, const int32_t* len, int32_t n_seq, float threshold,
                   float tail, float* emb, int32_t lde, int32_t emb_rows, const int32_t* emb_off,
                   const int32_t* emb_cap, int32_t* fire_t_host, int32_t* n_fire_host,
                   int32_t* token_num_host, void* stream) {
  WN_CHECK(h && alpha && off && len && emb && emb_off && emb_cap && fire_t_host && n_fire_host &&
               token_num_host, "cif_fire: null argument");
  WN_CHECK(threshold == 1.0f, "cif_fire: threshold must be 1.0 (the scan subtracts 1 on a fire)");
  WN_CHECK(tail >= 0.f && tail <= 1.0f, "cif_fire: tail_threshold must be in [0, 1]");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && rows > 0 && emb_rows > 0, "cif_fire: n_seq / rows");
  WN_CHECK(d > 0 && d <= CIF_MAX_D && ldh >= d && lde >= d, "cif_fire: d / strides");
  WN_CHECK(pf_packed_ok(off, len, n_seq, rows),
           "cif_fire: rows outside the buffer, unordered or overlapping");
  WN_CHECK(pf_packed_ok(emb_off, emb_cap, n_seq, emb_rows),
           "cif_fire: embedding rows outside the buffer, unordered or overlapping");
  hipStream_t s = (hipStream_t)stream;
  // at most one fire per frame: every alpha the scan reads lies in [0, 1]
  std::vector<float> ah(rows);
  WN_HIP(hipMemcpyAsync(ah.data(), alpha, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < n_seq; ++i)
    for (int t = 0; t < len[i]; ++t)
      WN_CHECK(ah[off[i] + t] >= 0.f && ah[off[i] + t] <= 1.0f,
               "cif_fire: an alpha outside [0, 1]");
  static thread_local DevBuf desc, res;
  std::vector<int> hd((size_t)4 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    hd[i] = off[i]; hd[n_seq + i] = len[i];
    hd[2 * n_seq + i] = emb_off[i]; hd[3 * n_seq + i] = emb_cap[i];
  }
  WN_TRY(pf_upload_ints(desc, hd, s));
  WN_TRY(res.ensure(((size_t)emb_rows + 2 * n_seq) * sizeof(int)));
  WN_HIP(hipMemsetAsync(res.p, 0xff, ((size_t)emb_rows + 2 * n_seq) * sizeof(int), s));
  const int* dd = desc.as<int>();
  CifFireArgs a;
  a.h = h; a.ldh = ldh; a.alpha = alpha;
  a.off = dd; a.len = dd + n_seq; a.emb_off = dd + 2 * n_seq; a.emb_cap = dd + 3 * n_seq;
  a.emb = emb; a.lde = lde;
  a.fire_t = res.as<int>(); a.n_fire = a.fire_t + emb_rows; a.token_num = a.n_fire + n_seq;
  a.B = n_seq; a.d = d; a.tail = tail;
  WN_TRY(cif_fire(a, s));
  WN_HIP(hipMemcpyAsync(fire_t_host, a.fire_t, (size_t)emb_rows * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(n_fire_host, a.n_fire, (size_t)n_seq * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(token_num_host, a.token_num, (size_t)n_seq * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
