// C ABI (include/wenet_amd.h), handle life cycle: weight ingestion into the shared model block
// (ModelData, model_state.h), create / clone / destroy, operand precision, the encode gate,
// profiling, debug and tuning switches.
#include "model_state.h"
#include "weight_stage.h"

namespace wn {
namespace {

// ---------------------------------------------------------------------------
// weight ingestion
// fuse several Linear layers along the output dimension; part `no_bias_part` (if >= 0) has no
// bias in the state dict (key_bias: false): zeros in its place
int stage_fused(const Src& src, HostStage& hs, const std::string& name,
                const std::vector<std::string>& parts, int out_each, int in,
                int no_bias_part = -1) {
  std::vector<float> w((size_t)parts.size() * out_each * in),
      b((size_t)parts.size() * out_each, 0.f);
  for (size_t i = 0; i < parts.size(); ++i) {
    WN_GET(pw, parts[i] + ".weight", (int64_t)out_each * in);
    memcpy(w.data() + i * out_each * in, pw, sizeof(float) * out_each * in);
    if ((int)i == no_bias_part) continue;
    WN_GET(pb, parts[i] + ".bias", out_each);
    memcpy(b.data() + i * out_each, pb, sizeof(float) * out_each);
  }
  hs.add(name + ".weight", w.data(), w.size());
  hs.add(name + ".bias", b.data(), b.size());
  return 0;
}

int stage_decoder(const Src& src, HostStage& hs, const std::string& pfx,
                  int nlayers, const wn_config& c) {
  const int d = c.d_model, V = c.vocab;
  WN_GET(emb, pfx + ".embed.0.weight", (int64_t)V * d);
  hs.add(pfx + ".embed", emb, (size_t)V * d);
  WN_TRY(stage_norm(src, hs, pfx + ".after_norm", d));
  if (c.dec_learned_pos) {
    // LearnablePositionalEncoding (embedding.py:167-175): `pe` is a weight, (1, max_len, d)
    WN_GET(pe, pfx + ".embed.1.pe", (int64_t)c.dec_max_pos * d);
    hs.add(pfx + ".pe", pe, (size_t)c.dec_max_pos * d);
  }
  if (src.has(pfx + ".output_layer.weight")) {
    // (tie_word_embedding: init_model clones / ties the embedding into it, real checkpoints
    // carry both)
    WN_TRY(stage_linear(src, hs, pfx + ".output_layer", V, d));
  } else {
    // a state dict with the tied weight stored once: the embedding and a zero bias
    hs.add(pfx + ".output_layer.weight", emb, (size_t)V * d);
    hs.alloc(pfx + ".output_layer.bias", V);
  }
  for (int j = 0; j < nlayers; ++j) {
    const std::string p = pfx + ".decoders." + std::to_string(j);
    WN_TRY(stage_fused(src, hs, p + ".self_qkv",
                       {p + ".self_attn.linear_q", p + ".self_attn.linear_k",
                        p + ".self_attn.linear_v"}, d, d, c.dec_key_bias ? 1 : -1));
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, p + ".src_attn.linear_q", d, d));
    WN_TRY(stage_fused(src, hs, p + ".src_kv",
                       {p + ".src_attn.linear_k", p + ".src_attn.linear_v"}, d,
                       d, c.dec_src_key_bias ? 0 : -1));
    WN_TRY(stage_linear(src, hs, p + ".src_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, p + ".feed_forward.w_1", c.dec_ffn_dim, d));
    WN_TRY(stage_linear(src, hs, p + ".feed_forward.w_2", d, c.dec_ffn_dim));
    for (const char* n : {"norm1", "norm2", "norm3"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
  }
  return 0;
}

}  // namespace
}  // namespace wn

// ===========================================================================
extern "C" {

const char* wn_last_error(void) { return last_error_cstr(); }
const char* wn_version(void) { return "wenet_amd 0.1 (gfx950, fp32 MFMA)"; }

// wn_model_create / wn_model_create_transducer (tcfg == nullptr: no predictor / joint) /
// wn_model_create_transducer_stateless (scfg != nullptr: a stateless predictor, no LSTM) /
// wn_model_create_firered (fcfg != nullptr, cabi_firered.hip: the FireRedASR-AED encoder)
// wn_model_create_branchformer (bcfg != nullptr, cabi_branchformer.hip)
// wn_model_create_squeezeformer (qcfg != nullptr, cabi_squeezeformer.hip)
}  // extern "C"

int create_model_impl(const wn_config* cfg, const wn_transducer_config* tcfg,
                         const wn_stateless_predictor_config* scfg,
                         const wn_firered_config* fcfg, const wn_branchformer_config* bcfg,
                         const wn_squeezeformer_config* qcfg,
                         const wn_efficonformer_config* ecfg, const wn_tensor* weights,
                         int32_t n_weights, int32_t device, wn_model** out) {
  WN_CHECK(cfg && weights && out, "wn_model_create: null argument");
  const wn_config& c = *cfg;
  const bool fr = fcfg != nullptr;
  if (fr) {
    WN_CHECK(!tcfg, "firered: no transducer head");
    WN_CHECK(c.encoder_type == 0 && c.input_layer == 0 && c.cnn_norm == 0 && c.causal == 0 &&
             c.use_dynamic_chunk == 0 && c.static_chunk_size == 0 && c.activation == 0,
             "firered: conformer layers, layer_norm conv module, full context, swish");
    WN_CHECK(fcfg->sub_channels >= 1 && fcfg->sub_channels <= 256,
             "firered: sub_channels must be in [1, 256]");
    WN_CHECK(fcfg->conv_inner_factor == 4, "firered: conv_inner_factor must be 4");
    WN_CHECK(fcfg->max_frames >= 1 && fcfg->max_frames <= 8192,
             "firered: max_frames must be in [1, 8192]");
    WN_CHECK(fcfg->attn_norm_eps > 0.f, "firered: attn_norm_eps must be > 0");
    WN_CHECK(c.d_model == 64 || c.d_model == 128 || c.d_model == 256 || c.d_model == 512 ||
                 c.d_model == 1280,
             "firered: the depthwise conv over 2 d_model channels has kernels for d_model 64, "
             "128, 256, 512 and 1280");
  }
  const bool bf = bcfg != nullptr;
  if (bf) {
    const wn_branchformer_config& b = *bcfg;
    WN_CHECK(!tcfg && !fr, "branchformer: an asr_model head only (no transducer on these encoders)");
    WN_CHECK(b.kind == 1 || b.kind == 2, "branchformer: kind must be 1 (branchformer) or 2 "
                                         "(e_branchformer)");
    WN_CHECK(c.encoder_type == 0 && c.input_layer == 0,
             "branchformer: the Conv2dSubsampling4 front end (encoder_type 0, input_layer 0)");
    WN_CHECK(b.head_dim == 32 || b.head_dim == 64,
             "branchformer: d_model / attention_heads must be 32 or 64 (other head widths have "
             "no attention kernel)");
    WN_CHECK(c.n_heads > 0 && c.n_heads < 256 && c.d_model == c.n_heads * b.head_dim,
             "branchformer: d_model must be n_heads * head_dim");
    WN_CHECK(b.cgmlp_units >= 128 && b.cgmlp_units % 128 == 0 &&
                 b.cgmlp_units / 2 <= CSGU_MAX_C,
             "branchformer: cgmlp_linear_units / 2 must be a multiple of 64 up to 1024 (csgu_gate)");
    WN_CHECK(b.cgmlp_kernel >= 1 && b.cgmlp_kernel <= CSGU_MAX_K &&
                 (c.causal || b.cgmlp_kernel % 2 == 1),
             "branchformer: cgmlp_conv_kernel must be in [1, 63], odd unless causal");
    WN_CHECK(b.kind == 1 || (b.merge_kernel >= 1 && b.merge_kernel <= CSGU_MAX_K &&
                             (c.causal || b.merge_kernel % 2 == 1)),
             "branchformer: merge_conv_kernel must be in [1, 63], odd unless causal");
    WN_CHECK(b.linear_after_conv == 0 || b.linear_after_conv == 1,
             "branchformer: linear_after_conv is 0 or 1");
  }
  const bool sq = qcfg != nullptr;
  if (sq) {
    const wn_squeezeformer_config& q = *qcfg;
    WN_CHECK(!tcfg && !fr && !bf, "squeezeformer: an asr_model head only");
    WN_CHECK(c.encoder_type == 0 && c.input_layer == 0 && c.activation == 0,
             "squeezeformer: the conv2d front end (encoder_type 0, input_layer 0), swish");
    WN_CHECK(c.d_model == 64 || c.d_model == 128 || c.d_model == 256 || c.d_model == 512,
             "squeezeformer: encoder_dim must be 64, 128, 256 or 512");
    WN_CHECK((q.reduce_idx == -1 && q.recover_idx == -1) ||
                 (q.reduce_idx >= 0 && q.reduce_idx < q.recover_idx && q.recover_idx < c.n_layers),
             "squeezeformer: reduce_idx / recover_idx must both be -1 or satisfy 0 <= reduce_idx "
             "< recover_idx < n_layers");
    WN_CHECK(q.reduce_kernel == 5 || q.reduce_kernel == 1,
             "squeezeformer: reduce_kernel must be 5 (conv1d) or 1 (stream)");
    WN_CHECK(q.do_rel_shift == 0 || q.do_rel_shift == 1, "squeezeformer: do_rel_shift is 0 or 1");
    WN_CHECK(!(q.do_rel_shift && c.static_chunk_size > 0),
             "squeezeformer: do_rel_shift with static_chunk_size > 0 (the shift kernel is full "
             "context only)");
    WN_CHECK(!(q.reduce_idx >= 0 && c.static_chunk_size > 0 && c.static_chunk_size % 2 != 0),
             "squeezeformer: an odd static_chunk_size with a time reduction is no chunk window at "
             "the half rate");
  }
  const bool ef = ecfg != nullptr;
  if (ef) WN_TRY(efficonformer_config_check(c, *ecfg, tcfg || fr || bf || sq));
  WN_CHECK(c.d_model % 64 == 0 && c.n_heads > 0 && (bf || ef || c.d_model / c.n_heads == 64),
           "d_model / n_heads must be 64 (all reference Conformer configs)");
  WN_CHECK(c.dec_layers == 0 || c.dec_heads == 0 ||
               (c.d_model % c.dec_heads == 0 &&
                (c.d_model / c.dec_heads == 64 || c.d_model / c.dec_heads == 32)),
           "decoder head dim must be 32 or 64");
  WN_CHECK(c.ffn_dim % 32 == 0 && c.feat_dim >= 7 && c.feat_dim <= 128,
           "unsupported ffn_dim / feat_dim");
  WN_CHECK(c.dec_activation == 0 || c.dec_activation == 1, "dec_activation: 0 relu, 1 gelu");
  WN_CHECK(!c.dec_learned_pos || (c.dec_max_pos >= 1 && !c.bidirectional),
           "learned decoder positions need dec_max_pos >= 1 and a single decoder");
  const bool tf = c.encoder_type == 1;
  WN_CHECK(c.encoder_type == 0 || c.encoder_type == 1, "unknown encoder_type");
  WN_CHECK(tf ? c.input_layer == 1 : c.input_layer == 0,
           "supported pairs: conformer + conv2d, transformer + conv1d2");
  WN_CHECK(tf || (c.cnn_kernel >= 1 && (c.causal || c.cnn_kernel % 2 == 1)),
           "cnn_module_kernel must be odd for a non-causal conv module");
  WN_HIP(hipSetDevice(device));
  std::unique_ptr<wn_model> m(new wn_model());
  m->cfg = c;
  m->device = device;
  if (tcfg) { m->tr.on = true; m->tr.c = *tcfg; }
  if (tcfg && scfg) m->tr.sp = *scfg;
  if (fr) { m->fr.on = true; m->fr.c = *fcfg; }
  if (bf) { m->bf.on = true; m->bf.c = *bcfg; }
  if (sq) { m->sq.on = true; m->sq.c = *qcfg; }
  if (ef) { m->ef.on = true; m->ef.c = *ecfg; }
  // the block this call fills; the handle (and every clone of it) sees it as const
  const std::shared_ptr<ModelData> data = std::make_shared<ModelData>();
  m->data = data;
  ModelData& W = *data;
  Src src;
  for (int i = 0; i < n_weights; ++i)
    src.t[weights[i].name] = {weights[i].data, weights[i].numel};

  const int d = c.d_model, F = c.ffn_dim, V = c.vocab, K = c.cnn_kernel;
  const int F2 = m->F2();
  HostStage hs;
  if (c.has_cmvn) {
    WN_GET(mean, "encoder.global_cmvn.mean", c.feat_dim);
    WN_GET(istd, "encoder.global_cmvn.istd", c.feat_dim);
    hs.add("cmvn.mean", mean, c.feat_dim);
    hs.add("cmvn.istd", istd, c.feat_dim);
  }
  const int Fin = c.feat_dim;
  const int K1 = cdiv(3 * Fin, 32) * 32;  // conv1d K, padded with zero weights
  if (tf) {
    // Conv1d (n, c, tap) -> [n][tap * C + c] (the taps of one output frame are
    // three consecutive channels-last input rows)
    WN_GET(w0, "encoder.embed.conv.0.weight", (int64_t)d * Fin * 3);
    WN_GET(b0, "encoder.embed.conv.0.bias", d);
    float* t = hs.alloc("tconv1.w", (size_t)d * K1);
    for (int n = 0; n < d; ++n)
      for (int ch = 0; ch < Fin; ++ch)
        for (int k = 0; k < 3; ++k)
          t[(size_t)n * K1 + (size_t)k * Fin + ch] = w0[((size_t)n * Fin + ch) * 3 + k];
    hs.add("tconv1.b", b0, d);
    WN_GET(w2, "encoder.embed.conv.2.weight", (int64_t)d * d * 3);
    WN_GET(b2, "encoder.embed.conv.2.bias", d);
    t = hs.alloc("tconv2.w", (size_t)d * 3 * d);
    for (int n = 0; n < d; ++n)
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < 3; ++k)
          t[(size_t)n * 3 * d + (size_t)k * d + ch] = w2[((size_t)n * d + ch) * 3 + k];
    hs.add("tconv2.b", b2, d);
  } else if (fr) {
    // FireRedConv2dSubsampling4 (firered/subsampling.py:42-49): C channels, direct kernels
    const int C = fcfg->sub_channels;
    WN_GET(w0, "encoder.embed.conv.0.weight", (int64_t)C * 9);
    WN_GET(b0, "encoder.embed.conv.0.bias", C);
    float* t = hs.alloc("fr.conv1.w", (size_t)9 * C);          // (C,1,3,3) -> [tap][c]
    for (int ch = 0; ch < C; ++ch)
      for (int k = 0; k < 9; ++k) t[k * C + ch] = w0[ch * 9 + k];
    hs.add("fr.conv1.b", b0, C);
    WN_GET(w2, "encoder.embed.conv.2.weight", (int64_t)C * C * 9);
    WN_GET(b2, "encoder.embed.conv.2.bias", C);
    t = hs.alloc("fr.conv2.w", (size_t)9 * C * C);             // (n,c,3,3) -> [tap][c][n]
    for (int n = 0; n < C; ++n)
      for (int ch = 0; ch < C; ++ch)
        for (int k = 0; k < 9; ++k)
          t[((size_t)k * C + ch) * C + n] = w2[((size_t)n * C + ch) * 9 + k];
    hs.add("fr.conv2.b", b2, C);
    // out Linear(C * F2 -> d): the kernels write the reference's own column order c * F2 + f
    WN_TRY(stage_linear(src, hs, "encoder.embed.out.0", d, C * F2));
  } else if (ef && ecfg->front_rate == 2) {
    WN_TRY(efficonformer_stage_front2(src, hs, c, m->F1()));   // (cabi_efficonformer.hip)
  } else {  // conv1 (d,1,3,3) -> [tap][c]
    // (squeezeformer: DepthwiseConv2dSubsampling4 without dw_stride is the same pair of convs
    // under other names, squeezeformer/subsampling.py:52-67)
    const std::string n_c1 = sq ? "encoder.embed.pw_conv" : "encoder.embed.conv.0";
    const std::string n_c2 = sq ? "encoder.embed.dw_conv" : "encoder.embed.conv.2";
    const std::string n_out = sq ? "encoder.embed.input_proj.0" : "encoder.embed.out.0";
    WN_GET(w0, n_c1 + ".weight", (int64_t)d * 9);
    WN_GET(b0, n_c1 + ".bias", d);
    float* t = hs.alloc("conv1.w", (size_t)9 * d);
    for (int ch = 0; ch < d; ++ch)
      for (int k = 0; k < 9; ++k) t[k * d + ch] = w0[ch * 9 + k];
    hs.add("conv1.b", b0, d);
    // conv2 (n, c, ky, kx) -> [n][(ky*3+kx)*d + c]
    WN_GET(w2, n_c2 + ".weight", (int64_t)d * d * 9);
    WN_GET(b2, n_c2 + ".bias", d);
    t = hs.alloc("conv2.w", (size_t)d * 9 * d);
    for (int n = 0; n < d; ++n)
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < 9; ++k)
          t[(size_t)n * 9 * d + (size_t)k * d + ch] =
              w2[((size_t)n * d + ch) * 9 + k];
    hs.add("conv2.b", b2, d);
    // out Linear(d*F2 -> d): input index c*F2+f  ->  f*d+c
    WN_GET(wo, n_out + ".weight", (int64_t)d * d * F2);
    WN_GET(bo, n_out + ".bias", d);
    t = hs.alloc("sub_out.w", (size_t)d * d * F2);
    for (int n = 0; n < d; ++n)
      for (int ch = 0; ch < d; ++ch)
        for (int f = 0; f < F2; ++f)
          t[(size_t)n * d * F2 + (size_t)f * d + ch] =
              wo[(size_t)n * d * F2 + (size_t)ch * F2 + f];
    if (sq) {
      // the sqrt(d) of RelPositionalEncoding sits in FRONT of input_proj here:
      // W (x sqrt d) + b = sqrt(d) (W x + b / sqrt d), the form the front end computes
      float* tb = hs.alloc("sub_out.b", d);
      for (int n = 0; n < d; ++n) tb[n] = (float)((double)bo[n] / sqrt((double)d));
    } else {
      hs.add("sub_out.b", bo, d);
    }
  }
  {  // positional table: the `pe` buffer (embedding.py:47-56)
    float* t = hs.alloc("pe", (size_t)c.max_pos * d);
    WN_CHECK(!tf || src.has("encoder.embed.pos_enc.pe"),
             "transformer encoder: encoder.embed.pos_enc.pe is required");
    if (src.has("encoder.embed.pos_enc.pe")) {
      WN_GET(pe, "encoder.embed.pos_enc.pe", (int64_t)c.max_pos * d);
      memcpy(t, pe, sizeof(float) * c.max_pos * d);
    } else {
      for (int pos = 0; pos < c.max_pos; ++pos)
        for (int i = 0; i < d; i += 2) {
          const float div = expf((float)i * -(logf(10000.0f) / (float)d));
          t[(size_t)pos * d + i] = sinf((float)pos * div);
          t[(size_t)pos * d + i + 1] = cosf((float)pos * div);
        }
    }
  }
  // ---- fbank tables (runtime/core/frontend/fbank.h:91-163) -----------------
  const FbankTables fbt = make_fbank_tables(c.feat_dim);   // (fbank_tables.h)
  stage_fbank_tables(fbt, hs, W);
  // (firered: final_norm false; squeezeformer: post-LN blocks, no after_norm)
  if (!fr && !sq) WN_TRY(stage_norm(src, hs, "encoder.after_norm", d));
  const bool has_ctc = src.has("ctc.ctc_lo.weight");
  if (has_ctc) WN_TRY(stage_linear(src, hs, "ctc.ctc_lo", V, d));
  for (int i = 0; tf && i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    WN_TRY(stage_norm(src, hs, p + ".norm1", d));
    WN_TRY(stage_norm(src, hs, p + ".norm2", d));
    {  // fused QKV; Whisper's linear_k has no bias (attention.py:29-75)
      std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d, 0.f);
      const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
      for (int j = 0; j < 3; ++j) {
        const std::string q = p + ".self_attn." + parts[j];
        WN_GET(pw, q + ".weight", (int64_t)d * d);
        memcpy(w.data() + (size_t)j * d * d, pw, sizeof(float) * d * d);
        if (j != 1 || c.key_bias) {
          WN_GET(pb, q + ".bias", d);
          memcpy(b.data() + (size_t)j * d, pb, sizeof(float) * d);
        }
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
    }
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, p + ".feed_forward.w_1", F, d));
    WN_TRY(stage_linear(src, hs, p + ".feed_forward.w_2", d, F));
  }
  if (fr) {
    // the plain normalisation in front of the folded QKV projection, and the relative position
    // rows: row r of the (2 max_frames - 1)-row table is the sinusoid of the relative position
    // max_frames - 1 - r (firered/attention.py:30-43, evaluated in fp32 like the module)
    float* u = hs.alloc("fr.unit.weight", d);
    for (int i = 0; i < d; ++i) u[i] = 1.0f;
    hs.alloc("fr.unit.bias", d);
    const int cap = fcfg->max_frames;
    float* t = hs.alloc("fr.rel_pe", (size_t)(2 * cap - 1) * d);
    for (int r = 0; r < 2 * cap - 1; ++r) {
      const float pos = (float)(cap - 1 - r);
      for (int i = 0; i < d; i += 2) {
        const float div = expf((float)i * -(logf(10000.0f) / (float)d));
        t[(size_t)r * d + i] = sinf(pos * div);
        t[(size_t)r * d + i + 1] = cosf(pos * div);
      }
    }
  }
  for (int i = 0; fr && i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    const int d2 = 2 * d;
    for (const char* n : {"norm_ff_macaron", "norm_conv", "norm_ff", "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    WN_TRY(stage_norm(src, hs, p + ".conv_module.norm", d2));
    for (const char* ff : {"feed_forward_macaron", "feed_forward"}) {
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_1", F, d));
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
    }
    {  // layer_norm_q / k / v folded into the QKV projection, in fp64: the three LayerNorms
       // normalise the same x, so LN(x; g, b) W^T = LN(x; 1, 0) (W diag(g))^T + W b
      std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d);
      const char* parts[3] = {"q", "k", "v"};
      for (int j = 0; j < 3; ++j) {
        WN_GET(pw, p + ".self_attn.linear_" + parts[j] + ".weight", (int64_t)d * d);
        WN_GET(g, p + ".self_attn.layer_norm_" + parts[j] + ".weight", d);
        WN_GET(be, p + ".self_attn.layer_norm_" + parts[j] + ".bias", d);
        for (int o = 0; o < d; ++o) {
          double acc = 0.0;
          for (int k = 0; k < d; ++k) {
            w[((size_t)j * d + o) * d + k] = (float)((double)pw[(size_t)o * d + k] * (double)g[k]);
            acc += (double)pw[(size_t)o * d + k] * (double)be[k];
          }
          b[(size_t)j * d + o] = (float)acc;
        }
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
    }
    // (linear_out carries a bias only with query_bias, transformer/attention.py:77)
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d,
                        src.has(p + ".self_attn.linear_out.bias")));
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_pos", d, d, false));
    WN_GET(bu, p + ".self_attn.pos_bias_u", d);
    WN_GET(bv, p + ".self_attn.pos_bias_v", d);
    hs.add(p + ".pos_bias_u", bu, d);
    hs.add(p + ".pos_bias_v", bv, d);
    {  // pointwise_conv1 (4d, d, 1), no bias: GLU halves [0, 2d) | [2d, 4d), rows permuted per
       // 64 as [32 a | 32 gate]; the GLU of a zero frame is 0 (cpad)
      WN_GET(w1, p + ".conv_module.pointwise_conv1.weight", (int64_t)2 * d2 * d);
      std::vector<float> w((size_t)2 * d2 * d);
      for (int g = 0; g < d2 / 32; ++g)
        for (int j = 0; j < 32; ++j) {
          const int ch = g * 32 + j;
          memcpy(&w[(size_t)(g * 64 + j) * d], &w1[(size_t)ch * d], sizeof(float) * d);
          memcpy(&w[(size_t)(g * 64 + 32 + j) * d], &w1[(size_t)(d2 + ch) * d],
                 sizeof(float) * d);
        }
      hs.add(p + ".pw1.weight", w.data(), w.size());
      hs.alloc(p + ".pw1.bias", 2 * d2);
      hs.alloc(p + ".cpad", d2);
    }
    {  // depthwise (2d,1,K), no bias -> [K][2d]
      WN_GET(wd, p + ".conv_module.depthwise_conv.weight", (int64_t)d2 * K);
      std::vector<float> w((size_t)K * d2);
      for (int ch = 0; ch < d2; ++ch)
        for (int k = 0; k < K; ++k) w[(size_t)k * d2 + ch] = wd[(size_t)ch * K + k];
      hs.add(p + ".dw.weight", w.data(), w.size());
      hs.alloc(p + ".dw.bias", d2);
    }
    WN_TRY(stage_linear(src, hs, p + ".conv_module.pointwise_conv2", d, d2, false));
  }
  for (int i = 0; bf && i < c.n_layers; ++i) {
    // BranchformerEncoderLayer / EBranchformerEncoderLayer.  (pooling_proj1/2 and weight_proj1/2
    // of a Branchformer layer serve merge_method learned_ave only: not read.)
    const std::string p = "encoder.encoders." + std::to_string(i);
    const wn_branchformer_config& b = *bcfg;
    const int H = c.n_heads, hd = b.head_dim, dq = H * 64, U = b.cgmlp_units, C = U / 2;
    for (const char* n : {"norm_mha", "norm_mlp", "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    if (b.kind == 2) {
      WN_TRY(stage_norm(src, hs, p + ".norm_ff_macaron", d));
      WN_TRY(stage_norm(src, hs, p + ".norm_ff", d));
      for (const char* ff : {"feed_forward_macaron", "feed_forward"}) {
        WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_1", F, d));
        WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
      }
    }
    {  // Q | K | V, linear_pos and pos_bias_u / v as H heads of 64 columns: head h's hd rows,
       // then 64 - hd zero rows (head_dim 32: every added product of the attention is an
       // exact zero; head_dim 64: the reference's own layout)
      std::vector<float> w((size_t)3 * dq * d, 0.f), bq((size_t)3 * dq, 0.f);
      const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
      for (int j = 0; j < 3; ++j) {
        WN_GET(pw, p + ".attn." + parts[j] + ".weight", (int64_t)d * d);
        WN_GET(pb, p + ".attn." + parts[j] + ".bias", d);
        for (int h = 0; h < H; ++h)
          for (int r = 0; r < hd; ++r) {
            memcpy(&w[((size_t)j * dq + h * 64 + r) * d], &pw[(size_t)(h * hd + r) * d],
                   sizeof(float) * d);
            bq[(size_t)j * dq + h * 64 + r] = pb[h * hd + r];
          }
      }
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", bq.data(), bq.size());
      WN_GET(pp, p + ".attn.linear_pos.weight", (int64_t)d * d);
      WN_GET(bu, p + ".attn.pos_bias_u", d);
      WN_GET(bv, p + ".attn.pos_bias_v", d);
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
      // linear_out [d][d] -> [d][dq]: zero columns under the padded context columns
      WN_GET(po, p + ".attn.linear_out.weight", (int64_t)d * d);
      WN_GET(pob, p + ".attn.linear_out.bias", d);
      std::vector<float> wo((size_t)d * dq, 0.f);
      for (int n = 0; n < d; ++n)
        for (int h = 0; h < H; ++h)
          memcpy(&wo[(size_t)n * dq + h * 64], &po[(size_t)n * d + h * hd], sizeof(float) * hd);
      hs.add(p + ".self_attn.linear_out.weight", wo.data(), wo.size());
      hs.add(p + ".self_attn.linear_out.bias", pob, d);
    }
    WN_TRY(stage_linear(src, hs, p + ".cgmlp.channel_proj1.0", U, d));
    WN_TRY(stage_norm(src, hs, p + ".cgmlp.csgu.norm", C));
    {  // depthwise (C,1,K) -> [K][C]
      const int Kc = b.cgmlp_kernel;
      WN_GET(wd, p + ".cgmlp.csgu.conv.weight", (int64_t)C * Kc);
      WN_GET(bd, p + ".cgmlp.csgu.conv.bias", C);
      std::vector<float> w((size_t)Kc * C);
      for (int ch = 0; ch < C; ++ch)
        for (int k = 0; k < Kc; ++k) w[(size_t)k * C + ch] = wd[(size_t)ch * Kc + k];
      hs.add(p + ".csgu.dw.weight", w.data(), w.size());
      hs.add(p + ".csgu.dw.bias", bd, C);
    }
    if (b.linear_after_conv) WN_TRY(stage_linear(src, hs, p + ".cgmlp.csgu.linear", C, C));
    WN_TRY(stage_linear(src, hs, p + ".cgmlp.channel_proj2", d, C));
    if (b.kind == 2) {  // depthwise_conv_fusion (2d,1,Km) -> [Km][2d]
      const int Km = b.merge_kernel, d2 = 2 * d;
      WN_GET(wd, p + ".depthwise_conv_fusion.weight", (int64_t)d2 * Km);
      WN_GET(bd, p + ".depthwise_conv_fusion.bias", d2);
      std::vector<float> w((size_t)Km * d2);
      for (int ch = 0; ch < d2; ++ch)
        for (int k = 0; k < Km; ++k) w[(size_t)k * d2 + ch] = wd[(size_t)ch * Km + k];
      hs.add(p + ".merge.dw.weight", w.data(), w.size());
      hs.add(p + ".merge.dw.bias", bd, d2);
    }
    WN_TRY(stage_linear(src, hs, p + ".merge_proj", d, 2 * d));
  }
  if (sq) {
    WN_TRY(stage_norm(src, hs, "encoder.preln", d));
    if (qcfg->reduce_idx >= 0) {
      const int Kr = qcfg->reduce_kernel;
      WN_GET(wd, "encoder.time_reduction_layer.dw_conv.weight", (int64_t)d * Kr);
      WN_GET(bd, "encoder.time_reduction_layer.dw_conv.bias", d);
      std::vector<float> w((size_t)Kr * d);
      for (int ch = 0; ch < d; ++ch)
        for (int k = 0; k < Kr; ++k) w[(size_t)k * d + ch] = wd[(size_t)ch * Kr + k];
      hs.add("sq.red.dw.weight", w.data(), w.size());
      hs.add("sq.red.dw.bias", bd, d);
      WN_TRY(stage_linear(src, hs, "encoder.time_reduction_layer.pw_conv", d, d));
      WN_TRY(stage_linear(src, hs, "encoder.time_recover_layer", d, d));
    }
  }
  for (int i = 0; sq && i < c.n_layers; ++i) {
    // SqueezeformerEncoderLayer.  `ada_scale * x + ada_bias` in front of a module folds into the
    // module's first Linear, in fp64: W' = W diag(s), b' = W a + b.
    const std::string p = "encoder.encoders." + std::to_string(i);
    // dst rows [row0, row0 + out) of a [.][d] matrix
    auto fold = [&](const std::string& lin, const std::string& ada, int out, float* w, float* b,
                    const int* perm) -> int {
      WN_GET(pw, lin + ".weight", (int64_t)out * d);
      WN_GET(pb, lin + ".bias", out);
      WN_GET(sc, ada + ".ada_scale", d);
      WN_GET(ab, ada + ".ada_bias", d);
      for (int o = 0; o < out; ++o) {
        const int r = perm ? perm[o] : o;
        double acc = (double)pb[o];
        for (int k = 0; k < d; ++k) {
          w[(size_t)r * d + k] = (float)((double)pw[(size_t)o * d + k] * (double)sc[k]);
          acc += (double)pw[(size_t)o * d + k] * (double)ab[k];
        }
        b[r] = (float)acc;
      }
      return 0;
    };
    for (const char* n : {"layer_norm1", "layer_norm2", "layer_norm3", "layer_norm4"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    {
      std::vector<float> w((size_t)3 * d * d), b((size_t)3 * d);
      const char* parts[3] = {"linear_q", "linear_k", "linear_v"};
      for (int j = 0; j < 3; ++j)
        WN_TRY(fold(p + ".self_attn." + parts[j], p + ".self_attn", d, &w[(size_t)j * d * d],
                    &b[(size_t)j * d], nullptr));
      hs.add(p + ".qkv.weight", w.data(), w.size());
      hs.add(p + ".qkv.bias", b.data(), b.size());
    }
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_pos", d, d, false));
    WN_GET(bu, p + ".self_attn.pos_bias_u", d);
    WN_GET(bv, p + ".self_attn.pos_bias_v", d);
    hs.add(p + ".pos_bias_u", bu, d);
    hs.add(p + ".pos_bias_v", bv, d);
    for (const char* ff : {"ffn1", "ffn2"}) {
      std::vector<float> w((size_t)F * d), b(F);
      WN_TRY(fold(p + "." + ff + ".w_1", p + "." + ff, F, w.data(), b.data(), nullptr));
      hs.add(p + "." + ff + ".w_1.weight", w.data(), w.size());
      hs.add(p + "." + ff + ".w_1.bias", b.data(), b.size());
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
    }
    {  // pointwise_conv1 (2d, d, 1): rows permuted per 64 as [32 a | 32 gate].  The reference
       // pads the causal conv's K - 1 ZERO frames behind the adaptive scale and in front of
       // pointwise_conv1, so a padded frame is the GLU of the UNFOLDED bias
      std::vector<int> perm(2 * d);
      for (int g = 0; g < d / 32; ++g)
        for (int j = 0; j < 32; ++j) {
          perm[g * 32 + j] = g * 64 + j;
          perm[d + g * 32 + j] = g * 64 + 32 + j;
        }
      std::vector<float> w((size_t)2 * d * d), b(2 * d), cp(d);
      WN_TRY(fold(p + ".conv_module.pointwise_conv1", p + ".conv_module", 2 * d, w.data(),
                  b.data(), perm.data()));
      WN_GET(b1, p + ".conv_module.pointwise_conv1.bias", 2 * d);
      for (int ch = 0; ch < d; ++ch)
        cp[ch] = (float)((double)b1[ch] / (1.0 + exp(-(double)b1[d + ch])));
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
    WN_TRY(stage_linear(src, hs, p + ".conv_module.pointwise_conv2", d, d));
  }
  if (ef) WN_TRY(efficonformer_stage_layers(src, hs, c, *ecfg));   // (cabi_efficonformer.hip)
  for (int i = 0; !tf && !fr && !bf && !sq && !ef && i < c.n_layers; ++i) {
    const std::string p = "encoder.encoders." + std::to_string(i);
    for (const char* n : {"norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff",
                          "norm_final"})
      WN_TRY(stage_norm(src, hs, p + "." + n, d));
    if (c.cnn_norm == 0) {
      WN_TRY(stage_norm(src, hs, p + ".conv_module.norm", d));
    } else {
      // eval-mode BatchNorm1d (convolution.py:77-81,139-143) as a per-channel
      // affine: y = x * scale + shift, scale = w / sqrt(running_var + eps),
      // shift = b - running_mean * scale; staged in the norm's weight / bias slots
      const std::string q = p + ".conv_module.norm";
      WN_GET(bw, q + ".weight", d);
      WN_GET(bb, q + ".bias", d);
      WN_GET(bm, q + ".running_mean", d);
      WN_GET(bv, q + ".running_var", d);
      std::vector<float> sc(d), sh(d);
      for (int ch = 0; ch < d; ++ch) {
        const float inv = 1.0f / sqrtf(bv[ch] + c.norm_eps);
        sc[ch] = bw[ch] * inv;
        sh[ch] = bb[ch] - bm[ch] * sc[ch];
      }
      hs.add(q + ".weight", sc.data(), sc.size());
      hs.add(q + ".bias", sh.data(), sh.size());
    }
    for (const char* ff : {"feed_forward_macaron", "feed_forward"}) {
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_1", F, d));
      WN_TRY(stage_linear(src, hs, p + "." + ff + ".w_2", d, F));
    }
    WN_TRY(stage_fused(src, hs, p + ".qkv",
                       {p + ".self_attn.linear_q", p + ".self_attn.linear_k",
                        p + ".self_attn.linear_v"}, d, d));
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_out", d, d));
    WN_TRY(stage_linear(src, hs, p + ".self_attn.linear_pos", d, d, false));
    WN_GET(bu, p + ".self_attn.pos_bias_u", d);
    WN_GET(bv, p + ".self_attn.pos_bias_v", d);
    hs.add(p + ".pos_bias_u", bu, d);
    hs.add(p + ".pos_bias_v", bv, d);
    {  // pointwise_conv1 (2d, d, 1): rows permuted per 64 as [32 a | 32 gate]
      WN_GET(w1, p + ".conv_module.pointwise_conv1.weight", (int64_t)2 * d * d);
      WN_GET(b1, p + ".conv_module.pointwise_conv1.bias", 2 * d);
      std::vector<float> w((size_t)2 * d * d), b(2 * d), cp(d);
      for (int g = 0; g < d / 32; ++g)
        for (int j = 0; j < 32; ++j) {
          const int ch = g * 32 + j;
          memcpy(&w[(size_t)(g * 64 + j) * d], &w1[(size_t)ch * d],
                 sizeof(float) * d);
          memcpy(&w[(size_t)(g * 64 + 32 + j) * d], &w1[(size_t)(d + ch) * d],
                 sizeof(float) * d);
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
  const bool has_dec = c.dec_layers > 0;
  if (has_dec) {
    if (c.bidirectional) {
      WN_TRY(stage_decoder(src, hs, "decoder.left_decoder", c.dec_layers, c));
      if (c.dec_r_layers > 0)
        WN_TRY(stage_decoder(src, hs, "decoder.right_decoder", c.dec_r_layers, c));
    } else {
      WN_TRY(stage_decoder(src, hs, "decoder", c.dec_layers, c));
    }
  }
  if (tcfg) {
    // RNNPredictor (predictor.py:60-88) and TransducerJoint (joint.py:34-49)
    const wn_transducer_config& tc = *tcfg;
    const int E = tc.pred_embed, H = tc.pred_hidden, P = tc.pred_out, J = tc.join_dim;
    WN_CHECK(!tf, "transducer: Conformer encoders only");
    if (scfg) {
      const wn_stateless_predictor_config& sc = *scfg;
      WN_CHECK(sc.kind == 1 || sc.kind == 2,
               "stateless predictor: kind must be 1 (embedding) or 2 (conv)");
      WN_CHECK(E >= 1 && E <= 1024 && P == E && H == 0 && tc.pred_layers == 0,
               "stateless predictor: pred_embed == pred_out in [1, 1024], pred_hidden == "
               "pred_layers == 0");
      WN_CHECK(sc.context >= 1 && sc.context <= 16 && sc.heads >= 1 && sc.heads <= 16,
               "stateless predictor: context and heads must be in [1, 16]");
      WN_CHECK(sc.kind == 1 || sc.heads == 1,
               "stateless predictor: a conv predictor has heads == 1");
      WN_CHECK(sc.activation == 0 || sc.activation == 1,
               "stateless predictor: activation 0 (swish) or 1 (relu)");
      WN_CHECK(sc.norm_eps > 0.f, "stateless predictor: norm_eps must be > 0");
    } else {
      WN_CHECK(E >= 1 && E <= 1024 && H >= 1 && H <= 1024 && P >= 1 && P <= 1024 &&
               tc.pred_layers >= 1 && tc.pred_layers <= 8,
               "transducer: predictor widths must be in [1, 1024], 1 to 8 LSTM layers");
    }
    WN_CHECK(J >= 32 && J <= 1024 && J % 32 == 0,
             "transducer: join_dim must be a multiple of 32 in [32, 1024]");
    WN_CHECK(tc.blank >= 0 && tc.blank < V, "transducer: blank id outside the vocabulary");
    WN_GET(emb, "predictor.embed.weight", (int64_t)V * E);
    hs.add("predictor.embed.weight", emb, (size_t)V * E);
    if (scfg) {
      const int C = scfg->context;
      WN_TRY(stage_norm(src, hs, "predictor.norm", E));
      if (scfg->kind == 1) {
        // (pos_embed.bias, present with `bias: true`, is read by neither forward nor forward_step)
        WN_GET(pos, "predictor.pos_embed.weight", (int64_t)scfg->heads * E * C);
        hs.add("predictor.pos_embed.weight", pos, (size_t)scfg->heads * E * C);
        WN_TRY(stage_linear(src, hs, "predictor.ffn", E, E));
      } else {
        WN_GET(cw, "predictor.conv.weight", (int64_t)E * C);
        hs.add("predictor.conv.weight", cw, (size_t)E * C);
        if (scfg->conv_bias) {
          WN_GET(cb, "predictor.conv.bias", E);
          hs.add("predictor.conv.bias", cb, E);
        }
      }
    }
    for (int l = 0; l < tc.pred_layers; ++l) {
      const std::string sfx = "_l" + std::to_string(l);
      const int in = l == 0 ? E : H;
      WN_GET(wi, "predictor.rnn.weight_ih" + sfx, (int64_t)4 * H * in);
      WN_GET(wh, "predictor.rnn.weight_hh" + sfx, (int64_t)4 * H * H);
      WN_GET(bi, "predictor.rnn.bias_ih" + sfx, 4 * H);
      WN_GET(bh, "predictor.rnn.bias_hh" + sfx, 4 * H);
      hs.add("predictor.rnn.weight_ih" + sfx, wi, (size_t)4 * H * in);
      hs.add("predictor.rnn.weight_hh" + sfx, wh, (size_t)4 * H * H);
      hs.add("predictor.rnn.bias_ih" + sfx, bi, 4 * H);
      hs.add("predictor.rnn.bias_hh" + sfx, bh, 4 * H);
    }
    if (!scfg) { WN_TRY(stage_linear(src, hs, "predictor.projection", P, H)); }
    WN_TRY(stage_linear(src, hs, "joint.enc_ffn", J, d));
    WN_TRY(stage_linear(src, hs, "joint.pred_ffn", J, P));
    WN_TRY(stage_linear(src, hs, "joint.ffn_out", V, J));
  }
  // ---- upload ---------------------------------------------------------------
  WN_TRY(W.weights.ensure(hs.data.size() * sizeof(float)));
  W.n_weight_elems = (int64_t)hs.data.size();
  WN_HIP(hipMemcpy(W.weights.p, hs.data.data(), hs.data.size() * sizeof(float),
                   hipMemcpyHostToDevice));
  const float* base = W.weights.as<float>();
  for (auto& kv : hs.at) W.w[kv.first] = base + kv.second.first;
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& p, int o, int i, bool bias = true) {
    Linear l; l.w = P(p + ".weight"); l.b = bias ? P(p + ".bias") : nullptr;
    l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& p) {
    Norm n; n.w = P(p + ".weight"); n.b = P(p + ".bias"); return n;
  };
  if (c.has_cmvn) { W.cmvn_mean = P("cmvn.mean"); W.cmvn_istd = P("cmvn.istd"); }
  if (tf) {
    W.tconv1.w = P("tconv1.w"); W.tconv1.b = P("tconv1.b");
    W.tconv1.out = d; W.tconv1.in = K1;
    W.tconv2.w = P("tconv2.w"); W.tconv2.b = P("tconv2.b");
    W.tconv2.out = d; W.tconv2.in = 3 * d;
  } else if (fr) {
    const int C = fcfg->sub_channels;
    W.conv1_w = P("fr.conv1.w"); W.conv1_b = P("fr.conv1.b");
    W.conv2.w = P("fr.conv2.w"); W.conv2.b = P("fr.conv2.b");
    W.conv2.out = C; W.conv2.in = 9 * C;
    W.sub_out = LIN("encoder.embed.out.0", d, C * F2);
  } else if (ef && ecfg->front_rate == 2) {   // conv2d2: one conv, then the projection
    W.conv1_w = P("conv1.w"); W.conv1_b = P("conv1.b");
    W.sub_out.w = P("sub_out.w"); W.sub_out.b = P("sub_out.b");
    W.sub_out.out = d; W.sub_out.in = d * m->F1();
  } else {
    W.conv1_w = P("conv1.w"); W.conv1_b = P("conv1.b");
    W.conv2.w = P("conv2.w"); W.conv2.b = P("conv2.b");
    W.conv2.out = d; W.conv2.in = 9 * d;
    W.sub_out.w = P("sub_out.w"); W.sub_out.b = P("sub_out.b");
    W.sub_out.out = d; W.sub_out.in = d * F2;
  }
  W.pe = P("pe");
  WN_TRY(bind_fbank_tables(fbt, W));
  if (!fr && !sq) W.after_norm = NORM("encoder.after_norm");
  if (has_ctc) W.ctc = LIN("ctc.ctc_lo", V, d);
  if (tf) {
    W.tf_layers.resize(c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) {
      const std::string p = "encoder.encoders." + std::to_string(i);
      TfLayer& L = W.tf_layers[i];
      L.n1 = NORM(p + ".norm1"); L.n2 = NORM(p + ".norm2");
      L.qkv = LIN(p + ".qkv", 3 * d, d);
      L.out = LIN(p + ".self_attn.linear_out", d, d);
      L.ff1 = LIN(p + ".feed_forward.w_1", F, d);
      L.ff2 = LIN(p + ".feed_forward.w_2", d, F);
    }
  } else if (fr) {
    // p = linear_pos(pos_emb) depends on weights only: every layer's rows for all distances
    // |r| < max_frames, projected once ((2 max_frames - 1) x d floats per layer)
    const int rows = 2 * fcfg->max_frames - 1;
    W.layers.resize(c.n_layers);
    WN_TRY(W.pos_tabs.ensure((size_t)c.n_layers * rows * d * sizeof(float)));
    for (int i = 0; i < c.n_layers; ++i) {
      const std::string p = "encoder.encoders." + std::to_string(i);
      EncLayer& L = W.layers[i];
      L.norm_ff_mac = NORM(p + ".norm_ff_macaron");
      L.norm_mha = NORM("fr.unit");
      L.norm_conv = NORM(p + ".norm_conv");
      L.norm_ff = NORM(p + ".norm_ff");
      L.norm_final = NORM(p + ".norm_final");
      L.conv_norm = NORM(p + ".conv_module.norm");
      L.ffm1 = LIN(p + ".feed_forward_macaron.w_1", F, d);
      L.ffm2 = LIN(p + ".feed_forward_macaron.w_2", d, F);
      L.ff1 = LIN(p + ".feed_forward.w_1", F, d);
      L.ff2 = LIN(p + ".feed_forward.w_2", d, F);
      L.qkv = LIN(p + ".qkv", 3 * d, d);
      L.out = LIN(p + ".self_attn.linear_out", d, d,
                  W.w.count(p + ".self_attn.linear_out.bias") != 0);
      L.pw1 = LIN(p + ".pw1", 4 * d, d);
      L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, 2 * d, false);
      L.bias_u = P(p + ".pos_bias_u");
      L.bias_v = P(p + ".pos_bias_v");
      L.pos_w = P(p + ".self_attn.linear_pos.weight");
      L.dw_wt = P(p + ".dw.weight");
      L.dw_b = P(p + ".dw.bias");
      L.cpad = P(p + ".cpad");
      L.pos_tab = W.pos_tabs.as<float>() + (size_t)i * rows * d;
      Linear lp; lp.w = L.pos_w; lp.b = nullptr; lp.out = d; lp.in = d;
      WN_TRY(linear(lp, P("fr.rel_pe"), d, L.pos_tab, d, rows, 0));
    }
  } else if (bf) {
    const wn_branchformer_config& b = *bcfg;
    const int dq = c.n_heads * 64, U = b.cgmlp_units, C = U / 2;
    W.layers.resize(c.n_layers);
    WN_TRY(W.pos_tabs.ensure((size_t)c.n_layers * c.max_pos * dq * sizeof(float)));
    for (int i = 0; i < c.n_layers; ++i) {
      const std::string p = "encoder.encoders." + std::to_string(i);
      EncLayer& L = W.layers[i];
      L.norm_mha = NORM(p + ".norm_mha");
      L.norm_mlp = NORM(p + ".norm_mlp");
      L.norm_final = NORM(p + ".norm_final");
      if (b.kind == 2) {
        L.norm_ff_mac = NORM(p + ".norm_ff_macaron");
        L.norm_ff = NORM(p + ".norm_ff");
        L.ffm1 = LIN(p + ".feed_forward_macaron.w_1", F, d);
        L.ffm2 = LIN(p + ".feed_forward_macaron.w_2", d, F);
        L.ff1 = LIN(p + ".feed_forward.w_1", F, d);
        L.ff2 = LIN(p + ".feed_forward.w_2", d, F);
      }
      L.qkv = LIN(p + ".qkv", 3 * dq, d);
      L.out = LIN(p + ".self_attn.linear_out", d, dq);
      L.bias_u = P(p + ".pos_bias_u");
      L.bias_v = P(p + ".pos_bias_v");
      L.pos_w = P(p + ".self_attn.linear_pos.weight");
      L.proj1 = LIN(p + ".cgmlp.channel_proj1.0", U, d);
      L.csgu_norm = NORM(p + ".cgmlp.csgu.norm");
      L.csgu_wt = P(p + ".csgu.dw.weight");
      L.csgu_b = P(p + ".csgu.dw.bias");
      if (b.linear_after_conv) L.csgu_lin = LIN(p + ".cgmlp.csgu.linear", C, C);
      L.proj2 = LIN(p + ".cgmlp.channel_proj2", d, C);
      if (b.kind == 2) {
        L.merge_wt = P(p + ".merge.dw.weight");
        L.merge_b = P(p + ".merge.dw.bias");
      }
      L.merge_proj = LIN(p + ".merge_proj", d, 2 * d);
      // p = linear_pos(pos_emb) depends on weights only: [max_pos][H x 64] per layer
      L.pos_tab = W.pos_tabs.as<float>() + (size_t)i * c.max_pos * dq;
      Linear lp; lp.w = L.pos_w; lp.b = nullptr; lp.out = dq; lp.in = d;
      WN_TRY(linear(lp, W.pe, d, L.pos_tab, dq, c.max_pos, 0));
    }
  } else if (sq) {
    const wn_squeezeformer_config& q = *qcfg;
    W.sq_preln = NORM("encoder.preln");
    if (q.reduce_idx >= 0) {
      W.sq_red_wt = P("sq.red.dw.weight");
      W.sq_red_b = P("sq.red.dw.bias");
      W.sq_red_pw = LIN("encoder.time_reduction_layer.pw_conv", d, d);
      W.sq_recover = LIN("encoder.time_recover_layer", d, d);
    }
    W.layers.resize(c.n_layers);
    WN_TRY(W.pos_tabs.ensure((size_t)c.n_layers * c.max_pos * d * sizeof(float)));
    for (int i = 0; i < c.n_layers; ++i) {
      const std::string p = "encoder.encoders." + std::to_string(i);
      EncLayer& L = W.layers[i];
      L.norm_mha = NORM(p + ".layer_norm1");
      L.norm_ff_mac = NORM(p + ".layer_norm2");
      L.norm_conv = NORM(p + ".layer_norm3");
      L.norm_final = NORM(p + ".layer_norm4");
      L.conv_norm = NORM(p + ".conv_module.norm");
      L.ffm1 = LIN(p + ".ffn1.w_1", F, d);
      L.ffm2 = LIN(p + ".ffn1.w_2", d, F);
      L.ff1 = LIN(p + ".ffn2.w_1", F, d);
      L.ff2 = LIN(p + ".ffn2.w_2", d, F);
      L.qkv = LIN(p + ".qkv", 3 * d, d);
      L.out = LIN(p + ".self_attn.linear_out", d, d);
      L.pw1 = LIN(p + ".pw1", 2 * d, d);
      L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, d);
      L.bias_u = P(p + ".pos_bias_u");
      L.bias_v = P(p + ".pos_bias_v");
      L.pos_w = P(p + ".self_attn.linear_pos.weight");
      L.dw_wt = P(p + ".dw.weight");
      L.dw_b = P(p + ".dw.bias");
      L.cpad = P(p + ".cpad");
      // p = linear_pos(pos_emb): the blocks between the reduction and the recovery run at the
      // half rate on pos_emb[:, ::2] -- (max_pos + 1) / 2 rows of pe with a row stride of 2 d
      const bool half = q.reduce_idx >= 0 && i >= q.reduce_idx && i < q.recover_idx;
      L.pos_tab = W.pos_tabs.as<float>() + (size_t)i * c.max_pos * d;
      Linear lp; lp.w = L.pos_w; lp.b = nullptr; lp.out = d; lp.in = d;
      if (half) WN_TRY(linear(lp, W.pe, 2 * d, L.pos_tab, d, (c.max_pos + 1) / 2, 0));
      else WN_TRY(linear(lp, W.pe, d, L.pos_tab, d, c.max_pos, 0));
    }
  } else if (ef) {
    WN_TRY(efficonformer_bind(W, c, *ecfg));   // (cabi_efficonformer.hip)
  } else {
    W.layers.resize(c.n_layers);
    WN_TRY(W.pos_tabs.ensure((size_t)c.n_layers * c.max_pos * d * sizeof(float)));
  }
  for (int i = 0; !tf && !fr && !bf && !sq && !ef && i < c.n_layers; ++i) {
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
    L.pw2 = LIN(p + ".conv_module.pointwise_conv2", d, d);
    L.bias_u = P(p + ".pos_bias_u");
    L.bias_v = P(p + ".pos_bias_v");
    L.pos_w = P(p + ".self_attn.linear_pos.weight");
    L.dw_wt = P(p + ".dw.weight");
    L.dw_b = P(p + ".dw.bias");
    L.cpad = P(p + ".cpad");
    // p = linear_pos(pos_emb) depends on weights only (attention.py:395-396):
    // project the whole table once instead of per batch and layer.
    L.pos_tab = W.pos_tabs.as<float>() + (size_t)i * c.max_pos * d;
    Linear lp; lp.w = L.pos_w; lp.b = nullptr; lp.out = d; lp.in = d;
    WN_TRY(linear(lp, W.pe, d, L.pos_tab, d, c.max_pos, 0));
  }
  auto DEC = [&](Decoder& D, const std::string& pfx, int nl) {
    D.embed = P(pfx + ".embed");
    D.pe = W.pe;  // same sinusoid table (embedding.py:47-56), same d_model
    D.xscale = sqrtf((float)d);
    D.max_pos = c.max_pos;
    if (c.dec_learned_pos) { D.pe = P(pfx + ".pe"); D.xscale = 1.0f; D.max_pos = c.dec_max_pos; }
    D.after = NORM(pfx + ".after_norm");
    D.out = LIN(pfx + ".output_layer", V, d);
    D.layers.resize(nl);
    for (int j = 0; j < nl; ++j) {
      const std::string p = pfx + ".decoders." + std::to_string(j);
      DecLayer& L = D.layers[j];
      L.n1 = NORM(p + ".norm1"); L.n2 = NORM(p + ".norm2"); L.n3 = NORM(p + ".norm3");
      L.self_qkv = LIN(p + ".self_qkv", 3 * d, d);
      L.self_out = LIN(p + ".self_attn.linear_out", d, d);
      L.src_q = LIN(p + ".src_attn.linear_q", d, d);
      L.src_kv = LIN(p + ".src_kv", 2 * d, d);
      L.src_out = LIN(p + ".src_attn.linear_out", d, d);
      L.ff1 = LIN(p + ".feed_forward.w_1", c.dec_ffn_dim, d);
      L.ff2 = LIN(p + ".feed_forward.w_2", d, c.dec_ffn_dim);
    }
  };
  if (has_dec) {
    if (c.bidirectional) {
      DEC(W.left, "decoder.left_decoder", c.dec_layers);
      if (c.dec_r_layers > 0) DEC(W.right, "decoder.right_decoder", c.dec_r_layers);
    } else {
      DEC(W.left, "decoder", c.dec_layers);
    }
  }
  if (tcfg) {
    const wn_transducer_config& tc = *tcfg;
    W.pred_embed = P("predictor.embed.weight");
    W.pred_rnn.resize(tc.pred_layers);
    for (int l = 0; l < tc.pred_layers; ++l) {
      const std::string sfx = "_l" + std::to_string(l);
      W.pred_rnn[l] = {P("predictor.rnn.weight_ih" + sfx), P("predictor.rnn.weight_hh" + sfx),
                       P("predictor.rnn.bias_ih" + sfx), P("predictor.rnn.bias_hh" + sfx)};
    }
    if (!scfg) W.pred_proj = LIN("predictor.projection", tc.pred_out, tc.pred_hidden);
    if (scfg) {
      W.pred_norm = NORM("predictor.norm");
      if (scfg->kind == 1) {
        W.pred_pos = P("predictor.pos_embed.weight");
        W.pred_ffn = LIN("predictor.ffn", tc.pred_embed, tc.pred_embed);
      } else {
        W.pred_conv_w = P("predictor.conv.weight");
        if (scfg->conv_bias) W.pred_conv_b = P("predictor.conv.bias");
      }
    }
    W.j_enc = LIN("joint.enc_ffn", tc.join_dim, d);
    W.j_pred = LIN("joint.pred_ffn", tc.join_dim, tc.pred_out);
    W.j_out = LIN("joint.ffn_out", V, tc.join_dim);
  }
  // (firered, branchformer, squeezeformer: the plain fp32 path, no six-product / row-block images of the
  // encoder's weights; the decoders and the CTC head get theirs as in every other model)
  WN_TRY(build_x6_images(c, W, /*skip_encoder=*/fr || bf || sq || ef));
  WN_HIP(hipDeviceSynchronize());
  *out = m.release();
  return 0;
}

extern "C" {

int wn_model_create(const wn_config* cfg, const wn_tensor* weights,
                    int32_t n_weights, int32_t device, wn_model** out) {
  return create_model_impl(cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, weights, n_weights, device, out);
}

int wn_model_create_transducer(const wn_config* cfg, const wn_transducer_config* tcfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out) {
  WN_CHECK(tcfg, "wn_model_create_transducer: null argument");
  return create_model_impl(cfg, tcfg, nullptr, nullptr, nullptr, nullptr, nullptr, weights, n_weights, device, out);
}

int wn_model_create_transducer_stateless(const wn_config* cfg, const wn_transducer_config* tcfg,
                                         const wn_stateless_predictor_config* scfg,
                                         const wn_tensor* weights, int32_t n_weights,
                                         int32_t device, wn_model** out) {
  WN_CHECK(tcfg && scfg, "wn_model_create_transducer_stateless: null argument");
  return create_model_impl(cfg, tcfg, scfg, nullptr, nullptr, nullptr, nullptr, weights, n_weights, device, out);
}

void wn_model_destroy(wn_model* m) { delete m; }

int wn_model_clone(const wn_model* src, wn_model** out) {
  WN_CHECK(src && out, "wn_model_clone: null argument");
  WN_HIP(hipSetDevice(src->device));
  std::unique_ptr<wn_model> m(new wn_model());
  m->data = src->data;      // weights, views and tables are read-only: shared
  m->cfg = src->cfg;
  m->tr.on = src->tr.on; m->tr.c = src->tr.c; m->tr.sp = src->tr.sp;
  m->fr.on = src->fr.on; m->fr.c = src->fr.c;
  m->bf.on = src->bf.on; m->bf.c = src->bf.c;
  m->sq.on = src->sq.on; m->sq.c = src->sq.c;
  m->ef.on = src->ef.on; m->ef.c = src->ef.c;
  m->pf.on = src->pf.on; m->pf.c = src->pf.c;
  m->sv.on = src->sv.on; m->sv.c = src->sv.c;
  m->device = src->device;
  m->prec = src->prec;
  m->fp8_ffn = src->fp8_ffn;
  m->tune_ovr = src->tune_ovr;
  m->ctx_buf = src->ctx_buf; m->ctx = src->ctx;
  *out = m.release();
  return 0;
}

int wn_model_set_precision(wn_model* m, int32_t precision) {
  WN_CHECK(m, "wn_model_set_precision: null model");
  WN_CHECK(precision == PREC_F32 || precision == PREC_BF16 || precision == PREC_FP8,
           "wn_model_set_precision: 0 (fp32), 1 (bf16 operands, fp32 accumulate) or 2 "
           "(bf16 + MXFP8 feed-forward GEMMs)");
  WN_CHECK(!m->fr.on || precision == PREC_F32,
           "wn_model_set_precision: a FireRed handle stays fp32 (no bf16 / fp8 kernels for its "
           "encoder)");
  WN_CHECK(!m->bf.on || precision == PREC_F32,
           "wn_model_set_precision: a Branchformer handle stays fp32 (no bf16 / fp8 kernels for "
           "its encoder)");
  WN_CHECK(!m->sq.on || precision == PREC_F32,
           "wn_model_set_precision: a Squeezeformer handle stays fp32 (no bf16 / fp8 kernels for "
           "its encoder)");
  WN_CHECK(!m->ef.on || precision == PREC_F32,
           "wn_model_set_precision: an Efficient Conformer handle stays fp32 (no bf16 / fp8 "
           "kernels for its encoder)");
  WN_CHECK(!m->pf.on || precision == PREC_F32,
           "wn_model_set_precision: a Paraformer handle stays fp32 (no bf16 / fp8 kernels for its "
           "encoder and decoder)");
  WN_CHECK(!m->sv.on || precision == PREC_F32,
           "wn_model_set_precision: a SenseVoice handle stays fp32 (no bf16 / fp8 kernels for its "
           "encoder)");
  const ModelData& W = *m->data;
  // the images belong to the model block: whichever handle asks first builds them, every
  // clone (made before or after) reads the same ones
  std::lock_guard<std::mutex> lock(W.lazy);
  if (precision != PREC_F32 && !W.weights_bf16.p && W.n_weight_elems > 0) {
    // one-time bf16 image of the weight slab for the bf16-storage GEMMs (same
    // element offsets)
    WN_HIP(hipSetDevice(m->device));
    DevBuf img;
    WN_TRY(img.ensure((size_t)W.n_weight_elems * 2));
    WN_TRY(convert_f32_to_bf16(W.weights.as<float>(), img.p, W.n_weight_elems, nullptr));
    WN_HIP(hipStreamSynchronize(nullptr));
    W.weights_bf16.swap(img);
  }
  if (precision == PREC_FP8 && !W.mx_built) {
    // one-time MXFP8 images of the feed-forward weights (w_1, w_2 of every encoder
    // layer): e4m3 [N][K] + block scales [K/128][N]
    WN_HIP(hipSetDevice(m->device));
    std::vector<const Linear*> ws;
    for (const auto& L : W.layers) { ws.push_back(&L.ffm1); ws.push_back(&L.ffm2);
                                     ws.push_back(&L.ff1); ws.push_back(&L.ff2); }
    for (const auto& L : W.tf_layers) { ws.push_back(&L.ff1); ws.push_back(&L.ff2); }
    size_t bytes = 0;
    for (const Linear* l : ws)
      if (l->w && l->in % 128 == 0)
        bytes += ((size_t)l->out * l->in + 255) / 256 * 256 + (size_t)(l->in / 128) * l->out * 4;
    DevBuf buf;
    std::map<const float*, ModelData::MxW> at;
    if (bytes > 0) {
      WN_TRY(buf.ensure(bytes));
      char* p = buf.as<char>();
      for (const Linear* l : ws) {
        if (!l->w || l->in % 128 != 0) continue;
        char* q = p;
        p += ((size_t)l->out * l->in + 255) / 256 * 256;
        unsigned* sc = reinterpret_cast<unsigned*>(p);
        p += (size_t)(l->in / 128) * l->out * 4;
        WN_TRY(mx_quantize(l->w, l->in, l->out, l->in, q, sc, l->out, nullptr));
        at[l->w] = ModelData::MxW{q, sc};
      }
      WN_HIP(hipStreamSynchronize(nullptr));
    }
    W.weights_mx.swap(buf);
    W.mx_at.swap(at);
    W.mx_built = true;
  }
  m->prec = precision == PREC_F32 ? PREC_F32 : PREC_BF16;
  m->fp8_ffn = precision == PREC_FP8;
  return 0;
}

int32_t wn_model_get_precision(const wn_model* m) {
  return m ? (m->fp8_ffn ? (int32_t)PREC_FP8 : m->prec) : -1;
}

int32_t wn_batch_size(const wn_model* m) { return m ? m->B : -1; }

int wn_model_set_encode_gate(wn_model* m, void* event) {
  WN_CHECK(m, "wn_model_set_encode_gate: null handle");
  m->enc_gate = (hipEvent_t)event;
  return 0;
}

int wn_profile_enable(wn_model* m, int32_t on) {
  WN_CHECK(m, "wn_profile_enable: null model");
  m->prof_on = on != 0;
  m->prof_stride = on > 1 ? (unsigned)on : 6u;   // on = 1: every 6th launch; on = N > 1: every N-th
  m->prof_used = 0;
  m->prof_flops = 0.0;
  return 0;
}

const char* wn_profile_kernel_name(const wn_model* m) {
  return m ? m->prof_kernel : "";
}

int32_t wn_profile_ffn_split(const wn_model* m) { return m ? m->prof_split : 0; }

int wn_profile_gemm_clocks(uint64_t* out64) {
  WN_CHECK(out64, "wn_profile_gemm_clocks: null output");
  if (wn::tune().x6_probe == 8)   // the row-block kernel's phase stamps (tools/x6r_clocks.py)
    return wn::gemm_x6r_clocks(reinterpret_cast<unsigned long long*>(out64));
  if (wn::tune().lp_probe & 4)   // the pipelined bf16 / MXFP8 kernel stamped last (tools/lp_clocks.py)
    return wn::gemm_lp_clocks(reinterpret_cast<unsigned long long*>(out64));
  return wn::gemm_x6_clocks(reinterpret_cast<unsigned long long*>(out64));
}

int wn_profile_ffn_clocks(uint64_t* out64) {
  WN_CHECK(out64, "wn_profile_ffn_clocks: null output");
  return wn::ffn_x6f_clocks(reinterpret_cast<unsigned long long*>(out64));
}

int wn_profile_collect(wn_model* m, int32_t* n_launches, double* total_ms,
                       double* total_flops) {
  WN_CHECK(m && n_launches && total_ms && total_flops, "wn_profile_collect: null");
  double ms = 0.0;
  for (size_t i = 0; i + 1 < m->prof_used; i += 2) {
    WN_HIP(hipEventSynchronize(m->prof_ev[i + 1]));
    float t = 0.f;
    WN_HIP(hipEventElapsedTime(&t, m->prof_ev[i], m->prof_ev[i + 1]));
    ms += t;
  }
  *n_launches = (int32_t)(m->prof_used / 2);
  *total_ms = ms;
  *total_flops = m->prof_flops;
  m->prof_used = 0;
  m->prof_flops = 0.0;
  return 0;
}

int wn_debug_set(wn_model* m, const char* key, int32_t value) {
  WN_CHECK(m && key, "wn_debug_set: null argument");
  const std::string k(key);
  if (k == "n_layers") m->dbg_layers = value;
  else if (k == "skip_after_norm") m->dbg_skip_after_norm = value;
  else { set_error("wn_debug_set: unknown key " + k); return -1; }
  return 0;
}

int wn_tune_set(const char* key, int32_t value) {
  WN_CHECK(key, "wn_tune_set: null key");
  const std::string k(key);
  int* f = tune_field(g_tune_default, k);
  if (!f) { set_error("wn_tune_set: unknown key " + k); return -1; }
  WN_CHECK(value != TUNE_INHERIT, "wn_tune_set: INT32_MIN is the per-handle 'inherit' marker");
  if (tune_check(k, value, "wn_tune_set") != 0) return -1;
  *f = value;
  return 0;
}

int wn_model_tune_set(wn_model* m, const char* key, int32_t value) {
  WN_CHECK(m && key, "wn_model_tune_set: null argument");
  WN_ENTER(m);
  const std::string k(key);
  int* f = tune_field(m->tune_ovr, k);
  if (!f) { set_error("wn_model_tune_set: unknown key " + k); return -1; }
  if (tune_check(k, value, "wn_model_tune_set") != 0) return -1;
  *f = value;
  return 0;
}

int wn_tune_get(const wn_model* m, const char* key, int32_t* value) {
  WN_CHECK(key && value, "wn_tune_get: null argument");
  const std::string k(key);
  Tune eff = g_tune_default;
  if (m) tune_resolve(m->tune_ovr, &eff);
  const int* f = tune_field(eff, k);
  if (!f) { set_error("wn_tune_get: unknown key " + k); return -1; }
  *value = *f;
  return 0;
}

int wn_workspace_create(int32_t device, wn_model** out) {
  WN_CHECK(out, "wn_workspace_create: null argument");
  WN_HIP(hipSetDevice(device));
  wn_model* m = new wn_model();
  memset(&m->cfg, 0, sizeof(m->cfg));
  m->device = device;
  *out = m;
  return 0;
}

}  // extern "C"
