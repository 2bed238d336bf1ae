// C ABI (include/wenet_amd.h), SenseVoice Small handles (`model: sensevoice_small`,
// wenet/models/sensevoice/sensevoice_small_model.py): the entry point that creates one, the query
// ids of the next encode, what wn_encode runs on it (sv_front, the encoders0 / encoders stack,
// after_norm, the tp_encoders stack, tp_norm) and the operator hook of the front end.  The layer
// stacks are the Paraformer's (pf_encoder_layers, cabi_paraformer.hip): a plain fp32 path.
// In the hook offsets, lengths and ids are HOST arrays, checked against the caller's buffers
// BEFORE anything is launched: every loop bound of a kernel comes from a length validated on the
// host.
#include "model_state.h"
#include "weight_stage.h"

namespace wn {
namespace {

const int SV_DEFAULT_QID[SV_QUERY] = {0, 1, 2, 15};   // auto | event | emotion | woitn

bool sv_qid_ok(const int32_t* qid, int n) {
  for (int i = 0; i < n; ++i)
    if (qid[i] < 0 || qid[i] >= SV_EMBED) return false;
  return true;
}

std::string sv_layer_name(const char* stack, int i) {
  return std::string("encoder.") + stack + "." + std::to_string(i);
}

// one AliParaformerEncoderLayer over `in` input columns (ld columns in the staged image)
int sv_stage_layer(const Src& src, HostStage& hs, const std::string& q, int in, int ld, int d,
                   int F, int K) {
  WN_TRY(stage_norm(src, hs, q + ".norm1", in));
  WN_TRY(stage_norm(src, hs, q + ".norm2", d));
  if (ld != in) {   // K = 560 -> 576 with zero columns: the fp32 GEMM needs K % 32 == 0
    WN_GET(w, q + ".self_attn.linear_q_k_v.weight", (int64_t)3 * d * in);
    WN_GET(b, q + ".self_attn.linear_q_k_v.bias", 3 * d);
    float* t = hs.alloc(q + ".self_attn.linear_q_k_v.weight", (size_t)3 * d * ld);
    for (int o = 0; o < 3 * d; ++o)
      memcpy(t + (size_t)o * ld, w + (size_t)o * in, sizeof(float) * in);
    hs.add(q + ".self_attn.linear_q_k_v.bias", b, 3 * d);
  } else {
    WN_TRY(stage_linear(src, hs, q + ".self_attn.linear_q_k_v", 3 * d, in));
  }
  {  // fsmn_block.weight (d, 1, K) -> [K][d] tap-major (merge_dwconv)
    WN_GET(w, q + ".self_attn.fsmn_block.weight", (int64_t)d * K);
    float* t = hs.alloc(q + ".self_attn.fsmn", (size_t)K * d);
    for (int ch = 0; ch < d; ++ch)
      for (int k = 0; k < K; ++k) t[(size_t)k * d + ch] = w[(size_t)ch * K + k];
  }
  WN_TRY(stage_linear(src, hs, q + ".self_attn.linear_out", d, d));
  WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_1", F, d));
  WN_TRY(stage_linear(src, hs, q + ".feed_forward.w_2", d, F));
  return 0;
}

}  // namespace
}  // namespace wn

// wn_encode on a SenseVoice handle.  Every utterance is encoded as the reference encodes it
// ALONE (the Paraformer's deviation): 4 query rows + ceil(len / 6) LFR rows whose frame
// indices clamp to the utterance's own last frame; an utterance without frames has no rows.
int encode_sensevoice(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                      int T, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const wn_sensevoice_config& p = m->sv.c;
  const int d = c.d_model, F = c.ffn_dim, D0 = p.lfr_m * c.feat_dim;
  const int ld0 = cdiv(D0, 32) * 32;
  // the stored ids serve this encode only, however it ends
  std::vector<int> qid;
  qid.swap(m->sv.qid);
  auto out_len = [&](int n) { return n > 0 ? (n + p.lfr_n - 1) / p.lfr_n + SV_QUERY : 0; };
  const int Tp = out_len(T);
  WN_CHECK(B < 32768, "wn_encode: more than 32767 utterances");
  WN_CHECK(qid.empty() || (int)qid.size() == B * SV_QUERY,
           "wn_encode: B = " + std::to_string(B) + " differs from the B = " +
               std::to_string(qid.size() / SV_QUERY) + " of wn_sensevoice_set_queries");
  WN_CHECK(Tp - SV_QUERY <= p.max_frames,
           "wn_encode: an utterance of " + std::to_string(T) + " frames gives " +
               std::to_string(Tp - SV_QUERY) + " LFR frames, more than the " +
               std::to_string(p.max_frames) + " the position rows of this handle cover");
  if (qid.empty()) {
    qid.resize((size_t)B * SV_QUERY);
    for (int i = 0; i < B * SV_QUERY; ++i) qid[i] = SV_DEFAULT_QID[i % SV_QUERY];
  }
  std::vector<int> off(B), len(B), desc((size_t)B * (1 + SV_QUERY));
  int M = 0, max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    desc[b] = L;
    off[b] = M; len[b] = out_len(L); M += len[b];
    max_len = std::max(max_len, len[b]);
    if (enc_lens_host) enc_lens_host[b] = len[b];
  }
  std::copy(qid.begin(), qid.end(), desc.begin() + B);
  WN_TRY(set_layout(m, B, Tp, off, len, M, s));
  WN_TRY(m->stage.end(s));
  if (M > 0) {
    WN_TRY(m->sv_stage.begin(desc.size() * sizeof(int) + 256));
    WN_TRY(m->sv_stage.put(m->sv_desc, desc.data(), desc.size() * sizeof(int), s));
    WN_TRY(m->sv_stage.end(s));
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * std::max(d, ld0) * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * F * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    WN_TRY(m->enc.ensure((size_t)M * d * sizeof(float)));
    SvFrontArgs fa;
    fa.feats = feats_dev; fa.mean = W.cmvn_mean; fa.istd = W.cmvn_istd; fa.embed = W.sv.embed;
    fa.pe = W.pf.pe; fa.ln_w = W.pf.enc[0].n1.w; fa.ln_b = W.pf.enc[0].n1.b;
    fa.out = m->t1.as<float>(); fa.ldo = ld0;
    fa.len = m->sv_desc.as<int>(); fa.off = m->d_off.as<int>(); fa.qid = fa.len + B;
    fa.B = B; fa.T = T; fa.F = c.feat_dim; fa.m = p.lfr_m; fa.n = p.lfr_n; fa.max_rows = max_len;
    fa.xscale = sqrtf((float)d); fa.eps = c.norm_eps;
    WN_TRY(sv_front(fa, s));
    WN_TRY(pf_encoder_layers(m, W.pf.enc, c.n_layers, true, ld0, p.kernel_size, B, M, max_len, s));
    // after_norm (through the output buffer, back into the residual rows), the second stack, then
    // tp_norm into the handle's encoder output
    float* x = m->x.as<float>();
    WN_TRY(ln(W.after_norm, x, m->enc.as<float>(), M, d, c.norm_eps, s));
    WN_HIP(hipMemcpyAsync(x, m->enc.p, (size_t)M * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    WN_TRY(pf_encoder_layers(m, W.sv.tp, p.tp_blocks, false, d, p.kernel_size, B, M, max_len, s));
    WN_TRY(ln(W.sv.tp_norm, x, m->enc.as<float>(), M, d, c.norm_eps, s));
  } else {
    WN_TRY(m->enc.ensure((size_t)d * sizeof(float)));
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

int wn_model_create_sensevoice(const wn_config* cfg, const wn_sensevoice_config* scfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out) {
  WN_CHECK(cfg && scfg && weights && out, "wn_model_create_sensevoice: null argument");
  const wn_config& c = *cfg;
  const wn_sensevoice_config& p = *scfg;
  const int d = c.d_model, H = c.n_heads, F = c.ffn_dim, V = c.vocab, K = p.kernel_size;
  WN_CHECK(p.n_query == SV_QUERY, "sensevoice: n_query must be 4");
  WN_CHECK(p.n_embed == SV_EMBED, "sensevoice: n_embed must be 16");
  WN_CHECK(H > 0 && H < 256 && (d == H * 64 || d == H * 128),
           "sensevoice: d_model / attention_heads must be 64 or 128");
  WN_CHECK(d % 64 == 0 && d <= 1280, "sensevoice: d_model % 64, at most 1280");
  WN_CHECK(F > 0 && F % 32 == 0, "sensevoice: linear_units % 32");
  WN_CHECK(c.n_layers >= 1 && p.tp_blocks >= 0, "sensevoice: num_blocks / tp_blocks");
  WN_CHECK(p.lfr_m >= 1 && p.lfr_n >= 1 && c.feat_dim >= 1 && p.lfr_m * c.feat_dim <= LFR_MAX_D &&
               (p.lfr_m * c.feat_dim) % 4 == 0,
           "sensevoice: lfr_m * input_dim at most 576");
  WN_CHECK(K >= 1 && K <= CSGU_MAX_K && K % 2 == 1, "sensevoice: kernel_size odd, in [1, 63]");
  WN_CHECK(p.max_frames >= 1 && p.max_frames <= 8192, "sensevoice: max_frames in [1, 8192]");
  WN_CHECK(c.has_cmvn == 1, "sensevoice: global_cmvn is required (the model asserts it)");
  WN_CHECK(V >= 1 && c.norm_eps > 0.f, "sensevoice: vocab / norm_eps");
  WN_HIP(hipSetDevice(device));
  std::unique_ptr<wn_model> m(new wn_model());
  m->cfg = c;
  m->device = device;
  m->sv.on = true; m->sv.c = p;
  const std::shared_ptr<ModelData> data = std::make_shared<ModelData>();
  m->data = data;
  ModelData& W = *data;
  Src src;
  for (int i = 0; i < n_weights; ++i) src.t[weights[i].name] = {weights[i].data, weights[i].numel};
  const int D0 = p.lfr_m * c.feat_dim, ld0 = cdiv(D0, 32) * 32;
  HostStage hs;
  {
    WN_GET(mean, "global_cmvn.mean", D0);
    WN_GET(istd, "global_cmvn.istd", D0);
    hs.add("cmvn.mean", mean, D0);
    hs.add("cmvn.istd", istd, D0);
    WN_GET(e, "embed.weight", (int64_t)SV_EMBED * D0);
    hs.add("sv.embed", e, (size_t)SV_EMBED * D0);
  }
  const FbankTables fbt = make_fbank_tables(c.feat_dim);
  stage_fbank_tables(fbt, hs, W);
  const int pe_rows = p.max_frames + SV_QUERY + 1;
  {  // WhisperPositionalEncoding of depth D0 (transformer/embedding.py:150-164), rebuilt in fp64:
     // [sin | cos] halves over D0 / 2 timescales; row p = position p
    float* t = hs.alloc("pf.pe", (size_t)pe_rows * D0);
    const int half = D0 / 2;
    const double inc = log(10000.0) / (double)(half - 1);
    for (int pos = 0; pos < pe_rows; ++pos)
      for (int i = 0; i < half; ++i) {
        const double st = (double)pos * exp(-inc * (double)i);
        t[(size_t)pos * D0 + i] = (float)sin(st);
        t[(size_t)pos * D0 + half + i] = (float)cos(st);
      }
  }
  hs.alloc("pf.zero_bias", d);
  auto enc_name = [&](int i) {
    return i == 0 ? std::string("encoder.encoders0.0") : sv_layer_name("encoders", i - 1);
  };
  for (int i = 0; i < c.n_layers; ++i)
    WN_TRY(sv_stage_layer(src, hs, enc_name(i), i == 0 ? D0 : d, i == 0 ? ld0 : d, d, F, K));
  WN_TRY(stage_norm(src, hs, "encoder.after_norm", d));
  for (int i = 0; i < p.tp_blocks; ++i)
    WN_TRY(sv_stage_layer(src, hs, sv_layer_name("tp_encoders", i), d, d, d, F, K));
  WN_TRY(stage_norm(src, hs, "encoder.tp_norm", d));
  WN_TRY(stage_linear(src, hs, "ctc.ctc_lo", V, d));
  // ---- upload -------------------------------------------------------------------------------
  WN_TRY(W.weights.ensure(hs.data.size() * sizeof(float)));
  W.n_weight_elems = (int64_t)hs.data.size();
  WN_HIP(hipMemcpy(W.weights.p, hs.data.data(), hs.data.size() * sizeof(float),
                   hipMemcpyHostToDevice));
  const float* base = W.weights.as<float>();
  for (auto& kv : hs.at) W.w[kv.first] = base + kv.second.first;
  auto P = [&](const std::string& n) { return W.w.at(n); };
  auto LIN = [&](const std::string& q, int o, int i) {
    Linear l; l.w = P(q + ".weight"); l.b = P(q + ".bias"); l.out = o; l.in = i; return l;
  };
  auto NORM = [&](const std::string& q) {
    Norm n; n.w = P(q + ".weight"); n.b = P(q + ".bias"); return n;
  };
  auto LAYER = [&](const std::string& q, int in) {
    PfEncLayer L;
    L.n1 = NORM(q + ".norm1"); L.n2 = NORM(q + ".norm2");
    L.qkv = LIN(q + ".self_attn.linear_q_k_v", 3 * d, in);
    L.out = LIN(q + ".self_attn.linear_out", d, d);
    L.ff1 = LIN(q + ".feed_forward.w_1", F, d);
    L.ff2 = LIN(q + ".feed_forward.w_2", d, F);
    L.fsmn_wt = P(q + ".self_attn.fsmn");
    return L;
  };
  W.cmvn_mean = P("cmvn.mean"); W.cmvn_istd = P("cmvn.istd");
  WN_TRY(bind_fbank_tables(fbt, W));
  W.after_norm = NORM("encoder.after_norm");
  W.ctc = LIN("ctc.ctc_lo", V, d);
  W.pf.pe = P("pf.pe");
  W.pf.zero_bias = P("pf.zero_bias");
  for (int i = 0; i < c.n_layers; ++i) W.pf.enc.push_back(LAYER(enc_name(i), i == 0 ? ld0 : d));
  for (int i = 0; i < p.tp_blocks; ++i)
    W.sv.tp.push_back(LAYER(sv_layer_name("tp_encoders", i), d));
  W.sv.tp_norm = NORM("encoder.tp_norm");
  W.sv.embed = P("sv.embed");
  // (the plain fp32 path: no six-product / row-block images, as for the Paraformer)
  WN_HIP(hipDeviceSynchronize());
  *out = m.release();
  return 0;
}

int wn_sensevoice_set_queries(wn_model* m, const int32_t* qid_host, int32_t B) {
  WN_CHECK(m, "wn_sensevoice_set_queries: null model");
  WN_ENTER(m);
  WN_CHECK(m->sv.on, "wn_sensevoice_set_queries: not a SenseVoice handle");
  if (!qid_host) { m->sv.qid.clear(); return 0; }
  WN_CHECK(B > 0 && B < 32768, "wn_sensevoice_set_queries: B out of range");
  WN_CHECK(sv_qid_ok(qid_host, B * SV_QUERY),
           "wn_sensevoice_set_queries: qid_host holds an id outside [0, 16)");
  m->sv.qid.assign(qid_host, qid_host + (size_t)B * SV_QUERY);
  return 0;
}

int wn_op_sv_front(const float* feats, const float* mean, const float* istd, const float* embed,
                   const float* pe, int32_t pe_rows, const float* ln_w, const float* ln_b,
                   float* out, int32_t ldo, int32_t out_rows, const int32_t* lens,
                   const int32_t* out_off, const int32_t* qid, int32_t* out_len, int32_t B,
                   int32_t T, int32_t F, int32_t m, int32_t n, float xscale, float eps,
                   void* stream) {
  WN_CHECK(feats && embed && pe && ln_w && ln_b && out && lens && out_off && qid && out_len,
           "sv_front: null argument");
  WN_CHECK((mean == nullptr) == (istd == nullptr), "sv_front: mean and istd come together");
  WN_CHECK(B > 0 && B < 65536 && T > 0 && F > 0 && m > 0 && n > 0, "sv_front: B / T / F / m / n");
  WN_CHECK(m * F <= LFR_MAX_D && ldo >= m * F && ldo <= LFR_MAX_D,
           "sv_front: m * F <= ldo <= 576");
  WN_CHECK(sv_qid_ok(qid, B * SV_QUERY), "sv_front: a query id outside [0, 16)");
  int max_rows = 0;
  std::vector<int> h((size_t)B * (2 + SV_QUERY));
  int64_t end = 0;
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens[b] >= 0 && lens[b] <= T, "sv_front: a length outside [0, T]");
    out_len[b] = lens[b] > 0 ? (lens[b] + n - 1) / n + SV_QUERY : 0;
    max_rows = std::max(max_rows, out_len[b]);
    // rows inside [0, out_rows), ascending, disjoint
    WN_CHECK(out_off[b] >= end && (int64_t)out_off[b] + out_len[b] <= out_rows,
             "sv_front: rows outside the buffer, unordered or overlapping");
    end = (int64_t)out_off[b] + out_len[b];
    h[b] = lens[b]; h[B + b] = out_off[b];
  }
  std::copy(qid, qid + (size_t)B * SV_QUERY, h.begin() + 2 * B);
  WN_CHECK(max_rows > 0, "sv_front: empty");
  WN_CHECK(max_rows + 1 <= pe_rows, "sv_front: position rows outside the table");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(desc.ensure(h.size() * sizeof(int)));
  WN_HIP(hipMemcpyAsync(desc.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipStreamSynchronize(s));
  SvFrontArgs a;
  a.feats = feats; a.mean = mean; a.istd = istd; a.embed = embed; a.pe = pe;
  a.ln_w = ln_w; a.ln_b = ln_b; a.out = out; a.ldo = ldo;
  a.len = desc.as<int>(); a.off = a.len + B; a.qid = a.len + 2 * B;
  a.B = B; a.T = T; a.F = F; a.m = m; a.n = n; a.max_rows = max_rows;
  a.xscale = xscale; a.eps = eps;
  return sv_front(a, s);
}

}  // extern "C"
