// Engine of libwenet_amd: the error string and the tune tables, linear() and its GEMM routing
// (v_mfma_f32 / six-product / bf16 / MXFP8 kernels), the weight plane images, the subsampling
// front ends with their small kernels, the row layout of a batch and the Transformer layers.
// The Conformer layers are conformer.hip; the state is model_state.h; the C ABI is cabi_*.hip.
#include <algorithm>
#include "model_state.h"

namespace wn {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
const char* last_error_cstr() { return g_error.c_str(); }

}  // namespace wn

thread_local const std::map<const float*, ModelData::MxW>* t_mx = nullptr;
// plane images of the current model's weights and its activation-image scratch: linear()
// routes the large fp32 GEMMs to the six-product kernel through them (gemm_x6.hip)
thread_local const std::map<const float*, const void*>* t_x6 = nullptr;
thread_local DevBuf* t_x6_a = nullptr;

// ---- tuning knobs (tune.h) --------------------------------------------------------------------
namespace wn {
Tune g_tune_default;
thread_local const Tune* t_tune = nullptr;

int* tune_field(Tune& t, const std::string& key) {
#define X(name, dflt) if (key == #name) return &t.name;
  WN_TUNE_KEYS(X)
#undef X
  return nullptr;
}

int tune_check(const std::string& key, int32_t value, const char* who) {
  if (value == TUNE_INHERIT) return 0;
  if (key == "rnnt_lookahead" && (value < 1 || value > 16)) {
    set_error(std::string(who) + ": rnnt_lookahead must be in [1, 16]");
    return -1;
  }
#ifndef WN_ABLATION
  if (key == "x6_probe" && (value & ~12) != 0) {
    set_error(std::string(who) + ": x6_probe 1 / 2 (no MFMAs / no DMA) need a WN_ABLATION build");
    return -1;
  }
  if (key == "ffn_x6f_var" && value != 0 && value != 25088) {
    set_error(std::string(who) + ": ffn_x6f_var variants other than the clock-stamp form "
              "(25088) need a WN_ABLATION build");
    return -1;
  }
  if (key == "attn_x6_var" && value != 0) {
    set_error(std::string(who) + ": attn_x6_var needs a WN_ABLATION build");
    return -1;
  }
  if (key == "ffn_x6f_ring" && value != 3) {
    set_error(std::string(who) + ": ffn_x6f_ring needs a WN_ABLATION build");
    return -1;
  }
#endif
  return 0;
}

void tune_resolve(const Tune& ovr, Tune* eff) {
#define X(name, dflt) eff->name = ovr.name != TUNE_INHERIT ? ovr.name : g_tune_default.name;
  WN_TUNE_KEYS(X)
#undef X
}

Tune tune_all_inherit() {
  Tune t;
#define X(name, dflt) t.name = TUNE_INHERIT;
  WN_TUNE_KEYS(X)
#undef X
  return t;
}
}  // namespace wn


// bf16-storage form of the bf16 mode: LayerNorm output, FFN hidden and attention
// context are written as bf16 (their only consumers are GEMMs that round them to
// bf16 first thing), the GEMMs read the bf16 image of the weight slab.
bool bf16_store_active() {
  return t_gemm_prec == PREC_BF16 && tune().bf16_store != 0 && tune().attn_bf16 != 0 &&
         t_wslab_bf16 != nullptr;
}

int upload_desc(wn_model* m, DevBuf& buf, const std::vector<int>& v,
                hipStream_t s) {
  return m->stage.put(buf, v.data(), v.size() * sizeof(int), s);
}

// a_bf16 / c_bf16: A / C are bf16 matrices in the same buffers (lda / ldc stay the
// element counts) -- only under bf16_store_active().
thread_local bool t_linear_took_x6 = false;   // what the last linear() of this thread ran on

int linear(const Linear& l, const float* A, int lda, float* C, int ldc, int M,
           hipStream_t s, int act, const float* resid, int ldr, float alpha, bool glu, bool a_bf16,
           bool c_bf16) {
  // Large fp32 GEMMs (the d = 512 encoders' projections, the decoders' GEMMs over B x N x L
  // rows): split A into planes (one pass, 4 B in / 6 B out) and run the six-product kernel
  // -- worth it from ~6 GFLOP on, where the split is a few per cent of the GEMM it halves.
  if (t_gemm_prec == PREC_F32 && tune().gemm_x6 != 0 && tune().x6_linear != 0 && t_x6 && t_x6_a && !glu &&
      !a_bf16 && !c_bf16 && l.in % 16 == 0 && l.out % 4 == 0 && lda % 4 == 0 && ldc % 4 == 0 &&
      (resid == nullptr || ldr % 4 == 0) && M >= 512 &&
      2.0 * M * (double)l.out * l.in >= 1e8 * g_x6_linear_min) {
    auto it = t_x6->find(l.w);
    if (it != t_x6->end()) {
      t_linear_took_x6 = true;
      WN_TRY(t_x6_a->ensure(x6_bytes(M, l.in)));
      WN_TRY(x6_split(A, M, l.in, lda, t_x6_a->as<char>(), s));
      X6Args x;
      x.A3 = t_x6_a->as<char>(); x.B3 = it->second; x.M = M; x.N = l.out; x.K = l.in;
      x.epi = 0; x.bias = l.b; x.resid = resid; x.ldr = ldr; x.alpha = alpha; x.act = act;
      x.C = C; x.ldc = ldc;
      return gemm_x6(x, s);
    }
  }
  t_linear_took_x6 = false;
  GemmArgs g;
  g.A = A; g.W = l.w; g.bias = l.b; g.C = C; g.resid = resid;
  g.M = M; g.N = l.out; g.K = l.in; g.lda = lda; g.ldc = ldc; g.ldr = ldr;
  g.alpha = alpha; g.act = act; g.glu = glu;
  g.a_bf16 = a_bf16; g.c_bf16 = c_bf16;
  return gemm_f32(g, s);
}

int ln(const Norm& n, const float* x, float* y, int M, int D, float eps,
       hipStream_t s, bool y_bf16) {
  return layernorm(x, D, n.w, n.b, y, D, M, D, eps, s, y_bf16);
}

// behind the last encoder layer: m->enc = after_norm(m->x) (debug: x as it stands)
int after_norm_out(wn_model* m, hipStream_t s) {
  const int d = m->cfg.d_model, M = m->rows;
  WN_TRY(m->enc.ensure((size_t)std::max(M, 1) * d * sizeof(float)));
  if (m->dbg_skip_after_norm) {
    WN_HIP(hipMemcpyAsync(m->enc.p, m->x.p, (size_t)M * d * sizeof(float),
                          hipMemcpyDeviceToDevice, s));
    return 0;
  }
  return ln(m->data->after_norm, m->x.as<float>(), m->enc.as<float>(), M, d, m->cfg.norm_eps, s);
}

// Plane images (gemm_x6.hip) of the encoder's feed-forward weights, once per model.
int build_x6_images(const wn_config& cfg, ModelData& W, bool skip_encoder) {
  std::vector<const Linear*> ws;
  static const std::vector<EncLayer> no_layers;
  const std::vector<EncLayer>& enc_layers = skip_encoder ? no_layers : W.layers;
  for (const auto& L : enc_layers) { ws.push_back(&L.ffm1); ws.push_back(&L.ffm2);
                                    ws.push_back(&L.ff1); ws.push_back(&L.ff2);
                                    ws.push_back(&L.qkv); ws.push_back(&L.out);
                                    ws.push_back(&L.pw2); ws.push_back(&L.pw1); }
  for (const Decoder* D : {&W.left, &W.right})
    for (const auto& L : D->layers) {
      ws.push_back(&L.self_qkv); ws.push_back(&L.self_out); ws.push_back(&L.src_q);
      ws.push_back(&L.src_kv); ws.push_back(&L.src_out); ws.push_back(&L.ff1);
      ws.push_back(&L.ff2);
    }
  // the Transformer encoder of the Whisper configuration (round 3): its fp32 mode goes through
  // linear() -> split pass + six-product GEMM like every other large fp32 GEMM
  for (const auto& L : W.tf_layers) { ws.push_back(&L.qkv); ws.push_back(&L.out);
                                       ws.push_back(&L.ff1); ws.push_back(&L.ff2); }
  if (W.conv2.w && !skip_encoder) ws.push_back(&W.conv2);   // [d][(ky*3+kx)*d + c]: 16-channel k blocks per tap
  if (W.sub_out.w && !skip_encoder) ws.push_back(&W.sub_out);   // K slices straight from conv2's fp32 output
  std::vector<const Linear*> vocab;          // V rows; the image pads them to a multiple of 32
  if (W.ctc.w) vocab.push_back(&W.ctc);
  for (const Decoder* D : {&W.left, &W.right})
    if (D->out.w) vocab.push_back(&D->out);
  for (const Linear* l : vocab) ws.push_back(l);
  size_t bytes = 0;
  for (const Linear* l : ws)
    if (l->w && l->in % 16 == 0) bytes += x6_bytes(l->out, l->in);
  if (bytes > 0) {
    WN_TRY(W.weights_x6.ensure(bytes));
    char* p = W.weights_x6.as<char>();
    for (const Linear* l : ws) {
      if (!l->w || l->in % 16 != 0 || W.x6_at.count(l->w)) continue;
      WN_TRY(x6_split(l->w, l->out, l->in, l->in, p, nullptr));
      W.x6_at[l->w] = p;
      p += x6_bytes(l->out, l->in);
    }
  }
  // fused six-product feed-forward module (ffn_x6f.hip, d_model 256): the second layer's image
  // with the k slots of a 16-unit block in the order a lane holds its hidden values
  if (cfg.d_model == 256) {
    std::vector<const Linear*> w2s;
    for (const auto& L : enc_layers) { w2s.push_back(&L.ffm2); w2s.push_back(&L.ff2); }
    size_t pbytes = 0;
    for (const Linear* l : w2s)
      if (l->w && l->in % 64 == 0 && l->out == 256) pbytes += x6_bytes(l->out, l->in);
    if (pbytes > 0) {
      WN_TRY(W.weights_x6p.ensure(pbytes));
      char* q = W.weights_x6p.as<char>();
      for (const Linear* l : w2s) {
        if (!l->w || l->in % 64 != 0 || l->out != 256 || W.x6p_at.count(l->w)) continue;
        WN_TRY(x6_split_perm(l->w, l->out, l->in, l->in, q, nullptr));
        W.x6p_at[l->w] = q;
        q += x6_bytes(l->out, l->in);
      }
    }
  }
  // QKV projections of 4-head / d_model-256 encoders, rows regrouped per head (gemm_x6r.hip
  // epi 4: wave h of a row block owns [Q_h | K_h | V_h]): new row h 192 + part 64 + j = old row
  // part 256 + h 64 + j.  One fp32 staging copy, then the ordinary split
  if (cfg.d_model == 256 && cfg.n_heads == 4) {
    size_t n_q = 0;
    for (const auto& L : enc_layers)
      if (L.qkv.w && L.qkv.b && L.qkv.out == 768 && L.qkv.in == 256 && L.pos_tab) ++n_q;
    if (n_q > 0) {
      const size_t img = x6_bytes(768, 256), per = img + 768 * sizeof(float);
      DevBuf stage;
      WN_TRY(stage.ensure((size_t)768 * 256 * sizeof(float)));
      WN_TRY(W.weights_x6q.ensure(n_q * per));
      char* q = W.weights_x6q.as<char>();
      for (const auto& L : enc_layers) {
        if (!(L.qkv.w && L.qkv.b && L.qkv.out == 768 && L.qkv.in == 256 && L.pos_tab) ||
            W.x6q_at.count(L.qkv.w))
          continue;
        float* qb = reinterpret_cast<float*>(q + img);
        for (int h = 0; h < 4; ++h)
          for (int part = 0; part < 3; ++part) {
            const size_t nr = (size_t)h * 192 + part * 64, orow = (size_t)part * 256 + h * 64;
            WN_HIP(hipMemcpyAsync(stage.as<float>() + nr * 256, L.qkv.w + orow * 256,
                                  64 * 256 * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
            WN_HIP(hipMemcpyAsync(qb + nr, L.qkv.b + orow, 64 * sizeof(float),
                                  hipMemcpyDeviceToDevice, nullptr));
          }
        WN_TRY(x6_split(stage.as<float>(), 768, 256, 256, q, nullptr));
        W.x6q_at[L.qkv.w] = {q, qb};
        q += per;
      }
      WN_HIP(hipStreamSynchronize(nullptr));   // `stage` goes away with this scope
    }
  }
  // the six-product kernel stores 16-B pieces: the vocabulary-sized layers run with N = V
  // rounded up to 4 (the image rows past V are zero, their bias too) and their logits rows
  // get that pitch
  size_t b4_floats = 0;
  for (const Linear* l : vocab)
    if (l->b && l->out % 4 != 0) b4_floats += (size_t)(l->out + 3) / 4 * 4;
  if (b4_floats > 0) {
    WN_TRY(W.bias4_buf.ensure(b4_floats * sizeof(float)));
    WN_HIP(hipMemsetAsync(W.bias4_buf.p, 0, b4_floats * sizeof(float), nullptr));
    float* q = W.bias4_buf.as<float>();
    for (const Linear* l : vocab) {
      if (!l->b || l->out % 4 == 0 || W.bias4.count(l->w)) continue;
      WN_HIP(hipMemcpyAsync(q, l->b, (size_t)l->out * sizeof(float), hipMemcpyDeviceToDevice,
                            nullptr));
      W.bias4[l->w] = q;
      q += (l->out + 3) / 4 * 4;
    }
  }
  return 0;
}

// A vocabulary-sized layer (N = V, any V) into a logits buffer whose rows have the pitch ldc
// (>= V rounded up to 4): the six-product GEMM when the layer has a plane image (and, for V % 4 !=
// 0, a padded bias), else linear().
int vocab_linear(wn_model* m, const Linear& l, const float* A, int lda, float* C, int ldc,
                 int M, hipStream_t s) {
  const ModelData& W = *m->data;
  const int V = l.out, V4 = (V + 3) / 4 * 4;
  WN_CHECK(ldc >= V4 && ldc % 4 == 0, "vocab_linear: pitch");
  const void* w6 = nullptr;
  const float* bias = l.b;
  if (t_gemm_prec == PREC_F32 && tune().gemm_x6 != 0 && tune().x6_linear != 0 &&
      l.in % 16 == 0 && lda % 4 == 0 && M >= 512) {
    auto it = W.x6_at.find(l.w);
    if (it != W.x6_at.end()) w6 = it->second;
    if (w6 && V != V4 && l.b) {     // ragged V: the padded copy of the bias, or no x6
      bias = nullptr;
      auto ib = W.bias4.find(l.w);
      if (ib != W.bias4.end()) bias = ib->second;
      if (!bias) w6 = nullptr;
    }
  }
  if (!w6) return linear(l, A, lda, C, ldc, M, s);
  WN_TRY(m->x6_lin.ensure(x6_bytes(M, l.in)));
  WN_TRY(x6_split(A, M, l.in, lda, m->x6_lin.as<char>(), s));
  X6Args x;
  x.A3 = m->x6_lin.as<char>(); x.B3 = w6; x.M = M; x.N = V4; x.K = l.in;
  x.epi = 0; x.bias = bias; x.C = C; x.ldc = ldc;
  return gemm_x6(x, s);
}

// ---- small kernels of the subsampling front ends and the padded-output scatter ---------------
namespace wn {
namespace {

// x6 conv2: base pixel (plane image row of conv1's output, even-first order inside a
// frame) of GEMM row (g, f2): frame off1[u] + 2 t2, position f2 (= f1 2 f2)
// (fstep 1: plane image with the even f1 first; 2: the plain channels-last tensor)
__global__ void build_conv2_pix_kernel(const int* row_utt2, const int* off2, const int* off1,
                                       int M, int F1, int F2, int fstep, int* a_pix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * F2) return;
  const int g = i / F2, f2 = i % F2;
  const int u = row_utt2[g];
  a_pix[i] = (off1[u] + 2 * (g - off2[u])) * F1 + fstep * f2;
}

__global__ void build_conv2_rows_kernel(const int* row_utt2, const int* off2,
                                        const int* off1, int M, int F1, int F2,
                                        int C, int64_t* a_row_off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * F2) return;
  const int g = i / F2, f2 = i % F2;
  const int u = row_utt2[g];
  const int t2 = g - off2[u];
  const int64_t t1 = off1[u] + 2 * t2;
  a_row_off[i] = (t1 * F1 + 2 * f2) * (int64_t)C;
}

// packed rows -> padded (B, Tp, D) with zero fill
__global__ void scatter_padded_kernel(const float* src, int lds, const int* off,
                                      const int* len, int Tp, int D4,
                                      float* dst) {
  const int b = blockIdx.y, t = blockIdx.x;
  f32x4* d = reinterpret_cast<f32x4*>(dst + ((int64_t)b * Tp + t) * D4 * 4);
  if (t < len[b]) {
    const f32x4* s =
        reinterpret_cast<const f32x4*>(src + (int64_t)(off[b] + t) * lds);
    for (int i = threadIdx.x; i < D4; i += blockDim.x) d[i] = s[i];
  } else {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < D4; i += blockDim.x) d[i] = z;
  }
}

// Conv1dSubsampling2 front end: utterance b becomes the packed segment
// [0, x_0 .. x_{len-1}, 0, 0] (len + 3 rows of F floats) so that the k=3, pad=1
// convolution over time is a plain GEMM over three consecutive rows.
__global__ void pad_feats_kernel(const float* feats, int T, int F, const int* seg_off,
                                 const int* len, const float* mean,
                                 const float* istd, float* xpad) {
  const int b = blockIdx.y, j = blockIdx.x;
  const int L = len[b];
  if (j >= L + 3) return;
  float* dst = xpad + (int64_t)(seg_off[b] + j) * F;
  const int t = j - 1;
  if (t >= 0 && t < L) {
    const float* src = feats + ((int64_t)b * T + t) * F;
    for (int i = threadIdx.x; i < F; i += blockDim.x) {
      float v = src[i];
      if (mean) v = (v - mean[i]) * istd[i];
      dst[i] = v;
    }
  } else {
    for (int i = threadIdx.x; i < F; i += blockDim.x) dst[i] = 0.f;
  }
}

__global__ void zero_rows_kernel(float* base, int D4, const int* rows, int n) {
  const int r = blockIdx.x;
  if (r >= n) return;
  f32x4* d = reinterpret_cast<f32x4*>(base + (int64_t)rows[r] * D4 * 4);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < D4; i += blockDim.x) d[i] = z;
}

}  // namespace
}  // namespace wn

// packed encoder rows -> the caller's padded (B, Tp, D) tensor (wn_encode, encode_transformer)
int scatter_padded(const float* src, int lds, const int* off, const int* len, int B, int Tp, int D,
                   float* dst, hipStream_t s) {
  hipLaunchKernelGGL(scatter_padded_kernel, dim3(Tp, B), dim3(64), 0, s, src, lds, off, len, Tp,
                     D / 4, dst);
  WN_HIP(hipGetLastError());
  return 0;
}

// ---- set the per-utterance row layout of the current batch -----------------
int set_layout(wn_model* m, int B, int Tp, const std::vector<int>& off,
               const std::vector<int>& len, int rows, hipStream_t s) {
  m->B = B; m->Tp = Tp; m->off = off; m->len = len; m->rows = rows;
  m->mem_cache_valid = false;
  if (m->kv_ready) {     // a prefetch nobody consumed may still be reading m->enc
    (void)hipStreamWaitEvent(s, m->side.e1, 0);
    m->kv_ready = false;
  }
  std::vector<int> row_utt(std::max(rows, 1), -1);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < len[b]; ++t) row_utt[off[b] + t] = b;
  // Block list of the six-product self attention (attention_x6.hip, 64 queries per block),
  // appended to the row_utt upload: (sequence << 16 | head << 8 | query block), the blocks with
  // two live 32-query groups first, the "light" last blocks of sequences with an odd number of
  // query tiles behind them, longer sequences first inside each class.  The dispatcher deals
  // blocks to the CUs in this order, so the ones a CU gets on top of its two full blocks are
  // the cheap ones (round 6: 531 equal-looking blocks on 256 CUs -- the CUs with three set the
  // kernel's time).
  m->attn_blk_off = (int)((row_utt.size() + 15) / 16 * 16);
  m->attn_n_blk = 0;
  {
    const int H = m->cfg.n_heads;
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len[x] > len[y]; });
    std::vector<int> tab;
    if (B < 65536 && H < 256)
      for (int light = 0; light < 2; ++light)
        for (int b : order) {
          const int nqb = (len[b] + 63) / 64;
          for (int qb = 0; qb < nqb && qb < 256; ++qb) {
            const bool is_light = len[b] - qb * 64 <= 32;
            if ((int)is_light != light) continue;
            for (int h = 0; h < H; ++h) tab.push_back((b << 16) | (h << 8) | qb);
          }
        }
    row_utt.resize(m->attn_blk_off + tab.size(), -1);
    std::copy(tab.begin(), tab.end(), row_utt.begin() + m->attn_blk_off);
    m->attn_n_blk = (int)tab.size();
  }
  WN_TRY(m->stage.begin((size_t)(row_utt.size() + 4 * B + 64) * sizeof(int) + 1024));
  WN_TRY(upload_desc(m, m->d_off, off, s));
  WN_TRY(upload_desc(m, m->d_len, len, s));
  WN_TRY(upload_desc(m, m->d_row_utt, row_utt, s));
  m->ctc_valid = false;
  return 0;
}

// GlobalCMVN + Conv2dSubsampling4 + RelPositionalEncoding scale for a padded
// Conv2dSubsampling's out Linear(d * F2 -> d) * sqrt(d) (subsampling.py:225-226, embedding.py:144)
// on the six-product GEMM (round 3).  K = 4864 / 9728 and N = d give 31 row tiles at config 2: the
// K dimension is cut into S slices (tiles x S fills the CUs once), the fp32 rows of conv2's output
// are split into planes in registers (no plane image of the 154-MB tensor), the slice partials
// are added by ffn_reduce_ln together with the bias, the scale and layer 0's norm_ff_macaron
// (x starts as zeros: 0 + alpha (sum + b) is alpha (sum + b) exactly).  191 us on v_mfma_f32
// (102 TF, r05e) before.  Returns 1 if it ran, 0 if the shape stays on linear().
int sub_out_linear(wn_model* m, int M, int F2, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, K = F2 * d;
  if (t_gemm_prec != PREC_F32 || tune().gemm_x6 == 0 || W.layers.empty() ||
      (d != 256 && d != 512) || K % 16 != 0 || M < 512 || (int64_t)M * K * 4 >= ((int64_t)1 << 31) ||
      bf16_store_active())
    return 0;
  auto it = W.x6_at.find(W.sub_out.w);
  if (it == W.x6_at.end()) return 0;
  const int bm = 256;
  const int tiles = cdiv(M, bm) * cdiv(d, 256), nkb = K / 16;
  int S = 0;
  for (int t = std::min(16, 256 / std::max(tiles, 1)); t >= 2; --t)
    if (nkb % t == 0) { S = t; break; }
  if (S < 2) return 0;
  WN_TRY(m->ffn_part.ensure((size_t)S * M * d * sizeof(float)));
  X6Args g;
  g.A = m->c2.as<float>(); g.lda = K; g.a_bytes = (int64_t)M * K * 4;
  g.B3 = it->second; g.M = M; g.N = d; g.K = K; g.epi = 1; g.ksplit = S; g.bm = bm;
  g.C = m->ffn_part.as<float>();
  WN_TRY(gemm_x6(g, s));
  WN_HIP(hipMemsetAsync(m->x.p, 0, (size_t)M * d * sizeof(float), s));
  const EncLayer& L0 = W.layers[0];
  WN_TRY(ffn_reduce_ln(m->x.as<float>(), m->ffn_part.as<float>(), S, W.sub_out.b, sqrtf((float)d),
                       L0.norm_ff_mac.w, L0.norm_ff_mac.b, nullptr, nullptr, m->t1.as<float>(), M,
                       d, c.norm_eps, 0, s));
  m->ln0_done = true;
  return 1;
}

// (B, T, F) feature batch: sets the row layout and leaves x = embed(xs) in m->x
// (encoder.py:155-157, subsampling.py:203-228, embedding.py:134-147).  `pos0` is
// the position of the first output frame (streaming offset).
// consume the handle's encode gate (wn_model_set_encode_gate): everything queued on `s` after
// this point waits for the event; idempotent
int encode_gate_wait(wn_model* m, hipStream_t s) {
  if (m->enc_gate) {
    hipEvent_t e = m->enc_gate;
    m->enc_gate = nullptr;
    WN_HIP(hipStreamWaitEvent(s, e, 0));
  }
  return 0;
}

// How subsample_conv2d4 runs conv2 for M output frames / M1 conv1 frames under the calling
// thread's precision and tune() (the function switches on this, wn_op_conv2d4 reports it);
// *w6: the plane image of conv2's weight for the two six-product kinds.
int conv2_kind(const wn_model* m, int M, int M1, const void** w6) {
  const ModelData& W = *m->data;
  const int d = m->cfg.d_model, F1 = m->F1(), F2 = m->F2();
  // fp32 on the bf16 matrix cores (gemm_x6.hip): conv1 writes the plane image of its
  // output, conv2 gathers its rows from it
  *w6 = nullptr;
  if (t_gemm_prec == PREC_F32 && tune().gemm_x6 != 0 && d % 32 == 0 &&
      F1 <= 64 &&
      (M * F2 >= 4096 || tune().gemm_x6 == 2)) {
    auto it = W.x6_at.find(W.conv2.w);
    if (it != W.x6_at.end()) *w6 = it->second;
  }
  if (*w6 && (tune().x6_af32 != 0 || tune().x6_conv_af32 != 0) &&
      (int64_t)M1 * F1 * d * 4 < ((int64_t)1 << 31))
    return CONV2_X6_AF32;
  return *w6 ? CONV2_X6_PLANES : CONV2_GEMM_F32;
}

int subsample_conv2d4(wn_model* m, const float* feats_dev,
                      const int32_t* feat_lens_host, int B, int T,
                      int32_t* enc_lens_host, int pos0, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, F1 = m->F1(), F2 = m->F2();
  const int Tp = ((T - 1) / 2 - 1) / 2;
  m->ln0_done = false;
  m->front_route = 0;
  WN_CHECK(pos0 + Tp <= c.max_pos, "utterance longer than the positional table");
  std::vector<int> off2(B), len2(B), off1(B), len1(B);
  int M = 0, M1 = 0, max_t1 = 0;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    // mask[:, :, 2::2][:, :, 2::2] (subsampling.py:228): frames 6 + 4k < L
    const int l2 = L > 6 ? (L - 7) / 4 + 1 : 0;
    off2[b] = M; len2[b] = l2; M += l2;
    const int l1 = l2 > 0 ? 2 * l2 + 1 : 0;
    off1[b] = M1; len1[b] = l1; M1 += l1;
    max_t1 = std::max(max_t1, l1);
    if (enc_lens_host) enc_lens_host[b] = l2;
  }
  WN_TRY(set_layout(m, B, Tp, off2, len2, M, s));
  if (M == 0) WN_TRY(m->stage.end(s));
  if (M > 0) {
    WN_TRY(upload_desc(m, m->d_off1, off1, s));
    WN_TRY(upload_desc(m, m->d_len1, len1, s));
    WN_TRY(m->stage.end(s));
    // encode gate, position 0 (the default): the wait for the previous decode sits BEHIND this
    // call's descriptor uploads -- five small host -> device copies, ~22 us of copy kernels plus
    // their launch gaps that otherwise stand in the encoder chain (two-stream timeline r13b) --
    // and in front of conv1
    if (tune().enc_gate_pos == 0) WN_TRY(encode_gate_wait(m, s));
    WN_TRY(m->c1.ensure((size_t)M1 * F1 * d * sizeof(float)));
    WN_TRY(m->c2.ensure((size_t)M * F2 * d * sizeof(float)));
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * c.ffn_dim * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    WN_TRY(m->d_a_row_off.ensure((size_t)M * F2 * sizeof(int64_t)));
    const void* w6 = nullptr;
    const int kind = conv2_kind(m, M, M1, &w6);
    if (kind == CONV2_X6_AF32) {
      // conv1 as always (fp32, channels last); conv2 gathers its A rows from it, 64 B per
      // pixel and k block, and splits them in registers
      WN_TRY(m->c1.ensure((size_t)M1 * F1 * d * sizeof(float)));
      Conv1Args c1;
      c1.feats = feats_dev; c1.mean = W.cmvn_mean; c1.istd = W.cmvn_istd;
      c1.w = W.conv1_w; c1.bias = W.conv1_b; c1.out = m->c1.as<float>();
      c1.t1_off = m->d_off1.as<int>(); c1.t1_len = m->d_len1.as<int>();
      c1.B = B; c1.T = T; c1.F = c.feat_dim; c1.F1 = F1; c1.C = d; c1.max_t1 = max_t1;
      WN_TRY(cmvn_conv1_relu(c1, s));
      int* pix = reinterpret_cast<int*>(m->d_a_row_off.as<int64_t>());
      hipLaunchKernelGGL(build_conv2_pix_kernel, dim3(cdiv(M * F2, 256)), dim3(256), 0, s,
                         m->d_row_utt.as<int>(), m->d_off.as<int>(), m->d_off1.as<int>(), M,
                         F1, F2, 2, pix);
      WN_HIP(hipGetLastError());
      X6Args g;
      g.A = m->c1.as<float>(); g.a_bytes = (int64_t)M1 * F1 * d * 4;
      g.B3 = w6; g.M = M * F2; g.N = d; g.K = 9 * d;
      g.epi = 0; g.bias = W.conv2.b; g.act = ACT_RELU; g.C = m->c2.as<float>(); g.ldc = d;
      g.a_pix = pix; g.conv_kbc = d / 16;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) g.tap_delta[ky * 3 + kx] = ky * F1 + kx;
      const X6ConvForm form = gemm_x6_conv_form(g);
      WN_TRY(gemm_x6(g, s));
      WN_TRY(linear(W.sub_out, m->c2.as<float>(), F2 * d, m->x.as<float>(), d, M,
                    s, ACT_NONE, nullptr, 0, sqrtf((float)d)));
      m->front_route = front_route_code(kind, form, false, t_linear_took_x6);
      return 0;
    }
    if (kind == CONV2_X6_PLANES) {
      const int tiles = cdiv(M1 * F1, 32);
      WN_TRY(m->c1.ensure(x6_bytes(M1 * F1, d)));
      Conv1Args c1;
      c1.feats = feats_dev; c1.mean = W.cmvn_mean; c1.istd = W.cmvn_istd;
      c1.w = W.conv1_w; c1.bias = W.conv1_b; c1.out = nullptr;
      c1.out3 = m->c1.as<char>(); c1.tiles = tiles;
      c1.t1_off = m->d_off1.as<int>(); c1.t1_len = m->d_len1.as<int>();
      c1.B = B; c1.T = T; c1.F = c.feat_dim; c1.F1 = F1; c1.C = d; c1.max_t1 = max_t1;
      WN_TRY(cmvn_conv1_relu(c1, s));
      int* pix = reinterpret_cast<int*>(m->d_a_row_off.as<int64_t>());
      hipLaunchKernelGGL(build_conv2_pix_kernel, dim3(cdiv(M * F2, 256)), dim3(256), 0, s,
                         m->d_row_utt.as<int>(), m->d_off.as<int>(), m->d_off1.as<int>(), M,
                         F1, F2, 1, pix);
      WN_HIP(hipGetLastError());
      // the front end (HBM-bound: 10 MB of features -> the ~1-GB plane image) may run beside
      // the previous decode's matrix-bound encoder; conv2 and everything behind it may not
      WN_TRY(encode_gate_wait(m, s));
      X6Args g;
      g.A3 = m->c1.as<char>(); g.B3 = w6; g.M = M * F2; g.N = d; g.K = 9 * d;
      g.epi = 0; g.bias = W.conv2.b; g.act = ACT_RELU; g.C = m->c2.as<float>(); g.ldc = d;
      g.a_pix = pix; g.a_tiles = tiles; g.conv_kbc = d / 16;
      g.conv_taps = 9;
      {   // scratch for the K-slice partials of the last, partial round of tiles (gemm_x6.hip)
        const int ncu = 256;   // (as in gemm_x6())
        const int t256 = cdiv(M * F2, 256), rem = t256 - t256 / ncu * ncu;
        if (d <= 256 && t256 >= ncu && rem > 0 && rem <= ncu / 2) {
          const size_t need = (size_t)4 * ((size_t)M * F2 - (size_t)(t256 - rem) * 256) * d *
                              sizeof(float);
          WN_TRY(m->ffn_part.ensure(need));
          g.part = m->ffn_part.as<float>(); g.part_bytes = m->ffn_part.cap;
        }
      }
      const int ne = (F1 + 1) / 2;
      for (int ky = 0; ky < 3; ++ky) {
        g.tap_delta[ky * 3 + 0] = ky * F1;            // f1 = 2 f2     (even, position f2)
        g.tap_delta[ky * 3 + 1] = ky * F1 + ne;       // f1 = 2 f2 + 1 (odd, position ne + f2)
        g.tap_delta[ky * 3 + 2] = ky * F1 + 1;        // f1 = 2 f2 + 2 (even, position f2 + 1)
      }
      const X6ConvForm form = gemm_x6_conv_form(g);
      WN_TRY(gemm_x6(g, s));
      const int r = sub_out_linear(m, M, F2, s);
      if (r < 0) return r;
      if (r == 0)
        WN_TRY(linear(W.sub_out, m->c2.as<float>(), F2 * d, m->x.as<float>(), d, M,
                      s, ACT_NONE, nullptr, 0, sqrtf((float)d)));
      m->front_route = front_route_code(kind, form, r != 0, r == 0 && t_linear_took_x6);
      return 0;
    }
    // GlobalCMVN + conv1 + ReLU                        encoder.py:155, subsampling.py:188
    Conv1Args c1;
    c1.feats = feats_dev; c1.mean = W.cmvn_mean; c1.istd = W.cmvn_istd;
    c1.w = W.conv1_w; c1.bias = W.conv1_b; c1.out = m->c1.as<float>();
    c1.t1_off = m->d_off1.as<int>(); c1.t1_len = m->d_len1.as<int>();
    c1.B = B; c1.T = T; c1.F = c.feat_dim; c1.F1 = F1; c1.C = d; c1.max_t1 = max_t1;
    WN_TRY(cmvn_conv1_relu(c1, s));
    // conv2 + ReLU as an implicit GEMM                 subsampling.py:191-192
    hipLaunchKernelGGL(build_conv2_rows_kernel, dim3(cdiv(M * F2, 256)),
                       dim3(256), 0, s, m->d_row_utt.as<int>(),
                       m->d_off.as<int>(), m->d_off1.as<int>(), M, F1, F2, d,
                       m->d_a_row_off.as<int64_t>());
    WN_HIP(hipGetLastError());
    GemmArgs g;
    g.A = m->c1.as<float>(); g.W = W.conv2.w; g.bias = W.conv2.b;
    g.C = m->c2.as<float>(); g.M = M * F2; g.N = d; g.K = 9 * d; g.ldc = d;
    g.act = ACT_RELU; g.a_row_off = m->d_a_row_off.as<int64_t>();
    g.conv_C = d; g.conv_sy = (int64_t)F1 * d; g.conv_sx = d;
    WN_TRY(gemm_f32(g, s));
    // Linear(d*F2 -> d) * sqrt(d)                      subsampling.py:225-226, embedding.py:144
    WN_TRY(linear(W.sub_out, m->c2.as<float>(), F2 * d, m->x.as<float>(), d, M,
                  s, ACT_NONE, nullptr, 0, sqrtf((float)d)));
    m->front_route = front_route_code(kind, X6ConvForm(), false, t_linear_took_x6);
  }
  return 0;
}

// TransformerEncoder (Whisper style): x += MHA(LN(x)); x += FFN(LN(x)); final LN
// (encoder_layer.py:94-127, encoder.py:176-181).
int transformer_layers(wn_model* m, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, M = m->rows;
  float* x = m->x.as<float>();
  float* t1 = m->t1.as<float>();
  float* t2 = m->t2.as<float>();
  float* hb = m->hbuf.as<float>();
  float* qkv = m->qkv.as<float>();
  const float eps = c.norm_eps;
  int max_len = 0;
  for (int b = 0; b < m->B; ++b) max_len = std::max(max_len, m->len[b]);
  const int act = c.activation == 1 ? ACT_GELU : ACT_SILU;
  const bool h16 = bf16_store_active();  // t1, t2, hb hold bf16 (see there)
  const int n_run = m->dbg_layers >= 0 ? std::min(m->dbg_layers, c.n_layers)
                                      : c.n_layers;
  for (int li = 0; li < n_run; ++li) {
    const TfLayer& L = W.tf_layers[li];
    WN_TRY(ln(L.n1, x, t1, M, d, eps, s, h16));
    // bf16-storage form: Q | K | V leave the GEMM as bf16 (the attention kernel rounds
    // them to bf16 first thing anyway): half the GEMM's store and the attention's stream
    const bool q16 = h16 && tune().qkv_bf16 != 0;
    WN_TRY(linear(L.qkv, t1, d, qkv, 3 * d, M, s, ACT_NONE, nullptr, 0, 1.0f, false,
                  h16, q16));
    AttnArgs a;
    if (q16) {
      const __bf16* qh = reinterpret_cast<const __bf16*>(qkv);
      a.Q = reinterpret_cast<const float*>(qh);
      a.K = reinterpret_cast<const float*>(qh + d);
      a.V = reinterpret_cast<const float*>(qh + 2 * d);
      a.qkv_bf16 = true;
    } else {
      a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d;
    }
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.O = t2; a.ldo = d; a.o_bf16 = h16;
    a.q_off = a.kv_off = m->d_off.as<int>();
    a.q_len = a.kv_len = m->d_len.as<int>();
    a.n_seq = m->B; a.n_heads = c.n_heads; a.max_q_len = max_len;
    a.mask_mode = 0;
    a.scale = 1.0f / sqrtf(64.0f);
    WN_TRY(attention(a, s));
    WN_TRY(linear(L.out, t2, d, x, d, M, s, ACT_NONE, x, d, 1.0f, false, h16));
    WN_TRY(ffn_module(m, L.n2, L.ff1, L.ff2, act, 1.0f, false, h16, s));
  }
  return after_norm_out(m, s);
}

// Conv1dSubsampling2 + WhisperPositionalEncoding + the layers above
// (subsampling.py:117-171, embedding.py:150-164, encoder.py:122-181).
int encode_transformer(wn_model* m, const float* feats_dev,
                       const int32_t* feat_lens_host, int B, int T,
                       float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int d = c.d_model, F = c.feat_dim;
  // output frames: conv(k3, s2, p1) keeps floor((T-1)/2)+1; the mask keeps
  // x_mask[:, :, (T+1)%2::2] (subsampling.py:171): frame t' is valid iff
  // 2t' + (T+1)%2 < len
  const int Tp = (T - 1) / 2 + 1;
  const int par = (T + 1) % 2;
  WN_CHECK(Tp <= c.max_pos, "utterance longer than the positional table");
  std::vector<int> seg(B), off2(B), len2(B), lens(B);
  int rows_pad = 0, M = 0;
  std::vector<int> zero_rows;
  for (int b = 0; b < B; ++b) {
    const int L = feat_lens_host[b];
    WN_CHECK(L >= 0 && L <= T, "wn_encode: feature length out of range");
    lens[b] = L;
    seg[b] = rows_pad;
    rows_pad += L + 3;
    const int l2 = L > par ? (L - par + 1) / 2 : 0;   // #{t' : 2t' + par < L}
    off2[b] = M; len2[b] = l2; M += l2;
    if (enc_lens_host) enc_lens_host[b] = l2;
    zero_rows.push_back(seg[b]);                       // conv2's left zero pad
    // conv1 position L exists in the reference only as a padded frame of a
    // longer batch; when the utterance fills the tensor it is conv2's right
    // zero pad instead
    if (L == T) zero_rows.push_back(seg[b] + 1 + L);
  }
  m->B = B; m->Tp = Tp; m->off = off2; m->len = len2; m->rows = M;
  m->ctc_valid = false;
  m->mem_cache_valid = false;
  if (m->kv_ready) {     // a prefetch nobody consumed may still be reading m->enc
    (void)hipStreamWaitEvent(s, m->side.e1, 0);
    m->kv_ready = false;
  }
  if (M == 0) {
    WN_TRY(m->stage.begin((size_t)B * 16 + 1024));
    WN_TRY(upload_desc(m, m->d_off, off2, s));
    WN_TRY(upload_desc(m, m->d_len, len2, s));
    WN_TRY(m->stage.end(s));
  } else {
    std::vector<int64_t> a_off((size_t)M);
    std::vector<int> row_t((size_t)M);
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < len2[b]; ++t) {
        // conv2 output t' reads conv1 positions 2t'-1 .. 2t'+1 = c1pad rows
        // seg + 2t' .. seg + 2t' + 2
        a_off[off2[b] + t] = (int64_t)(seg[b] + 2 * t) * d;
        row_t[off2[b] + t] = t;
      }
    WN_TRY(m->stage.begin((size_t)M * 16 + (size_t)B * 64 * 5 + zero_rows.size() * 4 +
                          64 * 12 + 4096));
    WN_TRY(upload_desc(m, m->d_off, off2, s));
    WN_TRY(upload_desc(m, m->d_len, len2, s));
    {
      std::vector<int> row_utt(M, -1);
      for (int b = 0; b < B; ++b)
        for (int t = 0; t < len2[b]; ++t) row_utt[off2[b] + t] = b;
      WN_TRY(upload_desc(m, m->d_row_utt, row_utt, s));
      m->attn_n_blk = 0;      // (no block list behind this row_utt)
    }
    WN_TRY(upload_desc(m, m->d_off1, seg, s));
    WN_TRY(upload_desc(m, m->d_len1, lens, s));
    WN_TRY(upload_desc(m, m->d_row_t, row_t, s));
    WN_TRY(upload_desc(m, m->d_zero_rows, zero_rows, s));
    WN_TRY(m->stage.put(m->d_a_row_off, a_off.data(), a_off.size() * sizeof(int64_t), s));
    WN_TRY(m->stage.end(s));
    const int K1 = W.tconv1.in;  // 3F rounded up to 32 (zero weights)
    WN_TRY(m->xpad.ensure(((size_t)rows_pad * F + K1 + 64) * sizeof(float)));
    WN_TRY(m->c1.ensure(((size_t)rows_pad + 2) * d * sizeof(float)));
    WN_TRY(m->x.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t1.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->t2.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->pos_rows.ensure((size_t)M * d * sizeof(float)));
    WN_TRY(m->hbuf.ensure((size_t)M * c.ffn_dim * sizeof(float)));
    WN_TRY(m->qkv.ensure((size_t)M * 3 * d * sizeof(float)));
    int max_len = 0;
    for (int b = 0; b < B; ++b) max_len = std::max(max_len, lens[b]);
    // the K padding of the last rows reads a few floats past the data: keep
    // them finite (they meet zero weights)
    WN_HIP(hipMemsetAsync(m->xpad.as<float>() + (size_t)rows_pad * F, 0,
                          (size_t)(K1 + 64) * sizeof(float), s));
    hipLaunchKernelGGL(pad_feats_kernel, dim3(max_len + 3, B), dim3(64), 0, s,
                       feats_dev, T, F, m->d_off1.as<int>(), m->d_len1.as<int>(),
                       W.cmvn_mean, W.cmvn_istd, m->xpad.as<float>());
    WN_HIP(hipGetLastError());
    // conv1 (k3, pad 1) + GELU: output row r = taps at xpad rows r, r+1, r+2
    // -> c1pad row r + 1 (row seg_b is the zero pad in front of utterance b)
    GemmArgs g1;
    g1.A = m->xpad.as<float>(); g1.W = W.tconv1.w; g1.bias = W.tconv1.b;
    g1.C = m->c1.as<float>() + d; g1.M = rows_pad - 2; g1.N = d; g1.K = K1;
    g1.lda = F; g1.ldc = d; g1.act = ACT_GELU;
    WN_CHECK(F % 4 == 0, "conv1d2 front end: feature dim must be a multiple of 4");
    WN_TRY(gemm_f32(g1, s));
    hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)zero_rows.size()), dim3(64), 0,
                       s, m->c1.as<float>(), d / 4, m->d_zero_rows.as<int>(),
                       (int)zero_rows.size());
    WN_HIP(hipGetLastError());
    // positional rows pe[t'] (xscale = 1, embedding.py:156)
    WN_TRY(copy_rows(W.pe, d, m->d_row_t.as<int>(), m->pos_rows.as<float>(), d,
                     nullptr, M, d, s));
    // conv2 (k3, stride 2, pad 1) + GELU, + pe: gathered rows of c1pad
    GemmArgs g2;
    g2.A = m->c1.as<float>(); g2.W = W.tconv2.w; g2.bias = W.tconv2.b;
    g2.C = m->x.as<float>(); g2.M = M; g2.N = d; g2.K = 3 * d; g2.ldc = d;
    g2.act = ACT_GELU; g2.resid = m->pos_rows.as<float>(); g2.ldr = d;
    g2.a_row_off = m->d_a_row_off.as<int64_t>();
    g2.conv_C = 3 * d; g2.conv_sy = 0; g2.conv_sx = 0;
    WN_TRY(gemm_f32(g2, s));
    WN_TRY(transformer_layers(m, s));
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

