// C ABI (include/wenet_amd.h), the attention decoders: the decoder launch sequence over a
// ragged batch of hypothesis rows, the autoregressive searches, and the rescoring pass (one
// pass behind wn_rescore and the diagnostic wn_attention_rescoring).
#include "model_state.h"

namespace wn {
namespace {

// decoder input rows: embed[tok] * scale + pe[pos]
__global__ void embed_kernel(const int* tok, const int* pos, const float* emb,
                             const float* pe, float scale, int D4, float* x) {
  const int r = blockIdx.x;
  const f32x4* e = reinterpret_cast<const f32x4*>(emb + (int64_t)tok[r] * D4 * 4);
  const f32x4* p = reinterpret_cast<const f32x4*>(pe + (int64_t)pos[r] * D4 * 4);
  f32x4* o = reinterpret_cast<f32x4*>(x + (int64_t)r * D4 * 4);
  for (int i = threadIdx.x; i < D4; i += blockDim.x) o[i] = e[i] * scale + p[i];
}

// log_softmax(row)[target] -- forward_attention_decoder's log_softmax
// (asr_model.py:541-546) fused with the gather of search.py:431-441.
__global__ __launch_bounds__(256) void row_logp_at_kernel(
    const float* logits, int ld, int V, const int* target, float* out) {
  __shared__ float red[8];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)row * ld;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, x[i]);
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sm = 0.f;
  for (int i = tid; i < V; i += 256) sm += expf(x[i] - mx);
  sm = wave_sum(sm);
  if (lane == 0) red[4 + wave] = sm;
  __syncthreads();
  if (tid == 0)
    out[row] = (x[target[row]] - mx) - logf(red[4] + red[5] + red[6] + red[7]);
}

// The workspace of a decoder pass over R token rows: the activations, `logit_rows` rows of
// logits at a pitch of `ld` floats, `out_floats` floats of results in r_out.  (The
// cross-attention K / V is sized by decoder_layers, which projects it.)
int decoder_ws(wn_model* m, size_t R, size_t logit_rows, size_t ld, size_t out_floats) {
  const size_t d = m->cfg.d_model;
  WN_TRY(m->r_x.ensure(R * d * sizeof(float)));
  WN_TRY(m->r_t1.ensure(R * d * sizeof(float)));
  WN_TRY(m->r_t2.ensure(R * d * sizeof(float)));
  WN_TRY(m->r_qkv.ensure(R * 3 * d * sizeof(float)));
  WN_TRY(m->r_h.ensure(R * m->cfg.dec_ffn_dim * sizeof(float)));
  WN_TRY(m->r_logits.ensure(logit_rows * ld * sizeof(float)));
  return m->r_out.ensure(out_floats * sizeof(float));
}

// Cross attention over GROUPS of sequences that share their keys (the hypotheses of one
// utterance in a rescoring pass: consecutive rows, the same encoder frames): one attention
// "sequence" per group instead of one per hypothesis -- full 64-query tiles and the K / V rows
// staged once per 64 queries instead of once per hypothesis.  Per query row the same keys in the
// same tile order: the same bits.
struct CrossGroups {
  const int* q_off; const int* q_len; const int* kv_off; const int* kv_len;
  int n_seq, max_q;
};

// Prompt prefill of the prompted beam search: the self-attention K | V of the B x P prompt rows
// (utterance-major) of every layer go into the search's cache, steps 0..P-1 at the utterance's
// first slot (attn_search.hip)
struct PrefillCache {
  float* cache; size_t layer_stride;
  int B, P, N;
};

// FFN activation of the decoders: ReLU, or the Whisper decoder's exact GELU
inline int dec_act(const wn_config& c) { return c.dec_activation == 1 ? ACT_GELU : ACT_RELU; }

// The decoders' self / cross attention by head width: heads of 64 on attention() as ever (the
// scale is the literal 0.125f), heads of 32 directly on attention_d32 -- never through
// attention_form(), so their attention stays fp32 on bf16 and fp8 handles.
inline int dec_attention(const wn_config& c, AttnArgs& a, hipStream_t s) {
  if (c.d_model / c.dec_heads == 32) {
    a.scale = 1.0f / sqrtf(32.0f);
    return attention_d32(a, s);
  }
  a.scale = 0.125f;
  return attention(a, s);
}

// embed + the decoder layers over a ragged batch of R token rows (n_seq
// sequences); the result stays in m->r_x.  With `mem_cache` the cross-attention
// K/V projections of the encoder output are computed once per batch and layer
// and reused by later calls (the autoregressive search calls this per step).
int decoder_layers(wn_model* m, const Decoder& D, int R, int n_seq, int max_q,
                   const int* d_tok, bool mem_cache, hipStream_t s,
                   const int* self_kvlen = nullptr, const float* kv_base = nullptr,
                   const CrossGroups* cg = nullptr, const PrefillCache* pc = nullptr) {
  const wn_config& c = m->cfg;
  const int d = c.d_model, Menc = m->rows;
  const int act = dec_act(c);
  float* x = m->r_x.as<float>();
  float* t1 = m->r_t1.as<float>();
  float* t2 = m->r_t2.as<float>();
  float* qkv = m->r_qkv.as<float>();
  float* hb = m->r_h.as<float>();
  const float eps = c.norm_eps;
  const size_t mem_layer = (size_t)Menc * 2 * d;
  const bool fill_cache = mem_cache && !m->mem_cache_valid;
  if (mem_cache)
    WN_TRY(m->r_mem_all.ensure(D.layers.size() * mem_layer * sizeof(float)));
  else
    WN_TRY(m->r_mem.ensure(mem_layer * sizeof(float)));
  // embed(V,d) * sqrt(d) + pe                          embedding.py:58-76
  // (the learned table of the Whisper decoder: xscale = 1, embedding.py:167-175)
  hipLaunchKernelGGL(embed_kernel, dim3(R), dim3(64), 0, s, d_tok,
                     m->r_pos.as<int>(), D.embed, D.pe, D.xscale, d / 4, x);
  WN_HIP(hipGetLastError());
  int li = 0;
  bool ln1_done = false;      // t1 already holds this layer's norm1(x) (the previous FFN's reduce)
  for (const DecLayer& L : D.layers) {
    // causal self attention                             decoder_layer.py:100-121
    if (!ln1_done) WN_TRY(ln(L.n1, x, t1, R, d, eps, s));
    ln1_done = false;
    WN_TRY(linear(L.self_qkv, t1, d, qkv, 3 * d, R, s));
    if (pc)
      WN_TRY(attn_prompt_cache_store(qkv, d, pc->B, pc->P, pc->N,
                                     pc->cache + (size_t)li * pc->layer_stride, s));
    AttnArgs a;
    a.Q = qkv; a.K = qkv + d; a.V = qkv + 2 * d; a.ldq = a.ldk = a.ldv = 3 * d;
    a.O = t2; a.ldo = d;
    a.q_off = a.kv_off = m->r_qoff.as<int>();
    a.q_len = a.kv_len = m->r_qlen.as<int>();
    // padded batches (wn_decoder_forward): keys past the sequence length are
    // masked for every query, padded query rows included (mask.py make_pad_mask
    // & subsequent_mask, decoder.py:171-177)
    if (self_kvlen) a.kv_len = self_kvlen;
    a.n_seq = n_seq; a.n_heads = c.dec_heads; a.max_q_len = max_q;
    a.mask_mode = 1;
    WN_TRY(dec_attention(c, a, s));
    WN_TRY(linear(L.self_out, t2, d, x, d, R, s, ACT_NONE, x, d));
    // cross attention over the utterance's encoder frames   decoder_layer.py:123-138
    // (K/V projected once per utterance, not once per hypothesis)
    WN_TRY(ln(L.n2, x, t1, R, d, eps, s));
    WN_TRY(linear(L.src_q, t1, d, t2, d, R, s));
    // kv_base: projected ahead of this pass (wn_rescore_prefetch)
    const float* mem = kv_base ? kv_base + (size_t)li * mem_layer
                       : mem_cache ? m->r_mem_all.as<float>() + (size_t)li * mem_layer
                                   : m->r_mem.as<float>();
    if (!kv_base && (!mem_cache || fill_cache))
      WN_TRY(linear(L.src_kv, m->enc.as<float>(), d, const_cast<float*>(mem), 2 * d, Menc, s));
    AttnArgs cx;
    cx.Q = t2; cx.ldq = d; cx.K = mem; cx.V = mem + d; cx.ldk = cx.ldv = 2 * d;
    cx.O = t1; cx.ldo = d;
    cx.q_off = m->r_qoff.as<int>(); cx.q_len = m->r_qlen.as<int>();
    cx.kv_off = m->r_kvoff.as<int>(); cx.kv_len = m->r_kvlen.as<int>();
    cx.n_seq = n_seq; cx.n_heads = c.dec_heads; cx.max_q_len = max_q;
    if (cg) {
      cx.q_off = cg->q_off; cx.q_len = cg->q_len; cx.kv_off = cg->kv_off; cx.kv_len = cg->kv_len;
      cx.n_seq = cg->n_seq; cx.max_q_len = cg->max_q;
    }
    cx.mask_mode = 0;
    WN_TRY(dec_attention(c, cx, s));
    WN_TRY(linear(L.src_out, t1, d, x, d, R, s, ACT_NONE, x, d));
    // FFN (ReLU; GELU in the Whisper decoder)            decoder_layer.py:140-147
    WN_TRY(ln(L.n3, x, t1, R, d, eps, s));
    // large batches (a rescoring pass): the six-product GEMM pair with the hidden tensor as a
    // plane image; its reduce adds b_2 and the residual and applies the NEXT LayerNorm (the
    // next layer's norm1, or after_norm behind the last layer: the callers' own after_norm
    // call then recomputes the same rows)
    const int fS = ffn_x6_pair(m, L.ff1, L.ff2, act, t1, R, s);
    if (fS < 0) return -2;
    if (fS > 0) {
      const bool last = (size_t)li + 1 == D.layers.size();
      const Norm& nx = last ? D.after : D.layers[li + 1].n1;
      WN_TRY(ffn_reduce_ln(x, m->ffn_part.as<float>(), fS, L.ff2.b, 1.0f, nx.w, nx.b, nullptr,
                           nullptr, t1, R, d, eps, 0, s));
      ln1_done = !last;
    } else {
      WN_TRY(linear(L.ff1, t1, d, hb, c.dec_ffn_dim, R, s, act));
      WN_TRY(linear(L.ff2, hb, c.dec_ffn_dim, x, d, R, s, ACT_NONE, x, d));
    }
    ++li;
  }
  if (fill_cache) m->mem_cache_valid = true;
  return 0;
}

int run_decoder(wn_model* m, const Decoder& D, int R, int n_seq, int max_q,
                const int* d_tok, const int* d_tgt, float* out_dev,
                hipStream_t s, const float* kv_base = nullptr, const CrossGroups* cg = nullptr) {
  const wn_config& c = m->cfg;
  const int d = c.d_model, V = c.vocab;
  WN_TRY(decoder_layers(m, D, R, n_seq, max_q, d_tok, false, s, nullptr, kv_base, cg));
  float* t1 = m->r_t1.as<float>();
  WN_TRY(ln(D.after, m->r_x.as<float>(), t1, R, d, c.norm_eps, s));
  // (the caller sized r_logits for a pitch of V rounded up to 4)
  WN_TRY(vocab_linear(m, D.out, t1, d, m->r_logits.as<float>(), (V + 3) / 4 * 4, R, s));
  hipLaunchKernelGGL(row_logp_at_kernel, dim3(R), dim3(256), 0, s,
                     m->r_logits.as<float>(), (V + 3) / 4 * 4, V, d_tgt, out_dev);
  WN_HIP(hipGetLastError());
  return 0;
}

// Decoder input / target rows of one hypothesis sequence q = (utterance, hypothesis slot):
// ys_in = [sos] + hyp (add_sos_eos, common.py:113-155), the reversed sequence for the
// right-to-left decoder (asr_model.py:491-536), and what each position is scored on
// (search.py:431-449: hyp[j] at position j, eos at position L; r_decoder_out[L-1-j] scores
// hyp[j], so the reversed rows score their own next token).  The n-best is read where the
// prefix beam search left it on the device (or where wn_rescore uploaded it).
__global__ void rescore_rows_kernel(const int* __restrict__ seq_src, const int* __restrict__ qoff,
                                    const int* __restrict__ qlen,
                                    const int* __restrict__ hyp_tokens, int max_len, int sos,
                                    int eos, int V, int* __restrict__ tok, int* __restrict__ rtok,
                                    int* __restrict__ pos, int* __restrict__ tgt,
                                    int* __restrict__ rtgt) {
  const int q = blockIdx.x;
  const int L = qlen[q] - 1, o = qoff[q];
  const int* h = hyp_tokens + (int64_t)seq_src[q] * max_len;
  for (int j = threadIdx.x; j <= L; j += blockDim.x) {
    // ids are < V by construction (top-k indices / host-checked); the clamp only keeps a
    // corrupted buffer from indexing outside the embedding table
    const int a = j == 0 ? sos : min(max(h[j - 1], 0), V - 1);
    const int r = j == 0 ? sos : min(max(h[L - j], 0), V - 1);
    tok[o + j] = a;
    rtok[o + j] = r;
    pos[o + j] = j;
    tgt[o + j] = j < L ? min(max(h[j], 0), V - 1) : eos;
    rtgt[o + j] = j < L ? min(max(h[L - 1 - j], 0), V - 1) : eos;
  }
}

struct RescoreArgs {
  const float* lp_l; const float* lp_r;      // [R] log-prob of each row's target, both decoders
  const int* seq_first;                      // [B + 1] first sequence of each utterance
  const int* seq_src;                        // [n_seq] (utt * beam + hyp slot)
  const int* qoff; const int* qlen;          // [n_seq] first row, rows (= len(hyp) + 1)
  const double* ctc_scores;                  // [B][beam] (DecodeResult.nbest_scores)
  int beam, max_len, use_r2l;
  double ctc_weight;
  float w_l, w_r;                            // fp32(1 - reverse_weight), fp32(reverse_weight)
  int* best_idx; float* best_score; double* conf; float* all_scores; double* tok_conf;
};

// The score arithmetic of attention_rescoring (search.py:424-457) for one utterance per
// wavefront, one hypothesis per lane, in the reference's dtypes and ORDER: the gathered
// log-probs are fp32 tensor elements, `score` accumulates them in fp32 left to right (the
// right-to-left decoder's from position L-1 down), Python-float operands are rounded to fp32
// where they meet the fp32 tensor (1 - reverse_weight, reverse_weight, ctc_score * ctc_weight
// -- that product itself is fp64), math.exp() is fp64.  __f*_rn: no FMA contraction.
__global__ __launch_bounds__(64) void rescore_reduce_kernel(RescoreArgs a) {
  __shared__ float s_score[64];
  __shared__ double s_conf[64];
  __shared__ int s_best;
  const int b = blockIdx.x, i = threadIdx.x;
  const int q0 = a.seq_first[b], n = a.seq_first[b + 1] - q0;
  if (i < n) {
    const int q = q0 + i, L = a.qlen[q] - 1;
    const float* l = a.lp_l + a.qoff[q];
    float score = 0.f;
    for (int j = 0; j < L; ++j) score = __fadd_rn(score, l[j]);
    score = __fadd_rn(score, l[L]);
    if (a.use_r2l) {
      const float* r = a.lp_r + a.qoff[q];
      float rs = 0.f;
      for (int j = 0; j < L; ++j) rs = __fadd_rn(rs, r[L - 1 - j]);
      rs = __fadd_rn(rs, r[L]);
      score = __fadd_rn(__fmul_rn(score, a.w_l), __fmul_rn(rs, a.w_r));
    }
    s_conf[i] = exp((double)__fdiv_rn(score, (float)(L + 1)));
    const int slot = a.seq_src[q];
    score = __fadd_rn(score, (float)(a.ctc_scores[slot] * a.ctc_weight));
    s_score[i] = score;
    a.all_scores[slot] = score;
  }
  __syncthreads();
  if (i == 0) {
    // `if score > best_score` from -inf, first maximum wins, NaN never does
    int best = 0;
    float bs = -INFINITY;
    for (int k = 0; k < n; ++k)
      if (s_score[k] > bs) { bs = s_score[k]; best = k; }
    s_best = best;
    a.best_idx[b] = n > 0 ? a.seq_src[q0 + best] - b * a.beam : 0;
    a.best_score[b] = bs;
    a.conf[b] = n > 0 ? s_conf[best] : 0.0;
  }
  __syncthreads();
  if (n <= 0) return;
  const int q = q0 + s_best, L = a.qlen[q] - 1;
  const float* l = a.lp_l + a.qoff[q];
  const float* r = a.lp_r + a.qoff[q];
  for (int j = i; j < L; j += 64) {
    double c = exp((double)l[j]);
    if (a.use_r2l) c = (c + exp((double)r[L - 1 - j])) / 2;
    a.tok_conf[(int64_t)b * a.max_len + j] = c;
  }
}

// What rescore_pass leaves for its caller: the ragged batch and where the log-probs are.
struct RescoreBatch {
  std::vector<int> seq_src, qoff, qlen;  // per sequence: utt * beam + hyp slot, first row, rows
  int R = 0;                             // token rows of the whole batch
  bool use_r2l = false;
  const float* lp_l = nullptr;           // [R] log-prob of each row's target, in m->r_out
  const float* lp_r = nullptr;           // ... of the right-to-left decoder (with use_r2l)
  const double* d_scores = nullptr;      // the n-best's CTC scores on the device, if it has any
};

// The decoder passes of attention_rescoring (search.py:374-449) over an n-best of the current
// batch: one sequence per (utterance, hypothesis), rows built on the device
// (rescore_rows_kernel), the left-to-right and -- with `want_r2l` and a right decoder -- the
// right-to-left decoder over them; the per-row log-probs stay in m->r_out.  n_hyps_host ==
// nullptr: the n-best of the handle's last prefix beam search, where that left it on the
// device.  ctc_scores_host may be null (a caller that only wants the log-probs): none uploaded.
int rescore_pass(wn_model* m, const char* who, int beam, const int32_t* n_hyps_host,
                 const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
                 const double* ctc_scores_host, int max_len, bool want_r2l, hipStream_t s,
                 RescoreBatch* rb) {
  const ModelData& W = *m->data;
  const wn_config& c = m->cfg;
  const int B = m->B, d = c.d_model, V = c.vocab;
  const std::string pfx = std::string(who) + ": ";
  // ---- where the n-best comes from -----------------------------------------------------
  const bool from_beam = n_hyps_host == nullptr;
  const int* d_tokens = nullptr;
  if (from_beam) {
    // the last wn_ctc_prefix_beam_search of this handle: tokens and scores are still in its
    // device block, counts and lengths in the pinned copy of it
    WN_CHECK(m->pb_valid && m->pb_B == B,
             pfx + "no prefix beam result of the current batch on this handle (pass the "
             "n-best explicitly, or call wn_ctc_prefix_beam_search first)");
    WN_CHECK(!hyp_lens_host && !hyp_tokens_host && !ctc_scores_host,
             pfx + "n_hyps == NULL takes the whole n-best from the handle");
    WN_CHECK(beam == m->pb_beam && max_len == m->pb_max_len,
             pfx + "beam / max_len differ from the prefix beam search's");
    n_hyps_host = reinterpret_cast<const int*>(m->pb_host.p + m->pb_o_nh);
    hyp_lens_host = reinterpret_cast<const int*>(m->pb_host.p + m->pb_o_len);
    d_tokens = reinterpret_cast<const int*>(m->pb_out.as<char>() + m->pb_o_tok);
    rb->d_scores = reinterpret_cast<const double*>(m->pb_out.as<char>() + m->pb_o_sc);
  }
  rb->use_r2l = want_r2l && !W.right.layers.empty();
  // ---- ragged hypothesis batch: one sequence per (utterance, hypothesis) ----------------
  std::vector<int>&seq_src = rb->seq_src, &qoff = rb->qoff, &qlen = rb->qlen;
  std::vector<int> seq_first(B + 1), kvoff, kvlen;
  int R = 0, max_q = 0;
  for (int b = 0; b < B; ++b) {
    seq_first[b] = (int)seq_src.size();
    WN_CHECK(n_hyps_host[b] >= 0 && n_hyps_host[b] <= beam, pfx + "n_hyps");
    if (n_hyps_host[b] > 0)
      WN_CHECK(m->len[b] > 0, pfx + "utterance without encoder frames");
    for (int i = 0; i < n_hyps_host[b]; ++i) {
      const int L = hyp_lens_host[b * beam + i];
      WN_CHECK(L >= 0 && L <= max_len, pfx + "hypothesis length");
      WN_CHECK(L + 1 <= W.left.max_pos, pfx + "hypothesis longer than the positional table");
      if (!from_beam) {
        const int32_t* h = hyp_tokens_host + ((int64_t)b * beam + i) * max_len;
        for (int j = 0; j < L; ++j)
          WN_CHECK(h[j] >= 0 && h[j] < V, pfx + "token id out of range");
      }
      seq_src.push_back(b * beam + i);
      qoff.push_back(R); qlen.push_back(L + 1);
      kvoff.push_back(m->off[b]); kvlen.push_back(m->len[b]);
      R += L + 1;
      max_q = std::max(max_q, L + 1);
    }
  }
  const int n_seq = (int)seq_src.size();
  seq_first[B] = n_seq;
  rb->R = R;
  // cross-attention groups: all hypothesis rows of an utterance against its encoder frames
  std::vector<int> gq_off, gq_len, gkv_off, gkv_len;
  int g_max_q = 0;
  for (int b = 0; b < B; ++b) {
    const int q0 = seq_first[b], q1 = seq_first[b + 1];
    if (q1 <= q0) continue;
    const int rows = qoff[q1 - 1] + qlen[q1 - 1] - qoff[q0];
    gq_off.push_back(qoff[q0]); gq_len.push_back(rows);
    gkv_off.push_back(m->off[b]); gkv_len.push_back(m->len[b]);
    g_max_q = std::max(g_max_q, rows);
  }
  const size_t nb = (size_t)B * beam;
  WN_TRY(m->stage.begin((size_t)(5 * n_seq + 5 * B + 64) * sizeof(int) + 8192 +
                        (from_beam ? 0 : nb * max_len * sizeof(int) + nb * sizeof(double) + 256)));
  if (!from_beam) {
    // tokens | scores in one device block, the prefix beam search's own row pitch
    const size_t tok_bytes = (nb * max_len * sizeof(int) + 7) / 8 * 8;
    WN_TRY(m->r_hyp.ensure(tok_bytes + nb * sizeof(double)));
    WN_TRY(m->stage.put_at(m->r_hyp.p, hyp_tokens_host, nb * max_len * sizeof(int), s));
    d_tokens = m->r_hyp.as<int>();
    if (ctc_scores_host) {
      WN_TRY(m->stage.put_at(m->r_hyp.as<char>() + tok_bytes, ctc_scores_host,
                             nb * sizeof(double), s));
      rb->d_scores = reinterpret_cast<const double*>(m->r_hyp.as<char>() + tok_bytes);
    }
  }
  WN_TRY(upload_desc(m, m->r_seqsrc, seq_src, s));
  WN_TRY(upload_desc(m, m->r_seqfirst, seq_first, s));
  WN_TRY(upload_desc(m, m->r_qoff, qoff, s));
  WN_TRY(upload_desc(m, m->r_qlen, qlen, s));
  WN_TRY(upload_desc(m, m->r_kvoff, kvoff, s));
  WN_TRY(upload_desc(m, m->r_kvlen, kvlen, s));
  WN_TRY(upload_desc(m, m->r_gqoff, gq_off, s));
  WN_TRY(upload_desc(m, m->r_gqlen, gq_len, s));
  WN_TRY(upload_desc(m, m->r_gkvoff, gkv_off, s));
  WN_TRY(upload_desc(m, m->r_gkvlen, gkv_len, s));
  WN_TRY(m->stage.end(s));
  CrossGroups cgrp;
  cgrp.q_off = m->r_gqoff.as<int>(); cgrp.q_len = m->r_gqlen.as<int>();
  cgrp.kv_off = m->r_gkvoff.as<int>(); cgrp.kv_len = m->r_gkvlen.as<int>();
  cgrp.n_seq = (int)gq_off.size(); cgrp.max_q = g_max_q;
  const CrossGroups* cg = tune().rescore_groups != 0 && !gq_off.empty() ? &cgrp : nullptr;
  const int Rp = std::max(R, 1);
  for (DevBuf* bf : {&m->r_tok, &m->r_rtok, &m->r_pos, &m->r_tgt, &m->r_rtgt})
    WN_TRY(bf->ensure((size_t)Rp * sizeof(int)));
  WN_TRY(decoder_ws(m, Rp, Rp, (V + 3) / 4 * 4, (size_t)2 * Rp));
  float* o_l = m->r_out.as<float>();
  float* o_r = o_l + Rp;
  rb->lp_l = o_l; rb->lp_r = o_r;
  if (n_seq == 0) return 0;
  hipLaunchKernelGGL(rescore_rows_kernel, dim3(n_seq), dim3(64), 0, s, m->r_seqsrc.as<int>(),
                     m->r_qoff.as<int>(), m->r_qlen.as<int>(), d_tokens, max_len, c.sos, c.eos,
                     V, m->r_tok.as<int>(), m->r_rtok.as<int>(), m->r_pos.as<int>(),
                     m->r_tgt.as<int>(), m->r_rtgt.as<int>());
  WN_HIP(hipGetLastError());
  // cross-attention K | V projected while the prefix beam search ran (wn_rescore_prefetch)?
  const float* kv_l = nullptr;
  const float* kv_r = nullptr;
  if (m->kv_ready) {
    // an outstanding prefetch is ALWAYS ordered in front of this pass and consumed here:
    // usable or not (e.g. prefetched without the right-to-left decoder, rescored with it),
    // its GEMMs on the side stream read m->enc and write r_kv_all while the decoder pass
    // below would run beside them (round-4 advice)
    WN_HIP(hipStreamWaitEvent(s, m->side.e1, 0));
    if (m->kv_rows == m->rows && m->kv_nl == (int)W.left.layers.size() &&
        (!rb->use_r2l || m->kv_nr == (int)W.right.layers.size())) {
      kv_l = m->r_kv_all.as<float>();
      kv_r = kv_l + (size_t)m->kv_nl * m->rows * 2 * d;
    } else {
      m->kv_ready = false;
    }
  }
  WN_TRY(run_decoder(m, W.left, R, n_seq, max_q, m->r_tok.as<int>(), m->r_tgt.as<int>(), o_l,
                     s, kv_l, cg));
  if (rb->use_r2l)
    WN_TRY(run_decoder(m, W.right, R, n_seq, max_q, m->r_rtok.as<int>(),
                       m->r_rtgt.as<int>(), o_r, s, kv_r, cg));
  return 0;
}

// One GEMM of a decoder step of the prompted search, M = B x beam rows: the skinny kernel
// (gemm_skinny.hip; tune dec_skinny) with the fp32 weights, or in the bf16 mode the handle's
// bf16 weight image; shapes it does not take, and dec_skinny = 0, run on linear().
int step_linear(wn_model* m, bool skinny, const Linear& l, const float* A, int lda, float* C,
                int ldc, int M, hipStream_t s, int act = ACT_NONE, const float* resid = nullptr,
                int ldr = 0) {
  const void* wh = nullptr;
  if (skinny && t_gemm_prec == PREC_BF16) {
    if (t_wslab_bf16 && l.w >= t_wslab_f32 && l.w < t_wslab_f32 + t_wslab_elems)
      wh = reinterpret_cast<const char*>(t_wslab_bf16) + (size_t)(l.w - t_wslab_f32) * 2;
    else
      skinny = false;
  }
  if (!skinny || M > 256 || l.in % 32 != 0 || lda % 4 != 0)
    return linear(l, A, lda, C, ldc, M, s, act, resid, ldr);
  SkinnyArgs g;
  g.A = A; g.lda = lda; g.W = wh ? nullptr : l.w; g.Wh = wh; g.bias = l.b;
  g.resid = resid; g.ldr = ldr; g.C = C; g.ldc = ldc; g.M = M; g.N = l.out; g.K = l.in;
  g.act = act;
  g.split_k = gemm_skinny_split(l.out, l.in, wh != nullptr);
  WN_TRY(m->sk_part.ensure(gemm_skinny_ws_bytes(M, l.out, g.split_k)));
  g.part = m->sk_part.as<float>(); g.part_bytes = m->sk_part.cap;
  return gemm_skinny(g, s);
}

// attention_beam_search (search.py:252-371) for the current batch, entirely on the
// device: one decoder row per running hypothesis and step (self-attention K/V cache
// addressed through per-hypothesis ancestor paths, cross-attention K/V projected once),
// beam bookkeeping in beam_update_kernel; the host only reads the "all ended" counter.
//
// prompt_host == nullptr: the classic search behind wn_attention_beam_search -- every hypothesis
// starts as <sos>, one cross-attention sequence per hypothesis, every GEMM on linear().
// prompt_host (B, P): the Whisper branch behind wn_attention_beam_search_prompt -- the prompt
// rows are prefilled once per utterance and shared through the paths, the steps stop at the
// decoder's positional table, the hypotheses of an utterance are ONE cross-attention sequence,
// and the step GEMMs may run on the skinny kernel.
int beam_search_run(wn_model* m, int beam, int maxlen, float length_penalty,
                    const int32_t* prompt_host, int P, int32_t* tokens_host, int32_t* lens_host,
                    hipStream_t s) {
  const Decoder& D = m->data->left;
  const bool prompted = prompt_host != nullptr;
  WN_CHECK(!D.layers.empty(), "attention beam search: the model has no attention decoder");
  WN_CHECK(beam >= 1 && beam <= 64 && maxlen >= 1 && tokens_host && lens_host,
           "attention beam search: beam_size in [1, 64], maxlen >= 1");
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int d = c.d_model, V = c.vocab, B = m->B, N = beam, BN = B * N, Menc = m->rows;
  const int act = dec_act(c);
  WN_CHECK(beam <= V, "attention beam search: beam larger than the vocabulary");
  if (!prompted)
    WN_CHECK(maxlen + 1 <= D.max_pos, "attention beam search: longer than the positional table");
  else
    WN_CHECK(P <= D.max_pos, "attention beam search: prompt longer than the positional table");
  // the last step: hypotheses of `last` tokens produce token last + 1.  The reference asserts
  // in PositionalEncoding.position_encoding once a step needs position max_pos; the prompted
  // search stops there and returns the best hypothesis so far (deviations)
  const int last = prompted ? std::min(maxlen, D.max_pos) : maxlen;
  const int first = prompted ? P : 1;
  const int W = std::max(maxlen, P) + 2;          // columns of the token / path rows
  const int nl = (int)D.layers.size();
  const bool skinny = prompted && tune().dec_skinny != 0;
  m->ab_truncated = false;
  for (int b = 0; b < B; ++b)
    WN_CHECK(m->len[b] > 0, "attention beam search: utterance without encoder frames");
  // ---- descriptors -------------------------------------------------------------------
  // cross attention of the steps: one query row per hypothesis, or (prompted) the N
  // consecutive rows of an utterance as one sequence -- its keys staged once, the same keys in
  // the same tile order per query row
  const int n_cx = prompted ? B : BN, cx_q = prompted ? N : 1;
  std::vector<int> qoff(n_cx), qlen(n_cx, cx_q), kvoff(n_cx), kvlen(n_cx);
  for (int r = 0; r < n_cx; ++r) {
    const int b = prompted ? r : r / N;
    qoff[r] = r * cx_q; kvoff[r] = m->off[b]; kvlen[r] = m->len[b];
  }
  const int RP = prompted ? B * P : 0;             // prefill rows
  WN_TRY(m->stage.begin((size_t)(4 * n_cx + 3 * RP + 4 * B + BN + 128) * sizeof(int) + 8192));
  DevBuf& b_qoff = prompted ? m->r_gqoff : m->r_qoff;
  DevBuf& b_qlen = prompted ? m->r_gqlen : m->r_qlen;
  DevBuf& b_kvoff = prompted ? m->r_gkvoff : m->r_kvoff;
  DevBuf& b_kvlen = prompted ? m->r_gkvlen : m->r_kvlen;
  WN_TRY(upload_desc(m, b_qoff, qoff, s));
  WN_TRY(upload_desc(m, b_qlen, qlen, s));
  WN_TRY(upload_desc(m, b_kvoff, kvoff, s));
  WN_TRY(upload_desc(m, b_kvlen, kvlen, s));
  if (prompted) {
    // the prefill as a ragged decoder batch: B sequences of P rows; and, per hypothesis, the
    // prefill row whose output it continues from (the utterance's last prompt position)
    std::vector<int> tok(RP), pos(RP), poff(B), plen(B, P), pkvoff(B), pkvlen(B), lastrow(BN);
    for (int b = 0; b < B; ++b) {
      poff[b] = b * P; pkvoff[b] = m->off[b]; pkvlen[b] = m->len[b];
      for (int j = 0; j < P; ++j) {
        const int t = prompt_host[(size_t)b * P + j];
        WN_CHECK(t >= 0 && t < V, "attention beam search: prompt token id out of range");
        tok[b * P + j] = t; pos[b * P + j] = j;
      }
      for (int n = 0; n < N; ++n) lastrow[b * N + n] = b * P + P - 1;
    }
    WN_TRY(upload_desc(m, m->ab_prompt, tok, s));
    WN_TRY(upload_desc(m, m->r_pos, pos, s));
    WN_TRY(upload_desc(m, m->r_qoff, poff, s));
    WN_TRY(upload_desc(m, m->r_qlen, plen, s));
    WN_TRY(upload_desc(m, m->r_kvoff, pkvoff, s));
    WN_TRY(upload_desc(m, m->r_kvlen, pkvlen, s));
    WN_TRY(upload_desc(m, m->r_tgt, lastrow, s));
  }
  WN_TRY(m->stage.end(s));
  WN_TRY(decoder_ws(m, std::max(BN, RP), BN, V, (size_t)2 * BN * N));
  // self-attention K | V cache [layer][step][slot][2d]: sized for the steps actually run,
  // not for maxlen = T' (the reference's cache grows with the decoded length too,
  // decoder.py:226-281): starts at 32 steps and doubles, the used prefix of every layer is
  // carried over
  int cap_steps = std::max(std::min(last, 32), prompted ? P : 1);
  size_t cache_layer = (size_t)cap_steps * BN * 2 * d;
  WN_TRY(m->ab_cache.ensure(nl * cache_layer * sizeof(float)));
  auto grow_cache = [&](int used_steps) -> int {
    const int cap2 = std::min(last, cap_steps * 2);
    const size_t layer2 = (size_t)cap2 * BN * 2 * d;
    DevBuf nb;
    WN_TRY(nb.ensure(nl * layer2 * sizeof(float)));
    for (int li = 0; li < nl; ++li)
      WN_HIP(hipMemcpyAsync(nb.as<float>() + li * layer2, m->ab_cache.as<float>() + li * cache_layer,
                            (size_t)used_steps * BN * 2 * d * sizeof(float),
                            hipMemcpyDeviceToDevice, s));
    WN_HIP(hipStreamSynchronize(s));            // before the old buffer is freed
    m->ab_cache.swap(nb);
    cap_steps = cap2;
    cache_layer = layer2;
    return 0;
  };
  const size_t mem_layer = (size_t)Menc * 2 * d;
  WN_TRY(m->r_mem_all.ensure(nl * mem_layer * sizeof(float)));
  // state: 2 x {score, end, tok, path} + last_tok + n_done + out_tok + out_len
  const size_t n_int = (size_t)2 * (BN + BN + (size_t)BN * W * 2) + BN + 16 + (size_t)B * W + B;
  WN_TRY(m->ab_state.ensure(n_int * sizeof(int)));
  int* base = m->ab_state.as<int>();
  float* score[2]; int* endf[2]; int* tok[2]; int* path[2];
  for (int k = 0; k < 2; ++k) {
    score[k] = reinterpret_cast<float*>(base); base += BN;
    endf[k] = base; base += BN;
    tok[k] = base; base += (size_t)BN * W;
    path[k] = base; base += (size_t)BN * W;
  }
  int* last_tok = base; base += BN;
  int* n_done = base; base += 16;
  int* out_tok = base; base += (size_t)B * W;
  int* out_len = base;
  if (prompted)
    WN_TRY(attn_beam_init_prompt(BN, N, W, m->ab_prompt.as<int>(), P, score[0], endf[0], tok[0],
                                 path[0], last_tok, s));
  else
    WN_TRY(attn_beam_init(BN, N, W, c.sos, score[0], endf[0], tok[0], path[0], last_tok, s));
  WN_HIP(hipMemsetAsync(n_done, 0, sizeof(int), s));
  float* x = m->r_x.as<float>();
  float* t1 = m->r_t1.as<float>();
  float* t2 = m->r_t2.as<float>();
  float* qkv = m->r_qkv.as<float>();
  float* hb = m->r_h.as<float>();
  float* tv = m->r_out.as<float>();
  int* ti = reinterpret_cast<int*>(tv + (size_t)BN * N);
  const float eps = c.norm_eps;
  int cur = 0, len = first, done_host = 0;
  for (int i = first; i <= last; ++i) {
    if (done_host == BN) break;
    const int step = i - 1;                       // position of the newest token
    const bool prefill = prompted && i == P;
    if (prefill) {
      // positions 0..P-1 of every utterance in one causal pass over B x P rows; K | V into the
      // cache, then every hypothesis continues from its utterance's last prompt row
      PrefillCache pc{m->ab_cache.as<float>(), cache_layer, B, P, N};
      WN_TRY(decoder_layers(m, D, RP, B, P, m->ab_prompt.as<int>(), true, s, nullptr, nullptr,
                            nullptr, &pc));
      WN_TRY(copy_rows(x, d, m->r_tgt.as<int>(), t2, d, nullptr, BN, d, s));
      WN_TRY(ln(D.after, t2, t1, BN, d, eps, s));
    } else {
    if (step >= cap_steps) WN_TRY(grow_cache(step));
    WN_TRY(attn_step_embed(last_tok, step, D.embed, D.pe, D.xscale, d, BN, x, s));
    for (int li = 0; li < nl; ++li) {
      const DecLayer& L = D.layers[li];
      WN_TRY(ln(L.n1, x, t1, BN, d, eps, s));
      WN_TRY(step_linear(m, skinny, L.self_qkv, t1, d, qkv, 3 * d, BN, s));
      WN_TRY(attn_self_step(qkv, d, c.dec_heads, BN, m->ab_cache.as<float>() + li * cache_layer,
                            step, path[cur], W, t2, s));
      WN_TRY(step_linear(m, skinny, L.self_out, t2, d, x, d, BN, s, ACT_NONE, x, d));
      WN_TRY(ln(L.n2, x, t1, BN, d, eps, s));
      WN_TRY(step_linear(m, skinny, L.src_q, t1, d, t2, d, BN, s));
      float* mem = m->r_mem_all.as<float>() + (size_t)li * mem_layer;
      if (!m->mem_cache_valid) WN_TRY(linear(L.src_kv, m->enc.as<float>(), d, mem, 2 * d, Menc, s));
      AttnArgs cx;
      cx.Q = t2; cx.ldq = d; cx.K = mem; cx.V = mem + d; cx.ldk = cx.ldv = 2 * d;
      cx.O = t1; cx.ldo = d;
      cx.q_off = b_qoff.as<int>(); cx.q_len = b_qlen.as<int>();
      cx.kv_off = b_kvoff.as<int>(); cx.kv_len = b_kvlen.as<int>();
      cx.n_seq = n_cx; cx.n_heads = c.dec_heads; cx.max_q_len = cx_q;
      cx.mask_mode = 0;
      WN_TRY(dec_attention(c, cx, s));
      WN_TRY(step_linear(m, skinny, L.src_out, t1, d, x, d, BN, s, ACT_NONE, x, d));
      WN_TRY(ln(L.n3, x, t1, BN, d, eps, s));
      WN_TRY(step_linear(m, skinny, L.ff1, t1, d, hb, c.dec_ffn_dim, BN, s, act));
      WN_TRY(step_linear(m, skinny, L.ff2, hb, c.dec_ffn_dim, x, d, BN, s, ACT_NONE, x, d));
    }
    m->mem_cache_valid = true;
    WN_TRY(ln(D.after, x, t1, BN, d, eps, s));
    }
    // log_softmax(output_layer(after_norm(x))) -> the N best (log-prob, token) per row
    WN_TRY(step_linear(m, skinny, D.out, t1, d, m->r_logits.as<float>(), V, BN, s));
    CtcRowArgs r;
    r.logits = m->r_logits.as<float>(); r.ld = V; r.M = BN; r.V = V; r.k = N;
    r.blank = -1; r.blank_penalty = 0.f;
    r.topk_val = tv; r.topk_idx = ti; r.logp = nullptr; r.ld_out = V;
    WN_TRY(ctc_logsoftmax_topk(r, s));
    WN_HIP(hipMemsetAsync(n_done, 0, sizeof(int), s));
    WN_TRY(attn_beam_update(B, N, i, W, c.eos, V, tv, ti, score[cur], endf[cur], tok[cur],
                            path[cur], score[cur ^ 1], endf[cur ^ 1], tok[cur ^ 1],
                            path[cur ^ 1], last_tok, n_done, s, prefill));
    cur ^= 1;
    len = i + 1;
    // "all hypotheses ended" is polled every 4th step: a step run after the end only appends
    // eos to finished hypotheses and leaves their scores alone (mask_finished_scores /
    // _preds), and the result strips eos (search.py:355-371) -- same output, 3 of 4 host
    // round trips fewer
    if ((i & 3) == 0 || i == last) {
      WN_HIP(hipMemcpyAsync(&done_host, n_done, sizeof(int), hipMemcpyDeviceToHost, s));
      WN_HIP(hipStreamSynchronize(s));
    }
  }
  // stopped by the positional table, not by T' or by the hypotheses: say so
  m->ab_truncated = prompted && last < maxlen && last >= first && done_host != BN;
  WN_TRY(attn_beam_finish(B, N, len, W, c.eos, length_penalty, score[cur], tok[cur], out_tok,
                          out_len, s, first));
  std::vector<int> ot((size_t)B * W), ol(B);
  WN_HIP(hipMemcpyAsync(ot.data(), out_tok, ot.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(ol.data(), out_len, ol.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  for (int b = 0; b < B; ++b) {
    lens_host[b] = std::min(ol[b], maxlen);
    for (int j = 0; j < lens_host[b]; ++j) tokens_host[(size_t)b * maxlen + j] = ot[(size_t)b * W + j];
  }
  return 0;
}

}  // namespace
}  // namespace wn

// ===========================================================================
extern "C" {

int wn_decoder_next_topk(wn_model* m, int32_t n_seq, const int32_t* seq_utt_host,
                         const int32_t* seq_lens_host, const int32_t* tokens_host,
                         int32_t max_len, int32_t topk, float* logp_host,
                         int32_t* idx_host, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "decoder step: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  const ModelData& W = *m->data;
  WN_CHECK(!W.left.layers.empty(), "decoder step: the model has no attention decoder");
  WN_CHECK(n_seq > 0 && seq_utt_host && seq_lens_host && tokens_host && logp_host &&
               idx_host && max_len > 0, "decoder step: bad argument");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int d = c.d_model, V = c.vocab;
  WN_CHECK(topk >= 1 && topk <= V, "decoder step: top-k");
  std::vector<int> tok, pos, qoff(n_seq), qlen(n_seq), kvoff(n_seq), kvlen(n_seq),
      last(n_seq);
  int max_q = 0;
  for (int i = 0; i < n_seq; ++i) {
    const int u = seq_utt_host[i], L = seq_lens_host[i];
    WN_CHECK(u >= 0 && u < m->B, "decoder step: utterance index");
    WN_CHECK(L >= 1 && L <= max_len && L <= W.left.max_pos, "decoder step: sequence length");
    WN_CHECK(m->len[u] > 0, "decoder step: utterance without encoder frames");
    qoff[i] = (int)tok.size(); qlen[i] = L;
    kvoff[i] = m->off[u]; kvlen[i] = m->len[u];
    max_q = std::max(max_q, L);
    for (int j = 0; j < L; ++j) {
      const int t = tokens_host[(int64_t)i * max_len + j];
      WN_CHECK(t >= 0 && t < V, "decoder step: token id");
      tok.push_back(t);
      pos.push_back(j);
    }
    last[i] = qoff[i] + L - 1;
  }
  const int R = (int)tok.size();
  WN_TRY(m->stage.begin((size_t)(2 * R + 5 * n_seq + 64) * sizeof(int) + 4096));
  WN_TRY(upload_desc(m, m->r_tok, tok, s));
  WN_TRY(upload_desc(m, m->r_pos, pos, s));
  WN_TRY(upload_desc(m, m->r_qoff, qoff, s));
  WN_TRY(upload_desc(m, m->r_qlen, qlen, s));
  WN_TRY(upload_desc(m, m->r_kvoff, kvoff, s));
  WN_TRY(upload_desc(m, m->r_kvlen, kvlen, s));
  WN_TRY(upload_desc(m, m->r_tgt, last, s));
  WN_TRY(m->stage.end(s));
  WN_TRY(decoder_ws(m, R, n_seq, V, (size_t)2 * n_seq * topk));   // (n_seq <= R: every L >= 1)
  WN_TRY(decoder_layers(m, W.left, R, n_seq, max_q, m->r_tok.as<int>(), true, s));
  // y = log_softmax(output_layer(after_norm(x[:, -1])))   decoder.py:275-281
  float* t2 = m->r_t2.as<float>();
  float* t1 = m->r_t1.as<float>();
  WN_TRY(copy_rows(m->r_x.as<float>(), d, m->r_tgt.as<int>(), t2, d, nullptr, n_seq, d, s));
  WN_TRY(ln(W.left.after, t2, t1, n_seq, d, c.norm_eps, s));
  WN_TRY(linear(W.left.out, t1, d, m->r_logits.as<float>(), V, n_seq, s));
  float* tv = m->r_out.as<float>();
  int* ti = reinterpret_cast<int*>(tv + (size_t)n_seq * topk);
  CtcRowArgs r;
  r.logits = m->r_logits.as<float>(); r.ld = V; r.M = n_seq; r.V = V; r.k = topk;
  r.blank = -1; r.blank_penalty = 0.f;
  r.topk_val = tv; r.topk_idx = ti; r.logp = nullptr; r.ld_out = V;
  WN_TRY(ctc_logsoftmax_topk(r, s));
  WN_HIP(hipMemcpyAsync(logp_host, tv, (size_t)n_seq * topk * sizeof(float),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(idx_host, ti, (size_t)n_seq * topk * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_attention_beam_search(wn_model* m, int32_t beam, int32_t maxlen, float length_penalty,
                             int32_t* tokens_host, int32_t* lens_host, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "attention beam search: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  return beam_search_run(m, beam, maxlen, length_penalty, nullptr, 1, tokens_host, lens_host,
                         (hipStream_t)stream);
}

int wn_attention_beam_search_prompt(wn_model* m, int32_t beam, int32_t maxlen,
                                    float length_penalty, const int32_t* prompt_host, int32_t P,
                                    int32_t* tokens_host, int32_t* lens_host, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "attention beam search: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  WN_CHECK(prompt_host && P >= 1, "attention beam search: null / empty prompt");
  return beam_search_run(m, beam, maxlen, length_penalty, prompt_host, P, tokens_host,
                         lens_host, (hipStream_t)stream);
}

int32_t wn_attention_truncated(const wn_model* m) { return m ? (m->ab_truncated ? 1 : 0) : -1; }

int wn_decoder_forward(wn_model* m, int32_t utt, int32_t which, int32_t n_seq,
                       const int32_t* tokens_host, const int32_t* lens_host,
                       int32_t max_len, float* logp_dev, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "decoder forward: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  WN_CHECK(tokens_host && lens_host && logp_dev, "decoder forward: null argument");
  WN_CHECK(utt >= 0 && utt < m->B && m->len[utt] > 0,
           "decoder forward: utterance index / no encoder frames");
  WN_CHECK(which == 0 || which == 1, "decoder forward: which must be 0 (left) or 1 (right)");
  const Decoder& D = which == 0 ? m->data->left : m->data->right;
  WN_CHECK(!D.layers.empty(), "decoder forward: the model has no such decoder");
  WN_CHECK(n_seq > 0 && max_len > 0 && max_len <= D.max_pos,
           "decoder forward: bad batch shape / longer than the positional table");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int d = c.d_model, V = c.vocab;
  const int R = n_seq * max_len;
  std::vector<int> tok(R), pos(R), qoff(n_seq), qlen(n_seq), kvoff(n_seq), kvlen(n_seq),
      slen(n_seq);
  for (int i = 0; i < n_seq; ++i) {
    WN_CHECK(lens_host[i] >= 1 && lens_host[i] <= max_len, "decoder forward: length");
    qoff[i] = i * max_len; qlen[i] = max_len; slen[i] = lens_host[i];
    kvoff[i] = m->off[utt]; kvlen[i] = m->len[utt];
    for (int j = 0; j < max_len; ++j) {
      const int t = tokens_host[(size_t)i * max_len + j];
      WN_CHECK(t >= 0 && t < V, "decoder forward: token id out of range");
      tok[(size_t)i * max_len + j] = t;
      pos[(size_t)i * max_len + j] = j;
    }
  }
  WN_TRY(m->stage.begin((size_t)(2 * R + 5 * n_seq + 64) * sizeof(int) + 4096));
  WN_TRY(upload_desc(m, m->r_tok, tok, s));
  WN_TRY(upload_desc(m, m->r_pos, pos, s));
  WN_TRY(upload_desc(m, m->r_qoff, qoff, s));
  WN_TRY(upload_desc(m, m->r_qlen, qlen, s));
  WN_TRY(upload_desc(m, m->r_kvoff, kvoff, s));
  WN_TRY(upload_desc(m, m->r_kvlen, kvlen, s));
  WN_TRY(upload_desc(m, m->r_tgt, slen, s));  // self-attention key lengths
  WN_TRY(m->stage.end(s));
  WN_TRY(decoder_ws(m, R, R, (V + 3) / 4 * 4, (size_t)2 * R));
  WN_TRY(decoder_layers(m, D, R, n_seq, max_len, m->r_tok.as<int>(), false, s,
                        m->r_tgt.as<int>()));
  float* t1 = m->r_t1.as<float>();
  WN_TRY(ln(D.after, m->r_x.as<float>(), t1, R, d, c.norm_eps, s));
  WN_TRY(linear(D.out, t1, d, m->r_logits.as<float>(), V, R, s));
  // log_softmax over the vocabulary of every row (asr_model.py:543-546)
  CtcRowArgs a;
  a.logits = m->r_logits.as<float>(); a.ld = V; a.M = R; a.V = V; a.k = 1;
  a.blank = 0; a.blank_penalty = 0.f;
  a.topk_val = m->r_out.as<float>();
  a.topk_idx = reinterpret_cast<int*>(m->r_out.as<float>() + R);
  a.logp = logp_dev; a.ld_out = V;
  return ctc_logsoftmax_topk(a, s);
}

// The per-token log-probs of a rescoring pass, (B, beam, max_len + 1) per decoder (a
// diagnostic: the tests replay the score arithmetic of wn_rescore on them).  The same pass as
// wn_rescore's; rows past a hypothesis' length + 1 and absent hypotheses read 0, and so does
// the whole right-to-left array without a right decoder or with reverse_weight == 0.
int wn_attention_rescoring(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
                           const int32_t* hyp_lens_host,
                           const int32_t* hyp_tokens_host, int32_t max_len,
                           float reverse_weight, float* l2r_logp_host,
                           float* r2l_logp_host, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "rescoring: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  WN_CHECK(!m->data->left.layers.empty(), "rescoring: the model has no attention decoder");
  WN_CHECK(n_hyps_host && hyp_lens_host && hyp_tokens_host && l2r_logp_host &&
               r2l_logp_host, "rescoring: null argument");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  RescoreBatch rb;
  WN_TRY(rescore_pass(m, "rescoring", beam, n_hyps_host, hyp_lens_host, hyp_tokens_host, nullptr,
                      max_len, reverse_weight > 0.f, s, &rb));
  const size_t out_n = (size_t)m->B * beam * (max_len + 1);
  memset(l2r_logp_host, 0, out_n * sizeof(float));
  memset(r2l_logp_host, 0, out_n * sizeof(float));
  const int R = rb.R;
  if (R == 0) return 0;
  std::vector<float> hl(R), hr(R, 0.f);
  WN_HIP(hipMemcpyAsync(hl.data(), rb.lp_l, R * sizeof(float), hipMemcpyDeviceToHost, s));
  if (rb.use_r2l)
    WN_HIP(hipMemcpyAsync(hr.data(), rb.lp_r, R * sizeof(float), hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  for (size_t q = 0; q < rb.seq_src.size(); ++q) {
    const int64_t o = (int64_t)rb.seq_src[q] * (max_len + 1);
    for (int j = 0; j < rb.qlen[q]; ++j) {
      l2r_logp_host[o + j] = hl[rb.qoff[q] + j];
      r2l_logp_host[o + j] = hr[rb.qoff[q] + j];
    }
  }
  return 0;
}

int wn_rescore_prefetch(wn_model* m, int32_t use_right_decoder, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "wn_rescore_prefetch: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  const ModelData& W = *m->data;
  hipStream_t s = (hipStream_t)stream;
  if (m->kv_ready) {       // an earlier prefetch of this batch: ordered behind it
    WN_HIP(hipStreamWaitEvent(s, m->side.e1, 0));
    m->kv_ready = false;
  }
  if (tune().rescore_prefetch == 0 || W.left.layers.empty() || m->rows <= 0) return 0;
  WN_HIP(hipSetDevice(m->device));
  const int d = m->cfg.d_model, Menc = m->rows;
  const bool r2l = use_right_decoder != 0 && !W.right.layers.empty();
  std::vector<const Linear*> kv;
  for (const DecLayer& L : W.left.layers) kv.push_back(&L.src_kv);
  if (r2l) for (const DecLayer& L : W.right.layers) kv.push_back(&L.src_kv);
  const size_t mem_layer = (size_t)Menc * 2 * d;
  WN_TRY(m->r_kv_all.ensure(kv.size() * mem_layer * sizeof(float)));
  WN_TRY(m->side.ensure());
  WN_HIP(hipEventRecord(m->side.e0, s));            // the encoder output is complete
  WN_HIP(hipStreamWaitEvent(m->side.st, m->side.e0, 0));
  hipStream_t ss = m->side.st;
  // all layers project the SAME rows: split the encoder output into planes once and run the
  // six-product GEMM per layer (linear() would split it once per layer) -- where linear()
  // would take that route at all
  bool x6ok = t_gemm_prec == PREC_F32 && tune().gemm_x6 != 0 && tune().x6_linear != 0 && t_x6 &&
              Menc >= 512 && d % 16 == 0 &&
              2.0 * Menc * (2.0 * d) * d >= 1e8 * 60;
  if (x6ok)
    for (const Linear* l : kv) x6ok = x6ok && t_x6->count(l->w) != 0;
  if (x6ok) {
    WN_TRY(m->r_enc3.ensure(x6_bytes(Menc, d)));
    WN_TRY(x6_split(m->enc.as<float>(), Menc, d, d, m->r_enc3.as<char>(), ss));
  }
  for (size_t i = 0; i < kv.size(); ++i) {
    float* dst = m->r_kv_all.as<float>() + i * mem_layer;
    if (x6ok) {
      X6Args x;
      x.A3 = m->r_enc3.as<char>(); x.B3 = t_x6->find(kv[i]->w)->second; x.M = Menc;
      x.N = 2 * d; x.K = d; x.epi = 0; x.bias = kv[i]->b; x.C = dst; x.ldc = 2 * d;
      WN_TRY(gemm_x6(x, ss));
    } else {
      WN_TRY(linear(*kv[i], m->enc.as<float>(), d, dst, 2 * d, Menc, ss));
    }
  }
  WN_HIP(hipEventRecord(m->side.e1, ss));
  m->kv_ready = true; m->kv_rows = Menc;
  m->kv_nl = (int)W.left.layers.size(); m->kv_nr = r2l ? (int)W.right.layers.size() : 0;
  return 0;
}

int wn_rescore(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
               const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
               const double* ctc_scores_host, int32_t max_len, double ctc_weight,
               double reverse_weight, int32_t* best_idx_host, float* best_score_host,
               double* confidence_host, double* tok_conf_host, float* all_scores_host,
               void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p, "wn_rescore: no current batch");
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  WN_CHECK(!m->data->left.layers.empty(), "wn_rescore: the model has no attention decoder");
  WN_CHECK(best_idx_host && best_score_host, "wn_rescore: null output");
  WN_CHECK(!n_hyps_host || (hyp_lens_host && hyp_tokens_host && ctc_scores_host),
           "wn_rescore: null n-best");
  // (the reduce kernel holds one hypothesis per lane of a wavefront)
  WN_CHECK(beam >= 1 && beam <= 64 && max_len >= 1, "wn_rescore: beam must be 1..64");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const int B = m->B;
  RescoreBatch rb;
  WN_TRY(rescore_pass(m, "wn_rescore", beam, n_hyps_host, hyp_lens_host, hyp_tokens_host,
                      ctc_scores_host, max_len, reverse_weight > 0.0, s, &rb));
  // results, one block: tok_conf | conf | best_score | best_idx | all_scores
  const size_t nb = (size_t)B * beam;
  const size_t o_tc = 0, o_cf = o_tc + (size_t)B * max_len * sizeof(double),
               o_bs = o_cf + (size_t)B * sizeof(double), o_bi = o_bs + (size_t)B * sizeof(float),
               o_as = o_bi + (size_t)B * sizeof(int), o_end = o_as + nb * sizeof(float);
  WN_TRY(m->r_res.ensure(o_end));
  WN_TRY(m->r_host.ensure(o_end));
  WN_HIP(hipMemsetAsync(m->r_res.p, 0, o_end, s));
  char* rbk = m->r_res.as<char>();
  RescoreArgs a;
  a.lp_l = rb.lp_l; a.lp_r = rb.lp_r;
  a.seq_first = m->r_seqfirst.as<int>(); a.seq_src = m->r_seqsrc.as<int>();
  a.qoff = m->r_qoff.as<int>(); a.qlen = m->r_qlen.as<int>();
  a.ctc_scores = rb.d_scores; a.beam = beam; a.max_len = max_len; a.use_r2l = rb.use_r2l ? 1 : 0;
  a.ctc_weight = ctc_weight;
  a.w_l = (float)(1.0 - reverse_weight); a.w_r = (float)reverse_weight;
  a.best_idx = reinterpret_cast<int*>(rbk + o_bi);
  a.best_score = reinterpret_cast<float*>(rbk + o_bs);
  a.conf = reinterpret_cast<double*>(rbk + o_cf);
  a.all_scores = reinterpret_cast<float*>(rbk + o_as);
  a.tok_conf = reinterpret_cast<double*>(rbk + o_tc);
  hipLaunchKernelGGL(rescore_reduce_kernel, dim3(B), dim3(64), 0, s, a);
  WN_HIP(hipGetLastError());
  WN_HIP(hipMemcpyAsync(m->r_host.p, rbk, o_end, hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  const char* hb = m->r_host.p;
  memcpy(best_idx_host, hb + o_bi, (size_t)B * sizeof(int));
  memcpy(best_score_host, hb + o_bs, (size_t)B * sizeof(float));
  if (confidence_host) memcpy(confidence_host, hb + o_cf, (size_t)B * sizeof(double));
  if (tok_conf_host) memcpy(tok_conf_host, hb + o_tc, (size_t)B * max_len * sizeof(double));
  if (all_scores_host) memcpy(all_scores_host, hb + o_as, nb * sizeof(float));
  return 0;
}

}  // extern "C"
