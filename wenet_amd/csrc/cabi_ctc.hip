// C ABI (include/wenet_amd.h), the CTC side: log-probs and top-k of the current batch, greedy
// and prefix beam search, blank filtering, the context graph, and the streaming sessions
// (wn_stream_*: the resumable prefix beam search).
#include "model_state.h"

// Everything a set owns is allocated in wn_stream_create or grows on the first call that needs
// it (the top-k / logits scratch, whose size depends on the chunk): a steady stream of chunks
// allocates nothing.
struct wn_stream_set {
  wn_model* m = nullptr;
  int n_slots = 0, beam = 0, max_frames = 0, blank = 0;
  float blank_thr = 0.8f;
  int64_t pool_ints = 0;             // per slot
  DevBuf state, pool;                // StreamState[n_slots] | 4 pools per slot (ctc.hip)
  DevBuf emit;                       // per slot: the last 1-best walked out (ctc.hip)
  std::vector<int> abs_t;            // host mirror of every slot's frame counter
  DevBuf desc;                       // slot | off | len of the call in flight
  Stager stage;
  DevBuf topk_val, topk_idx, logits;
  DevBuf out;                        // the results of a call, one block
  PinnedBuf host;                    // ... and where they land on the host
};

namespace wn {
namespace {

// packed rows -> padded (B, Tp, D) with zero fill, any width D: the (B,Tp,V) log-probs
__global__ void scatter_padded_any_kernel(const float* src, int lds,
                                          const int* off, const int* len,
                                          int Tp, int D, float* dst) {
  const int b = blockIdx.y, t = blockIdx.x;
  float* d = dst + ((int64_t)b * Tp + t) * D;
  if (t < len[b]) {
    const float* s = src + (int64_t)(off[b] + t) * lds;
    for (int i = threadIdx.x; i < D; i += blockDim.x) d[i] = s[i];
  } else {
    for (int i = threadIdx.x; i < D; i += blockDim.x) d[i] = 0.f;
  }
}

__global__ __launch_bounds__(256) void topk_raw_kernel(const float* x, int ld,
                                                        int V, int k,
                                                        float* tv, int* ti) {
  // top-k of an already normalised row (no log-softmax): k block-argmax rounds
  __shared__ float rv[4];
  __shared__ int ri[4];
  __shared__ float cv;
  __shared__ int ci;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = x + (int64_t)row * ld;
  float pv = INFINITY;
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += 256) {
      const float v = p[i];
      if ((v < pv || (v == pv && i > pi)) && (v > bv || (v == bv && i < bi))) {
        bv = v; bi = i;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (rv[w] > rv[0] || (rv[w] == rv[0] && ri[w] < ri[0])) { rv[0] = rv[w]; ri[0] = ri[w]; }
      cv = rv[0]; ci = ri[0];
      tv[(int64_t)row * k + r] = cv;
      ti[(int64_t)row * k + r] = ci;
    }
    __syncthreads();
    pv = cv; pi = ci;
  }
}

// WN_PB_CYCLES (debugging aid): the cycle counters workgroup 0 of a prefix beam search kernel
// leaves behind, printed after the launch.  `empty_too`: print a call that saw no frame as well.
struct PbCycles {
  long long* dev = nullptr;
  int arm(wn_model* m, long long** arg) {
    static const bool on = getenv("WN_PB_CYCLES") != nullptr;
    if (!on) return 0;
    WN_TRY(m->pb_dbg.ensure(8 * sizeof(long long)));
    *arg = dev = m->pb_dbg.as<long long>();
    return 0;
  }
  int print(const char* what, const char* tail, bool empty_too, hipStream_t s) const {
    if (!dev) return 0;
    long long h[5];
    WN_HIP(hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, s));
    WN_HIP(hipStreamSynchronize(s));
    if (empty_too || h[3] > 0)
      fprintf(stderr, "[wn] %s wg0: frames %lld, cycles/frame eval %.0f rank %.0f "
              "select %.0f; %s %lld cycles\n", what, h[3], (double)h[0] / h[3],
              (double)h[1] / h[3], (double)h[2] / h[3], tail, h[4]);
    return 0;
  }
};

struct StreamOutLayout {
  size_t sc, vit, nh, len, tlen, fd, tb, tok, tim, end;
  StreamOutLayout(size_t n, size_t rows, size_t max_len) {
    const size_t nr = n * rows;
    sc = 0; vit = sc + nr * sizeof(double); nh = vit + nr * sizeof(double);
    len = nh + n * sizeof(int); tlen = len + nr * sizeof(int); fd = tlen + nr * sizeof(int);
    tb = fd + n * sizeof(int); tok = tb + n * sizeof(int);
    tim = tok + nr * max_len * sizeof(int); end = tim + nr * max_len * sizeof(int);
  }
};

// argument checks of an advance call: nothing here touches the device or a session
int stream_check(const wn_stream_set* S, int n, const int32_t* slot_ids, const int32_t* n_t,
                 int Tp, const wn_stream_result* out) {
  WN_CHECK(n >= 1 && n <= S->n_slots, "wn_stream_advance: n must be in [1, n_slots]");
  WN_CHECK(out->n_hyps && out->hyp_lens && out->hyp_tlens && out->hyp_tokens &&
               out->hyp_times && out->hyp_scores && out->frames_decoded && out->trailing_blank,
           "wn_stream_advance: null output");
  WN_CHECK(S->m->ctx.keys == nullptr,
           "wn_stream_advance: a context graph is installed on this handle; context biasing "
           "is not supported in streaming sessions (its finalize() mutates the beam)");
  std::vector<char> seen(S->n_slots, 0);
  int longest = 1;
  for (int i = 0; i < n; ++i) {
    const int sl = slot_ids[i];
    WN_CHECK(sl >= 0 && sl < S->n_slots, "wn_stream_advance: slot id out of range");
    WN_CHECK(!seen[sl], "wn_stream_advance: a slot is named twice in one call");
    seen[sl] = 1;
    WN_CHECK(n_t[i] >= 0 && n_t[i] <= Tp, "wn_stream_advance: need 0 <= n_t <= Tp");
    if (S->abs_t[sl] + n_t[i] > S->max_frames) {
      set_error("wn_stream_advance: the session in slot " + std::to_string(sl) + " has " +
                std::to_string(S->abs_t[sl]) + " frames and would pass max_frames = " +
                std::to_string(S->max_frames) + " with " + std::to_string(n_t[i]) +
                " more; no session was advanced");
      return -1;
    }
    longest = std::max(longest, S->abs_t[sl] + n_t[i]);
  }
  WN_CHECK(out->max_len >= longest,
           "wn_stream_advance: max_len smaller than the frames a session has consumed");
  return 0;
}

// the search itself on top-k pairs already in S->topk_*; logp (pitch ld): the full rows
int stream_search(wn_stream_set* S, int n, const int32_t* slot_ids, const int32_t* n_t, int Tp,
                  const float* logp, int ld, int nbest, const wn_stream_result* out,
                  hipStream_t s) {
  const int beam = S->beam, rows = nbest ? beam : 1, max_len = out->max_len;
  std::vector<int> d(3 * (size_t)n);
  for (int i = 0; i < n; ++i) { d[i] = slot_ids[i]; d[n + i] = i * Tp; d[2 * n + i] = n_t[i]; }
  WN_TRY(S->stage.begin(d.size() * sizeof(int) + 64));
  WN_TRY(S->stage.put(S->desc, d.data(), d.size() * sizeof(int), s));
  WN_TRY(S->stage.end(s));
  const StreamOutLayout o(n, rows, max_len);
  WN_TRY(S->out.ensure(o.end));
  WN_TRY(S->host.ensure(o.end));
  char* ob = S->out.as<char>();
  StreamPrefixBeamArgs a;
  a.topk_val = S->topk_val.as<float>(); a.topk_idx = S->topk_idx.as<int>(); a.k = beam;
  a.off = S->desc.as<int>() + n; a.len = S->desc.as<int>() + 2 * n; a.B = n;
  a.beam = beam; a.blank = S->blank; a.max_len = S->max_frames;
  a.pool = S->pool.as<int>(); a.pool_stride = S->pool_ints;
  a.n_hyps = reinterpret_cast<int*>(ob + o.nh); a.hyp_lens = reinterpret_cast<int*>(ob + o.len);
  a.hyp_tlens = reinterpret_cast<int*>(ob + o.tlen);
  a.hyp_tokens = reinterpret_cast<int*>(ob + o.tok);
  a.hyp_times = reinterpret_cast<int*>(ob + o.tim);
  a.hyp_scores = reinterpret_cast<double*>(ob + o.sc);
  a.st.state = S->state.p; a.st.slot = S->desc.as<int>();
  a.st.nbest = nbest ? 1 : 0; a.st.out_stride = max_len;
  a.st.logp = logp; a.st.ld = ld; a.st.blank_thr = S->blank_thr;
  a.st.hyp_vit = reinterpret_cast<double*>(ob + o.vit);
  a.st.emit = S->emit.as<int>();
  a.st.frames = reinterpret_cast<int*>(ob + o.fd); a.st.trail = reinterpret_cast<int*>(ob + o.tb);
  PbCycles dbg;
  WN_TRY(dbg.arm(S->m, &a.dbg_cycles));
  WN_TRY(ctc_prefix_beam_stream(a, s));
  WN_TRY(dbg.print("stream search", "state store + emit", false, s));
  WN_HIP(hipMemcpyAsync(S->host.p, ob, o.end, hipMemcpyDeviceToHost, s));
  // the kernel is queued: the sessions have consumed their frames whatever the copy does
  for (int i = 0; i < n; ++i) S->abs_t[slot_ids[i]] += n_t[i];
  WN_HIP(stream_wait(s));
  const char* hb = S->host.p;
  const int* nh = reinterpret_cast<const int*>(hb + o.nh);
  const int* hl = reinterpret_cast<const int*>(hb + o.len);
  const int* htl = reinterpret_cast<const int*>(hb + o.tlen);
  const double* sc = reinterpret_cast<const double*>(hb + o.sc);
  const double* vit = reinterpret_cast<const double*>(hb + o.vit);
  memcpy(out->n_hyps, nh, (size_t)n * sizeof(int));
  memcpy(out->frames_decoded, hb + o.fd, (size_t)n * sizeof(int));
  memcpy(out->trailing_blank, hb + o.tb, (size_t)n * sizeof(int));
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < beam; ++j) {
      const size_t dst = (size_t)i * beam + j, src = (size_t)i * rows + j;
      const bool have = j < rows;   // (1-best mode: the other rows read as an empty beam slot)
      const int nl = have ? std::min(std::max(hl[src], 0), max_len) : 0;
      const int ntl = have ? std::min(std::max(htl[src], 0), max_len) : 0;
      out->hyp_lens[dst] = nl; out->hyp_tlens[dst] = ntl;
      out->hyp_scores[dst] = have ? sc[src] : -HUGE_VAL;
      if (out->hyp_viterbi) out->hyp_viterbi[dst] = have ? vit[src] : -HUGE_VAL;
      if (have) {
        memcpy(out->hyp_tokens + dst * max_len, hb + o.tok + src * max_len * sizeof(int),
               (size_t)nl * sizeof(int));
        memcpy(out->hyp_times + dst * max_len, hb + o.tim + src * max_len * sizeof(int),
               (size_t)ntl * sizeof(int));
      }
    }
  }
  return 0;
}

}  // namespace
}  // namespace wn

// ===========================================================================
extern "C" {

int wn_ctc_logprobs(wn_model* m, int32_t topk, int32_t blank_id,
                    float blank_penalty, float* logp_dev, int32_t Tp,
                    void* stream) {
  WN_CHECK(m && m->B > 0, "wn_ctc_logprobs: no current batch (call wn_encode)");
  WN_ENTER(m);
  m->pb_valid = false;
  PrecisionScope prec_scope(m);
  const ModelData& W = *m->data;
  WN_CHECK(W.ctc.w, "wn_ctc_logprobs: this handle has no weights");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int M = m->rows, V = c.vocab;
  const int k = std::max(1, topk);
  WN_CHECK(k <= V, "top-k larger than the vocabulary");
  WN_CHECK(!logp_dev || Tp == m->Tp, "wn_ctc_logprobs: Tp mismatch");
  m->ctc_rows = M; m->ctc_k = k;
  int ldv = V;
  if (M > 0) {
    // logits rows at a pitch of V rounded up to 32 floats: whole 128-byte lines per row, so
    // that the GEMM's column tiles (multiples of 128 columns) never share a line -- at a pitch
    // of V rounded up to 4 (round 5) the tile edges fell inside lines written by two blocks on
    // two XCDs, and the counters showed the read-modify-write: 140 MB READ + 168 MB written
    // by a GEMM whose operands are 19 MB and whose result is 134 MB (r13b)
    const int V4 = (V + 31) / 32 * 32;
    ldv = V4;
    WN_TRY(m->logits.ensure((size_t)M * V4 * sizeof(float)));
    WN_TRY(m->topk_val.ensure((size_t)M * k * sizeof(float)));
    WN_TRY(m->topk_idx.ensure((size_t)M * k * sizeof(int)));
    WN_TRY(vocab_linear(m, W.ctc, m->enc.as<float>(), c.d_model, m->logits.as<float>(), V4, M,
                        s));
    CtcRowArgs r;
    r.logits = m->logits.as<float>(); r.ld = V4; r.M = M; r.V = V; r.k = k;
    r.blank = blank_id; r.blank_penalty = blank_penalty > 0.f ? blank_penalty : 0.f;
    r.topk_val = m->topk_val.as<float>(); r.topk_idx = m->topk_idx.as<int>();
    // normalised rows are written back in place when the caller wants them
    r.logp = logp_dev ? m->logits.as<float>() : nullptr; r.ld_out = V4;
    WN_TRY(ctc_logsoftmax_topk(r, s));
  }
  if (logp_dev) {
    if (M > 0) {
      hipLaunchKernelGGL(scatter_padded_any_kernel, dim3(m->Tp, m->B), dim3(256),
                         0, s, m->logits.as<float>(), ldv, m->d_off.as<int>(),
                         m->d_len.as<int>(), m->Tp, V, logp_dev);
      WN_HIP(hipGetLastError());
    } else {
      WN_HIP(hipMemsetAsync(logp_dev, 0, (size_t)m->B * m->Tp * V * sizeof(float), s));
    }
  }
  m->ctc_valid = true;
  return 0;
}

int wn_set_ctc_probs(wn_model* m, const float* logp_dev, const int32_t* lens_host,
                     int32_t B, int32_t Tp, int32_t V, int32_t topk,
                     void* stream) {
  WN_CHECK(m && logp_dev && lens_host && B > 0 && Tp > 0 && V > 0,
           "wn_set_ctc_probs: bad argument");
  WN_ENTER(m);
  m->pb_valid = false;
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const int k = std::max(1, topk);
  WN_CHECK(k <= V, "top-k larger than the vocabulary");
  std::vector<int> off(B), len(B);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens_host[b] >= 0 && lens_host[b] <= Tp, "length > Tp");
    off[b] = b * Tp; len[b] = lens_host[b];
  }
  WN_TRY(set_layout(m, B, Tp, off, len, B * Tp, s));
  WN_TRY(m->stage.end(s));
  const int M = B * Tp;
  WN_TRY(m->topk_val.ensure((size_t)M * k * sizeof(float)));
  WN_TRY(m->topk_idx.ensure((size_t)M * k * sizeof(int)));
  hipLaunchKernelGGL(topk_raw_kernel, dim3(M), dim3(256), 0, s, logp_dev, V, V,
                     k, m->topk_val.as<float>(), m->topk_idx.as<int>());
  WN_HIP(hipGetLastError());
  m->ctc_rows = M; m->ctc_k = k; m->ctc_valid = true;
  return 0;
}

int wn_ctc_greedy_search(wn_model* m, int32_t blank_id, int32_t* tokens_host,
                         int32_t* tok_lens_host, int32_t max_len, void* stream) {
  WN_CHECK(m && m->ctc_valid, "greedy: no CTC posteriors (call wn_ctc_logprobs)");
  WN_ENTER(m);
  WN_CHECK(tokens_host && tok_lens_host, "greedy: null output");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const int B = m->B;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = std::max(longest, m->len[b]);
  WN_CHECK(max_len >= longest, "greedy: max_len smaller than the longest utterance");
  const int ml = std::max(max_len, 1);
  WN_TRY(m->g_tok.ensure((size_t)B * ml * sizeof(int)));
  WN_TRY(m->g_len.ensure((size_t)B * sizeof(int)));
  WN_TRY(ctc_greedy_collapse(m->topk_idx.as<int>(), m->ctc_k, m->d_off.as<int>(),
                             m->d_len.as<int>(), B, blank_id, m->g_tok.as<int>(),
                             ml, m->g_len.as<int>(), s));
  WN_HIP(hipMemcpyAsync(tokens_host, m->g_tok.p, (size_t)B * ml * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(hipMemcpyAsync(tok_lens_host, m->g_len.p, (size_t)B * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  return 0;
}

int wn_filter_blank_embedding(wn_model* m, float* padded_out_dev, int32_t* n_keep_host,
                              int32_t* t_out, void* stream) {
  WN_CHECK(m && m->B > 0 && m->enc.p && m->ctc_valid && n_keep_host && t_out,
           "filter_blank_embedding: needs the encoder output and the CTC posteriors of the "
           "current batch (wn_encode / wn_set_encoder_out, then wn_ctc_logprobs)");
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const int B = m->B, d = m->cfg.d_model, M = m->rows;
  WN_CHECK(m->ctc_rows == M, "filter_blank_embedding: CTC posteriors of another layout");
  WN_TRY(m->nb_map.ensure((size_t)std::max(M, 1) * sizeof(int)));
  WN_TRY(m->nb_keep.ensure((size_t)B * sizeof(int)));
  WN_TRY(nonblank_map(m->topk_idx.as<int>(), m->ctc_k, m->d_off.as<int>(), m->d_len.as<int>(), B,
                      m->nb_map.as<int>(), m->nb_keep.as<int>(), s));
  std::vector<int> keep(B);
  WN_HIP(hipMemcpyAsync(keep.data(), m->nb_keep.p, (size_t)B * sizeof(int),
                        hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  int T = 0;
  for (int b = 0; b < B; ++b) { n_keep_host[b] = keep[b]; T = std::max(T, keep[b]); }
  *t_out = T;
  if (T == 0) {
    // a batch of silence: the reference fails here (pad_sequence of empty selections,
    // asr_model.py:165-172).  One silent batch must not end a long recognize.py run: the
    // layout and the encoder output stay as they are (rescoring then attends to the
    // unfiltered frames) and the caller is told through *t_out == 0.
    static bool warned = false;
    if (!warned) {
      fprintf(stderr, "[wenet_amd] filter_blank_embedding: no non-blank frame in the whole "
                      "batch; the encoder output is left unfiltered\n");
      warned = true;
    }
    return 0;
  }
  // new layout: utterance b keeps min(len[b], T) rows -- attention_rescoring slices the
  // zero-padded (B, T, d) tensor with the UNFILTERED lengths (asr_model.py:337-342,
  // search.py:396): the selected rows, then zero rows the decoder attends to as well
  std::vector<int> noff(B), nlen(B), old_off = m->off;
  int rows = 0;
  for (int b = 0; b < B; ++b) { noff[b] = rows; nlen[b] = std::min(m->len[b], T); rows += nlen[b]; }
  WN_TRY(m->nb_enc.ensure((size_t)std::max(rows, 1) * d * sizeof(float)));
  // descriptors of the OLD layout stay valid on the device until set_layout replaces them:
  // gather first (it reads d_off of the old layout through a private copy)
  WN_TRY(m->nb_off_old.ensure((size_t)B * sizeof(int)));
  WN_HIP(hipMemcpyAsync(m->nb_off_old.p, m->d_off.p, (size_t)B * sizeof(int),
                        hipMemcpyDeviceToDevice, s));
  WN_TRY(set_layout(m, B, T, noff, nlen, rows, s));
  WN_TRY(m->stage.end(s));
  WN_TRY(nonblank_gather(m->enc.as<float>(), m->nb_map.as<int>(), m->nb_off_old.as<int>(),
                         m->nb_keep.as<int>(), m->d_off.as<int>(), m->d_len.as<int>(),
                         m->d_row_utt.as<int>(), m->nb_enc.as<float>(), d, rows, s));
  m->enc.swap(m->nb_enc);
  if (padded_out_dev) {
    // the reference's return value: (B, T, d), utterance b's selected rows then zeros
    WN_HIP(hipMemsetAsync(padded_out_dev, 0, (size_t)B * T * d * sizeof(float), s));
    for (int b = 0; b < B; ++b)
      if (keep[b] > 0)
        WN_HIP(hipMemcpyAsync(padded_out_dev + (size_t)b * T * d,
                              m->enc.as<float>() + (size_t)noff[b] * d,
                              (size_t)std::min(keep[b], nlen[b]) * d * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

int wn_set_context_graph(wn_model* m, int32_t n_nodes, const int32_t* fail,
                         const double* node_score, const double* output_score,
                         const double* token_score, int32_t n_edges,
                         const int32_t* edge_from, const int32_t* edge_token,
                         const int32_t* edge_to, void* stream) {
  WN_CHECK(m, "context graph: null model");
  WN_ENTER(m);
  if (n_nodes <= 0) {
    m->ctx = CtxGraph();
    m->ctx_buf.reset();
    return 0;
  }
  WN_CHECK(fail && node_score && output_score && token_score,
           "context graph: null node array");
  WN_CHECK(n_edges >= 0 && (n_edges == 0 || (edge_from && edge_token && edge_to)),
           "context graph: null edge array");
  WN_CHECK(fail[0] == 0, "context graph: node 0 must be the root (fail[0] == 0)");
  for (int i = 0; i < n_nodes; ++i)
    WN_CHECK(fail[i] >= 0 && fail[i] < n_nodes, "context graph: fail arc out of range");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  unsigned slots = 16;
  while (slots < 2u * (unsigned)n_edges) slots *= 2;
  std::vector<unsigned long long> keys(slots, CTX_EMPTY);
  std::vector<int> vals(slots, -1);
  for (int i = 0; i < n_edges; ++i) {
    WN_CHECK(edge_from[i] >= 0 && edge_from[i] < n_nodes && edge_to[i] > 0 &&
                 edge_to[i] < n_nodes && edge_token[i] >= 0,
             "context graph: edge out of range");
    const unsigned long long key =
        ((unsigned long long)(unsigned)edge_from[i] << 32) | (unsigned)edge_token[i];
    unsigned h = ctx_slot(key, slots - 1);
    while (keys[h] != CTX_EMPTY) {
      WN_CHECK(keys[h] != key, "context graph: duplicate edge");
      h = (h + 1) & (slots - 1);
    }
    keys[h] = key;
    vals[h] = edge_to[i];
  }
  // one slab: keys | 3 x double[n] | fail[n] | vals[slots]
  const size_t o_keys = 0;
  const size_t o_ns = o_keys + slots * sizeof(unsigned long long);
  const size_t o_os = o_ns + (size_t)n_nodes * sizeof(double);
  const size_t o_ts = o_os + (size_t)n_nodes * sizeof(double);
  const size_t o_fail = o_ts + (size_t)n_nodes * sizeof(double);
  const size_t o_vals = o_fail + (size_t)n_nodes * sizeof(int);
  const size_t total = o_vals + slots * sizeof(int);
  std::vector<char> host(total);
  memcpy(host.data() + o_keys, keys.data(), slots * sizeof(unsigned long long));
  memcpy(host.data() + o_ns, node_score, (size_t)n_nodes * sizeof(double));
  memcpy(host.data() + o_os, output_score, (size_t)n_nodes * sizeof(double));
  memcpy(host.data() + o_ts, token_score, (size_t)n_nodes * sizeof(double));
  memcpy(host.data() + o_fail, fail, (size_t)n_nodes * sizeof(int));
  memcpy(host.data() + o_vals, vals.data(), slots * sizeof(int));
  // a fresh buffer: clones of this handle may still search with the old one
  auto buf = std::make_shared<DevBuf>();
  WN_TRY(buf->ensure(total));
  WN_HIP(hipMemcpyAsync(buf->p, host.data(), total, hipMemcpyHostToDevice, s));
  WN_HIP(hipStreamSynchronize(s));
  char* base = buf->as<char>();
  CtxGraph g;
  g.keys = reinterpret_cast<const unsigned long long*>(base + o_keys);
  g.node_score = reinterpret_cast<const double*>(base + o_ns);
  g.output_score = reinterpret_cast<const double*>(base + o_os);
  g.token_score = reinterpret_cast<const double*>(base + o_ts);
  g.fail = reinterpret_cast<const int*>(base + o_fail);
  g.vals = reinterpret_cast<const int*>(base + o_vals);
  g.mask = slots - 1;
  m->ctx_buf = buf;
  m->ctx = g;
  return 0;
}

int wn_ctc_prefix_beam_search(wn_model* m, int32_t beam, int32_t blank_id,
                              int32_t* n_hyps_host, int32_t* hyp_lens_host,
                              int32_t* hyp_tlens_host, int32_t* hyp_tokens_host,
                              int32_t* hyp_times_host, double* hyp_scores_host,
                              int32_t max_len, void* stream) {
  WN_CHECK(m && m->ctc_valid, "prefix beam: no CTC posteriors");
  WN_ENTER(m);
  WN_CHECK(m->ctc_k == beam, "prefix beam: wn_ctc_logprobs must be called with topk == beam");
  WN_CHECK(n_hyps_host && hyp_lens_host && hyp_tlens_host && hyp_tokens_host &&
               hyp_times_host && hyp_scores_host, "prefix beam: null output");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const int B = m->B;
  int longest = 0;
  for (int b = 0; b < B; ++b) longest = std::max(longest, m->len[b]);
  WN_CHECK(max_len >= longest && max_len >= 1, "prefix beam: max_len too small");
  const int64_t pool = prefix_beam_pool_ints(max_len, beam);
  WN_TRY(m->pb_pool.ensure((size_t)B * pool * sizeof(int)));
  const size_t nb = (size_t)B * beam;
  // the results in ONE device block -> one copy into pinned memory (six staged copies into the
  // caller's pageable arrays took ~130 us of host round trips per batch, r05f trace)
  const size_t o_sc = 0, o_nh = o_sc + nb * sizeof(double), o_len = o_nh + (size_t)B * sizeof(int),
               o_tlen = o_len + nb * sizeof(int), o_tok = o_tlen + nb * sizeof(int),
               o_tim = o_tok + nb * max_len * sizeof(int),
               o_end = o_tim + nb * max_len * sizeof(int);
  WN_TRY(m->pb_out.ensure(o_end));
  WN_TRY(m->pb_host.ensure(o_end));
  char* ob = m->pb_out.as<char>();
  PrefixBeamArgs a;
  a.topk_val = m->topk_val.as<float>(); a.topk_idx = m->topk_idx.as<int>();
  a.k = m->ctc_k; a.off = m->d_off.as<int>(); a.len = m->d_len.as<int>();
  a.B = B; a.beam = beam; a.blank = blank_id; a.max_len = max_len;
  a.pool = m->pb_pool.as<int>(); a.pool_stride = pool;
  a.n_hyps = reinterpret_cast<int*>(ob + o_nh); a.hyp_lens = reinterpret_cast<int*>(ob + o_len);
  a.hyp_tlens = reinterpret_cast<int*>(ob + o_tlen);
  a.hyp_tokens = reinterpret_cast<int*>(ob + o_tok);
  a.hyp_times = reinterpret_cast<int*>(ob + o_tim);
  a.hyp_scores = reinterpret_cast<double*>(ob + o_sc);
  a.cg = m->ctx;
  PbCycles dbg;
  WN_TRY(dbg.arm(m, &a.dbg_cycles));
  WN_TRY(ctc_prefix_beam(a, s));
  WN_TRY(dbg.print("prefix beam", "emit", true, s));
  m->pb_valid = false;
  WN_HIP(hipMemcpyAsync(m->pb_host.p, ob, o_end, hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  m->pb_valid = true; m->pb_B = B; m->pb_beam = beam; m->pb_max_len = max_len;
  m->pb_o_sc = o_sc; m->pb_o_nh = o_nh; m->pb_o_len = o_len; m->pb_o_tok = o_tok;
  const char* hb = m->pb_host.p;
  memcpy(n_hyps_host, hb + o_nh, (size_t)B * sizeof(int));
  memcpy(hyp_lens_host, hb + o_len, nb * sizeof(int));
  memcpy(hyp_tlens_host, hb + o_tlen, nb * sizeof(int));
  memcpy(hyp_scores_host, hb + o_sc, nb * sizeof(double));
  // tokens / times: only the used corner of each [max_len] row (the caller's arrays are
  // zero-initialised; the kernel writes nothing past a hypothesis' length that anyone reads)
  const int* hl = reinterpret_cast<const int*>(hb + o_len);
  const int* htl = reinterpret_cast<const int*>(hb + o_tlen);
  for (size_t i = 0; i < nb; ++i) {
    const int nl = std::min(std::max(hl[i], 0), (int)max_len);
    const int ntl = std::min(std::max(htl[i], 0), (int)max_len);
    memcpy(hyp_tokens_host + i * max_len, hb + o_tok + i * max_len * sizeof(int), nl * sizeof(int));
    memcpy(hyp_times_host + i * max_len, hb + o_tim + i * max_len * sizeof(int), ntl * sizeof(int));
  }
  return 0;
}

int wn_stream_create(wn_model* m, int32_t n_slots, int32_t beam, int32_t max_frames,
                     int32_t blank_id, wn_stream_set** out, void* stream) {
  WN_CHECK(m && out, "wn_stream_create: null argument");
  WN_CHECK(!m->fr.on, "wn_stream_create: the FireRed encoder does not stream");
  WN_CHECK(!m->bf.on, "wn_stream_create: a Branchformer encoder does not stream");
  WN_CHECK(!m->sq.on, "wn_stream_create: a Squeezeformer encoder does not stream");
  WN_CHECK(!m->ef.on, "wn_stream_create: an Efficient Conformer encoder does not stream");
  WN_CHECK(n_slots >= 1 && max_frames >= 1 && blank_id >= 0, "wn_stream_create: bad argument");
  WN_CHECK(beam >= 1, "wn_stream_create: beam_size must be positive");
  WN_CHECK(beam <= 16, "wn_stream_create: streaming sessions support beam sizes 1..16; larger "
                       "beams (17..64) are served by the one-shot wn_ctc_prefix_beam_search only");
  WN_CHECK((int64_t)max_frames * beam + 1 < (1ll << 29), "wn_stream_create: max_frames too large");
  WN_CHECK(m->ctx.keys == nullptr,
           "wn_stream_create: a context graph is installed on this handle; context biasing is "
           "not supported in streaming sessions (its finalize() mutates the beam)");
  WN_ENTER(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  std::unique_ptr<wn_stream_set> S(new wn_stream_set());
  S->m = m; S->n_slots = n_slots; S->beam = beam; S->max_frames = max_frames; S->blank = blank_id;
  S->pool_ints = prefix_beam_pool_ints(max_frames, beam);
  S->abs_t.assign(n_slots, 0);
  WN_TRY(S->state.ensure((size_t)n_slots * stream_state_bytes()));
  WN_TRY(S->pool.ensure((size_t)n_slots * S->pool_ints * sizeof(int)));
  WN_TRY(S->emit.ensure((size_t)n_slots * stream_emit_ints(max_frames) * sizeof(int)));
  WN_TRY(S->desc.ensure(3 * (size_t)n_slots * sizeof(int)));
  // results: the worst case of a 1-best call over all slots up front; an n-best call (the
  // final one of a session) grows it to what it needs once
  const StreamOutLayout o(n_slots, 1, max_frames);
  WN_TRY(S->out.ensure(o.end));
  WN_TRY(S->host.ensure(o.end));
  std::vector<int> all(n_slots);
  for (int i = 0; i < n_slots; ++i) all[i] = i;
  WN_TRY(S->stage.begin(all.size() * sizeof(int) + 64));
  WN_TRY(S->stage.put(S->desc, all.data(), all.size() * sizeof(int), s));
  WN_TRY(S->stage.end(s));
  WN_TRY(ctc_stream_reset(S->state.p, S->pool.as<int>(), S->pool_ints, max_frames, beam,
                          S->desc.as<int>(), n_slots, s));
  WN_HIP(hipStreamSynchronize(s));
  *out = S.release();
  return 0;
}

int wn_stream_destroy(wn_stream_set* set) {
  delete set;
  return 0;
}

int wn_stream_set_endpoint(wn_stream_set* set, float blank_threshold, float blank_scale) {
  WN_CHECK(set, "wn_stream_set_endpoint: null argument");
  WN_CHECK(blank_threshold > 0.f && blank_scale > 0.f, "wn_stream_set_endpoint: bad argument");
  set->blank_thr = blank_threshold * blank_scale;
  return 0;
}

int wn_stream_reset(wn_stream_set* set, int32_t n, const int32_t* slot_ids, void* stream) {
  WN_CHECK(set && slot_ids, "wn_stream_reset: null argument");
  WN_CHECK(n >= 1 && n <= set->n_slots, "wn_stream_reset: n must be in [1, n_slots]");
  for (int i = 0; i < n; ++i)
    WN_CHECK(slot_ids[i] >= 0 && slot_ids[i] < set->n_slots, "wn_stream_reset: slot id out of range");
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  WN_TRY(set->stage.begin((size_t)n * sizeof(int) + 64));
  WN_TRY(set->stage.put(set->desc, slot_ids, (size_t)n * sizeof(int), s));
  WN_TRY(set->stage.end(s));
  WN_TRY(ctc_stream_reset(set->state.p, set->pool.as<int>(), set->pool_ints, set->max_frames,
                          set->beam, set->desc.as<int>(), n, s));
  for (int i = 0; i < n; ++i) set->abs_t[slot_ids[i]] = 0;
  return 0;
}

int wn_stream_advance(wn_stream_set* set, int32_t n, const int32_t* slot_ids,
                      const float* logp_dev, const int32_t* n_t_host, int32_t Tp, int32_t V,
                      int32_t nbest, const wn_stream_result* out, void* stream) {
  WN_CHECK(set && slot_ids && logp_dev && n_t_host && out, "wn_stream_advance: null argument");
  WN_CHECK(Tp >= 1 && V >= 1, "wn_stream_advance: bad argument");
  WN_CHECK(set->beam <= V, "wn_stream_advance: top-k larger than the vocabulary");
  WN_CHECK(set->blank < V, "wn_stream_advance: blank_id outside the vocabulary");
  WN_TRY(stream_check(set, n, slot_ids, n_t_host, Tp, out));
  WN_ENTER(set->m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(set->m->device));
  const int M = n * Tp, k = set->beam;
  WN_TRY(set->topk_val.ensure((size_t)M * k * sizeof(float)));
  WN_TRY(set->topk_idx.ensure((size_t)M * k * sizeof(int)));
  hipLaunchKernelGGL(topk_raw_kernel, dim3(M), dim3(256), 0, s, logp_dev, V, V, k,
                     set->topk_val.as<float>(), set->topk_idx.as<int>());
  WN_HIP(hipGetLastError());
  return stream_search(set, n, slot_ids, n_t_host, Tp, logp_dev, V, nbest, out, s);
}

int wn_stream_advance_encoded(wn_stream_set* set, int32_t n, const int32_t* slot_ids,
                              const float* enc_out_dev, const int32_t* n_t_host, int32_t chunk,
                              int32_t nbest, const wn_stream_result* out, void* stream) {
  WN_CHECK(set && slot_ids && enc_out_dev && n_t_host && out,
           "wn_stream_advance_encoded: null argument");
  WN_CHECK(chunk >= 1, "wn_stream_advance_encoded: bad argument");
  wn_model* m = set->m;
  const ModelData& W = *m->data;
  WN_CHECK(W.ctc.w, "wn_stream_advance_encoded: this handle has no weights");
  WN_CHECK(set->beam <= m->cfg.vocab && set->blank < m->cfg.vocab,
           "wn_stream_advance_encoded: beam / blank_id outside the vocabulary");
  WN_TRY(stream_check(set, n, slot_ids, n_t_host, chunk, out));
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  const wn_config& c = m->cfg;
  const int M = n * chunk, V = c.vocab, k = set->beam;
  const int V4 = (V + 31) / 32 * 32;   // the row pitch of wn_ctc_logprobs
  WN_TRY(set->logits.ensure((size_t)M * V4 * sizeof(float)));
  WN_TRY(set->topk_val.ensure((size_t)M * k * sizeof(float)));
  WN_TRY(set->topk_idx.ensure((size_t)M * k * sizeof(int)));
  WN_TRY(vocab_linear(m, W.ctc, enc_out_dev, c.d_model, set->logits.as<float>(), V4, M, s));
  CtcRowArgs r;
  r.logits = set->logits.as<float>(); r.ld = V4; r.M = M; r.V = V; r.k = k;
  r.blank = set->blank; r.blank_penalty = 0.f;
  r.topk_val = set->topk_val.as<float>(); r.topk_idx = set->topk_idx.as<int>();
  r.logp = set->logits.as<float>(); r.ld_out = V4;   // normalised in place: the endpoint reads it
  WN_TRY(ctc_logsoftmax_topk(r, s));
  return stream_search(set, n, slot_ids, n_t_host, chunk, set->logits.as<float>(), V4, nbest, out,
                       s);
}

}  // extern "C"
