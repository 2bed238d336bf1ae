// C ABI (include/wenet_amd.h), forced alignment: wn_ctc_force_align = CTC head, emission gather,
// Viterbi trellis + backtrace (ctc_align.hip), one result copy into pinned memory.
#include "model_state.h"

namespace wn {
namespace {

// the argument checks: nothing here touches the device or the handle
int align_check(int blank_id, const int32_t* labels, const int32_t* label_lens, int max_label,
                const int32_t* lens, int B, int Tp, int V, const int32_t* status_host) {
  WN_CHECK(labels && label_lens && status_host, "wn_ctc_force_align: null argument");
  WN_CHECK(B >= 1 && Tp >= 1 && V >= 1 && max_label >= 0, "wn_ctc_force_align: bad argument");
  WN_CHECK(blank_id >= 0 && blank_id < V, "wn_ctc_force_align: blank_id outside the vocabulary");
  for (int b = 0; b < B; ++b) {
    WN_CHECK(label_lens[b] >= 0 && label_lens[b] <= max_label,
             "wn_ctc_force_align: label_len must be in [0, max_label]");
    if (lens) WN_CHECK(lens[b] >= 0 && lens[b] <= Tp, "wn_ctc_force_align: length > Tp");
    for (int i = 0; i < label_lens[b]; ++i) {
      const int id = labels[(size_t)b * max_label + i];
      if (id < 0 || id >= V) {
        set_error("wn_ctc_force_align: label id " + std::to_string(id) + " of utterance " +
                  std::to_string(b) + " is outside the vocabulary [0, " + std::to_string(V) + ")");
        return -1;
      }
      WN_CHECK(id != blank_id, "wn_ctc_force_align: blank_id among the labels");
    }
  }
  return 0;
}

}  // namespace
}  // namespace wn

extern "C" {

int wn_ctc_force_align(wn_model* m, int32_t blank_id, float blank_penalty,
                       const int32_t* labels_host, const int32_t* label_lens_host,
                       int32_t max_label, const float* logp_dev, const int32_t* lens_host,
                       int32_t B, int32_t Tp, int32_t V, int32_t* path_host, float* score_host,
                       int32_t* status_host, float* frame_logp_host, float* emit_host,
                       void* stream) {
  const bool given = logp_dev != nullptr;
  if (given) {
    WN_CHECK(lens_host, "wn_ctc_force_align: null lengths with caller-provided log-probs");
    WN_TRY(align_check(blank_id, labels_host, label_lens_host, max_label, lens_host, B, Tp, V,
                       status_host));
    WN_CHECK(m, "wn_ctc_force_align: null handle");
  } else {
    WN_CHECK(m && m->B > 0 && m->enc.p,
             "wn_ctc_force_align: no current batch (call wn_encode / wn_set_encoder_out)");
    WN_CHECK(!lens_host, "wn_ctc_force_align: lens_host without logp_dev");
    WN_CHECK(B == m->B && Tp == m->Tp, "wn_ctc_force_align: B / Tp are not the current batch's");
    V = m->cfg.vocab;
    WN_TRY(align_check(blank_id, labels_host, label_lens_host, max_label, nullptr, B, Tp, V,
                       status_host));
  }
  WN_ENTER(m);
  PrecisionScope prec_scope(m);
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));

  // rows: the packed layout of the current batch, or the caller's padded tensor
  const int M = given ? B * Tp : m->rows;
  std::vector<int> off(B), len(B);
  for (int b = 0; b < B; ++b) {
    off[b] = given ? b * Tp : m->off[b];
    len[b] = given ? lens_host[b] : m->len[b];
  }
  // descriptors, one upload: off | len | label_len | labels (B, LP) | bp_off (int64)
  const int LP = max_label + 1;
  int max_fast = -1, max_slow = -1;
  std::vector<int> d((size_t)3 * B + (size_t)B * LP);
  std::vector<int64_t> bp_off(B);
  int64_t bp_bytes = 0;
  for (int b = 0; b < B; ++b) {
    const int L = label_lens_host[b];
    d[b] = off[b]; d[B + b] = len[b]; d[2 * B + b] = L;
    int* lab = d.data() + 3 * (size_t)B + (size_t)b * LP;
    lab[0] = blank_id;
    for (int i = 0; i < LP - 1; ++i) lab[1 + i] = i < L ? labels_host[(size_t)b * max_label + i] : blank_id;
    if (2 * L + 1 <= ALIGN_FAST_S) max_fast = std::max(max_fast, L);
    else max_slow = std::max(max_slow, L);
    bp_off[b] = bp_bytes;
    bp_bytes += ctc_align_bp_bytes(len[b], L, ALIGN_FAST_S);
  }
  const size_t d_bytes = (d.size() * sizeof(int) + 7) / 8 * 8;
  WN_TRY(m->stage.begin(d_bytes + bp_off.size() * sizeof(int64_t) + 256));
  WN_TRY(m->al_desc.ensure(d_bytes + bp_off.size() * sizeof(int64_t)));
  WN_TRY(m->stage.put_at(m->al_desc.p, d.data(), d.size() * sizeof(int), s));
  WN_TRY(m->stage.put_at(m->al_desc.as<char>() + d_bytes, bp_off.data(),
                         bp_off.size() * sizeof(int64_t), s));
  WN_TRY(m->stage.end(s));
  const int* dd = m->al_desc.as<int>();

  // results, one block: score | status | path | frame log-probs | E (packed rows, pitch LP)
  const size_t o_sc = 0, o_st = o_sc + (size_t)B * sizeof(float),
               o_path = o_st + (size_t)B * sizeof(int),
               o_fl = o_path + (size_t)B * Tp * sizeof(int),
               o_e = (o_fl + (size_t)B * Tp * 2 * sizeof(float) + 255) / 256 * 256,
               o_end = o_e + (size_t)std::max(M, 1) * LP * sizeof(float);
  WN_TRY(m->al_out.ensure(o_end));
  WN_TRY(m->al_bp.ensure((size_t)bp_bytes + 64));
  char* ob = m->al_out.as<char>();
  float* E = reinterpret_cast<float*>(ob + o_e);

  if (M > 0) {
    AlignGatherArgs g;
    g.M = M; g.V = V; g.blank = blank_id;
    g.off = dd; g.len = dd + B; g.lab_len = dd + 2 * B; g.lab = dd + 3 * B; g.lab_pitch = LP;
    g.E = E; g.ldE = LP;
    if (given) {
      g.x = logp_dev; g.ld = V; g.normalize = 0; g.blank_penalty = 0.f;
      g.row_utt = nullptr; g.Tp = Tp;
    } else {
      const ModelData& W = *m->data;
      WN_CHECK(W.ctc.w, "wn_ctc_force_align: this handle has no weights");
      const int V4 = (V + 31) / 32 * 32;      // the row pitch of wn_ctc_logprobs
      WN_TRY(m->logits.ensure((size_t)M * V4 * sizeof(float)));
      WN_TRY(vocab_linear(m, W.ctc, m->enc.as<float>(), m->cfg.d_model, m->logits.as<float>(), V4,
                          M, s));
      g.x = m->logits.as<float>(); g.ld = V4; g.normalize = 1;
      g.blank_penalty = blank_penalty > 0.f ? blank_penalty : 0.f;
      g.row_utt = m->d_row_utt.as<int>(); g.Tp = Tp;
    }
    WN_TRY(ctc_align_gather(g, s));
  }
  AlignArgs a;
  a.E = E; a.ldE = LP; a.off = dd; a.len = dd + B; a.B = B; a.Tp = Tp;
  a.lab = dd + 3 * B; a.lab_pitch = LP; a.lab_len = dd + 2 * B;
  a.bp = m->al_bp.as<unsigned char>();
  a.bp_off = reinterpret_cast<const int64_t*>(m->al_desc.as<char>() + d_bytes);
  a.fast_S = ALIGN_FAST_S;
  a.path = reinterpret_cast<int*>(ob + o_path);
  a.frame_logp = frame_logp_host ? reinterpret_cast<float*>(ob + o_fl) : nullptr;
  a.score = reinterpret_cast<float*>(ob + o_sc);
  a.status = reinterpret_cast<int*>(ob + o_st);
  WN_TRY(ctc_align_viterbi(a, max_fast, max_slow, s));
  const size_t n_copy = emit_host ? o_end : (frame_logp_host ? o_e : o_fl);
  WN_TRY(m->al_host.ensure(n_copy));
  WN_HIP(hipMemcpyAsync(m->al_host.p, ob, n_copy, hipMemcpyDeviceToHost, s));
  WN_HIP(stream_wait(s));
  const char* hb = m->al_host.p;
  const int* st = reinterpret_cast<const int*>(hb + o_st);
  const float* sc = reinterpret_cast<const float*>(hb + o_sc);
  for (int b = 0; b < B; ++b) {
    status_host[b] = st[b];
    if (st[b] != 0) continue;
    if (score_host) score_host[b] = sc[b];
    const size_t n = (size_t)len[b];
    if (path_host)
      memcpy(path_host + (size_t)b * Tp, hb + o_path + (size_t)b * Tp * sizeof(int),
             n * sizeof(int));
    if (frame_logp_host)
      memcpy(frame_logp_host + (size_t)b * Tp * 2, hb + o_fl + (size_t)b * Tp * 2 * sizeof(float),
             n * 2 * sizeof(float));
    if (emit_host)
      memcpy(emit_host + (size_t)b * Tp * LP, hb + o_e + (size_t)off[b] * LP * sizeof(float),
             n * LP * sizeof(float));
  }
  return 0;
}

}  // extern "C"
