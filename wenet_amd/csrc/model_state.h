// Internal state of libwenet_amd shared by the engine (model.hip: front ends, weight images;
// conformer.hip: the Conformer layers) and the C ABI (cabi_*.hip: include/wenet_amd.h entry
// points, one file per subsystem): device buffers, the model block clones share (`ModelData`:
// weights and their re-laid-out views), the per-handle settings and workspace (`wn_model`), the
// per-call guards (one host thread per handle, operand precision of the calling thread).  No
// kernels here: each lives in the file that launches it.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wenet_amd.h"
#include "kernels.h"

namespace wn {

const char* last_error_cstr();


// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;             // owns its allocation
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) WN_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    WN_HIP(hipMalloc(&p, want));
    cap = want;
    return 0;
  }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Pinned host staging for the small per-call descriptor uploads.  The event
// makes the next call wait only for the previous call's H2D copies.
struct Stager {
  char* host = nullptr;
  size_t cap = 0, used = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
  Stager() = default;
  Stager(const Stager&) = delete;
  Stager& operator=(const Stager&) = delete;
  ~Stager() {
    if (host) (void)hipHostFree(host);
    if (ev) (void)hipEventDestroy(ev);
  }
  int begin(size_t need) {
    if (!ev) WN_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (pending) { WN_HIP(hipEventSynchronize(ev)); pending = false; }
    if (need > cap) {
      if (host) WN_HIP(hipHostFree(host));
      host = nullptr;
      cap = need + need / 4 + 4096;
      WN_HIP(hipHostMalloc((void**)&host, cap, hipHostMallocDefault));
    }
    used = 0;
    return 0;
  }
  int put(DevBuf& buf, const void* data, size_t bytes, hipStream_t s) {
    WN_TRY(buf.ensure(std::max<size_t>(bytes, 16)));
    if (bytes == 0) return 0;
    const size_t o = (used + 63) / 64 * 64;
    WN_CHECK(o + bytes <= cap, "descriptor staging overflow");
    memcpy(host + o, data, bytes);
    used = o + bytes;
    WN_HIP(hipMemcpyAsync(buf.p, host + o, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  // the same staged copy into a window of a buffer the caller sized
  int put_at(void* dst, const void* data, size_t bytes, hipStream_t s) {
    if (bytes == 0) return 0;
    const size_t o = (used + 63) / 64 * 64;
    WN_CHECK(o + bytes <= cap, "descriptor staging overflow");
    memcpy(host + o, data, bytes);
    used = o + bytes;
    WN_HIP(hipMemcpyAsync(dst, host + o, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  int end(hipStream_t s) {
    WN_HIP(hipEventRecord(ev, s));
    pending = true;
    return 0;
  }
};

// Pinned host memory that only grows: the landing area of result copies (ONE device -> host
// copy per search instead of one staged copy per pageable result array).
struct PinnedBuf {
  char* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) WN_HIP(hipHostFree(p));
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    WN_HIP(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
  }
};

// A second stream of the handle + the two events that order it with the caller's stream: work
// that does not depend on the search result runs there while the (latency-bound, few-CU) prefix
// beam search runs on the caller's stream -- wn_rescore_prefetch in cabi_decoder.hip.
struct SideStream {
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  SideStream() = default;
  SideStream(const SideStream&) = delete;
  SideStream& operator=(const SideStream&) = delete;
  int ensure() {
    if (st) return 0;
    WN_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    WN_HIP(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
    WN_HIP(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
    return 0;
  }
  ~SideStream() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
};

struct Linear { const float* w = nullptr; const float* b = nullptr; int out = 0, in = 0; };
struct Norm { const float* w = nullptr; const float* b = nullptr; };

struct EncLayer {
  Norm norm_ff_mac, norm_mha, norm_conv, norm_ff, norm_final, conv_norm;
  Linear ffm1, ffm2, ff1, ff2, qkv, out, pw1, pw2;
  const float* bias_u = nullptr; const float* bias_v = nullptr;
  const float* pos_w = nullptr;   // linear_pos.weight [d][d]
  float* pos_tab = nullptr;       // [max_pos][d] = linear_pos(pe)
  const float* dw_wt = nullptr;   // [K][d]
  const float* dw_b = nullptr;
  const float* cpad = nullptr;    // [d]
  // Branchformer / E-Branchformer layers (wn_model::bf.on, cabi_branchformer.hip): the cgMLP
  // branch and the merge; qkv / out / pos_tab / bias_u / bias_v then have the head layout of
  // bf.c.head_dim (32: heads zero-padded to 64 columns)
  Norm norm_mlp, csgu_norm;
  Linear proj1, proj2, csgu_lin, merge_proj;
  const float* csgu_wt = nullptr;   // [K][U/2]
  const float* csgu_b = nullptr;
  const float* merge_wt = nullptr;  // [merge_kernel][2d]
  const float* merge_b = nullptr;
  // Squeezeformer layers (wn_model::sq.on, cabi_squeezeformer.hip) are post-LN and reuse the
  // Conformer's slots: norm_mha / norm_ff_mac / norm_conv / norm_final = layer_norm1 .. 4,
  // ffm1 / ffm2 = ffn1, ff1 / ff2 = ffn2; qkv, ffm1, ff1 and pw1 hold the adaptive scale folded
  // in; pos_tab is linear_pos of pe[0::2] for a block that runs at the half rate
  // Efficient Conformer layers (wn_model::ef.on, cabi_efficonformer.hip): the Conformer's slots;
  // ef_rate = product of the strides in front of the layer (pos_tab is linear_pos of
  // pe[0::ef_rate]), ef_kernel its own cnn_module_kernel.  A grouped layer keeps Q | K | V, the
  // table and linear_out d wide and bias_u / bias_v (h, group * d_k); a plain one lays heads of 32
  // out as 64 columns like a Branchformer's
  int ef_rate = 1, ef_kernel = 0;
  bool ef_grouped = false, ef_stride = false;
};

struct TfLayer {  // TransformerEncoderLayer (encoder_layer.py:28-127)
  Norm n1, n2;
  Linear qkv, out, ff1, ff2;
};

struct DecLayer {
  Norm n1, n2, n3;
  Linear self_qkv, self_out, src_q, src_kv, src_out, ff1, ff2;
};

// Paraformer (cabi_paraformer.hip): AliParaformerEncoderLayer, SanmDecoderLayer, Cif
struct PfEncLayer {
  Norm n1, n2;
  Linear qkv, out, ff1, ff2;       // layer 0: qkv is [3 d][576], the 560 input columns zero-padded
  const float* fsmn_wt = nullptr;  // [K][d] tap-major
};
struct PfDecLayer {
  Norm n1, n2, n3, ffn_norm;
  Linear ff1, ff2, src_q, src_kv, src_out;   // ff2 has no bias
  const float* fsmn_wt = nullptr;
};
struct PfData {
  std::vector<PfEncLayer> enc;
  std::vector<PfDecLayer> dec;
  const float* pe = nullptr;         // [max_frames + 1][560] sinusoids (positions start at 1)
  const float* zero_bias = nullptr;  // [d]: the FSMN convs have no bias
  Linear cif_conv;                   // [d][3 d], column tap * d + c_in
  const float* cif_out_w = nullptr; const float* cif_out_b = nullptr;
  Norm dec3_n1, dec3_ffn_norm, dec_after;
  Linear dec3_ff1, dec3_ff2, dec_out;
};

// SenseVoice Small (cabi_sensevoice.hip): the first stack is PfData::enc (with pe and zero_bias),
// the second one and what the front end reads are here
struct SvData {
  std::vector<PfEncLayer> tp;        // encoder.tp_encoders
  Norm tp_norm;
  const float* embed = nullptr;      // [16][560] query rows
};

struct Decoder {
  const float* embed = nullptr;  // [V][d]
  const float* pe = nullptr;     // [max_pos][d] sinusoids, or the learned [dec_max_pos][d] table
  float xscale = 1.0f;           // embedding scale: sqrt(d) with sinusoids, 1 with the learned table
  int max_pos = 0;               // rows of pe
  Norm after;
  Linear out;
  std::vector<DecLayer> layers;
};
}  // namespace wn

using namespace wn;


// ===========================================================================
// What wn_model_create builds and every wn_model_clone()d handle shares: fixed once create
// returns (the handles hold it as const), except the tables at the end, which are built on
// first use under `lazy` and never change afterwards.
struct ModelData {
  DevBuf weights;                        // one slab for every weight
  int64_t n_weight_elems = 0;            // floats in the slab
  // plane images of the weights the six-product fp32 GEMM runs (gemm_x6.hip): fp32 weight
  // pointer -> X3 image
  DevBuf weights_x6;
  std::map<const float*, const void*> x6_at;
  DevBuf weights_x6p;                    // k-slot-permuted FFN w_2 images (ffn_x6f.hip)
  std::map<const float*, const void*> x6p_at;
  // QKV weights with the rows permuted per head ([Q_h | K_h | V_h] x 64) as X3 images + the
  // biases in the same order: the QKV projection that writes the attention's key-tile images
  // itself (gemm_x6r.hip epi 4); fp32 weight pointer -> (image, bias)
  DevBuf weights_x6q;
  std::map<const float*, std::pair<const void*, const float*>> x6q_at;
  // biases of the vocabulary-sized layers (CTC head, decoder output layers) padded with zeros
  // to a multiple of 4 columns: weight pointer -> padded bias
  DevBuf bias4_buf;
  std::map<const float*, const float*> bias4;
  std::map<std::string, const float*> w; // name -> device pointer
  // re-laid-out subsampling weights
  const float* conv1_w = nullptr; const float* conv1_b = nullptr;
  Linear conv2, sub_out;
  const float* cmvn_mean = nullptr; const float* cmvn_istd = nullptr;
  const float* pe = nullptr;
  Norm after_norm;
  Linear ctc;
  std::vector<EncLayer> layers;
  std::vector<TfLayer> tf_layers;       // encoder_type 1
  Linear tconv1, tconv2;                // Conv1dSubsampling2 as gathered-row GEMMs
  bool fbank_ok = true;
  Decoder left, right;
  DevBuf pos_tabs;
  // hybrid transducer (wn_model::tr.on): RNNPredictor + TransducerJoint
  struct LstmLayer { const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; };
  const float* pred_embed = nullptr;     // [V][pred_embed]
  std::vector<LstmLayer> pred_rnn;
  Linear pred_proj, j_enc, j_pred, j_out;
  // stateless predictors (wn_model::tr.sp.kind != 0; no LSTM layers): EmbeddingPredictor's
  // pos_embed.weight [heads][E][C] and ffn, ConvPredictor's conv [E][C] (+ bias), the LayerNorm
  const float* pred_pos = nullptr;
  const float* pred_conv_w = nullptr; const float* pred_conv_b = nullptr;
  Linear pred_ffn;
  Norm pred_norm;
  PfData pf;                             // wn_model::pf.on (sv.on: enc, pe, zero_bias)
  SvData sv;                             // wn_model::sv.on
  // Squeezeformer (wn_model::sq.on): preln, the time reduction's depthwise taps [K][d] + bias
  // and pointwise conv, time_recover_layer
  Norm sq_preln;
  const float* sq_red_wt = nullptr; const float* sq_red_b = nullptr;
  Linear sq_red_pw, sq_recover;
  // fbank tables
  const float* fb_window = nullptr; const float* fb_twiddle = nullptr;
  const float* fb_mel_w = nullptr;
  DevBuf fb_tab_i;

  // ---- built on first use ------------------------------------------------------------------
  // Look up or build under `lazy`, publish a finished buffer only (DevBuf::swap), then read
  // without the lock: a DevBuf that is set never changes, and std::map nodes do not move.  A
  // handle reads a precision image only after its own wn_model_set_precision returned (or the
  // one of the handle it was cloned from).
  mutable std::mutex lazy;
  mutable DevBuf weights_bf16;           // bf16 image of the slab (bf16 mode)
  // MXFP8 images of the FFN weights (fp8 mode): fp32 weight pointer ->
  // (e4m3 [N][K], block scales [K/128][N] dwords)
  struct MxW { const void* q; const unsigned* scale; };
  mutable DevBuf weights_mx;
  mutable std::map<const float*, MxW> mx_at;
  mutable bool mx_built = false;
  // Whisper log-mel: DFT / window tables, mel matrix per bin count
  mutable DevBuf lm_dft;
  mutable std::map<int, DevBuf> lm_mel;
  // resampler taps per (orig, new) rate pair (wn_resample)
  mutable std::map<std::pair<int, int>, DevBuf> rs_taps;
};

// A handle: the shared model block + this handle's settings, current batch and workspace.
struct wn_model {
  wn_config cfg;
  // wn_model_create_transducer: the predictor / joint widths (tr.on == false: an asr_model)
  // sp.kind != 0: wn_model_create_transducer_stateless (c.pred_layers == 0, c.pred_hidden == 0)
  struct {
    bool on = false;
    wn_transducer_config c = {};
    wn_stateless_predictor_config sp = {};
  } tr;
  // wn_model_create_firered: the FireRedASR-AED encoder (cabi_firered.hip); data->layers then
  // hold its shapes (pw1 4d x d, depthwise / conv_norm over 2d, pw2 d x 2d, norm_mha = the
  // plain normalisation in front of the folded QKV, pos_tab = 2 max_frames - 1 rows)
  struct {
    bool on = false;
    wn_firered_config c = {};
  } fr;
  // wn_model_create_branchformer: a Branchformer (kind 1) / E-Branchformer (kind 2) encoder
  // (cabi_branchformer.hip) behind the Conformer front end
  struct {
    bool on = false;
    wn_branchformer_config c = {};
  } bf;
  // wn_model_create_paraformer: SANM encoder, CIF predictor, SANM decoder (cabi_paraformer.hip);
  // data->layers / tf_layers stay empty, data->pf holds the weights
  struct {
    bool on = false;
    wn_paraformer_config c = {};
  } pf;
  // wn_model_create_squeezeformer: a Squeezeformer encoder (cabi_squeezeformer.hip)
  struct {
    bool on = false;
    wn_squeezeformer_config c = {};
  } sq;
  // ... its half-rate rows, their layout (off | len | row_utt in one block) and its own stager
  DevBuf sq_xh, sq_desc;
  Stager sq_stage;
  // wn_model_create_efficonformer: an Efficient Conformer encoder (cabi_efficonformer.hip)
  struct {
    bool on = false;
    wn_efficonformer_config c = {};
  } ef;
  // ... the rows behind a stride layer before they become x, the layouts of every rate (off |
  // len | row_utt per rate in one block) and their own stager
  DevBuf ef_x2, ef_desc;
  Stager ef_stage;
  DevBuf pf_alpha, pf_img, pf_emb, pf_int, pf_x, pf_y, pf_t, pf_o, pf_q, pf_kv, pf_h, pf_out;
  PinnedBuf pf_host;
  // wn_model_create_sensevoice: SenseVoice Small (cabi_sensevoice.hip); data->pf.enc and
  // data->sv hold the weights.  qid: the query ids wn_sensevoice_set_queries stored for the next
  // wn_encode (empty: the defaults); sv_desc = feature lengths | query ids on the device
  struct {
    bool on = false;
    wn_sensevoice_config c = {};
    std::vector<int> qid;
  } sv;
  DevBuf sv_desc;
  Stager sv_stage;
  int device = 0;
  // never null: wn_workspace_create gives an empty block
  std::shared_ptr<const ModelData> data = std::make_shared<ModelData>();
  bool fp8_ffn = false;                  // WN_PREC_FP8: prec == PREC_BF16 + MXFP8 FFN GEMMs
  DevBuf nb_map, nb_keep, nb_enc, nb_off_old;   // filter_blank_embedding scratch
  DevBuf x6_a, x6_h;                     // images of the GEMM input rows / the FFN hidden tensor
  DevBuf x6_lin;                         // image of linear()'s A operand (large fp32 GEMMs)
  DevBuf mx_sa, mx_sh;                   // block scales of the LN output / FFN hidden

  // ---- current batch ----------------------------------------------------
  int B = 0, Tp = 0, rows = 0;          // rows of the encoder-output layout
  std::vector<int> off, len;            // per utterance (rows layout)
  DevBuf d_off, d_len, d_row_utt, d_off1, d_len1, d_a_row_off;
  DevBuf c1, c2, x, t1, t2, hbuf, qkv, enc;
  DevBuf bf_cat, bf_mrg, bf_gate, bf_stats;   // Branchformer: [x1 | x2], its merge, the gated half
  DevBuf ffn_part;                      // hidden-slice partials of the fused FFN
  DevBuf attn_kbias;                    // per-key score term of the folded rel-pos attention
  DevBuf xpad, pos_rows, d_row_t, d_zero_rows;
  DevBuf ck_kv, ck_xext, ck_glu, ck_desc, ck_rowutt, ck_sess;  // forward_chunk scratch
  DevBuf lm_off, lm_foff, lm_nfr, lm_rowutt, lm_frames, lm_spec, lm_pw, lm_melout, lm_umax;
  // ctc
  int ctc_rows = 0, ctc_k = 0;
  bool ctc_valid = false;
  bool ln0_done = false;   // t1 already holds layer 0's norm_ff_macaron(x) (sub_out_linear)
  int front_route = 0;     // front_route_code() of the last subsample_conv2d4 (0: no rows)
  DevBuf logits, topk_val, topk_idx;
  // searches
  DevBuf pb_dbg;
  DevBuf g_tok, g_len, pb_pool;
  DevBuf pb_out;          // the prefix beam search's results, one block: counts | lengths | scores | tokens | times
  PinnedBuf pb_host;      // ... and where they land on the host
  // the n-best of the last wn_ctc_prefix_beam_search, still in pb_out / pb_host, for wn_rescore:
  // batch size, beam, row pitch and the byte offsets of the fields inside the block
  bool pb_valid = false;
  int pb_B = 0, pb_beam = 0, pb_max_len = 0;
  size_t pb_o_sc = 0, pb_o_nh = 0, pb_o_len = 0, pb_o_tok = 0;
  // forced alignment (cabi_align.hip): descriptors + labels | back pointers | results, one
  // block: score | status | path | frame log-probs | emissions
  DevBuf al_desc, al_bp, al_out;
  PinnedBuf al_host;
  // rescoring
  DevBuf r_tok, r_rtok, r_pos, r_tgt, r_rtgt, r_qoff, r_qlen, r_kvoff, r_kvlen;
  DevBuf r_x, r_t1, r_t2, r_qkv, r_h, r_mem, r_logits, r_out;
  DevBuf r_mem_all;            // per-layer cross-attention K/V of the current batch
  DevBuf r_seqsrc, r_seqfirst; // wn_rescore: sequence -> (utt, hyp) slot, first sequence per utterance
  DevBuf r_gqoff, r_gqlen, r_gkvoff, r_gkvlen;   // wn_rescore: cross-attention groups (one per utterance)
  DevBuf r_hyp;                // wn_rescore: host-given n-best (tokens | ctc scores) on the device
  DevBuf r_res;                // wn_rescore: results, one block
  PinnedBuf r_host;            // ... and where they land on the host
  DevBuf ab_cache, ab_state;   // `attention` mode: self-attention K|V cache, beam state
  DevBuf ab_prompt;            // ... its prompts (B, P) and the prefill descriptors
  DevBuf sk_part;              // split-K partials of the skinny step GEMMs (gemm_skinny.hip)
  // wn_transducer_greedy_search: enc_proj | predictor state and outputs | joint partials |
  // search state and tokens; the pinned n_active slots the host loop polls one group late
  DevBuf tr_enc, tr_f32, tr_i32, tr_tok;
  DevBuf tr_ctc;          // wn_transducer_beam_search: the CTC log-prob rows it fuses with
  int tr_beam_steps = 0;            // ... its last call: steps issued,
  int64_t tr_beam_advance = 0;      // rows that ran the LSTM step, summed over the steps
  // wn_transducer_score, its last call: GEMM rows (frames x trie nodes), what they would have
  // been without the trie (frames x sum of len + 1), trie nodes
  int64_t tr_score_rows = 0, tr_score_unshared = 0;
  int tr_score_nodes = 0;
  DevBuf tr_sc_f32, tr_sc_i32, tr_sc_logp;
  hipEvent_t tr_sc_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // its stage marks
  float tr_score_ms[4] = {0.f, 0.f, 0.f, 0.f};   // enc_proj, predictor, gather GEMM, lattice
  PinnedBuf tr_host;
  hipEvent_t tr_ev[2] = {nullptr, nullptr};
  ~wn_model() {
    for (hipEvent_t e : tr_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : tr_sc_ev) if (e) (void)hipEventDestroy(e);
  }
  bool ab_truncated = false;   // the last prompted search stopped at the positional table
  bool mem_cache_valid = false;

  SideStream side;             // wn_rescore_prefetch
  // cross-attention K | V of the current batch for every decoder layer (left, then right),
  // projected ahead of the rescoring pass (wn_rescore_prefetch), and the plane image of the
  // encoder output they were projected from
  DevBuf r_kv_all, r_enc3;
  // X3 plane image of t1 = LN(x) for the fused six-product FFN (tune().ffn_ximg): valid while
  // t1_img_ok (set by the producer launch, cleared by the consumer)
  DevBuf attn_img;      // key-tile images of the six-product attention (attention_x6.hip)
  int attn_blk_off = 0, attn_n_blk = 0;   // its block list inside d_row_utt (set_layout)
  DevBuf t1_img;
  bool t1_img_ok = false;
  bool kv_ready = false;
  // wn_model_set_encode_gate: one-shot event the next wn_encode waits for.  Where: behind its
  // descriptor uploads and in front of conv1 (tune enc_gate_pos = 0, default), or behind
  // CMVN + conv1 (= 1: chained encoders of several handles overlap that HBM-bound kernel);
  // conv paths that never reach either position wait once conv2 is queued (model.hip).  The
  // gate orders work for performance only -- each handle has its own workspace, no result
  // depends on it
  hipEvent_t enc_gate = nullptr;
  int kv_rows = 0, kv_nl = 0, kv_nr = 0;
  Stager stage;
  // optional HIP-event bracket around the FFN w_1 GEMM launches (the kernel
  // the roofline is quoted on); see wn_profile_*.
  std::vector<hipEvent_t> prof_ev;
  size_t prof_used = 0;
  bool prof_on = false;
  unsigned prof_seq = 0;
  unsigned prof_stride = 6;   // every prof_stride-th launch of the kernel is bracketed
  double prof_flops = 0.0;
  const char* prof_kernel = "gemm (FFN w_1)";  // what the bracketed launches were
  int prof_split = 1;        // hidden slices / K slices of the feed-forward module last run
  int prec = PREC_F32;       // GEMM operand precision (wn_model_set_precision)
  // one host thread per handle: the workspace, the descriptor staging and the
  // current batch are per-handle state.  Entry points take this flag and fail
  // loudly (status -4) instead of corrupting the staging buffer when a second
  // thread enters the same handle (use wn_model_clone for a second thread).
  std::atomic<bool> busy{false};
  // tuning knobs (tune.h): this handle's overrides (wn_model_tune_set; TUNE_INHERIT = follow
  // the process default) and the effective set WN_ENTER resolves for the call in flight
  Tune tune_ovr = tune_all_inherit();
  Tune tune_eff;
  int dbg_layers = -1;       // run only the first n encoder layers
  int dbg_skip_after_norm = 0;
  // context biasing tables (wn_set_context_graph); ctx.keys == nullptr: none
  std::shared_ptr<DevBuf> ctx_buf;
  CtxGraph ctx;
  DevBuf fb_off, fb_nfr;

  int F1() const { return (cfg.feat_dim - 1) / 2; }
  int F2() const { return (F1() - 1) / 2; }
};


// Wait for a stream whose last work item is milliseconds long and whose result the caller needs
// NOW (the searches' result copies): poll instead of sleeping on the completion interrupt, whose
// wake-up costs tens of microseconds per decode; after 50 ms (a stuck or very long queue) fall
// back to the blocking wait.  wn_tune_set("sync_spin", 0) = always the blocking wait (A/B).
inline hipError_t stream_wait(hipStream_t s) {
  if (tune().sync_spin != 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0;; ++i) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return e;
      if ((i & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    }
  }
  return hipStreamSynchronize(s);
}

// One host thread per handle at a time; for the duration of the C-ABI call the handle's
// effective tuning set (tune.h: its overrides over the process defaults) is the calling
// thread's tune().
struct HandleGuard {
  wn_model* m;
  bool ok;
  const Tune* saved_tune;
  explicit HandleGuard(wn_model* m_) : m(m_), ok(false), saved_tune(t_tune) {
    bool expected = false;
    ok = m->busy.compare_exchange_strong(expected, true, std::memory_order_acquire);
    if (ok) {
      tune_resolve(m->tune_ovr, &m->tune_eff);
      t_tune = &m->tune_eff;
    }
  }
  ~HandleGuard() {
    if (ok) {
      t_tune = saved_tune;
      m->busy.store(false, std::memory_order_release);
    }
  }
};
#define WN_ENTER(m)                                                              \
  HandleGuard handle_guard(m);                                                   \
  if (!handle_guard.ok) {                                                        \
    ::wn::set_error("this wn_model handle is in use by another host thread; "    \
                    "one thread per handle (wn_model_clone gives a second one)"); \
    return -4;                                                                   \
  }

extern thread_local const std::map<const float*, ModelData::MxW>* t_mx;
// plane images of the current model's weights and its activation-image scratch: linear()
// routes the large fp32 GEMMs to the six-product kernel through them (gemm_x6.hip)
extern thread_local const std::map<const float*, const void*>* t_x6;
extern thread_local DevBuf* t_x6_a;

struct PrecisionScope {
  int saved;
  const float* s_f32; const void* s_bf16; int64_t s_elems;
  const std::map<const float*, ModelData::MxW>* s_mx;
  const std::map<const float*, const void*>* s_x6; DevBuf* s_x6_a;
  explicit PrecisionScope(const wn_model* m)
      : saved(t_gemm_prec), s_f32(t_wslab_f32), s_bf16(t_wslab_bf16),
        s_elems(t_wslab_elems), s_mx(t_mx), s_x6(t_x6), s_x6_a(t_x6_a) {
    const ModelData& W = *m->data;
    t_mx = m->fp8_ffn ? &W.mx_at : nullptr;
    t_x6 = &W.x6_at;
    t_x6_a = const_cast<DevBuf*>(&m->x6_lin);
    t_gemm_prec = m->prec;
    const bool img = m->prec == PREC_BF16 && W.weights_bf16.p;
    t_wslab_f32 = img ? W.weights.as<float>() : nullptr;
    t_wslab_bf16 = img ? W.weights_bf16.p : nullptr;
    t_wslab_elems = img ? W.n_weight_elems : 0;
  }
  ~PrecisionScope() {
    t_gemm_prec = saved;
    t_wslab_f32 = s_f32; t_wslab_bf16 = s_bf16; t_wslab_elems = s_elems;
    t_mx = s_mx;
    t_x6 = s_x6; t_x6_a = s_x6_a;
  }
};

// ---- engine (model.hip, conformer.hip) ----------------------------------------------------

bool bf16_store_active();
int upload_desc(wn_model* m, DevBuf& buf, const std::vector<int>& v, hipStream_t s);
// linear(): GEMMs from this many 0.1 GFLOP on go to the six-product kernel through a split pass
constexpr int g_x6_linear_min = 60;   // (40 / 20 measured slower at configs 3 / 4, r05l)
extern thread_local bool t_linear_took_x6;   // what the last linear() of this thread ran on
int linear(const Linear& l, const float* A, int lda, float* C, int ldc, int M, hipStream_t s,
           int act = ACT_NONE, const float* resid = nullptr, int ldr = 0, float alpha = 1.0f,
           bool glu = false, bool a_bf16 = false, bool c_bf16 = false);
int ln(const Norm& n, const float* x, float* y, int M, int D, float eps, hipStream_t s,
       bool y_bf16 = false);
int after_norm_out(wn_model* m, hipStream_t s);
// skip_encoder: no images of the encoder layers / subsampling weights (FireRed handles)
int build_x6_images(const wn_config& cfg, ModelData& W, bool skip_encoder = false);
int vocab_linear(wn_model* m, const Linear& l, const float* A, int lda, float* C, int ldc, int M,
                 hipStream_t s);
int scatter_padded(const float* src, int lds, const int* off, const int* len, int B, int Tp, int D,
                   float* dst, hipStream_t s);
int set_layout(wn_model* m, int B, int Tp, const std::vector<int>& off,
               const std::vector<int>& len, int rows, hipStream_t s);
int subsample_conv2d4(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                      int T, int32_t* enc_lens_host, int pos0, hipStream_t s);
int encode_gate_wait(wn_model* m, hipStream_t s);
// How subsample_conv2d4 ran (wn_model::front_route, wn_op_conv2d4's route_out).
enum Conv2Kind {
  CONV2_GEMM_F32 = 0,    // conv1 fp32, conv2 as the gathered-row v_mfma_f32 GEMM (gemm_f32)
  CONV2_X6_AF32 = 1,     // conv1 fp32, conv2 six-product with the fp32 gather
  CONV2_X6_PLANES = 2    // conv1 writes its plane image, conv2 six-product gathers from it
};
int conv2_kind(const wn_model* m, int M, int M1, const void** w6);
// bit 16: set (rows ran) | bit 13: linear() took the six-product kernel | bit 12: the projection
// ran as sub_out_linear | bits 8-11: K slices of conv2's tail | bits 4-7: X6ConvTile |
// bits 0-3: Conv2Kind
inline int front_route_code(int kind, const X6ConvForm& f, bool sub_out, bool linear_x6) {
  return kind | f.tile << 4 | f.slices << 8 | (int)sub_out << 12 | (int)linear_x6 << 13 | 1 << 16;
}
// (conformer.hip: the Conformer layers and the feed-forward routing)
int ffn_module(wn_model* m, const Norm& nrm, const Linear& w1, const Linear& w2, int act,
               float alpha, bool ln_done, bool h16, hipStream_t s);
int ffn_x6_split(int M, int F);
int ffn_x6_pair(wn_model* m, const Linear& w1, const Linear& w2, int act, const float* A, int M,
                hipStream_t s);
int encoder_layers(wn_model* m, int chunk, int left, hipStream_t s);
int encoder_layers_chunk(wn_model* m, int n_sess, int R, const int* offsets,
                         std::vector<ChunkSess>& sess, float* out, hipStream_t s);
// (cabi_firered.hip)
int encode_firered(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B, int T,
                   float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s);
// (cabi_branchformer.hip)
int encode_branchformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                        int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                        hipStream_t s);
// (cabi_squeezeformer.hip)
int encode_squeezeformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                         int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                         hipStream_t s);
// (cabi_efficonformer.hip)
namespace wn { struct Src; struct HostStage; }
int efficonformer_config_check(const wn_config& c, const wn_efficonformer_config& e,
                               bool other_family);
int efficonformer_stage_front2(const wn::Src& src, wn::HostStage& hs, const wn_config& c, int F1);
int efficonformer_stage_layers(const wn::Src& src, wn::HostStage& hs, const wn_config& c,
                               const wn_efficonformer_config& e);
int efficonformer_bind(ModelData& W, const wn_config& c, const wn_efficonformer_config& e);
int encode_efficonformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                         int T, int chunk, int left, float* enc_out_dev, int32_t* enc_lens_host,
                         hipStream_t s);
// (cabi_paraformer.hip)
int encode_paraformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                      int T, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s);
// AliParaformerEncoderLayer.forward (layers.py:144-180) over the current batch's M packed rows for
// the first n_run layers of `layers`: x1 = [x +] linear_out(attention) + fsmn(v); out = x1 +
// w_2(relu(w_1(LN(x1)))).  first_wide: layers[0] reads the ld0 columns the front end normalised
// into m->t1 and has no residual around the attention; every other layer reads and writes m->x.
// K: the FSMN taps.
int pf_encoder_layers(wn_model* m, const std::vector<wn::PfEncLayer>& layers, int n_run,
                      bool first_wide, int ld0, int K, int B, int M, int max_len, hipStream_t s);
// (cabi_sensevoice.hip)
int encode_sensevoice(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                      int T, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s);
// (cabi_model.hip: what every wn_model_create* entry point runs)
int create_model_impl(const wn_config* cfg, const wn_transducer_config* tcfg,
                      const wn_stateless_predictor_config* scfg, const wn_firered_config* fcfg,
                      const wn_branchformer_config* bcfg, const wn_squeezeformer_config* qcfg,
                      const wn_efficonformer_config* ecfg, const wn_tensor* weights,
                      int32_t n_weights, int32_t device, wn_model** out);
// (model.hip)
int encode_transformer(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int B,
                       int T, float* enc_out_dev, int32_t* enc_lens_host, hipStream_t s);

