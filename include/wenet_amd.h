/* libwenet_amd -- C ABI of the MI355X-native Conformer-ASR inference path.
 *
 * The reference (wenet-e2e/wenet) has NO operator / FFI boundary on this path:
 * `ASRModel.decode()` (wenet/models/transformer/asr_model.py:267-343) calls
 * torch.nn modules and the pure-Python functions of
 * wenet/models/transformer/search.py.  This header is the boundary a
 * maintainer would bind instead (ctypes stub in INTEGRATION.md); every entry
 * point names the reference function(s) it replaces.  The only C-ABI precedent
 * in the reference is the streaming recogniser runtime/core/api/wenet_api.h:27-108
 * (opaque handle, int status); the same style is kept here, but batch-oriented
 * and tensor-in / tensor-out.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (-1 bad argument, -2 HIP
 *    error, -3 missing / mis-shaped weight, -4 handle busy); wn_last_error() gives the thread-local message;
 *  - `*_dev` pointers are device (HBM) pointers owned by the caller (e.g. a
 *    torch-ROCm tensor's data_ptr()); `*_host` pointers are host memory;
 *  - `stream` is a hipStream_t (0 = default stream).  Launches are
 *    asynchronous; functions that fill host outputs synchronise `stream`
 *    before returning;
 *  - the library owns the weights and a workspace arena that grows on demand;
 *    one wn_model per process/GPU (one process per GPU for multi-GPU);
 *  - a handle is used by ONE host thread at a time (workspace, descriptor
 *    staging and current batch are per-handle state): a second thread that
 *    enters a busy handle gets -4 and must use its own wn_model_clone();
 *  - all arithmetic is fp32 (fp64 for the prefix-beam bookkeeping, like the
 *    reference's Python floats) unless wn_model_set_precision() opts a handle
 *    into bf16 operands; tokens / lengths are int32.
 */
#ifndef WENET_AMD_H_
#define WENET_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wn_model wn_model;

/* Parsed train.yaml (wenet/utils/init_model.py:100-181 reads the same keys). */
typedef struct {
  int32_t feat_dim;          /* input_dim, 80 */
  int32_t d_model;           /* encoder_conf.output_size */
  int32_t n_heads;           /* encoder_conf.attention_heads (d_model/n_heads must be 64) */
  int32_t ffn_dim;           /* encoder_conf.linear_units */
  int32_t n_layers;          /* encoder_conf.num_blocks */
  int32_t cnn_kernel;        /* encoder_conf.cnn_module_kernel */
  int32_t causal;            /* encoder_conf.causal */
  int32_t use_dynamic_chunk; /* encoder_conf.use_dynamic_chunk */
  int32_t static_chunk_size; /* encoder_conf.static_chunk_size */
  int32_t vocab;             /* output_dim */
  int32_t has_cmvn;
  int32_t dec_heads;         /* decoder_conf.attention_heads */
  int32_t dec_ffn_dim;       /* decoder_conf.linear_units */
  int32_t dec_layers;        /* decoder_conf.num_blocks (left-to-right) */
  int32_t dec_r_layers;      /* decoder_conf.r_num_blocks; 0 if not bitransformer */
  int32_t bidirectional;     /* decoder == 'bitransformer' */
  int32_t sos, eos;          /* asr_model.py:59-62 */
  int32_t max_pos;           /* positional table length (5000) */
  float norm_eps;            /* 1e-5 */
  /* encoder family (wenet/utils/init_model.py:52-97, class_utils.py:37-98) */
  int32_t encoder_type;      /* 0: conformer (rel_pos, conv2d, swish, macaron)
                                1: transformer (TransformerEncoderLayer,
                                   encoder_layer.py:28-127; Whisper encoder) */
  int32_t input_layer;       /* 0: conv2d (Conv2dSubsampling4)
                                1: conv1d2 (Conv1dSubsampling2, subsampling.py:117-171) */
  int32_t activation;        /* FFN activation: 0 swish/SiLU, 1 gelu (exact erf) */
  int32_t key_bias;          /* attention linear_k has a bias (Whisper: 0) */
  int32_t cnn_norm;          /* conv-module norm: 0 layer_norm, 1 batch_norm (eval:
                                running statistics; convolution.py:77-81) */
  /* decoder variants (the Whisper decoder, decoder.py:59-135); all 0 = the classic
   * TransformerDecoder: ReLU, sinusoid positions x sqrt(d), every projection biased */
  int32_t dec_activation;    /* decoder FFN activation: 0 relu, 1 gelu (exact erf) */
  int32_t dec_key_bias;      /* 0: self-attention linear_k has a bias; 1: it has none */
  int32_t dec_src_key_bias;  /* the same for the cross attention's linear_k */
  int32_t dec_learned_pos;   /* 1: decoder.embed.1.pe is a learned (1, dec_max_pos, d) weight,
                                added to the UNSCALED embedding (embedding.py:167-175) */
  int32_t dec_max_pos;       /* rows of that table (Whisper: 448) */
} wn_config;

/* One entry of the reference state_dict (fp32, host memory, C-contiguous). */
typedef struct {
  const char* name;
  const float* data;
  int64_t numel;
} wn_tensor;

const char* wn_last_error(void);
const char* wn_version(void);

/* Build a model from a reference state_dict; replaces
 * init_model + load_checkpoint + model.to(device)
 * (wenet/utils/init_model.py:184, wenet/utils/checkpoint.py:26-43,
 *  wenet/cli/model.py:109).  Weights are re-laid-out for the kernels. */
int wn_model_create(const wn_config* cfg, const wn_tensor* weights,
                    int32_t n_weights, int32_t device, wn_model** out);
void wn_model_destroy(wn_model* m);

/* A second handle on the same (immutable, shared) weights with its own
 * workspace and current batch: one handle per in-flight batch lets a host keep
 * several batches running on different streams (wenet_amd/pipeline.py).
 * Handles may be used from different host threads, one thread per handle. */
int wn_model_clone(const wn_model* src, wn_model** out);

/* Operand precision of the handle's contractions: the reference's
 * `recognize.py --dtype {fp32,bf16}` (wenet/bin/recognize.py:52-56,250-255: torch
 * autocast around model.decode).
 *   WN_PREC_F32  (default) fp32 operands, fp32 accumulation: the parity mode (identical
 *                greedy tokens, rescoring scores within 1e-3).  Large contractions run
 *                as six products of the operands' three exact bf16 planes on the bf16
 *                matrix cores (error against fp64 not above v_mfma_f32's:
 *                tests/test_gpu_x6.py); small ones, and everything under
 *                wn_tune_set("gemm_x6", 0), on v_mfma_f32_32x32x2_f32;
 *   WN_PREC_BF16 every Linear / pointwise-conv / subsampling-conv contraction
 *                rounds its two operands to bf16 (round to nearest even) and
 *                accumulates in fp32; the attention products likewise; LayerNorm,
 *                softmax, the depthwise conv and the searches stay fp32
 *                (autocast additionally rounds every result to bf16, so this
 *                mode is at least as precise as the reference's).  Tensors that
 *                only feed such a contraction may be KEPT as bf16 in HBM -- same
 *                values, the contraction rounds them first thing.
 *   WN_PREC_FP8  WN_PREC_BF16, and the two GEMMs of every encoder feed-forward module
 *                (w_1, w_2, positionwise_feed_forward.py:50-58) on OCP MXFP8 operands:
 *                e4m3 elements with one power-of-two (E8M0) scale per 32 consecutive
 *                k, for activations (quantised by the LayerNorm / by the w_1
 *                epilogue) and weights (quantised once here), multiplied on the
 *                block-scaled fp8 matrix cores with fp32 accumulation -- BASELINE.json
 *                configs[4] "MFMA fp8 FFN".  Shapes too small to fill the chip with
 *                256 x 256 tiles stay on the bf16 kernels.
 * Applies to later calls on this handle; clones inherit it.  The feature
 * frontends (wn_fbank, wn_log_mel, wn_resample) always run in fp32. */
#define WN_PREC_F32 0
#define WN_PREC_BF16 1
#define WN_PREC_FP8 2
int wn_model_set_precision(wn_model* m, int32_t precision);
int32_t wn_model_get_precision(const wn_model* m);

/* Number of utterances of the handle's CURRENT batch (what the last wn_encode /
 * wn_set_encoder_out / wn_set_ctc_probs installed; 0 before any, -1 for a null handle): the
 * per-utterance output arrays of the searches and of wn_rescore are sized by it.  No
 * reference counterpart -- the reference reads encoder_out.size(0) (search.py:385). */
int32_t wn_batch_size(const wn_model* m);

/* One-shot: the NEXT wn_encode on this handle waits for `event` (a hipEvent_t already
 * recorded by the caller, e.g. "the previous batch's encoder is finished" on another handle's
 * stream) INSIDE the call instead of the caller waiting in front of it -- behind the call's own
 * descriptor uploads and in front of GlobalCMVN + subsampling conv1 (the default, tune
 * enc_gate_pos = 0: the small host -> device copies of batch i+1 no longer stand in the chain of
 * encoders), or behind CMVN + conv1 (enc_gate_pos = 1: cmvn.py:36-47, subsampling.py:188-189,
 * the encoder's one HBM-bound kernel, then runs beside batch i's matrix-bound layers).  Used by
 * wenet_amd/pipeline.py; whatever way the call ends, the gate does not stay on the handle.
 * No reference counterpart (the reference decodes one batch at a time, recognize.py:289). */
int wn_model_set_encode_gate(wn_model* m, void* event);

/* A weight-less handle that only owns a workspace: enough for
 * wn_set_ctc_probs + the two CTC searches, i.e. for calling the reference's
 * free functions search.ctc_greedy_search / ctc_prefix_beam_search on a
 * caller-provided (B, T, V) log-prob tensor. */
int wn_workspace_create(int32_t device, wn_model** out);

/* ---- features ---------------------------------------------------------- */
/* processor.resample (dataset/processor.py:177-196): torchaudio's
 * Resample(orig_freq, new_freq) with its defaults -- polyphase windowed sinc
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), output length
 * ceil(new * n_in / orig) = wn_resample_length().  pcm_dev (n_in) -> out_dev
 * (n_out) float, both on the device; equal rates copy. */
int64_t wn_resample_length(int64_t n_in, int32_t orig_freq, int32_t new_freq);
int wn_resample(wn_model* m, const float* pcm_dev, int64_t n_in, int32_t orig_freq,
                int32_t new_freq, float* out_dev, int64_t n_out, void* stream);

/* compute_fbank (wenet/dataset/processor.py:226-256 -> kaldi.fbank with
 * num_mel_bins, 25 ms / 10 ms, dither 0, povey window; arithmetic restated
 * from runtime/core/frontend/fbank.h:250-327) + padding
 * (processor.py:526-577, without the sort).  pcm_dev holds the B waveforms
 * back to back, float in [-1, 1]; sample_off_host has B+1 entries.
 * feats_dev is (B, max_frames, feat_dim), zero padded.
 * n_frames_host receives 1 + (n - 400) / 160 per utterance. */
int wn_fbank(wn_model* m, const float* pcm_dev, const int64_t* sample_off_host,
             int32_t B, float* feats_dev, int32_t max_frames,
             int32_t* n_frames_host, void* stream);

/* compute_log_mel_spectrogram (wenet/dataset/processor.py:320-369, the Whisper
 * frontend): hann(400) STFT with hop 160 and reflect padding, power of all
 * frames but the last, slaney mel filters (librosa.filters.mel), log10 with
 * clamp 1e-10, floor at (utterance max - 8), (x + 4) / 4.  Same buffer
 * conventions as wn_fbank; n_frames = n_samples / 160; every utterance needs
 * more than 200 samples.  `padding` / `pad_or_trim` are applied by the caller
 * to the waveform. */
int wn_log_mel(wn_model* m, const float* pcm_dev, const int64_t* sample_off_host,
               int32_t B, int32_t n_mels, float* feats_dev, int32_t max_frames,
               int32_t* n_frames_host, void* stream);

/* ---- encoder ------------------------------------------------------------ */
/* ASRModel._forward_encoder / BaseEncoder.forward (asr_model.py:216-239,
 * encoder.py:122-181): GlobalCMVN, Conv2dSubsampling4, rel-pos encoding,
 * chunk mask, n_layers x ConformerEncoderLayer, after_norm.
 * feats_dev: (B, T, feat_dim) padded; feat_lens_host: B lengths.
 * decoding_chunk_size / num_left_chunks as in the reference (<0: full).
 * enc_lens_host (B) receives the subsampled lengths.  If enc_out_dev != NULL
 * it receives the padded (B, T', d_model) output, T' = ((T-1)/2-1)/2, rows
 * past each length zero-filled (the reference leaves unspecified values
 * there).  The packed encoder output stays resident in the model's workspace
 * as the "current batch" for the wn_ctc_* / wn_rescore calls below. */
int wn_encode(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host,
              int32_t B, int32_t T, int32_t decoding_chunk_size,
              int32_t num_left_chunks, float* enc_out_dev,
              int32_t* enc_lens_host, void* stream);

/* Streaming: BaseEncoder.forward_chunk (encoder.py:204-285) ==
 * ASRModel.forward_encoder_chunk (asr_model.py:385-427), batch 1, Conformer.
 *   feats_dev         (time, feat_dim) feature window of this chunk,
 *                     time = (chunk - 1) * 4 + 7 (shorter for the last chunk)
 *   offset            encoder frames emitted so far
 *   required_cache_size  < 0: keep all history; 0: none; > 0: that many frames
 *   att_cache_dev     (n_layers, heads, cache_t1, 128) K|V cache, NULL iff
 *                     cache_t1 == 0 (the reference's (0,0,0,0) tensor)
 *   cnn_cache_dev     (n_layers, 1, d_model, lorder) causal-conv left context,
 *                     NULL for the first chunk (zeros); lorder = cnn_kernel - 1
 *                     for causal models, 0 otherwise (no cnn cache at all)
 * Outputs: out_dev (chunk, d_model), chunk = ((time-1)/2-1)/2;
 * new_att_cache_dev (n_layers, heads, new_t1, 128) with
 *   new_t1 = cache_t1 + chunk - next_cache_start (encoder.py:258-263);
 * new_cnn_cache_dev like cnn_cache_dev.  The new caches must not alias the
 * inputs.  *chunk_out / *new_cache_t1_out (host, optional) return the two
 * sizes.  Nothing is synchronised; the handle's "current batch" is cleared. */
int wn_encode_chunk(wn_model* m, const float* feats_dev, int32_t time, int32_t offset,
                    int32_t required_cache_size, const float* att_cache_dev,
                    int32_t cache_t1, const float* cnn_cache_dev, float* out_dev,
                    float* new_att_cache_dev, float* new_cnn_cache_dev,
                    int32_t* chunk_out, int32_t* new_cache_t1_out, void* stream);

/* The same for n_sess streaming sessions in ONE call (the reference's
 * batched formulation is wenet/bin/export_onnx_gpu.py:83-232): feats_dev (n_sess, time,
 * feat_dim) -- every session contributes a window of the same length --, offsets_host /
 * cache_t1_host [n_sess] (sessions may be at different positions and hold caches of
 * different lengths), att_cache_dev / cnn_cache_dev / new_*_dev: host arrays of n_sess
 * device pointers, each tensor in the per-session layout above (entry NULL where that
 * session has none).  out_dev (n_sess, chunk, d_model); new_cache_t1_out [n_sess].
 * Every GEMM / LayerNorm runs on the n_sess * chunk rows at once; session b's attention
 * reads only its own [cache | chunk] keys at positions offset_b - cache_t1_b ... */
int wn_encode_chunk_batch(wn_model* m, int32_t n_sess, const float* feats_dev, int32_t time,
                          const int32_t* offsets_host, int32_t required_cache_size,
                          const float* const* att_cache_dev, const int32_t* cache_t1_host,
                          const float* const* cnn_cache_dev, float* out_dev,
                          float* const* new_att_cache_dev, float* const* new_cnn_cache_dev,
                          int32_t* chunk_out, int32_t* new_cache_t1_out, void* stream);

/* Use caller-provided padded encoder output (B, Tp, d_model) + lengths as the
 * current batch (for the reference's free functions that take encoder_out). */
int wn_set_encoder_out(wn_model* m, const float* enc_out_dev,
                       const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                       void* stream);

/* ---- CTC ---------------------------------------------------------------- */
/* ASRModel.ctc_logprobs (asr_model.py:254-265): Linear(d->V) + log_softmax
 * over the current batch, with top-k per frame (k = max(1, beam)) kept in the
 * workspace for the searches.  If logp_dev != NULL the full padded
 * (B, Tp, V) log-prob tensor is also written (rows past the length zeroed). */
int wn_ctc_logprobs(wn_model* m, int32_t topk, int32_t blank_id,
                    float blank_penalty, float* logp_dev, int32_t Tp,
                    void* stream);

/* Use caller-provided padded log-probs (B, Tp, V) + lengths as the current
 * CTC posteriors (for search.ctc_greedy_search / ctc_prefix_beam_search called
 * directly on a tensor); computes the per-frame top-k without re-normalising. */
int wn_set_ctc_probs(wn_model* m, const float* logp_dev,
                     const int32_t* lens_host, int32_t B, int32_t Tp,
                     int32_t V, int32_t topk, void* stream);

/* ctc_greedy_search (search.py:109-124): tokens_host is (B, max_len) int32,
 * tok_lens_host (B). max_len must be >= the longest subsampled length. */
int wn_ctc_greedy_search(wn_model* m, int32_t blank_id, int32_t* tokens_host,
                         int32_t* tok_lens_host, int32_t max_len, void* stream);

/* CTC forced alignment (ctc_utils.py:106 force_align, bin/alignment.py) of the CURRENT batch
 * (after wn_encode / wn_set_encoder_out) against given label lists: the CTC head, an emission
 * gather fused into the log-softmax row pass (the (B, T', V) log-probs are never written) and a
 * Viterbi trellis with its backtrace, one wave per utterance (DESIGN.md section 3 states the
 * rule: fp32, ties to stay, then step, then skip; the last label ends the path unless the
 * trailing blank is strictly better).  labels_host (B, max_label) int32, label_lens_host (B).
 * logp_dev != NULL: caller-provided NORMALISED log-probs (B, Tp, V) with lens_host (B) are
 * aligned INSTEAD of the current batch (works on a wn_workspace_create handle; the current
 * batch and its posteriors stay as they are); otherwise logp_dev / lens_host are NULL and B, Tp
 * must be the current batch's, V is ignored, blank_penalty as in wn_ctc_logprobs.
 * Outputs, host, each may be NULL except status_host: path_host (B, Tp) int32 label per frame;
 * score_host (B) float, the path's log-probability; status_host (B) 0 = ok, 1 = infeasible
 * (T' < labels + adjacent repeats; nothing else is written for that utterance);
 * frame_logp_host (B, Tp, 2) float: at frame t the log-prob of blank and of the label of the
 * token group t belongs to, i.e. the next label at or behind t on the path (what
 * bin/alignment.py get_frames_timestamp reads; trailing blank frames: blank twice);
 * emit_host (B, Tp, max_label + 1) float: column 0 blank, column 1 + i label i, zeros behind an
 * utterance's own labels.  Entries past an utterance's length are left untouched.  Label ids
 * outside [0, V), label_len > max_label or blank_id among the labels fail with -1 before
 * anything touches the device. */
int wn_ctc_force_align(wn_model* m, int32_t blank_id, float blank_penalty,
                       const int32_t* labels_host, const int32_t* label_lens_host,
                       int32_t max_label, const float* logp_dev, const int32_t* lens_host,
                       int32_t B, int32_t Tp, int32_t V, int32_t* path_host, float* score_host,
                       int32_t* status_host, float* frame_logp_host, float* emit_host,
                       void* stream);

/* Context biasing: install (n_nodes > 0) or clear (n_nodes == 0) a flattened
 * ContextGraph (wenet/utils/context_graph.py:101-265) on this handle; later
 * wn_ctc_prefix_beam_search calls are biased by it exactly like
 * ctc_prefix_beam_search(..., context_graph) (search.py:127-249): per-entry trie
 * state and bonus taken from the first contribution, second prune on
 * score + bonus, finalize() at the end.  All arrays are HOST arrays, copied.
 * Node 0 is the root (fail[0] = 0); `fail`, `node_score`, `output_score`,
 * `token_score` have n_nodes entries (ContextState.fail.id / node_score /
 * output_score / token_score); the trie arcs (ContextState.next) are the n_edges
 * triples edge_from[i] --edge_token[i]--> edge_to[i]. */
int wn_set_context_graph(wn_model* m, int32_t n_nodes, const int32_t* fail,
                         const double* node_score, const double* output_score,
                         const double* token_score, int32_t n_edges,
                         const int32_t* edge_from, const int32_t* edge_token,
                         const int32_t* edge_to, void* stream);

/* ctc_prefix_beam_search (search.py:127-249; context_graph = the graph set with
 * wn_set_context_graph, None by default).  Outputs,
 * all host: n_hyps (B); hyp_lens, hyp_tlens (B, beam); hyp_tokens, hyp_times
 * (B, beam, max_len); hyp_scores (B, beam) fp64.  beam <= 64 (<= 16 runs the
 * latency-tuned kernel).  Of every (max_len) row of hyp_tokens / hyp_times only the
 * first hyp_lens / hyp_tlens entries are written (one device -> pinned-host copy, then the
 * used corners): elements past a hypothesis' length keep what the caller put there.  The
 * n-best list also stays on the device for wn_attention_rescoring. */
int wn_ctc_prefix_beam_search(wn_model* m, int32_t beam, int32_t blank_id,
                              int32_t* n_hyps_host, int32_t* hyp_lens_host,
                              int32_t* hyp_tlens_host, int32_t* hyp_tokens_host,
                              int32_t* hyp_times_host, double* hyp_scores_host,
                              int32_t max_len, void* stream);

/* ---- streaming sessions: resumable CTC prefix beam search ------------------ */
/* The search half of the streaming decoder (runtime/core/decoder/ctc_prefix_beam_search.cc:
 * Search() keeps cur_hyps_ and abs_time_step_ across calls; asr_decoder.cc:87-132
 * AdvanceDecoding feeds it chunk by chunk) with the Python search's order rules
 * (search.py:127-249): a set of `n_slots` independent sessions whose beam, prefix / time
 * node pools, frame counter and endpoint counters live in HBM between calls.  Every call
 * names the sessions it touches by slot id; calls on one set must be ordered (one stream, or
 * events between streams).  A set belongs to the handle it was created on and must be
 * destroyed before it. */
typedef struct wn_stream_set wn_stream_set;

/* Where wn_stream_advance* put their results (all HOST arrays, the layout of
 * wn_ctc_prefix_beam_search with B = the n sessions of the call, in call order): n_hyps (n);
 * hyp_lens, hyp_tlens (n, beam); hyp_tokens, hyp_times (n, beam, max_len), of each row the
 * first hyp_lens / hyp_tlens entries written; hyp_scores = score(), hyp_viterbi =
 * viterbi_score() (n, beam) fp64; frames_decoded, trailing_blank (n): CtcEndpoint's
 * num_frames_decoded_ / num_frames_trailing_blank_ (ctc_endpoint.cc:48-60).  max_len must be
 * >= the frames any named session has consumed after the call.  hyp_viterbi may be NULL. */
typedef struct wn_stream_result {
  int32_t* n_hyps;
  int32_t* hyp_lens;
  int32_t* hyp_tlens;
  int32_t* hyp_tokens;
  int32_t* hyp_times;
  double* hyp_scores;
  double* hyp_viterbi;
  int32_t* frames_decoded;
  int32_t* trailing_blank;
  int32_t max_len;
} wn_stream_result;

/* Allocate the state of n_slots sessions, once: beam 1..16 (17..64 are the one-shot search's
 * range and are refused here), at most max_frames encoder frames per session (the node pools
 * hold max_frames * beam + 1 nodes each).  Every slot starts reset.  The handle may be a
 * weight-less workspace (wn_workspace_create) when only wn_stream_advance is used. */
int wn_stream_create(wn_model* m, int32_t n_slots, int32_t beam, int32_t max_frames,
                     int32_t blank_id, wn_stream_set** out, void* stream);
int wn_stream_destroy(wn_stream_set* set);

/* CtcEndpointConfig's blank_threshold / blank_scale (ctc_endpoint.h:27-54; defaults 0.8, 1.0):
 * a frame counts as trailing blank when expf(logp[blank]) > blank_threshold * blank_scale. */
int wn_stream_set_endpoint(wn_stream_set* set, float blank_threshold, float blank_scale);

/* Back to the root prefix (search.py:144-150), frame and endpoint counters to zero
 * (CtcPrefixBeamSearch::Reset, CtcEndpoint::Reset) for the n sessions in slot_ids (host). */
int wn_stream_reset(wn_stream_set* set, int32_t n, const int32_t* slot_ids, void* stream);

/* CtcPrefixBeamSearch::Search on the next frames of n sessions: logp_dev is (n, Tp, V)
 * log-probs on the device, session i consumes its first n_t_host[i] rows (0 <= n_t <= Tp; 0
 * leaves the session's state bit for bit).  Per-frame top-k as wn_set_ctc_probs, then the
 * resumable search; the result is each session's hypothesis list over everything it has
 * consumed so far -- exactly what wn_ctc_prefix_beam_search returns for those frames in one
 * call.  nbest == 0: only the 1-best of each session is walked out (n_hyps <= 1);
 * nbest != 0: the whole beam.  A call that would take a session past max_frames, or whose
 * max_len is too small, fails with -1 and changes no session.  A handle with a context graph
 * installed is refused: finalize() of the graph mutates the beam (search.py:229-234), which
 * a partial result must not do. */
int wn_stream_advance(wn_stream_set* set, int32_t n, const int32_t* slot_ids,
                      const float* logp_dev, const int32_t* n_t_host, int32_t Tp, int32_t V,
                      int32_t nbest, const wn_stream_result* out, void* stream);

/* The same on the encoder output of wn_encode_chunk_batch: enc_out_dev is (n, chunk, d_model)
 * on the device; the CTC head (Linear + log_softmax + top-k, as wn_ctc_logprobs) runs here, so
 * a streaming step is encoder chunk -> CTC head -> search without a host round trip between. */
int wn_stream_advance_encoded(wn_stream_set* set, int32_t n, const int32_t* slot_ids,
                              const float* enc_out_dev, const int32_t* n_t_host, int32_t chunk,
                              int32_t nbest, const wn_stream_result* out, void* stream);

/* ---- attention rescoring ------------------------------------------------- */
/* attention_rescoring + ASRModel.forward_attention_decoder
 * (search.py:374-458, asr_model.py:453-547) for ALL utterances and hypotheses
 * of the current batch in one pass (the reference loops utterance by
 * utterance).  hyps given on the host as produced by the prefix beam search:
 * n_hyps (B), hyp_lens (B, beam), hyp_tokens (B, beam, max_len).
 * Outputs (host): l2r_logp, r2l_logp (B, beam, max_len + 1): log-prob of each
 * hypothesis token then of <eos> under the left-to-right decoder, and of the
 * reversed sequence under the right-to-left decoder (zeros when
 * reverse_weight == 0 or the model has no right decoder). */
int wn_attention_rescoring(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
                           const int32_t* hyp_lens_host,
                           const int32_t* hyp_tokens_host, int32_t max_len,
                           float reverse_weight, float* l2r_logp_host,
                           float* r2l_logp_host, void* stream);

/* Optional, in front of wn_ctc_prefix_beam_search when wn_rescore follows on the same batch: the
 * part of attention_rescoring that does not depend on the hypotheses -- the cross-attention K / V
 * projections of the encoder output for every decoder layer (decoder_layer.py:123-138; the
 * reference recomputes them per utterance inside forward_attention_decoder) -- is queued on a
 * second stream of the handle, ordered behind `stream`'s work so far, and overlaps the search
 * (T' dependent steps on B workgroups while most CUs idle).  wn_rescore waits for it and skips
 * those projections; results are the same bits.  use_right_decoder: also for the right-to-left
 * decoder (reverse_weight > 0).  A new batch or layout (wn_encode, wn_set_encoder_out,
 * wn_filter_blank_embedding) voids the prefetch. */
int wn_rescore_prefetch(wn_model* m, int32_t use_right_decoder, void* stream);

/* attention_rescoring COMPLETE on the device (search.py:374-458; SURVEY.md 8b `wn_rescore`):
 * the decoder pass of wn_attention_rescoring, then one kernel does what search.py:424-457 does
 * in Python -- per hypothesis the fp32 left-to-right sum of the gathered log-probs + <eos>
 * (in the reference's order and dtypes), the right-to-left decoder's sum blended with
 * reverse_weight, `confidence = exp(score / (len + 1))`, `+ ctc_score * ctc_weight`, the
 * first-maximum arg-max over the hypotheses, and the winner's per-token confidences
 * (batched form in the reference: wenet/bin/export_onnx_gpu.py:666-724).
 *   n_hyps_host == NULL: the n-best is the one the LAST wn_ctc_prefix_beam_search of this
 *     handle left on the device (tokens and fp64 scores are read there; no host round trip);
 *     hyp_lens_host / hyp_tokens_host / ctc_scores_host must be NULL, beam / max_len the
 *     values that search was called with.
 *   otherwise: n_hyps (B), hyp_lens (B, beam), hyp_tokens (B, beam, max_len), ctc_scores
 *     (B, beam) host arrays (DecodeResult.nbest / nbest_scores of any source).
 * Outputs (host): best_idx (B) index into the utterance's n-best, best_score (B) fp32 (the
 * `.item()` of the reference's fp32 tensor), confidence (B) fp64, tok_conf (B, max_len) fp64
 * (first len(best hyp) entries), all_scores (B, beam) fp32 score of every hypothesis.
 * confidence / tok_conf / all_scores may be NULL.  beam <= 64. */
int wn_rescore(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
               const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
               const double* ctc_scores_host, int32_t max_len, double ctc_weight,
               double reverse_weight, int32_t* best_idx_host, float* best_score_host,
               double* confidence_host, double* tok_conf_host, float* all_scores_host,
               void* stream);

/* The decoder half of ASRModel.forward_attention_decoder (asr_model.py:453-547):
 * one decoder (`which` 0: decoder / left_decoder, 1: right_decoder,
 * decoder.py:146-201,430-463) over a PADDED batch of n_seq token rows for
 * utterance `utt` of the current batch -> log_softmax over the vocabulary of
 * every position, logp_dev (n_seq, max_len, vocab) on the device.  tokens_host
 * (n_seq, max_len) are the decoder inputs ([sos] + hyp, eos-padded); lens_host
 * the input lengths: keys past a row's length are masked, padded rows are
 * computed like the reference computes them. */
int wn_decoder_forward(wn_model* m, int32_t utt, int32_t which, int32_t n_seq,
                       const int32_t* tokens_host, const int32_t* lens_host,
                       int32_t max_len, float* logp_dev, void* stream);

/* ASRModel.filter_blank_embedding (asr_model.py:153-180), used by decode() in front of
 * attention_rescoring when model_conf.apply_non_blank_embedding is set (asr_model.py:337-342;
 * examples/aishell/s0/conf/train_u2++_lite_conformer.yaml): the encoder output of the CURRENT
 * batch is replaced by its rows whose CTC arg-max (of the posteriors wn_ctc_logprobs /
 * wn_set_ctc_probs left on the handle, blank penalty included) is not token 0, in order;
 * T = the largest number of kept rows in the batch; utterance b then has min(len_b, T) rows: its
 * kept rows followed by ZERO rows -- the reference hands attention_rescoring the zero-padded
 * (B, T, d) tensor together with the UNFILTERED lengths (search.py:396), so the decoder
 * attends to that padding too, and so does this path.  n_keep_host (B,): kept rows per
 * utterance; *t_out = T; padded_out_dev (optional, (B, T', d) or larger): the reference's
 * return tensor (B, T, d).  Only frames inside an utterance's length are considered (the
 * reference also looks at the padded frames of shorter utterances, whose encoder output is an
 * artefact of the padding; a batch of equal lengths or a single utterance is identical, and so
 * is a ragged batch none of whose padded frames comes out non-blank: tests/golden/
 * raggedlite_tiny.npz from the real reference, 1e-3.  Where padded frames ARE selected the
 * rescoring scores differ -- T and with it the number of zero rows every utterance carries
 * changes too: measured 0.10 on the random-weight case tests/golden/raggedlite_tiny_padded.npz,
 * same winners; tolerance 0.15 stated in tests/test_gpu_parity.py).  T == 0 (no non-blank frame
 * in the whole batch; the reference raises): nothing is changed, *t_out = 0, a warning is
 * printed once.  One host round trip (the kept-row counts). */
int wn_filter_blank_embedding(wn_model* m, float* padded_out_dev, int32_t* n_keep_host,
                              int32_t* t_out, void* stream);

/* attention_beam_search (search.py:252-371, the non-Whisper branch) over the CURRENT batch
 * (its encoder output is on the device after wn_encode / wn_set_encoder_out): B x beam
 * running hypotheses, one decoder row per hypothesis and step
 * (TransformerDecoder.forward_one_step, decoder.py:226-281, with a self-attention K/V
 * cache and the cross-attention K/V projected once), mask_finished_scores / _preds, the
 * N x N -> N re-ranking, the end flags and the final length-penalised arg-max all run on
 * the device; scores are fp32 like the reference's.  maxlen = the reference's
 * encoder_out.size(1).  tokens_host is (B, maxlen) int32 (the winner without <sos> /
 * <eos>), lens_host (B,).  beam <= 64.  The cache holds the steps actually run (it starts
 * at 32 steps and doubles), and the "all hypotheses ended" counter is read back every 4th
 * step: steps past the end only append <eos> to finished hypotheses, which the result strips. */
int wn_attention_beam_search(wn_model* m, int32_t beam, int32_t maxlen, float length_penalty,
                             int32_t* tokens_host, int32_t* lens_host, void* stream);

/* attention_beam_search, the Whisper branch (search.py:267-289): every hypothesis starts from
 * the P-token prompt of its utterance (add_whisper_tokens, common.py:159-238), prompt_host
 * (B, P) int32.  Prefill: the P prompt rows of each utterance go through the decoder ONCE per
 * utterance (causal self attention); their K | V land in cache steps 0..P-1 at the utterance's
 * first slot and every hypothesis' ancestor path points there.  Steps then run for
 * i = P .. min(maxlen, dec_max_pos): where the reference asserts in its positional table (a
 * hypothesis still open at position dec_max_pos) this path stops and returns the best hypothesis
 * so far; wn_attention_truncated() then reads 1.  Results are stripped of the prompt and of
 * <eot>; the length penalty counts the non-<eot> tokens of the whole row, prompt included.  The
 * cross attention runs one query sequence of `beam` rows per utterance (K / V rows staged once
 * per utterance).  With the tune key dec_skinny != 0 the step's GEMMs run on the skinny kernel
 * (gemm_skinny.hip); wn_attention_beam_search never does.  tokens_host (B, maxlen), lens_host
 * (B,).  P == 1 with prompt = <sos> is the classic search. */
int wn_attention_beam_search_prompt(wn_model* m, int32_t beam, int32_t maxlen,
                                    float length_penalty, const int32_t* prompt_host, int32_t P,
                                    int32_t* tokens_host, int32_t* lens_host, void* stream);
/* 1 if the handle's last wn_attention_beam_search_prompt stopped at the positional table with
 * a hypothesis still open, else 0 (-1: null handle). */
int32_t wn_attention_truncated(const wn_model* m);

/* One step of attention_beam_search (search.py:252-371): for every running
 * hypothesis (its utterance index in the current batch, its tokens so far
 * starting with <sos>), log_softmax(output_layer(after_norm(decoder(...)[:, -1])))
 * -- TransformerDecoder.forward_one_step, decoder.py:226-281 -- reduced to its
 * `topk` best (log-prob, token) pairs, sorted.  The cross-attention K/V of the
 * current batch are projected once and kept for the following steps; the self
 * attention is recomputed over the prefix (no self-attention cache).
 * tokens_host is (n_seq, max_len) int32; outputs are (n_seq, topk), host. */
int wn_decoder_next_topk(wn_model* m, int32_t n_seq, const int32_t* seq_utt_host,
                         const int32_t* seq_lens_host, const int32_t* tokens_host,
                         int32_t max_len, int32_t topk, float* logp_host,
                         int32_t* idx_host, void* stream);

/* ---- raw operators (used by the parity tests and by other hosts) ---------- */
/* C[M,N] = resid + alpha * act(A[M,K] * W[N,K]^T + bias); act: 0 none,
 * 1 SiLU, 2 ReLU.  fp32 on v_mfma_f32_32x32x2_f32. */
int wn_op_gemm(const float* A_dev, const float* W_dev, const float* bias_dev,
               const float* resid_dev, float* C_dev, int32_t M, int32_t N,
               int32_t K, float alpha, int32_t act, void* stream);
/* The same contraction with both operands rounded to bf16 (WN_PREC_BF16). */
int wn_op_gemm_bf16(const float* A_dev, const float* W_dev, const float* bias_dev,
                    const float* resid_dev, float* C_dev, int32_t M, int32_t N,
                    int32_t K, float alpha, int32_t act, void* stream);
/* The whole argument block of the fp32 / bf16-on-the-fly GEMM (csrc/gemm.hip, gemm_bf16.hip) as
 * the model's launchers fill it: strides, the GLU epilogue, gathered rows and the implicit
 * 3x3 / stride-2 operand (test infrastructure).  Everything is checked on the host BEFORE
 * anything is launched, so that no accepted call reads outside A's a_elems floats or writes
 * outside [0, M) x [0, N) (N / 2 with glu) of C.  a_row_off is a HOST array of M entries (or
 * NULL: plain rows of stride lda); element (row, k) of the operand then lives at
 * A[a_row_off[row] + (tap / 3) * conv_sy + (tap % 3) * conv_sx + k % conv_C], tap = k / conv_C,
 * with K == 9 * conv_C (3x3 taps) or K == conv_C (gathered rows). */
typedef struct wn_gemm_op {
  const float* A; const float* W; const float* bias; const float* resid; float* C;
  int32_t M, N, K;
  int32_t lda, ldc, ldr;
  float alpha;
  int32_t act;         /* 0 none, 1 SiLU, 2 ReLU, 3 exact GELU */
  int32_t glu;         /* W rows as [32 values | 32 gates] per 64; C has N / 2 columns */
  int32_t precision;   /* WN_PREC_F32 / WN_PREC_BF16 for this call */
  const int64_t* a_row_off;
  int64_t a_elems;     /* floats in the A buffer */
  int32_t conv_C;
  int64_t conv_sy, conv_sx;
} wn_gemm_op;
/* Calls gemm_f32 directly (never the six-product path).  *route_out = the kernel instantiation
 * that ran: BM/64 | BN/64 << 4 | WGM << 8 | WGN << 12 | (K tile / 32) << 16 | PF << 20 |
 * GLU << 22 | CONV << 23 | precision << 24 | act << 25 | resid << 27. */
int wn_op_gemm_ex(const wn_gemm_op* op, int32_t* route_out, void* stream);
/* The skinny GEMM of the decoder step (gemm_skinny.hip), M <= 256 (more is refused, -1):
 * C[M,N] = resid + act(A[M,K] * W[N,K]^T + bias), act 0 none / 2 ReLU / 3 exact GELU; a block
 * owns all M rows of 128 columns and one of split_k K slices (0 = the shape rule), the slice
 * partials are summed in slice order (no atomics: repeatable bits).  w_bf16 != 0: W is rounded
 * to a bf16 image first (the handle's weight image in the model path), A is rounded to bf16 on
 * its way into LDS, fp32 accumulate.  K % 32 == 0. */
int wn_op_gemm_skinny(const float* A_dev, const float* W_dev, const float* bias_dev,
                      const float* resid_dev, float* C_dev, int32_t M, int32_t N, int32_t K,
                      int32_t act, int32_t w_bf16, int32_t split_k, void* stream);
/* The bf16-STORAGE form of that contraction (the kernel the bf16 mode runs on
 * LayerNorm outputs / FFN hidden / attention context, which it keeps as bf16 in
 * HBM): A and W are rounded to bf16 images first, the GEMM reads those; C is fp32
 * (M, N) or, with c_bf16 != 0 and no residual, a bf16 (M, N) matrix. */
int wn_op_gemm_bf16_stored(const float* A_dev, const float* W_dev, const float* bias_dev,
                           const float* resid_dev, void* C_dev, int32_t M, int32_t N,
                           int32_t K, float alpha, int32_t act, int32_t c_bf16,
                           void* stream);
/* The reduced-precision GEMM kernels on operands that are ALREADY in their storage
 * type in HBM (what the model path hands them): dtype 1 = bf16 A (M, K) and W (N, K);
 * dtype 2 = OCP MXFP8: e4m3 A and W with one E8M0 block scale per 32 consecutive k of a
 * row, scales as dwords [K/128][pitch = M resp. N] (the 4 bytes of a dword = the 4 k
 * blocks of one 128-wide K tile), exactly what wn_op_mx_quantize writes.  c_mode 0: fp32
 * C (M, N); 1: bf16 C (bf16 operands, no residual); 2: MXFP8 C (MXFP8 operands, no
 * residual) with its block scales [N/128][M] in c_scale_dev.  Micro-benchmarks and the
 * operator tests call this. */
int wn_op_gemm_lowp(const void* A_dev, const void* W_dev, const void* a_scale_dev,
                    const void* w_scale_dev, const float* bias_dev,
                    const float* resid_dev, void* C_dev, void* c_scale_dev, int32_t M,
                    int32_t N, int32_t K, float alpha, int32_t act, int32_t c_mode,
                    int32_t dtype, void* stream);
/* x (rows, K) fp32 -> MXFP8: q (rows, K) e4m3 bytes + scale dwords [K/128][rows]
 * (block rule: the smallest power of two 2^e with amax <= 448 * 2^e; csrc/mxfp8.h). */
int wn_op_mx_quantize(const float* x_dev, int32_t rows, int32_t K, void* q_dev,
                      void* scale_dev, void* stream);
/* The whole argument block of the stored-operand GEMMs (csrc/gemm_bf16s.hip, gemm_bf16p.hip) as
 * the model's launchers fill it (test infrastructure).  Operands arrive in their storage type,
 * as with wn_op_gemm_lowp; nothing is converted.  dtype 1: bf16 A (M, lda) and W (N, K); dtype 2:
 * MXFP8, e4m3 A (M, lda) and W (N, K) with scale dwords [K/128][a_scale_pitch] /
 * [K/128][w_scale_pitch].  c_mode 0: fp32 C (M, ldc); 1: bf16 C (bf16 operands); 2: MXFP8 C
 * (MXFP8 operands) with its scale dwords [ceil(N/128)][c_scale_pitch].  lda / ldc are in
 * elements of A / C, ldr in floats.  glu (bf16 operands, fp32 C): W rows as [32 values |
 * 32 gates] per 64, C has N / 2 columns.  Every argument the kernels assume is checked on the
 * host BEFORE anything is launched, each with its own message: 16-byte aligned A, W, C, bias
 * and residual, lda % 8 (bf16) / % 16 (MXFP8), ldc % 4 / 8 / 16 by C mode, ldr % 4, lda >= K,
 * ldc and ldr not smaller than the output row, pitches not smaller than the rows, the byte sizes
 * of the buffers, no residual with a bf16 or MXFP8 C, K % 32 (bf16) or K % 128, K >= 256,
 * N % 8 (N % 32 with an MXFP8 C) for MXFP8. */
typedef struct wn_gemm_lowp_op {
  const void* A; const void* W; const float* bias; const float* resid; void* C;
  const void* a_scale; const void* w_scale; void* c_scale;
  int32_t M, N, K;
  int32_t lda, ldc, ldr;
  int32_t a_scale_pitch, w_scale_pitch, c_scale_pitch;
  float alpha;
  int32_t act;         /* 0 none, 1 SiLU, 2 ReLU, 3 GELU */
  int32_t glu;
  int32_t dtype;       /* 1 bf16, 2 MXFP8 */
  int32_t c_mode;      /* 0 fp32, 1 bf16, 2 MXFP8 */
  int64_t a_bytes, w_bytes;                               /* bytes in the A / W buffers */
  int64_t a_scale_bytes, w_scale_bytes, c_scale_bytes;    /* and in the scale arrays */
} wn_gemm_lowp_op;
/* Calls gemm_bf16_stored / gemm_mxfp8 directly.  *route_out = the kernel instantiation that ran:
 * the fields of wn_op_gemm_ex | MXFP8 elements << 19 | kernel family << 28 (1 gemm_bf16s_kernel,
 * 2 gemm_lp_kernel) | c_mode << 30 (the K tile field is 3 bits; PF is 2 for gemm_bf16s_kernel). */
int wn_op_gemm_lowp_ex(const wn_gemm_lowp_op* op, int32_t* route_out, void* stream);
/* wn_op_mx_quantize with every argument of the quantiser: x (rows, ld) fp32, ld % 4 == 0,
 * ld >= K, K % 32 == 0; q (rows, K) e4m3 bytes; scale dwords [ceil(K/128)][pitch], pitch >= rows
 * (of the last dword of a row only the bytes of blocks < K / 32 are written). */
int wn_op_mx_quantize_ex(const float* x_dev, int32_t ld, int32_t rows, int32_t K, void* q_dev,
                         void* scale_dev, int32_t pitch, void* stream);
/* The fused fp32 feed-forward module the encoder runs (csrc/ffn_fused.hip;
 * positionwise_feed_forward.py:50-58 inside encoder_layer.py:220-228): x_inout (M, D) +=
 * alpha * (act(X W1^T + b1) W2^T + b2) with X (M, D) the already normalised input, then
 * y_out = LayerNorm(x_inout; ln_w, ln_b, eps).  D in {256, 512}, F % 64 == 0, act 1 SiLU /
 * 2 ReLU / 3 GELU.  Operator tests and micro-benchmarks call this. */
int wn_op_ffn_fused(const float* X_dev, const float* W1_dev, const float* b1_dev,
                    const float* W2_dev, const float* b2_dev, float* x_inout_dev,
                    const float* ln_w_dev, const float* ln_b_dev, float* y_out_dev,
                    int32_t M, int32_t D, int32_t F, int32_t act, float alpha, float eps,
                    void* stream);
/* fp32 GEMM on the bf16 matrix cores (csrc/gemm_x6.hip): every fp32 operand is split
 * exactly into three bf16 planes and six of the nine plane products are accumulated in
 * fp32 (the dropped ones are below 2^-26 of a product).  C (M, N) = resid + alpha *
 * act(A W^T + bias); A (M, K), W (N, K) fp32 row-major, K % 16 == 0, N % 4 == 0.  `bm`:
 * block rows 128 / 256 (0 = auto); `reps` > 1 repeats the GEMM launch (micro-benchmarks).
 * Replaces torch.nn.functional.linear as the reference's layers call it
 * (positionwise_feed_forward.py:50-58, attention.py:100-176, convolution.py:120-148). */
int wn_op_gemm_x6(const float* A_dev, const float* W_dev, const float* bias_dev,
                  const float* resid_dev, float* C_dev, int32_t M, int32_t N, int32_t K,
                  float alpha, int32_t act, int32_t bm, int32_t reps, void* stream);
/* wn_op_ffn_fused's contract with both contractions as six bf16 plane products: by default
 * (d_model 256, SiLU / ReLU) ONE launch of csrc/ffn_x6f.hip with the hidden tensor in
 * registers; wn_tune_set("ffn_x6f", 0) or any other shape: two launches of the six-product
 * GEMM, the hidden tensor going from the first one's epilogue to the second as a plane image. */
int wn_op_ffn_x6(const float* X_dev, const float* W1_dev, const float* b1_dev,
                 const float* W2_dev, const float* b2_dev, float* x_inout_dev,
                 const float* ln_w_dev, const float* ln_b_dev, float* y_out_dev, int32_t M,
                 int32_t D, int32_t F, int32_t act, float alpha, float eps, int32_t reps,
                 void* stream);
/* Row-block six-product GEMM with the A rows in registers (csrc/gemm_x6r.hip), K = 256:
 * epi 0: C (M, N) = A W^T + bias, N in {256, 512, 768} (the QKV projection,
 * attention.py:109-131); epi 1 (N = 256): x <- x + alpha (A W^T + bias), y <- LayerNorm(x; ln_w,
 * ln_b, eps) -- the attention output projection / pointwise_conv2 with the residual and the
 * LayerNorm that follows (encoder_layer.py:238-240, 251-253).  `reps` launches (micro-benchmark;
 * epi 1 then accumulates into x every time). */
int wn_op_gemm_x6r(const float* A_dev, const float* W_dev, const float* bias_dev,
                   float* x_inout_dev, const float* ln_w_dev, const float* ln_b_dev,
                   float* y_dev, float* C_dev, int32_t M, int32_t N, int32_t epi, float alpha,
                   float eps, int32_t reps, void* stream);

/* The d_model = 512 row-block kernels (csrc/gemm_x6r512.hip), test / benchmark entry: K = 512;
 * epi 0: C (M, N) = A W^T + bias, N in {512, 1024, 1536, 2048}; epi 1: x_inout += alpha (A W^T +
 * bias), y = LayerNorm(x_inout), N = 512; epi 3: epi 1, then C (M, 512) = GLU(y W2^T + bias2)
 * with W2 (1024, 512) in the [32 values | 32 gates]-per-64 row order wn_model_create gives
 * pointwise_conv1 (y is written only if non-null). */
int wn_op_gemm_x6r512(const float* A, const float* W, const float* bias, float* x_inout,
                      const float* ln_w, const float* ln_b, float* y, const float* W2,
                      const float* bias2, float* C, int32_t M, int32_t N, int32_t epi, float alpha,
                      float eps, int32_t reps, void* stream);
/* out[i] = log_add(a[i], b[i]) (wenet/utils/common.py:302-310) in fp64 with the
 * routine the prefix beam search uses. */
int wn_op_log_add(const double* a_dev, const double* b_dev, double* out_dev,
                  int32_t n, void* stream);
int wn_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev,
                    float* y_dev, int32_t M, int32_t D, float eps, void* stream);

/* Operator hooks of the four kernel families that are not GEMMs (test infrastructure: the
 * arguments of the library's own launchers, checked on the host BEFORE anything is launched, so
 * that no accepted call can read or write outside the caller's buffers).  Offsets and lengths
 * are HOST arrays; everything else is a device pointer. */
typedef struct wn_attention_op {
  const void* Q; const void* K; const void* V;   /* fp32 [rows][ld*]; d_k = 64 per head */
  int32_t ldq, ldk, ldv;
  int32_t q_rows, kv_rows;                        /* rows of the Q / O and of the K / V buffers */
  const float* P; int32_t ldp, p_rows;            /* projected position table or NULL */
  const int32_t* p_off;                           /* host [n_seq] or NULL */
  const float* bias_u; const float* bias_v;       /* [n_heads][64], with P */
  void* O; int32_t ldo;                           /* fp32, or bf16 with WN_ATTN_O_BF16 */
  const int32_t* q_off; const int32_t* q_len;     /* host [n_seq]; ascending, disjoint */
  const int32_t* kv_off; const int32_t* kv_len;   /* host [n_seq]; equal to q_*: self attention */
  int32_t n_seq, n_heads;
  int32_t mask_mode, chunk_size, left_chunks;     /* 0 keys < kv_len, 1 causal, 2 chunk window */
  float scale;
  int32_t flags;       /* WN_ATTN_* */
  int32_t precision;   /* WN_PREC_F32 / WN_PREC_BF16 for this call */
  int32_t x6_galign;   /* six-product form: key tiles on the global 32-row blocks */
} wn_attention_op;
#define WN_ATTN_FOLD 1       /* rel-pos term folded inside the kernel (AttnArgs::fold) */
#define WN_ATTN_PREFOLD 2    /* ... by the separate pass (relpos_fold -> kbias); d = 256 / 512 */
#define WN_ATTN_QKV_BF16 4   /* precision 1: Q, K, V converted to bf16 matrices first (dense ld) */
#define WN_ATTN_O_BF16 8     /* precision 1: O is a bf16 matrix, ldo in elements */
/* *form_out = the kernel form the dispatch chose: kind | key_split << 4 | waves << 8 |
 * relpos << 12 | bf16_inputs << 13 | key_bias << 14; kind: 0 plain, 1 rel-pos (two contractions),
 * 2 rel-pos folded in the kernel, 3 six-product, 4 bf16 register-staged, 5 bf16 LDS-DMA. */
int wn_op_attention(const wn_attention_op* op, int32_t* form_out, void* stream);
/* Depthwise conv over time + LayerNorm (norm_mode 0) / affine (1) + SiLU over packed rows:
 * x [M][ldx], wt [K][D], y [M][ldy]; off / len host [B]; rows no utterance owns are skipped. */
int wn_op_dwconv(const float* x, int32_t ldx, const float* wt, const float* bias,
                 const float* cpad, const float* ln_w, const float* ln_b, int32_t norm_mode,
                 float* y, int32_t ldy, const int32_t* off, const int32_t* len, int32_t B,
                 int32_t M, int32_t D, int32_t K, int32_t causal, int32_t t_max, float eps,
                 void* stream);
/* GlobalCMVN (mean NULL: none) + Conv2d(1, C, 3, stride 2) + ReLU: feats (B, T, F), w [9][C],
 * out [out_rows][(F - 1) / 2][C]; t1_off / t1_len host [B].  plane_image != 0: through the
 * plane-image form of the six-product conv2 and back to the same layout. */
int wn_op_conv1(const float* feats, const float* mean, const float* istd, const float* w,
                const float* bias, float* out, const int32_t* t1_off, const int32_t* t1_len,
                int32_t B, int32_t T, int32_t F, int32_t C, int32_t out_rows,
                int32_t plane_image, void* stream);
/* Self attention WITH the relative shift (FireRedASR's FiredRelPositionMultiHeadedAttention, the
 * Transformer-XL form; csrc/firered.hip), fp32, d_k = 64, full context:
 *   score(i, j) = ((q_i + u) . k_j + (q_i + v) . p_{i-j}) * scale, softmax over the sequence's keys.
 * Q / K / V / O [rows][ld*]; off / len host [n_seq] (ascending, disjoint).  P [p_rows][ldp] holds
 * the projected position row of DISTANCE r = i - j in row p_center - r (the row order of the
 * reference's pos_emb); every |r| < max(len) must lie inside the table. */
int wn_op_attention_relshift(const float* Q, const float* K, const float* V, int32_t ldq,
                             int32_t ldk, int32_t ldv, int32_t rows, const float* P,
                             int32_t ldp, int32_t p_rows, int32_t p_center, const float* bias_u,
                             const float* bias_v, float* O, int32_t ldo, const int32_t* off,
                             const int32_t* len, int32_t n_seq, int32_t n_heads, float scale,
                             void* stream);
/* The FireRedASR front end up to the output projection (FireRedConv2dSubsampling4): GlobalCMVN
 * (mean NULL: none), six zero frames behind every utterance's own last frame, Conv2d(1, C, 3, 2)
 * + ReLU, Conv2d(C, C, 3, 2) + ReLU.  feats (B, T, F); w1 [9][C] and w2 [9][C_in][C_out]
 * tap-major; out [out_rows][ldo] with utterance b's frames from row out_off[b] (host [B]),
 * column c * F2 + f2.  out_len (host [B], written) = ((len + 6 - 3) / 2 + 1 - 3) / 2 + 1, 0 for
 * an empty utterance. */
int wn_op_firered_frontend(const float* feats, const float* mean, const float* istd,
                           const float* w1, const float* b1, const float* w2, const float* b2,
                           float* out, int32_t ldo, int32_t out_rows, const int32_t* lens,
                           const int32_t* out_off, int32_t* out_len, int32_t B, int32_t T,
                           int32_t F, int32_t C, void* stream);
/* The middle of a Branchformer cgMLP (ConvolutionalSpatialGatingUnit, csrc/branchformer.hip),
 * fp32, on packed rows: h [rows][ldh] holds r in columns [0, C) and the gate half in [C, 2 C);
 *   y = (depthwise_conv_K(LayerNorm_C(gate half)) + bias) * r       (gate == 0: without "* r")
 * with ln_w / ln_b [C] (eps 1e-5), wt [K][C] tap-major, bias [C], y [rows][ldy].  Utterance i is
 * rows off[i] .. off[i] + len[i] - 1 (host [n_seq], ascending, disjoint); frames outside it are
 * the conv's padding, never a neighbour's rows: K - 1 frames in front when causal, each entering
 * the conv as ln_b (the reference pads in front of the norm), else (K - 1) / 2 zero frames on
 * both sides.  C a multiple of 64 up to 1024; K in [1, 63], odd unless causal. */
int wn_op_csgu_gate(const float* h, int32_t ldh, int32_t rows, int32_t C, const float* ln_w,
                    const float* ln_b, const float* wt, const float* bias, int32_t K,
                    int32_t causal, int32_t gate, float* y, int32_t ldy, const int32_t* off,
                    const int32_t* len, int32_t n_seq, void* stream);
/* The E-Branchformer merge in front of merge_proj: y = c + depthwise_conv_K(c) + bias over the C
 * (= 2 d_model) channels of c [rows][ldc], zero padding (K - 1 in front when causal, else
 * symmetric), the same packed layout; y must not alias c. */
int wn_op_merge_dwconv(const float* c, int32_t ldc, int32_t rows, int32_t C, const float* wt,
                       const float* bias, int32_t K, int32_t causal, float* y, int32_t ldy,
                       const int32_t* off, const int32_t* len, int32_t n_seq, void* stream);
/* Output frames one workgroup of those two kernels owns (lengths around it are the edge cases). */
int32_t wn_csgu_time_tile(void);
/* Self attention with the Squeezeformer's wrapped shift (csrc/squeezeformer.hip; the reference's
 * rel_shift on a T x T score matrix, squeezeformer/attention.py:75-99), full context, d_k = 64,
 * fp32, one launch for all sequences.  Sequence i is rows off[i] .. off[i] + len[i] - 1 of Q / K /
 * V / O (host [n_seq], ascending, disjoint, inside `rows`); with T = len[i]
 *   score(a, b) = ((q_a + u) . k_b + S(a, b)) * scale
 *   S(a, b) = (q_a + v) . p[T - 1 - (a - b)]   for b <= a
 *           = 0                                for b == a + 1
 *           = (q_{a+1} + v) . p[b - a - 2]     for b >= a + 2
 * P [p_rows][ldp]: linear_pos of the first p_rows position rows, p_rows >= the longest len (rows
 * >= T of a shorter sequence are not read).  Strides in floats, multiples of 4, >= n_heads * 64. */
int wn_op_attention_sqshift(const float* Q, const float* K, const float* V, int32_t ldq,
                            int32_t ldk, int32_t ldv, int32_t rows, const float* P, int32_t ldp,
                            int32_t p_rows, const float* bias_u, const float* bias_v, float* O,
                            int32_t ldo, const int32_t* off, const int32_t* len, int32_t n_seq,
                            int32_t n_heads, float scale, void* stream);
/* The depthwise conv of a Squeezeformer time reduction: x [rows][ldx] packed full-rate rows
 * (utterance i: off[i], len[i]) -> y [out_rows][ldy] packed half-rate rows (utterance i:
 * out_off[i], (len[i] + 1) / 2 rows, inside out_rows, disjoint),
 *   y[t][c] = bias[c] + sum_k wt[k][c] * x[2 t - pad + k][c],   wt [K][C] tap-major,
 * frames outside the utterance's own [0, len) being zeros.  K = 5 with pad = 3, or K = 1 with
 * pad = 0.  C a multiple of 64; y must not overlap x. */
int wn_op_time_reduce(const float* x, int32_t ldx, int32_t rows, int32_t C, const float* wt,
                      const float* bias, int32_t K, int32_t pad, float* y, int32_t ldy,
                      int32_t out_rows, const int32_t* off, const int32_t* len,
                      const int32_t* out_off, int32_t n_seq, void* stream);
/* Time recovery: y[off[i] + t] = skip[off[i] + t] + z[z_off[i] + t / 2] for t < len[i]; skip / y
 * [rows][lds / ldy] full-rate, z [z_rows][ldz] half-rate ((len[i] + 1) / 2 rows from z_off[i]).
 * y may be skip; z must not overlap y. */
int wn_op_time_recover(const float* skip, int32_t lds, const float* z, int32_t ldz, int32_t z_rows,
                       float* y, int32_t ldy, int32_t rows, int32_t C, const int32_t* off,
                       const int32_t* len, const int32_t* z_off, int32_t n_seq, void* stream);

/* ---- Efficient Conformer kernels (wenet/models/efficient_conformer/; csrc/efficonformer.hip),
 * fp32, test hooks.  Offsets and lengths are HOST arrays (ascending, disjoint). */
/* Grouped self attention (GroupedRelPositionMultiHeadedAttention.pad4group / forward,
 * efficient_conformer/attention.py:83-126, 180-258), one launch for all sequences, head width
 * W = group * d_k of 96 or 192 (other widths are refused).  Q / K / V / O [rows][ld*] and P
 * [p_rows][ldp] are packed (frames, D) matrices, D = n_heads * width / group; sequence i is frames
 * off[i] .. off[i] + len[i] - 1 (of P: p_off[i] .. , p_off may be null: 0).  Head h of group row
 * r is flat elements [h W, (h + 1) W) of frames group r .. group r + group - 1: element e is
 * frame group r + e / D, column e % D.  Frames >= len[i] read as zeros in all four operands and
 * are not written.  bias_u / bias_v [n_heads][W].
 *   score(r, s) = ((q_r + u) . k_s + (q_r + v) . p_s) * scale  over all ceil(len / group) key rows
 * chunk_size > 0 (0: full context): with m = mask_step, query row r sees key row s iff
 *   m s < ((m r) / chunk_size + 1) * chunk_size, and for left_chunks >= 0 also
 *   m s >= ((m r) / chunk_size - left_chunks) * chunk_size   (mask[:, ::m, ::m] of
 * subsequent_chunk_mask, utils/mask.py).  Strides in floats, multiples of 4, >= D. */
int wn_op_attention_grouped(const float* Q, const float* K, const float* V, int32_t ldq,
                            int32_t ldk, int32_t ldv, int32_t rows, const float* P, int32_t ldp,
                            int32_t p_rows, const int32_t* p_off, const float* bias_u,
                            const float* bias_v, float* O, int32_t ldo, const int32_t* off,
                            const int32_t* len, int32_t n_seq, int32_t n_heads, int32_t group,
                            int32_t width, int32_t mask_step, int32_t chunk_size,
                            int32_t left_chunks, float scale, void* stream);
/* The depthwise conv of a StrideConv module with its norm and swish (ConvolutionModule.forward,
 * efficient_conformer/convolution.py:64-72, 141-146): x [rows][ldx] packed rows at the incoming
 * rate (utterance i: off[i], len[i]) -> y [out_rows][ldy] packed rows at ceil(len[i] / stride)
 * from out_off[i],
 *   c[t][ch] = bias[ch] + sum_k wt[k][ch] * x[stride t - pad + k][ch],  wt [K][D] tap-major,
 *   pad = (K - 1) / 2, or K - 1 with causal; y = SiLU(norm(c)), norm_mode 0: LayerNorm over the
 * channels (ln_w, ln_b, eps), 1: c * ln_w + ln_b.  Frames >= len[i] are zeros; frames < 0 are
 * zeros, or the vector cpad [D] when causal and cpad is not null (the module pads in front of
 * pointwise_conv1, convolution.py:117-119).  stride 2 only, K <= 63, D a multiple of 64 <= 512. */
int wn_op_stride_dwconv_ln_silu(const float* x, int32_t ldx, int32_t rows, int32_t D,
                                const float* wt, const float* bias, const float* cpad,
                                const float* ln_w, const float* ln_b, int32_t norm_mode,
                                float eps, int32_t K, int32_t causal, int32_t stride, float* y,
                                int32_t ldy, int32_t out_rows, const int32_t* off,
                                const int32_t* len, const int32_t* out_off, int32_t n_seq,
                                void* stream);
/* The stride layer's residual (StrideConformerEncoderLayer.forward, efficient_conformer/
 * encoder_layer.py:138-148: AvgPool1d(stride, stride, ceil_mode=True, count_include_pad=False)):
 *   y[out_off[i] + t] = z[out_off[i] + t] + mean(x[off[i] + 2 t .. min(2 t + 2, len[i]) - 1]),
 * t < ceil(len[i] / 2); z / y [out_rows][ldz / ldy], y may be z.  stride 2 only. */
int wn_op_avgpool_residual_add(const float* x, int32_t ldx, int32_t rows, const float* z,
                               int32_t ldz, float* y, int32_t ldy, int32_t out_rows, int32_t C,
                               int32_t stride, const int32_t* off, const int32_t* len,
                               const int32_t* out_off, int32_t n_seq, void* stream);

/* ---- Paraformer kernels (wenet/models/paraformer/; csrc/attention_d128.hip, paraformer.hip),
 * fp32, test hooks.  Offsets and lengths are HOST arrays (ascending, disjoint), everything else a
 * device pointer unless it is named *_host; every argument is checked before the first launch. */
/* Attention for heads of d_k = 128 (n_heads * 128 columns per row), full context, no position
 * term: O = softmax((Q K^T) * scale) V per (sequence, head).  Q / O and K / V have separate
 * layouts: self attention passes the same offsets twice, the decoder's cross attention passes
 * tokens and frames.  d_k = 64 stays with wn_op_attention. */
int wn_op_attention_d128(const float* Q, const float* K, const float* V, int32_t ldq,
                         int32_t ldk, int32_t ldv, int32_t q_rows, int32_t kv_rows, float* O,
                         int32_t ldo, const int32_t* q_off, const int32_t* q_len,
                         const int32_t* kv_off, const int32_t* kv_len, int32_t n_seq,
                         int32_t n_heads, float scale, void* stream);
/* Attention for heads of d_k = 32 (n_heads * 32 columns per row; csrc/attention_d32.hip): the
 * decoders of 8 heads at d_model 256.  The arguments of wn_op_attention_d128 plus mask_mode:
 * 0 = every key < kv_len (cross attention), 1 = causal, key j <= query i AND j < kv_len (kv_len
 * < q_len is the padded batch of wn_decoder_forward: keys at or past kv_len are hidden from every
 * query).  No position term, no kbias, no chunk window (mask_mode 2 is refused by name).  fp32
 * whatever the handles' compute type. */
int wn_op_attention_d32(const float* Q, const float* K, const float* V, int32_t ldq,
                        int32_t ldk, int32_t ldv, int32_t q_rows, int32_t kv_rows, float* O,
                        int32_t ldo, const int32_t* q_off, const int32_t* q_len,
                        const int32_t* kv_off, const int32_t* kv_len, int32_t n_seq,
                        int32_t n_heads, float scale, int32_t mask_mode, void* stream);
/* The LFR front end of every utterance ALONE (paraformer/layers.py:24-92): utterance b of
 * lens[b] frames gives out_len[b] = ceil(lens[b] / n) rows from row out_off[b]; row t stacks the
 * m frames n t - (m - 1) / 2 + f (each index clamped to [0, lens[b] - 1]), then GlobalCMVN over
 * the m F columns (mean NULL: none), x * xscale + pe[t + 1] (pe [pe_rows][m F]) and
 * LayerNorm(m F; ln_w, ln_b, eps).  Rows are ldo wide, m F <= ldo <= 576, zeros behind m F. */
int wn_op_lfr_front(const float* feats, const float* mean, const float* istd, const float* pe,
                    int32_t pe_rows, const float* ln_w, const float* ln_b, float* out,
                    int32_t ldo, int32_t out_rows, const int32_t* lens, const int32_t* out_off,
                    int32_t* out_len, int32_t B, int32_t T, int32_t F, int32_t m, int32_t n,
                    float xscale, float eps, void* stream);
/* LayerNorm over D <= 2048 columns (a multiple of 4; the statistics divide by D) of x [M][ldx];
 * columns D .. Dpad - 1 of y [M][ldy] are written as zeros. */
int wn_op_layernorm_wide(const float* x, int32_t ldx, const float* w, const float* b, float* y,
                         int32_t ldy, int32_t M, int32_t D, int32_t Dpad, float eps,
                         void* stream);
/* The CIF weights (paraformer/cif.py:64-78, cnn_groups 1, residual false) on packed rows h
 * [rows][ldh]: alpha[r] = relu(sigmoid(out_w . relu(conv1d_3(h)_r + conv_b) + out_b) * smooth -
 * noise) for every owned row, the conv's zero padding at each utterance's OWN ends.  conv_w is
 * [d][3 d] with column tap * d + c_in (tap 0 = the frame before); d a multiple of 32. */
int wn_op_cif_alpha(const float* h, int32_t ldh, int32_t rows, int32_t d, const float* conv_w,
                    const float* conv_b, const float* out_w, const float* out_b, float smooth,
                    float noise, float* alpha, const int32_t* off, const int32_t* len,
                    int32_t n_seq, void* stream);
/* The integrate-and-fire scan (paraformer/cif.py:110-142, 250-293) over len[i] + 1 frames of
 * utterance i: its alphas (device, [rows], each in [0, 1]: checked), then the tail frame (alpha =
 * tail, a zero hidden row).  threshold must be 1.0.  Embedding k of utterance i goes to emb row
 * emb_off[i] + k (k < emb_cap[i]) and its frame to fire_t_host[emb_off[i] + k]; n_fire_host[i]
 * counts the fires, token_num_host[i] = floor(sum of the alphas); rows n_fire .. token_num - 1 are
 * zeros with frame -1.  Entries of fire_t_host no embedding owns are -1. */
int wn_op_cif_fire(const float* h, int32_t ldh, int32_t rows, int32_t d, const float* alpha,
                   const int32_t* off, const int32_t* len, int32_t n_seq, float threshold,
                   float tail, float* emb, int32_t lde, int32_t emb_rows, const int32_t* emb_off,
                   const int32_t* emb_cap, int32_t* fire_t_host, int32_t* n_fire_host,
                   int32_t* token_num_host, void* stream);
/* The Conformer front end alone -- GlobalCMVN + Conv2dSubsampling4 + the sqrt(d) scale, what
 * wn_encode runs in front of layer 0 (at position 0), under the handle's precision and tuning
 * set -- and copies of what it left, each optional (NULL), DEVICE arrays, complete on return:
 *   c1 [sum t1_len][F1][d]  the conv1 activations conv2 read (t1_len = 2 l2 + 1 per utterance
 *                           with l2 > 0; the plane-image form is unpacked to fp32 first)
 *   c2 [M][F2][d]           conv2 + ReLU, M = sum l2
 *   x  [M][d]               the packed rows layer 0 reads
 * enc_lens_host [B] (or NULL) = l2.  *route_out = what ran, 0 if M == 0, else
 *   1 << 16 | linear_x6 << 13 | projection << 12 | slices << 8 | tile << 4 | kind
 *   kind        0 conv2 as the gathered-row v_mfma_f32 GEMM, 1 six-product with the fp32 gather,
 *               2 six-product gathering from conv1's plane image
 *   tile        (kinds 1, 2) 0 one launch of 128-row tiles, 1 one launch of 256-row tiles,
 *               2 256-row tiles + the remainder as 128-row tiles, 3 256-row tiles + the
 *               remainder as `slices` K slices
 *   projection  1 K slices + ffn_reduce_ln (with layer 0's first LayerNorm), 0 linear();
 *               linear_x6: that linear() went through the split pass + six-product GEMM
 * Refuses Conv1dSubsampling2 handles, T < 7 and lengths outside [0, T]. */
int wn_op_conv2d4(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host,
                  int32_t B, int32_t T, float* c1, float* c2, float* x,
                  int32_t* enc_lens_host, int32_t* route_out, void* stream);
/* CTC head tail: blank penalty, log-softmax, top-k (logp NULL: the top-k only). */
int wn_op_ctc_rows(const float* logits, int32_t ld, int32_t M, int32_t V, int32_t k,
                   int32_t blank, float blank_penalty, float* topk_val, int32_t* topk_idx,
                   float* logp, int32_t ld_out, void* stream);

/* Operator hooks of the `attention` decode mode's kernels (test infrastructure): each checks its
 * arguments and calls the launcher the search itself calls.  Every array is a DEVICE array except
 * n_done_host.  Index arrays a kernel dereferences (the path rows, last_tok of the embedding) are
 * read back and range-checked before the launch; the other arrays are only copied or clamped.
 * Layouts: qkv [n][3d] (Q | K | V), cache [steps][n][2d] (K | V), path / tok rows of max_len
 * ints, d = heads * 64 (attn_self_step: or heads * 32, the decoders of 8 heads at 256).
 *   attn_self_step   stores K | V of qkv into cache[step], then row r attends over positions
 *                    0..step, position j read from cache[j][path[r][j]]; out [n][d]
 *   attn_step_embed  x[r] = emb[last_tok[r]] * scale + pe[pos]; emb [V][d], pe [max_pos][d]
 *   attn_prompt_cache  K | V of prefill row b * P + j -> cache[j][b * N]; cache [P][B * N][2d]
 *   beam_init        the start state; prompt (B, P) or NULL (every row starts as sos)
 *   beam_update      one pruning step on parents of `step` tokens (1 <= step,
 *                    step + 1 <= max_len); *n_done_host = number of children that ended.  A NaN
 *                    candidate score ranks as -inf
 *   beam_finish      length penalty, first maximum, the winner without its first `prefix` tokens
 *                    and without eos into out_tok [B][max_len] / out_len [B] */
int wn_op_attn_self_step(const float* qkv_dev, int32_t d, int32_t heads, int32_t n,
                         float* cache_dev, int32_t step, const int32_t* path_dev,
                         int32_t max_len, float* out_dev, void* stream);
int wn_op_attn_step_embed(const int32_t* last_tok_dev, int32_t pos, const float* emb_dev,
                          int32_t V, const float* pe_dev, int32_t max_pos, float scale, int32_t d,
                          int32_t n, float* x_dev, void* stream);
int wn_op_attn_prompt_cache(const float* qkv_dev, int32_t d, int32_t B, int32_t P, int32_t N,
                            float* cache_dev, void* stream);
int wn_op_beam_init(int32_t B, int32_t N, int32_t max_len, int32_t sos, const int32_t* prompt_dev,
                    int32_t P, float* score_dev, int32_t* end_dev, int32_t* tok_dev,
                    int32_t* path_dev, int32_t* last_tok_dev, void* stream);
int wn_op_beam_update(int32_t B, int32_t N, int32_t step, int32_t max_len, int32_t eos,
                      int32_t V, const float* topv_dev, const int32_t* topi_dev,
                      const float* score_in, const int32_t* end_in, const int32_t* tok_in,
                      const int32_t* path_in, float* score_out, int32_t* end_out,
                      int32_t* tok_out, int32_t* path_out, int32_t* last_tok_dev,
                      int32_t shared_row, int32_t* n_done_host, void* stream);
int wn_op_beam_finish(int32_t B, int32_t N, int32_t len, int32_t max_len, int32_t eos,
                      float length_penalty, const float* score_dev, const int32_t* tok_dev,
                      int32_t* out_tok_dev, int32_t* out_len_dev, int32_t prefix, void* stream);

/* Operator hooks of the kernels that own a complete row (test infrastructure): thin wrappers of
 * the launchers the encoder calls, every argument checked on the host BEFORE anything is launched
 * (null pointers, M > 0, a width the launcher has a case for, row strides >= the width and
 * multiples of 4 elements, pitch >= M, S >= 1, mode in 0..2), so that no accepted call reads or
 * writes outside the caller's buffers.  Every array is a DEVICE array; eps sits inside the square
 * root (torch.nn.LayerNorm).
 *   layernorm_ex    y = LN(x; w, b); x (M, ldx), y (M, ldy) fp32 or, y_bf16 != 0, bf16 (ldy in
 *                   bf16 elements); y may be x.  D in {64, 128, 192, 256, 384, 512, 640, 768, 1024,
 *                   1280}
 *   layernorm2      y1 = LN(x; w1, b1), y2 = LN(y1; w2, b2) (fp32 or bf16) on dense (M, D) rows;
 *                   y1 may be x.  D in {64, 128, 256, 512, 768, 1024, 1280}
 *   layernorm_mx    LN(x) as MXFP8: q (M, D) e4m3 bytes, scale dwords [D/128][pitch] (byte
 *                   (c >> 5) & 3 of dword [c >> 7][row] for column c).  D in {256, ..., 1280} step 256
 *   ffn_reduce_ln   x_new = x + alpha (sum_s P[s] + b2), P [S][M][D], D in {256, 512}.  mode 0:
 *                   x <- x_new, y = LN(x_new; w, b); mode 1: x <- LN(x_new; w, b), y = LN(x; w2,
 *                   bb2); mode 2: x <- LN(x_new; w, b) only (y unused).  y3 != NULL: mode 1 with y
 *                   leaving as its plane image (csrc/x6.h) in y3 instead, y3_bytes >= the image of
 *                   M rows rounded up to 32: (D / 16) * ceil(M / 32) * 3072
 *   gemm_rowln      x_out = resid + alpha (A W^T + bias), y = LN(x_out; ln_w, ln_b); W (256, K),
 *                   K % 32 == 0, K >= 96, lda >= K, ldr / ldx / ldy >= 256; bias / resid may be
 *                   NULL, resid may be x_out, y may be A.  Calls the kernel whatever the
 *                   `gemm_rowln` tune switch says */
int wn_op_layernorm_ex(const float* x, int32_t ldx, const float* w, const float* b, void* y,
                       int32_t ldy, int32_t M, int32_t D, float eps, int32_t y_bf16, void* stream);
int wn_op_layernorm2(const float* x, const float* w1, const float* b1, const float* w2,
                     const float* b2, float* y1, void* y2, int32_t M, int32_t D, float eps,
                     int32_t y2_bf16, void* stream);
int wn_op_layernorm_mx(const float* x, int32_t ldx, const float* w, const float* b, void* q,
                       void* scale, int32_t pitch, int32_t M, int32_t D, float eps, void* stream);
int wn_op_ffn_reduce_ln(float* x, const float* P, int32_t S, const float* b2, float alpha,
                        const float* w, const float* b, const float* w2, const float* bb2, float* y,
                        void* y3, int64_t y3_bytes, int32_t M, int32_t D, float eps, int32_t mode,
                        void* stream);
int wn_op_gemm_rowln(const float* A, int32_t lda, const float* W, const float* bias,
                     const float* resid, int32_t ldr, float alpha, float* x_out, int32_t ldx,
                     const float* ln_w, const float* ln_b, float eps, float* y, int32_t ldy,
                     int32_t M, int32_t K, void* stream);

/* Measurement hook for bench.py: bracket launches of the dominant kernel (the
 * FFN w_1 GEMM, positionwise_feed_forward.py:58; every 6th launch, because each
 * event pair idles the GPU for ~10 us) with HIP events on the launch stream.  wn_profile_collect waits for them and returns the number of
 * launches, their summed duration and their summed algorithmic FLOPs
 * (2*M*N*K each) since the last enable/collect.  on = 1: every 6th launch; on = N > 1: every
 * N-th (bench.py's timed rounds use one bracket per decode, its single-stream roofline pass 6). */
int wn_profile_enable(wn_model* m, int32_t on);
int wn_profile_collect(wn_model* m, int32_t* n_launches, double* total_ms,
                       double* total_flops);
/* What the bracketed launches were (static string): the FFN w_1 GEMM -- in the fp32 mode the
 * fused six-product kernel of csrc/ffn_x6f.hip (w_1 + activation + w_2, d_model 256) or the
 * six-product w_1 GEMM of csrc/gemm_x6.hip -- or the fused v_mfma_f32 feed-forward kernel when
 * wn_tune_set("gemm_x6", 0) puts the fp32 path on it. */
const char* wn_profile_kernel_name(const wn_model* m);
/* Hidden slices S (fused forms: partial sums [S][M][d] reduced by the next kernel) or K slices
 * of the w_2 GEMM of the feed-forward module this handle ran last -- what bench.py prices the
 * algorithmic bytes of the roofline kernel with (positionwise_feed_forward.py:50-58 has no such
 * notion: it is a property of the launch geometry). */
int32_t wn_profile_ffn_split(const wn_model* m);
/* Measurement: shader-clock stamps [4 waves][24] written by the clock-stamp variants of the fused
 * feed-forward kernel (wn_tune_set("ffn_x6f_var", 8704 ...), tools/bench_x6.py --clocks): entry
 * i = start of sub-stage i of one block's last steady-state chunk, entry 8 = its end. */
int wn_profile_ffn_clocks(uint64_t* out64);
/* Same for the six-product tile GEMM (wn_tune_set("x6_probe", 4)): [8 waves][8] = entry, loop
 * start, loop end, kernel end (shader clock), 100-MHz real time at entry / end, k blocks.  While
 * wn_tune_set("lp_probe", 4 [| 8 first block | 16 last block]) is set, the stamps of the pipelined
 * bf16 / MXFP8 GEMM instead: entry, first tile landed, K loop end, last store issued, stores
 * drained, real time at entry / end, K tiles (tools/lp_clocks.py).  With "x6_probe" = 8: the
 * five phase stamps block 0 of the last row-block GEMM launch (csrc/gemm_x6r.hip) left: entry,
 * rows in LDS, planes in LDS, main loop done, stores drained (tools/x6r_clocks.py). */
int wn_profile_gemm_clocks(uint64_t* out64);

/* Test hook: "n_layers" = run only the first n encoder layers (-1: all),
 * "skip_after_norm" = 1 leaves out encoder.after_norm; lets the parity tests
 * compare every ConformerEncoderLayer output with the oracle. */
int wn_debug_set(wn_model* m, const char* key, int32_t value);

/* Tuning knobs: A/B switches between kernel forms, measurement probes and test hooks.  The key
 * list, what every value selects and the defaults (= the shipped configuration) are ONE table,
 * WN_TUNE_KEYS in wenet_amd/csrc/tune.h; unknown keys are an error.  Values that are wrong by
 * design (ablations) are refused unless the library was built with WN_ABLATION=1.
 *
 * wn_tune_set writes the PROCESS DEFAULT: what handle-less operators (wn_op_*) and every handle
 * without an override of its own see (tools/bench_*.py, bench.py --tune, most tests).
 * wn_model_tune_set writes ONE HANDLE's override (INT32_MIN = drop the override, follow the process
 * default again); a handle's entry points run on its effective set, resolved when the call enters
 * and current only for the calling thread, so two handles driven by two host threads can run
 * different kernel forms side by side.  wn_model_clone copies the overrides.  wn_tune_get reads
 * the effective value for a handle (NULL: the process default).
 * No counterpart in the reference: its kernels are chosen by torch's dispatcher. */
int wn_tune_set(const char* key, int32_t value);
int wn_model_tune_set(wn_model* m, const char* key, int32_t value);
int wn_tune_get(const wn_model* m, const char* key, int32_t* value);

/* ---- hybrid transducer (csrc/transducer.hip, csrc/cabi_transducer.hip) -----------------------
 *
 * A hybrid transducer (wenet/models/transducer/transducer.py; init_model.py:137-160) is an
 * asr_model -- encoder, CTC head, attention decoder: wn_config -- plus an RNNPredictor (LSTM,
 * predictor.py:60-88) and a TransducerJoint (prejoin linears, 'add', tanh; joint.py:34-49). */
typedef struct {
  int32_t pred_embed;        /* predictor_conf.embed_size, 1..1024 */
  int32_t pred_hidden;       /* predictor_conf.hidden_size, 1..1024 */
  int32_t pred_layers;       /* predictor_conf.num_layers, 1..8 */
  int32_t pred_out;          /* predictor_conf.output_size (= joint_conf.pred_output_size) */
  int32_t join_dim;          /* joint_conf.join_dim, a multiple of 32 up to 1024 */
  int32_t blank;             /* the transducer's blank id (init_model.py:146: 0) */
} wn_transducer_config;

/* wn_model_create for a `model: transducer` state dict: additionally ingests
 * predictor.{embed.weight, rnn.weight_ih_l*, rnn.weight_hh_l*, rnn.bias_ih_l*, rnn.bias_hh_l*,
 * projection.*} and joint.{enc_ffn, pred_ffn, ffn_out}.* into the shared model block (read-only
 * afterwards, shared by clones).  Every entry point of an asr_model handle works on the result.
 * The widths travel in a struct of their own and through an entry point of their own, NOT as
 * fields appended to wn_config: wn_config is passed by pointer without a size, so a caller
 * compiled against the shorter struct would have wn_model_create read past its end.  This way
 * wn_config and wn_model_create are unchanged, in layout and in behaviour, for every caller. */
int wn_model_create_transducer(const wn_config* cfg, const wn_transducer_config* tcfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out);

/* The reference's two stateless predictors (predictor.py:209-495): EmbeddingPredictor, a
 * multi-head, position-weighted mix of the last history_size + 1 token embeddings -> ffn ->
 * LayerNorm -> activation, and ConvPredictor, a depthwise conv over the same window -> LayerNorm
 * -> activation.  Like wn_transducer_config, a struct and an entry point of their own: nothing
 * an existing caller passes changes. */
typedef struct {
  int32_t kind;              /* 1 embedding, 2 conv */
  int32_t context;           /* predictor_conf.history_size + 1, 1..16 */
  int32_t heads;             /* predictor_conf.n_head, 1..16; conv: 1 */
  int32_t activation;        /* 0 swish, 1 relu */
  int32_t conv_bias;         /* conv only: predictor.conv.bias exists */
  float norm_eps;            /* predictor_conf.layer_norm_epsilon */
} wn_stateless_predictor_config;

/* wn_model_create_transducer for a stateless predictor: tcfg->pred_embed == tcfg->pred_out ==
 * embed_size (the reference asserts embed_size == output_size), tcfg->pred_layers == 0 and
 * tcfg->pred_hidden == 0.  Ingests predictor.{embed.weight, norm.*}, for an embedding predictor
 * predictor.{pos_embed.weight, ffn.*} (pos_embed.bias may be present and is not read: neither
 * forward nor forward_step of the reference reads it), for a conv predictor
 * predictor.conv.weight (and .bias with conv_bias), and joint.{enc_ffn, pred_ffn, ffn_out}.*.
 * Every transducer entry point works on the handle: a predictor advance is one launch of
 * rnnt_stateless_step (csrc/transducer_stateless.hip), whose window is the tail of the token row
 * the search keeps anyway, so such a handle has no h / c: the streaming state hooks write
 * nothing to their h / c arguments.  Results do not depend on the batch, the lookahead, the slot
 * or how a session's frames are split into calls, as for an LSTM handle. */
int wn_model_create_transducer_stateless(const wn_config* cfg, const wn_transducer_config* tcfg,
                                         const wn_stateless_predictor_config* scfg,
                                         const wn_tensor* weights, int32_t n_weights,
                                         int32_t device, wn_model** out);

/* FireRedASR-AED (`model: firered`, wenet/models/firered/): a Conformer-family encoder with the
 * 32-channel FireRedConv2dSubsampling4 front end, Transformer-XL relative-position attention WITH
 * the relative shift, three LayerNorms inside the attention (folded into the QKV weights on the
 * host, in fp64), a conv module at conv_inner_factor 4 (LayerNorm over 2 d_model channels), no
 * biases on linear_q/k/v/out and the convolutions, no after_norm.  Like wn_transducer_config, a
 * struct and an entry point of their own: wn_config and wn_model_create are unchanged. */
typedef struct {
  int32_t sub_channels;       /* FireRedConv2dSubsampling4 odim: 32 */
  int32_t conv_inner_factor;  /* encoder_conf.conv_inner_factor: 4 */
  int32_t max_frames;         /* cap on an utterance's encoder frames T': every layer keeps
                                 2 max_frames - 1 projected position rows */
  float attn_norm_eps;        /* eps of layer_norm_q / k / v: torch's default 1e-5 */
} wn_firered_config;

/* wn_model_create for a `model: firered` state dict (the names init_model gives it).  cfg:
 * encoder_type 0, input_layer 0, cnn_norm 0 (layer_norm), causal 0, no chunk sizes; the decoder
 * fields as for any left-to-right `transformer` decoder.  On the handle, wn_encode runs the
 * FireRed front end and layers -- every utterance as the reference encodes it ALONE: six zero
 * frames behind its own last frame, T' = ((len + 6 - 3) / 2 + 1 - 3) / 2 + 1, the padded output
 * has T' of the longest length T -- in fp32, full context only (chunk must be < 0); the CTC, the
 * `attention` search and the rescoring entry points then work on the encoder output unchanged.
 * wn_encode_chunk*, wn_stream_create, wn_op_conv2d4 and a bf16 / fp8 precision are refused on
 * such a handle. */
int wn_model_create_firered(const wn_config* cfg, const wn_firered_config* fcfg,
                            const wn_tensor* weights, int32_t n_weights, int32_t device,
                            wn_model** out);

/* Branchformer / E-Branchformer encoders (`encoder: branchformer` / `e_branchformer`,
 * wenet/models/branchformer/, wenet/models/e_branchformer/) under the asr_model head: the
 * Conformer front end and rel-pos attention, a convolutional gating MLP branch beside the
 * attention branch, the two merged by merge_proj over their concatenation (E-Branchformer: a
 * depthwise conv over the 2 d_model channels in front of it, and the macaron feed-forward
 * pair).  A struct and an entry point of their own: wn_config and wn_model_create are unchanged.
 * In wn_config, ffn_dim is the feed-forward width (kind 2; any multiple of 32 for kind 1) and
 * cnn_kernel is not read (1). */
typedef struct {
  int32_t kind;               /* 1 branchformer (merge_method concat), 2 e_branchformer */
  int32_t cgmlp_units;        /* cgmlp_linear_units U: U / 2 a multiple of 64 up to 1024 */
  int32_t cgmlp_kernel;       /* cgmlp_conv_kernel: 1..63, odd unless cfg.causal */
  int32_t merge_kernel;       /* merge_conv_kernel (kind 2): 1..63, odd unless cfg.causal */
  int32_t linear_after_conv;  /* use_linear_after_conv */
  int32_t head_dim;           /* d_model / n_heads: 64, or 32 (heads zero-padded to 64 columns) */
} wn_branchformer_config;

/* wn_model_create for such a state dict (the names init_model gives it; pooling_proj1/2 and
 * weight_proj1/2 of a Branchformer layer are not read).  On the handle, wn_encode runs the layer
 * stack in fp32 -- chunk / left set the attention mask only, as in the reference -- with every
 * utterance encoded as the reference encodes it ALONE: the cgMLP and merge convs see an
 * utterance's own frames, not the batch's padding or a neighbour.  The CTC, search, rescoring
 * and alignment entry points and wn_model_clone then work unchanged; wn_encode_chunk*,
 * wn_stream_create and a bf16 / fp8 precision are refused on such a handle. */
int wn_model_create_branchformer(const wn_config* cfg, const wn_branchformer_config* bcfg,
                                 const wn_tensor* weights, int32_t n_weights, int32_t device,
                                 wn_model** out);

/* ---- Paraformer (`model: paraformer`, wenet/models/paraformer/): SANM encoder behind the LFR
 * front end, CIF predictor, SANM decoder; fp32.  Of wn_config it reads feat_dim (80), d_model,
 * n_heads (d_model / n_heads in {64, 128}), ffn_dim, n_layers (encoder blocks, encoders0
 * included), vocab, has_cmvn (over lfr_m * feat_dim columns), dec_heads, dec_ffn_dim, norm_eps. */
typedef struct {
  int32_t lfr_m, lfr_n;        /* 7, 6 */
  int32_t kernel_size;         /* FSMN taps of encoder and decoder, odd (11) */
  int32_t dec_blocks;          /* decoder_conf.num_blocks == att_layer_num */
  int32_t max_frames;          /* encoder frames (LFR rows) a handle's position table covers */
  float threshold;             /* predictor_conf.threshold: must be 1.0 */
  float tail_threshold;        /* 0.45; in (0, 1) */
  float smooth_factor;         /* 1.0; in (0, 1] */
  float noise_threshold;       /* 0.0; >= 0 */
} wn_paraformer_config;
/* State dict names as init_model gives them; encoder.embed.pos_enc.pe is rebuilt here and the
 * timestamp branch (predictor.tp_*), `embed.weight` and the loss modules are accepted and not
 * read.  A CTC head (ctc.ctc_lo.*) is optional.  wn_encode on the handle runs the front end and
 * the encoder with every utterance encoded as the reference encodes it ALONE (T' = ceil(n / 6)
 * frames); wn_ctc_* and wn_ctc_force_align then work as on any handle.  No chunks, no streams,
 * no bf16 / fp8. */
int wn_model_create_paraformer(const wn_config* cfg, const wn_paraformer_config* pcfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out);
/* Predictor + decoder on the handle's CURRENT batch (the last wn_encode): HOST arrays tokens /
 * logp (B, max_tok), tok_lens (B).  tok_lens[b] = token_num = floor(sum alpha) of utterance b
 * (0: no token, nothing else written for it); tokens[b][i] = the arg-max of decoder row i, logp
 * its log-probability.  Optional (NULL): fire_frames (B, max_tok) the encoder frame every
 * embedding fired on (the tail frame is frame T'), n_fire (B).  max_tok (>= 1) is the row pitch
 * of these arrays and must hold the largest tok_lens: T' + 1 of the longest utterance always
 * suffices. */
int wn_paraformer_decode(wn_model* m, int32_t* tokens, int32_t* tok_lens, float* logp,
                         int32_t* fire_frames, int32_t* n_fire, int32_t max_tok, void* stream);

/* ---- SenseVoice Small (`model: sensevoice_small`, wenet/models/sensevoice/): four query rows
 * (language | event | emotion | text norm, rows of a 16 x 560 embedding table) in front of the LFR
 * rows of every utterance, the SANM encoder stack, after_norm, a second stack (tp_encoders) and
 * tp_norm, a CTC head; fp32.  Of wn_config it reads feat_dim (80), d_model, n_heads (d_model /
 * n_heads in {64, 128}), ffn_dim, n_layers (blocks of the first stack, encoders0 included),
 * vocab, has_cmvn (must be 1), norm_eps. */
typedef struct {
  int32_t lfr_m, lfr_n;        /* 7, 6 */
  int32_t kernel_size;         /* FSMN taps of both stacks, odd (11) */
  int32_t tp_blocks;           /* encoder_conf.tp_blocks (20) */
  int32_t max_frames;          /* LFR rows a handle's position table covers (+ the query rows) */
  int32_t n_query;             /* 4: any other value is refused */
  int32_t n_embed;             /* 16: any other value is refused */
} wn_sensevoice_config;
/* State dict names as init_model gives them: global_cmvn.mean / .istd (the model takes the CMVN
 * off its encoder), embed.weight (16, 560), encoder.encoders0.0.*, encoder.encoders.N.*,
 * encoder.after_norm.*, encoder.tp_encoders.N.*, encoder.tp_norm.*, ctc.ctc_lo.*; CMVN and the
 * CTC head are required.  encoder.embed.pos_enc.pe is rebuilt here.  wn_encode on the handle
 * encodes every utterance as the reference encodes it ALONE: ceil(n / 6) + 4 frames (none for
 * n == 0); wn_ctc_* then work as on any handle.  No chunks, no streams, no bf16 / fp8. */
int wn_model_create_sensevoice(const wn_config* cfg, const wn_sensevoice_config* scfg,
                               const wn_tensor* weights, int32_t n_weights, int32_t device,
                               wn_model** out);
/* The query ids (HOST, B x 4, each in [0, 16)) of the NEXT wn_encode only, which must run on B
 * utterances; qid_host NULL (B ignored) drops stored ids.  Without stored ids every utterance
 * gets (0, 1, 2, 15): language auto, the fixed event / emotion rows, no text normalisation. */
int wn_sensevoice_set_queries(wn_model* m, const int32_t* qid_host, int32_t B);
/* The SenseVoice front end alone (test hook; lens / out_off / qid are HOST arrays checked before
 * the launch): utterance b of lens[b] frames gives out_len[b] = ceil(lens[b] / n) + 4 rows from
 * row out_off[b] (0 rows for lens[b] == 0).  Row t < 4 is embed[qid[b][t]] (no CMVN), row t >= 4
 * the LFR row t - 4 with GlobalCMVN (mean NULL: none); every row takes x * xscale + pe[t + 1] and
 * LayerNorm(m F; ln_w, ln_b, eps).  Rows are ldo wide, m F <= ldo <= 576, zeros behind m F. */
int wn_op_sv_front(const float* feats, const float* mean, const float* istd, const float* embed,
                   const float* pe, int32_t pe_rows, const float* ln_w, const float* ln_b,
                   float* out, int32_t ldo, int32_t out_rows, const int32_t* lens,
                   const int32_t* out_off, const int32_t* qid, int32_t* out_len, int32_t B,
                   int32_t T, int32_t F, int32_t m, int32_t n, float xscale, float eps,
                   void* stream);

/* Squeezeformer encoders (`encoder: squeezeformer`, wenet/models/squeezeformer/) under the
 * asr_model head: the Conv2dSubsampling4-shaped front end (pw_conv / dw_conv / input_proj, the
 * sqrt(d) scale in FRONT of the projection), preln, post-LN blocks of attention / FFN / conv
 * module / FFN with an adaptive scale in front of every module, one time reduction in front of
 * block reduce_idx and its recovery in front of block recover_idx.  In wn_config, ffn_dim is
 * encoder_dim * feed_forward_expansion_factor, cnn_norm / cnn_kernel / causal describe the conv
 * module. */
typedef struct {
  int32_t reduce_idx;      /* block in front of which the time reduction sits, or -1: none */
  int32_t recover_idx;     /* block in front of which the recovery sits (> reduce_idx), or -1 */
  int32_t reduce_kernel;   /* 5: conv1d (padding 3), 1: stream (no padding) */
  int32_t do_rel_shift;    /* the wrapped rel_shift of squeezeformer/attention.py */
} wn_squeezeformer_config;

/* wn_model_create for such a state dict (the names init_model gives it), loaded strictly.  On
 * the handle, wn_encode runs the layer stack in fp32 with every utterance encoded as the
 * reference encodes it ALONE: T' = (len - 7) / 4 + 1 frames (the reference's batched mask counts
 * one frame more for every utterance shorter than the batch's longest), the shift wraps at the
 * utterance's own length, the convs and the time reduction see its own frames only.  chunk /
 * left set the attention mask only; a chunk mask is refused with do_rel_shift (the shift kernel
 * is full context), and an odd chunk size is refused on a model with a time reduction.
 * wn_encode_chunk*, wn_stream_create and a bf16 / fp8 precision are refused on such a handle. */
int wn_model_create_squeezeformer(const wn_config* cfg, const wn_squeezeformer_config* qcfg,
                                  const wn_tensor* weights, int32_t n_weights, int32_t device,
                                  wn_model** out);

/* Efficient Conformer encoders (`encoder: efficientConformer`, EfficientConformerEncoder,
 * wenet/models/efficient_conformer/encoder.py:38-295) under the asr_model head: the conv2d
 * (rate 4) or conv2d2 (rate 2, efficient_conformer/subsampling.py:25-75) front end, pre-LN
 * macaron Conformer layers of which the ones in group_mask run the grouped attention and the
 * ones in stride_layers halve the frame rate (StrideConformerEncoderLayer), after_norm.  In
 * wn_config, cnn_kernel is the kernel of the layers up to and including the first stride layer. */
typedef struct {
  int32_t group_size;        /* frames per group of a grouped layer */
  int32_t group_mask;        /* bit i: layer i runs GroupedRelPositionMultiHeadedAttention */
  int32_t n_stride;          /* stride layers, <= 4 (each of stride 2) */
  int32_t stride_layers[4];  /* ascending layer indices */
  int32_t stride_kernel;     /* 1: the conv kernel is halved (K / 2) behind every stride layer */
  int32_t front_rate;        /* 4: conv2d, 2: conv2d2 */
  int32_t head_dim;          /* d_model / n_heads: 32 or 64 */
} wn_efficonformer_config;

/* wn_model_create for such a state dict (the names init_model gives it; the stride layers'
 * concat_linear.* is never used by the reference and is not read).  On the handle, wn_encode runs
 * the layer stack in fp32 with every utterance encoded as the reference encodes it ALONE: the
 * zero frames of pad4group, the position rows and the average pool's last window end at the
 * utterance's own length.  chunk / left set the attention mask; a chunk mask whose size is not
 * divisible by the product of the strides is refused.  enc_lens_host and the padded output are
 * at the FINAL rate: ceil(.. ceil(T' / 2) .. / 2) frames.  wn_encode_chunk*, wn_stream_create
 * and a bf16 / fp8 precision are refused on such a handle. */
int wn_model_create_efficonformer(const wn_config* cfg, const wn_efficonformer_config* ecfg,
                                  const wn_tensor* weights, int32_t n_weights, int32_t device,
                                  wn_model** out);

/* Operator hook: one advance of a stateless predictor + joint.pred_ffn for M rows
 * (rnnt_stateless_step).  ctx_host (M, context) holds the window ids of every row, oldest first,
 * each in [-1, V) (-1: the zero vector).  w_dev, device pointers: embed.weight [V][E], then for
 * kind 1 pos_embed.weight [heads][E][context], ffn.weight, ffn.bias, for kind 2 conv.weight
 * [E][context], conv.bias (or NULL); then norm.weight, norm.bias, joint.pred_ffn.weight [J][E],
 * joint.pred_ffn.bias: 8 pointers for kind 1, 7 for kind 2.  advance_host (M) or NULL (all
 * rows): the rows with a zero are not written.  out_dev: (M, J). */
int wn_op_stateless_step(const wn_stateless_predictor_config* scfg, const int32_t* ctx_host,
                         const float* const* w_dev, const int32_t* advance_host, float* out_dev,
                         int32_t M, int32_t V, int32_t E, int32_t J, void* stream);

/* RNN-T greedy search over the handle's CURRENT batch (after wn_encode / wn_encode_chunk* /
 * wn_set_encoder_out): basic_greedy_search (wenet/models/transducer/search/greedy_search.py:6-54,
 * reached through Transducer.greedy_search, transducer.py:398-442), which the reference runs one
 * utterance and one symbol at a time, for the whole batch in lock-step.  A step evaluates the
 * joint network for the next F frames of every utterance under its current predictor output
 * (F = tune key "rnnt_lookahead", 1..16), takes their arg-max and consumes the window up to and
 * including its first non-blank frame; the predictor (embedding, LSTM layers, projection,
 * joint.pred_ffn) advances for the utterances that emitted.  The token lists do not depend on F
 * or on the batch: every joint row is summed over k in one fixed order.  Always fp32, whatever
 * the handle's precision (the encoder follows the handle).  The arg-max follows torch.argmax:
 * the lowest index on ties, and a NaN (from the caller's encoder output, say) counts as the
 * largest value, so a token is always an id in [0, vocab).
 *   n_steps        most symbols one frame may emit (the reference's n_steps, 64)
 *   tokens_host    (B, max_len) int32, tok_lens_host (B) int32
 *   max_len        row pitch of tokens_host; -1 with a message if an utterance decoded more
 *   steps_out      lock-step steps taken (may be NULL)
 * Returns -1 with a wn_last_error text on a handle that wn_model_create_transducer did not
 * build (no transducer weights). */
int wn_transducer_greedy_search(wn_model* m, int32_t n_steps, int32_t* tokens_host,
                                int32_t* tok_lens_host, int32_t max_len, int32_t* steps_out,
                                void* stream);

/* ---- streaming transducer sessions: resumable RNN-T greedy search ---------- */
/* wn_transducer_greedy_search for sessions that receive their encoder frames chunk by chunk (the
 * reference has no such entry point: its greedy search is one-shot, transducer.py:427 "TODO
 * forward chunk by chunk").  A set of `n_slots` independent sessions whose search state -- the
 * LSTM's h / c, the projected predictor output, the last token, the tokens with the encoder
 * frame of each, the frame counters -- lives in HBM between calls.  Feeding a session its frames
 * in any pieces gives the token list the one-shot search gives for all of them at once, and
 * after every call the list it gives for the frames so far; a session's state is bit for bit the
 * same whatever the pieces, the window (tune key "rnnt_lookahead"), its slot and the other
 * sessions of a call.  Every call names the sessions it touches by slot id; calls on one set must
 * be ordered (one stream, or events between streams).  A set belongs to the handle it was created
 * on and must be destroyed before it; its workspace is its own, so other searches on the handle
 * between two calls leave the sessions alone.  Always fp32, as the one-shot search. */
typedef struct wn_rnnt_stream_set wn_rnnt_stream_set;

/* Where wn_rnnt_stream_advance_encoded puts its results (all HOST arrays, the n sessions of the
 * call in call order): tok_lens (n) the tokens each session holds after the call; tokens, times
 * (n, max_len) the whole list so far and the absolute encoder frame of each token
 * (non-decreasing, at most n_steps equal entries), of each row the first tok_lens entries
 * written; frames_decoded (n) the frames the session has consumed; trailing_blank (n) the frames
 * consumed behind the frame of its last token, or all of them if it has none (this project's
 * definition: the reference has no RNN-T endpointing).  max_len must be >= what a session's
 * token count may become in the call: min(tokens before + n_t * n_steps, max_tokens).  steps:
 * the lock-step steps of the call, may be NULL. */
typedef struct wn_rnnt_stream_result {
  int32_t* tok_lens;
  int32_t* tokens;
  int32_t* times;
  int32_t* frames_decoded;
  int32_t* trailing_blank;
  int32_t max_len;
  int32_t* steps;
} wn_rnnt_stream_result;

/* Allocate the state of n_slots sessions (1..256), once: at most max_frames encoder frames and
 * max_tokens stored tokens per session, n_steps symbols per frame at most (the reference's
 * n_steps, 64).  Every slot starts reset.  -1 with a wn_last_error text on a handle that
 * wn_model_create_transducer did not build (no transducer weights). */
int wn_rnnt_stream_create(wn_model* m, int32_t n_slots, int32_t max_frames, int32_t max_tokens,
                          int32_t n_steps, wn_rnnt_stream_set** out, void* stream);
int wn_rnnt_stream_destroy(wn_rnnt_stream_set* set);

/* Zero predictor state, last token = blank, no tokens, counters to zero for the n sessions in
 * slot_ids (host); the other sessions keep their state bit for bit. */
int wn_rnnt_stream_reset(wn_rnnt_stream_set* set, int32_t n, const int32_t* slot_ids,
                         void* stream);

/* The search on the next frames of n sessions: enc_out_dev is the (n, chunk, d_model) encoder
 * output of wn_encode_chunk_batch on the device, session i consumes its first n_t_host[i] rows
 * (0 <= n_t <= chunk; 0 leaves the session's state bit for bit).  joint.enc_ffn runs once over the
 * n x chunk rows, then the lock-step loop of wn_transducer_greedy_search over the call's frames:
 * groups of 8 steps, at most chunk x (n_steps + 1) + 1 of them.  A token that the n_steps cap
 * emits on a call's last frame leaves its predictor step to the next call with frames.
 * Refused on the host, before any launch, with -1 and a wn_last_error text that names the
 * argument: n outside [1, n_slots]; a slot id out of range; the same slot twice in one call; n_t
 * outside [0, chunk]; a call that would take a session past max_frames; a max_len smaller than
 * stated above.  A refused call changes no session.
 * A session whose tokens pass max_tokens keeps counting and stops storing: the call returns -1
 * with "token buffer overflow" (the other sessions of the call did advance), and that session
 * must be reset. */
int wn_rnnt_stream_advance_encoded(wn_rnnt_stream_set* set, int32_t n, const int32_t* slot_ids,
                                   const float* enc_out_dev, const int32_t* n_t_host,
                                   int32_t chunk, const wn_rnnt_stream_result* out, void* stream);

/* Test hook: one slot's h, c (layers x H each), pred_proj (join_dim) and
 * {last_tok, stale, n_tok, frames, trailing_blank} copied to the host.  A handle with a
 * stateless predictor has no h / c (0 layers): nothing is written to them. */
int wn_rnnt_stream_state(wn_rnnt_stream_set* set, int32_t slot, float* h, float* c,
                         float* pred_proj, int32_t* scalars5, void* stream);

/* ---- streaming transducer sessions: resumable RNN-T prefix beam search ---------- */
/* wn_transducer_beam_search (below) for sessions that receive their encoder frames chunk by chunk
 * (no counterpart in the reference: its prefix beam search is one-shot).  A set of `n_slots`
 * sessions of `beam` slots each; a session's state -- n_live and frames, per slot the fp64 score,
 * the token row (at most one symbol per frame), the last token, whether the predictor step on it
 * is still owed (`pending`), the absolute frame of its last token, the LSTM's h / c and the
 * projected predictor output -- lives in HBM between calls.  The search is causal: after every
 * call a session's beam is the beam the one-shot search gives for the frames it has consumed, and
 * its stored state is bit for bit the same whatever the pieces, its slot and the other sessions
 * of a call.  (The scores equal the one-shot search's bit for bit where both runs take the same
 * GEMM route for joint.enc_ffn and the CTC head; a one-shot batch of >= 512 rows may take the
 * six-product GEMM for the CTC head, a chunk does not.)  The beam, the fusion weights and
 * max_frames are fixed when the set is created.  Calls on one set must be ordered; the set
 * belongs to the handle it was created on and must be destroyed before it; its workspace is its
 * own, so other searches on the handle between two calls leave the sessions alone.  Always
 * fp32 / fp64, as the one-shot search. */
typedef struct wn_rnnt_beam_stream_set wn_rnnt_beam_stream_set;

/* Where wn_rnnt_beam_stream_advance_encoded puts its results (all HOST arrays, the n sessions of
 * the call in call order): n_hyps (n) the live hypotheses of each session, best first; hyp_lens
 * (n, beam); hyp_tokens (n, beam, max_len), of each row the first hyp_lens entries written, tokens
 * without the leading blank; hyp_scores (n, beam) fp64, -inf beyond n_hyps; frames_decoded (n) the
 * frames the session has consumed; trailing_blank (n) the frames consumed behind the frame of the
 * best hypothesis' last token, or all of them if it has none (this project's definition: the
 * reference has no RNN-T endpointing).  max_len must be >= the frames any session of the call has
 * consumed after it (a hypothesis holds at most one token per frame). */
typedef struct wn_rnnt_beam_stream_result {
  int32_t* n_hyps;
  int32_t* hyp_lens;
  int32_t* hyp_tokens;
  double* hyp_scores;
  int32_t* frames_decoded;
  int32_t* trailing_blank;
  int32_t max_len;
} wn_rnnt_beam_stream_result;

/* Allocate the state of n_slots sessions (1..256), once; every slot starts reset.  Refused with
 * -1 and a wn_last_error text: a handle that wn_model_create_transducer did not build; beam
 * outside [1, 16] or above the vocabulary; max_frames < 1 or n_slots x beam x max_frames > 2^28;
 * a negative weight, both weights 0; ctc_weight > 0 on a handle without a CTC head. */
int wn_rnnt_beam_stream_create(wn_model* m, int32_t n_slots, int32_t beam, int32_t max_frames,
                               float ctc_weight, float transducer_weight,
                               wn_rnnt_beam_stream_set** out, void* stream);
int wn_rnnt_beam_stream_destroy(wn_rnnt_beam_stream_set* set);

/* The state the one-shot search starts an utterance from -- one live hypothesis [], score 0.0,
 * last token = blank with its predictor step owed, zero LSTM state, counters 0 -- for the n
 * sessions in slot_ids (host); the other sessions keep their state bit for bit. */
int wn_rnnt_beam_stream_reset(wn_rnnt_beam_stream_set* set, int32_t n, const int32_t* slot_ids,
                              void* stream);

/* The search on the next frames of n sessions: enc_out_dev is the (n, chunk, d_model) encoder
 * output of wn_encode_chunk_batch on the device, session i consumes its first n_t_host[i] rows
 * (0 <= n_t <= chunk; 0 leaves the session's state bit for bit and returns its current beam).
 * joint.enc_ffn -- and with ctc_weight > 0 the CTC head and its log-softmax -- run once over the
 * n x chunk rows, then exactly max(n_t) lock-step steps of wn_transducer_beam_search's frame
 * without a look at the device in between, then one copy of the results.  A token appended on a
 * session's last frame of the call leaves its predictor step to the next call with frames.
 * Refused on the host, before any launch, with -1 and a wn_last_error text that names the
 * argument: n outside [1, n_slots]; a slot id out of range; the same slot twice in one call; n_t
 * outside [0, chunk]; a call that would take a session past max_frames; a max_len smaller than
 * stated above.  A refused call changes no session. */
int wn_rnnt_beam_stream_advance_encoded(wn_rnnt_beam_stream_set* set, int32_t n,
                                        const int32_t* slot_ids, const float* enc_out_dev,
                                        const int32_t* n_t_host, int32_t chunk,
                                        const wn_rnnt_beam_stream_result* out, void* stream);

/* Test hook: one session's whole state copied to the host: counters2 = {n_live, frames}; scores
 * (beam) fp64; slot_ints (4, beam) = tok_len | last_tok | pending | last_time; tokens
 * (beam, max_frames), -1 behind tok_len; h, c (beam, layers, H); pred_proj (beam, join_dim).
 * Slots beyond n_live hold one fixed form (-inf, blank, -1, zeros).  A handle with a stateless
 * predictor has no h / c (0 layers): nothing is written to them. */
int wn_rnnt_beam_stream_state(wn_rnnt_beam_stream_set* set, int32_t slot, int32_t* counters2,
                              double* scores, int32_t* slot_ints, int32_t* tokens, float* h,
                              float* c, float* pred_proj, void* stream);

/* RNN-T prefix beam search over the handle's CURRENT batch: PrefixBeamSearch.prefix_beam_search
 * (wenet/models/transducer/search/prefix_beam_search.py:42-148, reached through
 * Transducer.beam_search, transducer.py:216-260), which the reference runs one utterance at a
 * time, for the whole batch in lock-step, one frame per step and at most one symbol per frame.
 * Per frame and live hypothesis: log_softmax of the joint row, the shallow fusion
 * log(transducer_weight exp(logp) + ctc_weight exp(ctc_logp)) in fp32, its `beam` largest
 * entries (lower index on equal values), candidate scores float32(score) + value held as
 * doubles, prefix fusion by token sequence with log_add in fp64 (the reference's call passes a
 * list to a function that takes its values one by one and raises; this is the evident intent),
 * a stable sort by score, the best `beam` kept.  A slot keeps the predictor state reached after
 * its whole hypothesis, so only the hypotheses that appended a token run the LSTM step.  Always
 * fp32 / fp64, whatever the handle's precision; ctc_weight == 0 does not run the CTC head.
 * `longest T'` steps are issued without a look at the device in between.
 *   beam              1..16 and at most the vocabulary
 *   ctc_weight, transducer_weight   >= 0, not both 0
 *   n_hyps_host       (B) hypotheses of each utterance (>= 1), in rank order
 *   hyp_lens_host     (B, beam); hyp_tokens_host (B, beam, max_len), without the leading blank
 *   hyp_scores_host   (B, beam) fp64; -inf beyond n_hyps
 *   max_len           row pitch of hyp_tokens_host; -1 with a message if a hypothesis is longer
 *                     (a hypothesis has at most T' tokens)
 * Returns -1 with a wn_last_error text on a handle that wn_model_create_transducer did not
 * build (no transducer weights). */
int wn_transducer_beam_search(wn_model* m, int32_t beam, float ctc_weight,
                              float transducer_weight, int32_t* n_hyps_host,
                              int32_t* hyp_lens_host, int32_t* hyp_tokens_host,
                              double* hyp_scores_host, int32_t max_len, void* stream);

/* Of the handle's last wn_transducer_beam_search: the steps it issued (the longest T') and the
 * joint rows that ran the predictor's LSTM step, summed over the steps (the others copied their
 * state).  Either pointer may be NULL. */
int wn_transducer_beam_stats(wn_model* m, int32_t* steps_out, int64_t* advance_rows_out);

/* Teacher-forced transducer score of host n-bests over the handle's CURRENT batch: per
 * hypothesis log P(y | x) = -RNN-T loss, what Transducer._cal_transducer_score
 * (wenet/models/transducer/transducer.py:161-186) takes from torchaudio's rnnt_loss for one
 * utterance at a time: Graves' forward algorithm over the log-softmax of the joint logits,
 *   alpha(t, u) = log_add(alpha(t-1, u) + lp_blank(t-1, u), alpha(t, u-1) + lp_label(t, u-1)),
 *   score = alpha(T'-1, U) + lp_blank(T'-1, U).
 * The (beam, T', U + 1, V) logits are never built: the hypotheses of an utterance go into a
 * prefix trie, the predictor runs once per trie node, the joint GEMM has one row per (frame,
 * node) and keeps only a row's log-sum-exp and its log-probs at the blank and at the tokens of
 * the node's children; the lattices run in fp64.  Always fp32 / fp64, whatever the handle's
 * precision; a hypothesis' score is the same bits alone or in any batch.  The hypothesis arrays
 * are laid out as for wn_rescore:
 *   beam              1..16
 *   n_hyps_host       (B), each in [1, beam]
 *   hyp_lens_host     (B, beam), each in [0, max_len]; hyp_tokens_host (B, beam, max_len),
 *                     tokens in [0, vocab), without the leading blank; max_len <= 4095.  As in
 *                     wn_rescore, the entries of hypotheses k >= n_hyps[b] are never read
 *   td_scores_host    (B, beam) fp64; -inf beyond n_hyps.  An utterance of ZERO frames scores
 *                     -inf for every hypothesis (no path ends in a blank of a frame).
 * Returns -1 with a wn_last_error text for a handle without transducer weights, a beam outside
 * 1..16, a token outside the vocabulary, a length outside [0, max_len], n_hyps outside
 * [1, beam]. */
int wn_transducer_score(wn_model* m, int32_t beam, const int32_t* n_hyps_host,
                        const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
                        int32_t max_len, double* td_scores_host, void* stream);

/* Of the handle's last wn_transducer_score: the joint GEMM rows it computed (frames x trie
 * nodes, summed over the utterances), the rows without prefix sharing (frames x (len + 1),
 * summed over the hypotheses) and the trie nodes of the batch.  Any pointer may be NULL. */
int wn_transducer_score_stats(wn_model* m, int64_t* rows_out, int64_t* rows_unshared_out,
                              int32_t* nodes_out);

/* Measurement (tools/bench_transducer.py --rescore): of the handle's last wn_transducer_score
 * made under wn_profile_enable(m, 1), device time in milliseconds between events on the call's
 * stream: ms_out[0] joint.enc_ffn of the encoder output, [1] the predictor over the trie with
 * joint.pred_ffn, [2] the joint log-prob gather GEMM, [3] the lattices.  Without profiling the
 * call records no events and the four values are 0. */
int wn_transducer_score_times(wn_model* m, float* ms_out);

/* Test hook, handle-less and HOST ONLY (no device is touched): the prefix trie of one
 * utterance's n_hyps (1..16) hypotheses (hyp_lens_host (n_hyps), hyp_tokens_host (n_hyps,
 * max_len)).  Node 0 is the empty prefix (parent -1, token `blank`, depth 0); nodes come in
 * level order, within a level in order of first appearance over the hypotheses in their given
 * order.  parent_out / token_out / depth_out: room for 1 + n_hyps * max_len entries,
 * *n_nodes_out are filled.  path_out (n_hyps, max_len + 1): the node of every prefix of a
 * hypothesis, len + 1 entries, then -1.  col_off_out (nodes + 1) / cols_out (2 nodes - 1): per
 * node the joint columns it is read at, `blank` first, then its children's tokens in node
 * order. */
int wn_op_rnnt_trie(int32_t n_hyps, const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host,
                    int32_t max_len, int32_t blank, int32_t* n_nodes_out, int32_t* parent_out,
                    int32_t* token_out, int32_t* depth_out, int32_t* path_out,
                    int32_t* col_off_out, int32_t* cols_out);

/* Test hook, handle-less: the joint network with a gathering log-softmax epilogue.  The first
 * eleven arguments are those of wn_op_joint_argmax.  Row m lists the columns
 * cols_host[col_off_host[m] .. col_off_host[m + 1]) (at most 17, each in [0, V); col_off_host
 * has M + 1 entries from 0); logp_host gets, one float per list entry,
 * logit[col] - logsumexp(row).  Entries of rows with row_enc_host[m] < 0 are not written by the
 * kernel and come back as NaN. */
int wn_op_joint_logp_gather(const float* enc_proj_dev, int32_t enc_rows,
                            const float* pred_proj_dev, int32_t pred_rows,
                            const int32_t* row_enc_host, const int32_t* row_pred_host,
                            const float* w_dev, const float* bias_dev, int32_t M, int32_t J,
                            int32_t V, const int32_t* col_off_host, const int32_t* cols_host,
                            float* logp_host, void* stream);

/* Test hook, handle-less: N RNN-T lattices by the forward algorithm in fp64.  Lattice n has
 * T_host[n] frames and U_host[n] labels (U <= 4095); lp_blank_host holds its T x (U + 1) blank
 * log-probs (t major), lp_label_host its T x U label log-probs, the lattices back to back.
 * scores_host (N): log P; -inf for T == 0.  -inf entries never give NaN. */
int wn_op_rnnt_lattice(int32_t N, const int32_t* T_host, const int32_t* U_host,
                       const float* lp_blank_host, const float* lp_label_host,
                       double* scores_host, void* stream);

/* Test hook, handle-less: one predictor step (RNNPredictor.forward_step, predictor.py:185-206,
 * without the embedding lookup).  x_dev (B, E): the embedding rows; w_host: 4 device pointers
 * per layer (weight_ih (4H, E or H), weight_hh (4H, H), bias_ih, bias_hh; gate order i, f, g, o);
 * h_dev / c_dev (n_layers, B, H) are updated in place for the rows whose advance_dev[b] != 0
 * (NULL: every row) and left bit for bit otherwise; with proj_w_dev (P, H) / proj_b_dev, out_dev
 * (B, P) gets the projection of the last layer's h for the same rows. */
int wn_op_lstm_step(const float* x_dev, const float* const* w_host, int32_t n_layers,
                    const float* proj_w_dev, const float* proj_b_dev, float* h_dev, float* c_dev,
                    const int32_t* advance_dev, float* out_dev, int32_t B, int32_t E, int32_t H,
                    int32_t P, void* stream);

/* Test hook, handle-less: the joint network + arg-max (TransducerJoint.forward, joint.py:62-92,
 * behind its prejoin linears, then argmax over the vocabulary).  Row m of M is
 * tanh(enc_proj_dev[row_enc_host[m]] + pred_proj_dev[row_pred_host[m]]) (rows of J floats;
 * row_enc_host[m] < 0: a row past its utterance's end, answered with idx -1 / max -inf) times
 * w_dev (V, J)^T plus bias_dev (V).  idx_host / max_host (M): the arg-max (lowest index on
 * ties, the first NaN before any number; the column-block partials go through the device
 * reduction of the search's advance kernel) and its logit.  J must be a multiple of 32, at most 1024. */
int wn_op_joint_argmax(const float* enc_proj_dev, int32_t enc_rows, const float* pred_proj_dev,
                       int32_t pred_rows, const int32_t* row_enc_host,
                       const int32_t* row_pred_host, const float* w_dev, const float* bias_dev,
                       int32_t M, int32_t J, int32_t V, int32_t* idx_host, float* max_host,
                       void* stream);

/* Test hook, handle-less: the joint network with a full-row epilogue, the transducer / CTC
 * fusion and the top-k of the beam search.  The first eleven arguments are those of
 * wn_op_joint_argmax.  ctc_logp_dev (ctc_rows, V): CTC log-probs, row row_ctc_host[m] for joint
 * row m (row_ctc_host NULL: row row_enc_host[m]); not read, and may be NULL, with
 * ctc_weight == 0.  val_host / idx_host (M, k): the k largest fused values
 * log(transducer_weight exp(logp) + ctc_weight exp(ctc)) (exp / log in fp64, rounded to fp32
 * once) and their columns, larger value
 * first, the lower index on equal values, a NaN ranked and returned as -inf -- so the indices
 * of a live row are always distinct columns in [0, V).  Rows with row_enc_host[m] < 0 answer
 * (-inf, -1).  fused_host (M, V), may be NULL: the fused rows (zeros for inert rows).
 * k in 1..16 and at most V; the weights >= 0 and not both 0. */
int wn_op_joint_fuse_topk(const float* enc_proj_dev, int32_t enc_rows, const float* pred_proj_dev,
                          int32_t pred_rows, const int32_t* row_enc_host,
                          const int32_t* row_pred_host, const float* w_dev, const float* bias_dev,
                          int32_t M, int32_t J, int32_t V, const float* ctc_logp_dev,
                          int32_t ctc_rows, const int32_t* row_ctc_host, float ctc_weight,
                          float transducer_weight, int32_t k, float* val_host, int32_t* idx_host,
                          float* fused_host, void* stream);

/* Test hook, handle-less: one frame of the beam step of wn_transducer_beam_search on
 * caller-given slots; every array is on the host.  In: lens_host (B) frames of each utterance,
 * n_live_host (B), scores_host (B, beam) fp64, tok_lens_host (B, beam), tokens_host
 * (B, beam, max_tok) (hypotheses without the leading blank), top_val_host / top_idx_host
 * (B, beam, beam) the top-k pairs of each slot's fused row.  Out: the new slots in rank order
 * (n_live_out, scores_out, tok_lens_out, tokens_out; token entries past a length are -1), and per
 * new slot src_out (the slot b x beam + j whose predictor state it takes; -1: none, also when the
 * utterance has no further frame), tok_out (the token it appended, else blank), advance_out
 * (the predictor steps on it) and row_enc_out (its joint row of the next frame, the utterances'
 * rows packed in order; -1: inert).  An utterance with frame >= its length moves on unchanged.
 * Live counts, token counts and top-k indices are range-checked before the launch. */
int wn_op_rnnt_beam_step(int32_t B, int32_t beam, int32_t blank, int32_t V, int32_t frame,
                         const int32_t* lens_host, int32_t max_tok, const int32_t* n_live_host,
                         const double* scores_host, const int32_t* tok_lens_host,
                         const int32_t* tokens_host, const float* top_val_host,
                         const int32_t* top_idx_host, int32_t* n_live_out, double* scores_out,
                         int32_t* tok_lens_out, int32_t* tokens_out, int32_t* src_out,
                         int32_t* tok_out, int32_t* advance_out, int32_t* row_enc_out,
                         void* stream);

/* The same frame in the carry mode of the resumable search (wn_rnnt_beam_stream_*): lens_host are
 * the frames of the CALL, frame0_host (B) the frames each utterance consumed before it.  In,
 * additionally, per slot (B, beam): last_time_host, pending_host and last_tok_host as the step
 * finds them.  On an utterance's last frame of the call src_out is written as on any other frame,
 * a token-appending slot reports pending_out = 1 with advance_out = 0, and row_enc_out stays -1.
 * An utterance with frame >= its length moves on with src_out[g] = g and keeps its tok_out (the
 * last_tok it came with) and pending_out.  last_time_out: frame0 + frame for a slot that
 * appended a token, else its source slot's last_time (a fused entry: the blank candidate's
 * slot); -1 for an empty slot. */
int wn_op_rnnt_beam_step_carry(int32_t B, int32_t beam, int32_t blank, int32_t V, int32_t frame,
                               const int32_t* lens_host, int32_t max_tok,
                               const int32_t* n_live_host, const double* scores_host,
                               const int32_t* tok_lens_host, const int32_t* tokens_host,
                               const float* top_val_host, const int32_t* top_idx_host,
                               const int32_t* frame0_host, const int32_t* last_time_host,
                               const int32_t* pending_host, const int32_t* last_tok_host,
                               int32_t* n_live_out, double* scores_out, int32_t* tok_lens_out,
                               int32_t* tokens_out, int32_t* src_out, int32_t* tok_out,
                               int32_t* advance_out, int32_t* row_enc_out, int32_t* pending_out,
                               int32_t* last_time_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WENET_AMD_H_ */
