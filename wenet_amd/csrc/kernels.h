// Launch wrappers of the non-GEMM kernels of libwenet_amd.
#pragma once
#include "common.h"

namespace wn {

// y[r,:] = LayerNorm(x[r,:]) * w + b, one wave per row; D in {64..1024, %64}.
// y_bf16: y is a bf16 matrix (ldy in bf16 elements) -- bf16-storage mode.
int layernorm(const float* x, int ldx, const float* w, const float* b, float* y,
              int ldy, int M, int D, float eps, hipStream_t s, bool y_bf16 = false);

// y = LayerNorm(x) written as MXFP8: q (M, D) e4m3 bytes + block scales
// [D/128][pitch] dwords (csrc/mxfp8.h); D % 256 == 0.
int layernorm_mx(const float* x, int ldx, const float* w, const float* b, void* q,
                 unsigned* scale, int pitch, int M, int D, float eps, hipStream_t s);

// y1 = LN(x; w1,b1), y2 = LN(y1; w2,b2) in one pass over contiguous [M][D] rows
// (y1 may alias x).
int layernorm2(const float* x, const float* w1, const float* b1, const float* w2,
               const float* b2, float* y1, float* y2, int M, int D, float eps,
               hipStream_t s, bool y2_bf16 = false);

// GlobalCMVN + Conv2d(1->C,3,stride 2) + ReLU over the padded (B,T,F) frame
// tensor, written packed channels-last: out[(t1_off[b]+t1)*F1 + f1][c].
struct Conv1Args {
  const float* feats;    // (B, T, F) padded
  const float* mean;     // [F] or null (no CMVN)
  const float* istd;     // [F]
  const float* w;        // [9][C]  (tap-major, reordered from (C,1,3,3))
  const float* bias;     // [C]
  float* out;            // [sum T1_b][F1][C]
  // instead of `out`: plane image (gemm_x6.hip) with one row per pixel, `tiles` 32-pixel
  // tiles; pixel = frame * F1 + pos, even f1 first (pos = f1 / 2), odd ones behind them
  char* out3 = nullptr;
  int tiles = 0;
  const int* t1_off;     // [B] packed row offset (in T1 frames)
  const int* t1_len;     // [B] number of T1 frames to produce
  int B, T, F, F1, C, max_t1;
};
int cmvn_conv1_relu(const Conv1Args& a, hipStream_t s);

// Depthwise conv over time + LayerNorm(channels) + SiLU (the middle of
// ConvolutionModule.forward).  x is the GLU output [rows][D].
struct DwConvArgs {
  const float* x; int ldx;
  const float* wt;      // [K][D] tap-major depthwise weights
  const float* bias;    // [D]
  const float* cpad;    // [D] value of a padded (masked / left-pad) frame
  const float* ln_w; const float* ln_b;
  int norm_mode = 0;    // 0: LayerNorm over channels (ln_w, ln_b); 1: per-channel
                        // affine y = x * ln_w + ln_b (eval-mode BatchNorm1d)
  float* y; int ldy;
  const int* row_utt;   // [M] utterance of each row (-1: skip)
  const int* off;       // [B] first row of utterance
  const int* len;       // [B] valid frames
  int M, D, K, causal, t_max;  // t_max: padded length T' of the batch
  float eps;
};
int dwconv_ln_silu(const DwConvArgs& a, hipStream_t s);

// Multi-head attention with online softmax (d_k = 64).  Optional relative
// position term: score = ((q+u).k + (q+v).p) * scale.
struct AttnArgs {
  const float* Q; const float* K; const float* V;
  int ldq, ldk, ldv;
  const float* P = nullptr; int ldp = 0;      // [T][h*64] projected pos table
  const int* p_off = nullptr;  // [n_seq] or null: key j of sequence s uses row p_off[s] + j
  const float* bias_u = nullptr; const float* bias_v = nullptr;  // [h][64]
  // folded rel-pos form (relpos_fold): K already holds k + p, kbias [key rows][n_heads] is
  // added to the score before the scale; P / bias_u / bias_v stay null
  const float* kbias = nullptr;
  // fold = true with P / bias_u / bias_v set: the same folding done INSIDE the fp32 attention
  // kernel while the keys are staged (no separate pass, K untouched)
  bool fold = false;
  float* O; int ldo;
  const int* q_off; const int* q_len;   // [n_seq]
  const int* kv_off; const int* kv_len; // [n_seq]
  int n_seq, n_heads, max_q_len;
  bool o_bf16 = false; // bf16 kernel only: O is a bf16 matrix (ldo in elements)
  bool qkv_bf16 = false;  // bf16 kernel only, no rel-pos: Q / K / V are bf16 (ld* in elements)
  float defer_thr = 0.f;   // DMA-staged bf16 kernel: deferred-rescale threshold (log2 units, 0 = off)
  int mask_mode = 0;   // 0: keys < kv_len; 1: causal; 2: chunk window
  int chunk_size = 0, left_chunks = -1;
  float scale = 0.125f;
  // scratch for the six-product form (attention_x6.hip): the key-tile images of this launch;
  // x6_rows = rows of the K / V matrix (all sequences)
  void* x6_img = nullptr; size_t x6_img_bytes = 0; int x6_rows = 0;
  // set by the launchers (tune attn_xcd): > 0 = the grid is 1-D and block b stands for logical
  // block xcd_block_order(b): all query blocks of a (sequence, head) on ONE XCD, whose L2 then
  // fetches that pair's keys / values once instead of once per query block; the value is the
  // number of query blocks per (sequence, head)
  int xcd_nqb = 0;
  // six-product form, key-tile images aligned to the GLOBAL 32-row blocks of the packed K / V
  // matrix (tile t = rows 32 t .. 32 t + 31, whatever sequences they belong to; the kernel
  // masks the slots outside its own sequence) instead of to each sequence's first key: the
  // tiles are then exactly the row blocks of the QKV projection, whose epilogue can write
  // them (x6_img_ready: the image is already there, no pack pass).  row_utt [x6_rows]: the
  // sequence of every row (pack pass with x6_galign)
  int x6_galign = 0;
  // six-product form: the launch's blocks in dispatch order, (sequence << 16 | head << 8 |
  // query block of 64) -- full blocks first, the light last blocks of odd sequences behind
  // them (model.hip set_layout); null = the (query block, head, sequence) grid
  const int* blk_tab = nullptr; int n_blk = 0;
  bool x6_img_ready = false;
  const int* row_utt = nullptr;
};
int attention(const AttnArgs& a, hipStream_t s);
// The kernel attention() runs for `a` under the calling thread's precision and tune(): the
// launchers branch on these, and wn_op_attention reports them to the tests.
enum AttnKind {
  ATTN_PLAIN = 0,      // attention_kernel<NW, false, KS> (with kbias: the pre-folded rel-pos form)
  ATTN_RELPOS = 1,     // attention_kernel<NW, true, KS>: two contractions per score
  ATTN_FOLD = 2,       // attention_kernel<NW, false, KS, true>: rel-pos folded while staging
  ATTN_X6 = 3,         // attention_x6.hip: pack pass + six-product kernel
  ATTN_BF16 = 4,       // attention_bf16_kernel, register-staged, nw waves
  ATTN_BF16_DMA = 5    // attention_bf16_dma_kernel, nw waves
};
struct AttnForm {
  int kind = ATTN_PLAIN;
  int ks = 1;             // fp32 kernels: key split
  int nw = 2;             // waves (32-query groups) per key half
  bool relpos = false;    // bf16 kernel: the rel-pos instantiation
  bool in16 = false;      // bf16 kernels: bf16 Q / K / V
  bool kbias = false;     // ATTN_PLAIN with the per-key score term
  int code() const {
    return kind | ks << 4 | nw << 8 | (int)relpos << 12 | (int)in16 << 13 | (int)kbias << 14;
  }
};
AttnForm attention_form(const AttnArgs& a);
AttnForm attention_bf16_form(const AttnArgs& a);
// rel-pos self attention as six bf16 plane products (attention_x6.hip): pack pass + kernel
size_t attention_x6_image_bytes(int rows, int n_seq, int n_heads);
bool attention_x6_supported(const AttnArgs& a);
int attention_x6(const AttnArgs& a, hipStream_t s);
int relpos_fold(float* K, int ldk, const float* P, int ldp, const float* bias_u,
                const float* bias_v, const int* row_utt, const int* off, const int* p_off,
                float* kbias, int n_heads, int M, int D, hipStream_t s);
// The same with bf16 MFMA operands (attention_bf16.hip); attention() routes here
// when the calling thread's precision is PREC_BF16 (and tune().attn_bf16 != 0).
int attention_bf16(const AttnArgs& a, hipStream_t s);

// Self attention with the relative shift (firered.hip; FireRedASR's Transformer-XL form):
// score(i, j) = ((q_i + u) . k_j + (q_i + v) . p_{i-j}) * scale over all keys of the sequence
// (full context only), d_k = 64, fp32.  P holds the projected position row of DISTANCE r = i - j
// in row p_center - r; every |r| < max_len must lie inside [0, p_rows).
struct RelShiftAttnArgs {
  const float* Q; const float* K; const float* V;
  int ldq, ldk, ldv;
  const float* P; int ldp;      // [p_rows][h*64]
  int p_center, p_rows;
  const float* bias_u; const float* bias_v;   // [h][64]
  float* O; int ldo;
  const int* off; const int* len;   // [n_seq] first row / rows of every sequence
  int n_seq, n_heads, max_len;
  float scale = 0.125f;
};
int attention_relshift(const RelShiftAttnArgs& a, hipStream_t s);

// Self attention with the Squeezeformer's WRAPPED shift (squeezeformer.hip; the reference's
// rel_shift on a T x T matrix), full context only, d_k = 64, fp32:
//   score(i, j) = ((q_i + u) . k_j + S(i, j)) * scale,   len = the sequence's OWN length,
//   S(i, j) = (q_i + v) . p[len - 1 - (i - j)]   for j <= i
//           = 0                                  for j == i + 1
//           = (q_{i+1} + v) . p[j - i - 2]       for j >= i + 2
// P [p_rows][h*64] is linear_pos of the first p_rows position rows; p_rows >= max_len.
struct SqShiftAttnArgs {
  const float* Q; const float* K; const float* V;
  int ldq, ldk, ldv;
  const float* P; int ldp;
  int p_rows;
  const float* bias_u; const float* bias_v;   // [h][64]
  float* O; int ldo;
  const int* off; const int* len;   // [n_seq] first row / rows of every sequence
  int n_seq, n_heads, max_len;
  float scale = 0.125f;
};
int attention_sqshift(const SqShiftAttnArgs& a, hipStream_t s);

// Squeezeformer time reduction (squeezeformer.hip): packed full-rate rows [sum len][C] ->
// packed half-rate rows [sum ceil(len / 2)][C],
//   y[off2[b] + t][c] = bias[c] + sum_k wt[k][c] * x[off[b] + 2 t - pad + k][c],
// frames outside the utterance's own [0, len) being zeros.  K = 5 with pad = 3 (conv1d) or
// K = 1 with pad = 0 (stream).  The frame the reference's conv yields behind ceil(len / 2) and
// cuts is not produced.
constexpr int TR_TILE = 32;        // half-rate frames per workgroup
struct TimeReduceArgs {
  const float* x; int ldx;
  const float* wt;                 // [K][C] tap-major
  const float* bias;               // [C]
  float* y; int ldy;
  const int* off; const int* len;  // [B] full-rate first row / frames
  const int* off2;                 // [B] half-rate first row
  int B, C, K, pad, max_len;       // max_len: full-rate frames of the longest utterance
};
int time_reduce_dwconv(const TimeReduceArgs& a, hipStream_t s);
// Time recovery: y[off[b] + t] = skip[off[b] + t] + z[off2[b] + t / 2], t < len[b] (y may be
// skip).  z is time_recover_layer of the half-rate rows: a Linear is row-wise, so this equals
// the reference's repeat-then-project.
struct TimeRecoverArgs {
  const float* skip; int lds;
  const float* z; int ldz;
  float* y; int ldy;
  const int* off; const int* len; const int* off2;
  int B, C, max_len;
};
int time_recover_add(const TimeRecoverArgs& a, hipStream_t s);

// Grouped self attention of the Efficient Conformer (efficonformer.hip;
// GroupedRelPositionMultiHeadedAttention, efficient_conformer/attention.py:83-126, 180-258), fp32.
// Q / K / V / P / O are packed (frames, D) matrices with their own row strides; sequence i is
// frames off[i] .. off[i] + len[i] - 1 (P: from p_off[i], or 0).  Group row r, head hh, element
// c < width: flat element e = hh * width + c of frames group * r .., i.e. frame group * r + e / D,
// column e % D; frames >= len[i] read as zeros in all four operands and are not written.
//   score(r, s) = ((q_r + u) . k_s + (q_r + v) . p_s) * scale   over ALL ceil(len / group) key rows
// chunk_size > 0: query row r sees key row s iff, with m = mask_step,
//   m s < ((m r) / chunk_size + 1) * chunk_size  and, for left_chunks >= 0,
//   m s >= ((m r) / chunk_size - left_chunks) * chunk_size        (mask[:, ::m, ::m], mask.py)
struct GroupedAttnArgs {
  const float* Q; const float* K; const float* V;
  int ldq, ldk, ldv;
  const float* P; int ldp;
  const int* p_off = nullptr;                   // [n_seq] or null
  const float* bias_u; const float* bias_v;     // [n_heads][width]
  float* O; int ldo;
  const int* off; const int* len;               // [n_seq] first frame / frames
  int n_seq, n_heads, group, width, D;          // D = n_heads * width / group
  int max_len;                                  // frames of the longest sequence
  int mask_step = 1, chunk_size = 0, left_chunks = -1;
  float scale;
};
int attention_grouped(const GroupedAttnArgs& a, hipStream_t s);

// Depthwise conv over time with stride 2 + LayerNorm over the channels (norm_mode 0) or the
// per-channel affine (1) + SiLU (efficonformer.hip; efficient_conformer/convolution.py:64-72,
// 141-146): packed rows at the incoming rate -> packed rows at ceil(len / stride),
//   c[t][ch] = bias[ch] + sum_k wt[k][ch] * x[stride t - pad + k][ch],  pad = (K - 1) / 2 or K - 1
// frames >= len being zeros, frames < 0 zeros or -- causal with cpad set -- the vector cpad.
struct StrideDwConvArgs {
  const float* x; int ldx;
  const float* wt;                 // [K][D] tap-major
  const float* bias;               // [D]
  const float* cpad = nullptr;     // [D] or null: a causal module's left-pad frame
  const float* ln_w; const float* ln_b;
  int norm_mode = 0;
  float* y; int ldy;
  const int* off; const int* len;  // [B] incoming-rate first row / frames
  const int* off2;                 // [B] outgoing-rate first row
  int B, D, K, causal, stride, max_len;
  float eps = 1e-5f;
};
int stride_dwconv_ln_silu(const StrideDwConvArgs& a, hipStream_t s);

// The stride layer's residual (efficonformer.hip; AvgPool1d(2, 2, ceil_mode=True,
// count_include_pad=False), efficient_conformer/encoder_layer.py:138-148):
//   y[off2[b] + t] = z[off2[b] + t] + mean(x[off[b] + 2 t .. min(2 t + 2, len) - 1]);  y may be z
struct AvgPoolResidArgs {
  const float* x; int ldx;
  const float* z; int ldz;
  float* y; int ldy;
  const int* off; const int* len; const int* off2;
  int B, C, stride, max_len;
};
int avgpool_residual_add(const AvgPoolResidArgs& a, hipStream_t s);

// FireRedASR front end (firered.hip): GlobalCMVN, six zero frames behind every utterance's own
// last frame, Conv2d(1->C,3,2) + ReLU, Conv2d(C->C,3,2) + ReLU.  Utterance b has
// t2_len[b] = ((len + 6 - 3) / 2 + 1 - 3) / 2 + 1 output frames and t1_len[b] = 2 t2_len[b] + 1
// rows of h1 (the conv1 frames conv2 reads).
struct FireRedFrontArgs {
  const float* feats;    // (B, T, F) padded
  const float* mean;     // [F] or null (no CMVN)
  const float* istd;     // [F]
  const float* w1;       // [9][C]       tap-major, from (C,1,3,3)
  const float* b1;       // [C]
  const float* w2;       // [9][C1][C2]  tap-major, from (C2,C1,3,3)
  const float* b2;       // [C]
  float* h1;             // scratch [sum t1_len][F1][C]
  float* out; int ldo;   // [sum t2_len][C * F2], column c * F2 + f2
  const int* len;        // [B] frames of the utterance
  const int* t1_off; const int* t1_len;
  const int* t2_off; const int* t2_len;
  int B, T, F, F1, F2, C, max_t2;
};
int firered_frontend(const FireRedFrontArgs& a, hipStream_t s);

// Branchformer / E-Branchformer (branchformer.hip): a depthwise conv over time, tiled so that a
// workgroup stages CSGU_TILE + K - 1 frames x 64 channels of ONE utterance once, fp32.  Frames
// outside the utterance's own [0, len) are the conv's padding (K - 1 in front when causal,
// (K - 1) / 2 on both sides otherwise); no row of a neighbour in the packed buffer is read.
constexpr int CSGU_TILE = 32;      // output frames per workgroup
constexpr int CSGU_MAX_K = 63;
constexpr int CSGU_MAX_C = 1024;   // gate channels the LayerNorm pre-pass holds in registers
struct DwTileArgs {
  const float* x; int ldx;        // [rows][ldx]: the C conv channels start at x
  const float* wt;                // [K][C] tap-major
  const float* bias;              // [C]
  float* y; int ldy;              // [rows][ldy]
  const int* off; const int* len; // [B] first row / frames of every utterance
  int B, C, K, causal, max_len;   // max_len: frames of the longest utterance
  // csgu_gate only: LayerNorm over the C channels in front of the conv (stats: scratch, one
  // (mean, rstd) per row, M rows); a padded frame is ln_b when causal (the reference pads in
  // front of the norm) and 0 otherwise; r (or null: the conv alone) multiplies the result
  const float* ln_w = nullptr; const float* ln_b = nullptr;
  float2* stats = nullptr; int M = 0; float eps = 1e-5f;
  const float* r = nullptr; int ldr = 0;
};
// y = (conv(LayerNorm(x)) + bias) [* r]: the ConvolutionalSpatialGatingUnit between the two
// projections of a cgMLP; C a multiple of 64 up to CSGU_MAX_C.
int csgu_gate(const DwTileArgs& a, hipStream_t s);
// y = x + conv(x) + bias with zero padding: the E-Branchformer merge in front of merge_proj.
// With a.r set, y = ((conv(x) + bias) + x) + r (the Paraformer's FSMN block with the residual
// around it; r may be y's own previous content only if it is another buffer than x).
int merge_dwconv(const DwTileArgs& a, hipStream_t s);
// y = r * g over [M][C] (use_linear_after_conv: the gate behind the extra Linear)
int csgu_mul(const float* r, int ldr, const float* g, int ldg, float* y, int ldy, int M, int C,
             hipStream_t s);

// Fused feed-forward module, fp32 (ffn_fused.hip): P[s] (S, M, D) = partial
// act(X W1^T + b1) W2^T over hidden slice s; ffn_reduce_ln then forms
// x += alpha (sum_s P[s] + b2) and the following LayerNorm(s).
struct FfnArgs {
  const float* X;     // [M][D] = LayerNorm(x)
  const float* W1;    // [F][D]
  const float* b1;    // [F]
  const float* W2;    // [D][F]
  float* P;           // [S][M][D]
  int M, D, F, S, act;
};
int ffn_fused_split(int M, int D, int F);
bool ffn_fused_supported(int M, int D, int F, int act);
int ffn_fused(const FfnArgs& a, hipStream_t s);
// mode 0: x <- x_new, y <- LN(x_new; w, b); mode 1: x <- LN(x_new; w, b),
// y <- LN(x; w2, b2); mode 2: x <- LN(x_new; w, b)
int ffn_reduce_ln(float* x, const float* P, int S, const float* b2, float alpha,
                  const float* w, const float* b, const float* w2, const float* bb2, float* y,
                  int M, int D, float eps, int mode, hipStream_t s);
// mode 1 with y leaving as the X3 plane image (M x 256) instead of fp32 rows: the same
// arithmetic per row, eight rows per block, the planes turned through LDS into whole
// 128-byte pieces of the image
int ffn_reduce_ln_img(float* x, const float* P, int S, const float* b2, float alpha,
                      const float* w, const float* b, const float* w2, const float* bb2,
                      void* y3, int M, int D, float eps, hipStream_t s);

// fp32 GEMM as six bf16 plane products (gemm_x6.hip).  Operands are "X3" images:
// x6_bytes(R, K) bytes for an R x K matrix, made by x6_split or by a GEMM's EPI 2.
struct X6Args {
  const void* A3 = nullptr;   // image of A (M x K)
  // instead of A3: A as plain row-major fp32 (lda floats per row, a_bytes = extent of the
  // buffer), split into planes in registers; with a_pix: the channels-last fp32 tensor
  const float* A = nullptr; int lda = 0; int64_t a_bytes = 0;
  const void* B3 = nullptr;   // image of W (N x K)
  int M = 0, N = 0, K = 0;
  int row0 = 0;               // first row of C this launch computes (multiple of 256)
  int ksplit = 1;             // K slices (epi 1 only)
  int bm = 0;                 // block rows 128 / 256, 0 = auto
  int nw = 0;                 // 128-row tiles: four waves, two blocks per CU; 8 forces the 8-wave form
  int epi = 0;                // 0: C = resid + alpha act(acc + bias); 1: P[slice][M][N] = acc;
                              // 2: C3 = X3 image of act(acc + bias)
  const float* bias = nullptr;
  const float* resid = nullptr; int ldr = 0;
  float alpha = 1.0f; int act = 0;
  float* C = nullptr; int ldc = 0;
  void* C3 = nullptr;
  // gathered A (implicit GEMM of a convolution): A3 is the image of the channels-last input
  // with one row per pixel (a_tiles 32-pixel tiles, conv_kbc = C / 16 k blocks per tap);
  // GEMM row r reads pixel a_pix[r] + tap_delta[tap]
  const int* a_pix = nullptr;
  int a_tiles = 0, conv_kbc = 0;
  int conv_taps = 0;          // > 0: K order (channel block, tap) instead of (tap, channel block)
  int tap_delta[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int probe = 0;              // ablation bits (tune().x6_probe)
  // gathered A (conv2): scratch for the K-slice partials of the last, partial round of tiles
  // (part_bytes >= slices x rows x N x 4); null: the remainder runs as 128-row tiles
  float* part = nullptr; size_t part_bytes = 0;
};
int gemm_x6_clocks(unsigned long long* out);   // probe & 4 stamps [8 waves][8]
size_t x6_bytes(int R, int K);
int x6_split(const float* src, int R, int K, int ld, void* dst, hipStream_t s);
int gemm_x6_bm(int M, int N, int ksplit);
int gemm_x6(const X6Args& a, hipStream_t s);
// The tile form gemm_x6() runs a gathered-A GEMM (a.a_pix: the subsampling conv2) in under the
// calling thread's tune(): its launch code switches on this, wn_op_conv2d4 reports it.
enum X6ConvTile {
  X6CONV_128 = 0,          // one launch of 128-row tiles
  X6CONV_256 = 1,          // one launch of 256-row tiles
  X6CONV_256_REM128 = 2,   // `full` 256-row tiles, the rows behind them as 128-row tiles
  X6CONV_256_KTAIL = 3     // `full` 256-row tiles, the rows behind them as `slices` K slices of
                           // 256-row tiles into a.part + conv_tail_reduce_kernel
};
struct X6ConvForm {
  int tile = X6CONV_128;
  int full = 0;            // 256-row tiles of the first launch (the two-launch forms)
  int slices = 0;          // K slices of the tail (X6CONV_256_KTAIL)
};
X6ConvForm gemm_x6_conv_form(const X6Args& a);
// Fused six-product feed-forward module (ffn_x6f.hip): hidden tensor in registers, d_model 256.
struct FfnX6Args {
  const float* X = nullptr;    // X = LayerNorm(x): [M][ldx] fp32 (split into planes in registers)
  int ldx = 0;
  // instead of X (round 5): the X3 plane image of LN(x) (M x 256, records [k block][row tile]
  // [plane]) written by the producer of LN(x) -- the epilogue of the pointwise_conv2 row-block
  // GEMM, ffn_reduce_ln_img -- so that the S hidden-slice blocks of a row tile load ready-made
  // operand fragments instead of each loading, turning and splitting the fp32 rows
  const void* X3 = nullptr;
  const void* W13 = nullptr;   // X3 image of W1: F x 256
  const void* W2p = nullptr;   // k-slot-permuted image of W2 (x6_split_perm): 256 x F
  const float* b1 = nullptr;   // [F]
  float* P = nullptr;          // [S][M][256] hidden-slice partials
  int M = 0, D = 0, F = 0, S = 0, act = 0;
};
int ffn_x6f_clocks(unsigned long long* out);   // VAR & 8192 stamps [4 waves][24]
int x6_split_perm(const float* src, int R, int K, int ld, void* dst, hipStream_t s);
int ffn_x6f_split(int M, int F);
bool ffn_x6f_supported(int M, int D, int F, int act);
int ffn_x6f(const FfnX6Args& a, hipStream_t s);


// x_out = resid + alpha (A W^T + bias), y = LayerNorm(x_out): GEMM with N = 256 whose
// block owns complete rows (gemm_rowln.hip)
struct RowLnArgs {
  const float* A; int lda;
  const float* W;         // [256][K]
  const float* bias;      // [256] or null
  const float* resid; int ldr;   // may alias x_out
  float alpha;
  float* x_out; int ldx;
  const float* ln_w; const float* ln_b; float eps;
  float* y; int ldy;      // may alias A (a block reads only the rows it writes)
  int M, N, K;
};
// Row-block six-product GEMM, K = 256, A rows in registers (gemm_x6r.hip)
struct X6RArgs {
  const float* A = nullptr; int lda = 0;     // [M][lda] fp32
  int K = 256;                               // 256 (gemm_x6r.hip) or 512 (gemm_x6r512.hip)
  const void* W3 = nullptr;                  // X3 image of W (N x K)
  const float* bias = nullptr;               // [N] or null
  int M = 0, N = 0;
  int epi = 0;          // 0: C = acc + bias; 1: x_out = resid + alpha (acc + bias), y = LN(x_out);
                        // 2: C = GLU(acc + bias), N / 2 columns (W rows permuted [32 a | 32 gate])
  float* C = nullptr; int ldc = 0;
  const float* resid = nullptr; int ldr = 0; float alpha = 1.0f;   // resid may alias x_out
  float* x_out = nullptr; int ldx = 0;
  const float* ln_w = nullptr; const float* ln_b = nullptr; float eps = 1e-5f;
  float* y = nullptr; int ldy = 0;           // may alias A (a block reads its rows first)
  // epi 1, K = 256: additionally / instead (y may be null then) the X3 plane image of y (M x N,
  // ceil(M / 32) row tiles) for a six-product consumer that wants fragments, not rows
  void* y3 = nullptr;
  // epi 3 = epi 1 chained with C = GLU(y W3b^T + bias2): W3b = X3 image of a 2 K x K weight
  // (rows [32 values | 32 gates] per 64), C [M][K]; y is stored only if set
  const void* W3b = nullptr; const float* bias2 = nullptr;
  // prologue fold (epi 0, N = 3 K -- the QKV projection behind a fused feed-forward module): the
  // A rows are NOT read from `A` but formed as ffn_reduce_ln (mode 0) forms them,
  //   x_new = pro_x + pro_alpha (sum_s pro_P[s] + pro_b2),  A = LayerNorm(x_new; ln_w, ln_b, eps),
  // x_new written back to pro_x ([M][K]); pro_P = [pro_S][M][K] slice partials
  const float* pro_P = nullptr; int pro_S = 0; const float* pro_b2 = nullptr;
  float pro_alpha = 0.f; float* pro_x = nullptr;
  // depthwise-conv prologue (epi 1, K = N = 256 -- pointwise_conv2 behind the middle of the
  // convolution module): the A rows are NOT read from `A` but formed as dwconv_ln_silu forms
  // them from dw.x (dw.y is ignored: the rows never reach HBM)
  int dw_on = 0;
  DwConvArgs dw;
  // epi 4 (K = 256, N = 768, with the prologue fold): the QKV projection of a layer whose self
  // attention runs as six plane products over GLOBAL-row-aligned key tiles (attention_x6.hip,
  // AttnArgs::x6_galign): W3 / bias hold the rows permuted per head ([Q_h | K_h | V_h] x 64,
  // h = 0..3 -- wave h of a block owns head h), Q goes to C (columns h 64 ..) as fp32 rows, and
  // the block's 32 rows ARE key tile blockIdx.x: K' = k + p planes, V^T planes and the per-key
  // scalars u.k + v.p of the four heads are written straight into the tile image (at_img),
  // the pack pass's arithmetic in its order -- bit-identical, one launch and 42 MB of traffic
  // per layer less.  at_P [T][at_ldp] = the layer's projected position table, at_u / at_v
  // [4][64], at_row_utt [M] / at_off [n_seq] / at_p_off (or null) give a row its position
  void* at_img = nullptr;
  const float* at_P = nullptr; int at_ldp = 0;
  const float* at_u = nullptr; const float* at_v = nullptr;
  const int* at_row_utt = nullptr; const int* at_off = nullptr; const int* at_p_off = nullptr;
};
int gemm_x6r_clocks(unsigned long long* out);   // phase stamps of the last x6r_kernel launch (gemm_x6r.hip)
bool gemm_x6r_supported(int M, int N, int K, int epi);
int gemm_x6r(const X6RArgs& a, hipStream_t s);          // dispatches on a.K
bool gemm_x6r512_supported(int M, int N, int epi);
int gemm_x6r512(const X6RArgs& a, hipStream_t s);
bool gemm_rowln_supported(int M, int N, int K);
int gemm_rowln(const RowLnArgs& a, hipStream_t s);

// CTC head tail: per row log-softmax statistics + top-k (descending, lower
// index first on ties) (+ optionally the full log-prob row).
struct CtcRowArgs {
  const float* logits; int ld;    // [M][V]
  int M, V, k;
  int blank; float blank_penalty;
  float* topk_val;   // [M][k] log-probs
  int* topk_idx;     // [M][k]
  float* logp;       // [M][ld_out] or null
  int ld_out;
};
int ctc_logsoftmax_topk(const CtcRowArgs& a, hipStream_t s);

// Greedy collapse (ctc_greedy_search): per utterance remove repeats + blanks.
// filter_blank_embedding (asr_model.py:153-180): rows whose CTC arg-max is not 0, compacted
int nonblank_map(const int* top1, int stride, const int* off, const int* len, int B, int* map,
                 int* n_keep, hipStream_t s);
int nonblank_gather(const float* src, const int* map, const int* off, const int* n_keep,
                    const int* noff, const int* nlen, const int* row_utt_new, float* dst, int D,
                    int rows_new, hipStream_t s);
int ctc_greedy_collapse(const int* top1, int top1_stride, const int* off,
                        const int* len, int B, int blank, int* out_tokens,
                        int out_stride, int* out_lens, hipStream_t s);

// CTC prefix beam search, one workgroup per utterance.
// Flattened ContextGraph (wenet/utils/context_graph.py): node 0 is the root;
// the trie edges live in an open-addressing hash table keyed by
// (state << 32 | token), linear probing, `mask` + 1 slots, empty = ~0.
struct CtxGraph {
  const int* fail = nullptr;              // [n_nodes]
  const double* node_score = nullptr;     // [n_nodes]
  const double* output_score = nullptr;   // [n_nodes]
  const double* token_score = nullptr;    // [n_nodes]
  const unsigned long long* keys = nullptr;
  const int* vals = nullptr;
  unsigned mask = 0;
};
constexpr unsigned long long CTX_EMPTY = ~0ull;
__host__ __device__ inline unsigned ctx_slot(unsigned long long key, unsigned mask) {
  unsigned long long z = key * 0x9E3779B97F4A7C15ull;
  z ^= z >> 29;
  return (unsigned)z & mask;
}

// The resumable search (ctc.hip, prefix_beam_kernel<.., StreamPrefixBeamArgs>): PrefixBeamArgs
// (below) with len[b] = new frames of the session in workgroup b, off[b] = its first top-k /
// log-prob row, max_len = the sessions' frame capacity, pool / pool_stride = the per-SLOT
// persistent pools; the outputs hold `nbest ? beam : 1` rows per session, token / time rows
// `out_stride` long.
struct StreamBeamArgs {
  void* state = nullptr;        // StreamState[n_slots] (ctc.hip)
  const int* slot = nullptr;    // [B] slot of each session of this launch (distinct)
  int nbest = 0;                // 1: emit the whole beam, 0: the 1-best only
  int out_stride = 0;
  const float* logp = nullptr;  // full log-prob rows (endpoint counters), pitch ld
  int ld = 0;
  float blank_thr = 0.f;        // blank_threshold * blank_scale
  double* hyp_vit = nullptr;    // [B][rows] viterbi_score()
  int* frames = nullptr;        // [B] frames decoded
  int* trail = nullptr;         // [B] trailing blank frames
  int* emit = nullptr;          // per slot stream_emit_ints(max_frames): the 1-best emission cache
};
struct PrefixBeamArgs {
  const float* topk_val; const int* topk_idx; int k;  // [rows][k]
  const int* off; const int* len; int B;
  int beam, blank, max_len;
  // node pools (device scratch): see prefix_beam.hip
  int* pool; int64_t pool_stride;  // ints per utterance
  // outputs
  int* n_hyps;          // [B]
  int* hyp_lens;        // [B][beam]
  int* hyp_tlens;       // [B][beam] length of the times list
  int* hyp_tokens;      // [B][beam][max_len]
  int* hyp_times;       // [B][beam][max_len]
  double* hyp_scores;   // [B][beam]
  // optional phase timing of workgroup 0 (s_memtime cycles, summed over
  // frames): [0] eval, [1] rank, [2] select/write, [3] frames, [4] emit
  long long* dbg_cycles = nullptr;
  CtxGraph cg;  // keys == nullptr: no context biasing
  int weak_hash = 0;  // tests: 2-bit prefix hash, so that the exact sequence test decides
};
struct StreamPrefixBeamArgs : PrefixBeamArgs { StreamBeamArgs st; };
int64_t prefix_beam_pool_ints(int max_len, int beam);
// out[i] = log_add(a[i], b[i]) with the search's own fp64 routine (parity test)
int log_add_pairs(const double* a, const double* b, double* out, int n,
                  hipStream_t s);
int ctc_prefix_beam(const PrefixBeamArgs& a, hipStream_t s);

int64_t stream_state_bytes();
int64_t stream_emit_ints(int max_frames);
int ctc_stream_reset(void* state, int* pool, int64_t pool_stride, int max_frames, int beam,
                     const int* slot_dev, int n, hipStream_t s);
int ctc_prefix_beam_stream(const StreamPrefixBeamArgs& a, hipStream_t s);

// CTC forced alignment (ctc_align.hip).  Labels per utterance: lab[b][0] = blank, lab[b][1 + i] =
// y[i], i < lab_len[b]; row pitch lab_pitch = longest label list + 1 = the width of E.
struct AlignGatherArgs {
  const float* x; int ld;          // [M][V] logits (normalize) or log-probs
  int M, V;
  int normalize;                   // take the log-softmax statistics of the row here
  int blank; float blank_penalty;  // (normalize only)
  const int* row_utt; int Tp;      // row -> utterance (-1: none), or null: row / Tp
  const int* off; const int* len;  // [B] first row, rows of the utterance
  const int* lab; int lab_pitch; const int* lab_len;
  float* E; int ldE;               // [M][ldE]: E[row][j] = logp[row][lab[j]], j <= L; zeros behind
};
int ctc_align_gather(const AlignGatherArgs& a, hipStream_t s);
constexpr int ALIGN_FAST_S = 256;  // states the one-wave trellis holds (4 per lane)
struct AlignArgs {
  const float* E; int ldE;
  const int* off; const int* len; int B, Tp;
  const int* lab; int lab_pitch; const int* lab_len;
  unsigned char* bp; const int64_t* bp_off;   // back pointer workspace, byte offset per utterance
  int fast_S;                      // = ALIGN_FAST_S
  int* path;                       // [B][Tp], entries past the length untouched
  float* frame_logp;               // [B][Tp][2]: E[t][blank], E[t][next label at or behind t]; or null
  float* score; int* status;       // [B]; status 1 = infeasible (T < L + repeats), nothing written
};
int64_t ctc_align_bp_bytes(int T, int L, int fast_S);
// max_fast_L / max_slow_L: the longest label list with 2 L + 1 <= / > ALIGN_FAST_S, -1 = none
int ctc_align_viterbi(const AlignArgs& a, int max_fast_L, int max_slow_L, hipStream_t s);

// Kaldi fbank (see fbank.hip).
struct FbankArgs {
  const float* pcm;          // all utterances back to back, float in [-1, 1]
  const int64_t* sample_off; // [B] first sample of each utterance (device)
  const int* n_frames;       // [B] (device)
  int B, max_frames, n_mel;
  const float* window;       // [400] povey
  const float* twiddle;      // [256][2] cos, -sin of 2*pi*k/512
  const int* mel_start; const int* mel_len; const int* mel_off;  // [n_mel]
  const float* mel_w;        // CSR weights
  float* feats;              // (B, max_frames, n_mel)
};
int fbank_kaldi(const FbankArgs& a, hipStream_t s);
// polyphase sinc resampler (see fbank.hip); taps [nnew][K]
int resample_sinc(const float* x, int64_t n_in, const float* taps, int K, int width,
                  int orig, int nnew, float* out, int64_t n_out, hipStream_t s);

// Whisper log-mel (see logmel.hip): K of the DFT GEMM (400 padded to 416), width
// of its output (201 cos + 201 sin rows), K of the mel GEMM (201 padded to 224).
constexpr int LOGMEL_K1 = 416;
constexpr int LOGMEL_NS = 402;
constexpr int LOGMEL_K2 = 224;
struct LogMelArgs {
  const float* pcm;            // waveforms back to back, float in [-1, 1]
  const int64_t* sample_off;   // [B + 1] (device)
  const int* row_utt;          // [rows] utterance of each packed frame
  const int* frame_off;        // [B] first packed frame of each utterance
  const float* window;         // [400] periodic hann
  float* frames;               // [rows][LOGMEL_K1]
};
int logmel_frames(const LogMelArgs& a, int rows, hipStream_t s);
int logmel_power(const float* spec, float* pw, int rows, hipStream_t s);
int logmel_finish(float* mel, int n_mels, const int* frame_off, const int* n_frames,
                  float* umax, int B, int max_frames, float* feats, hipStream_t s);

// `attention` decode mode, device side (attn_search.hip)
int attn_step_embed(const int* last_tok, int pos, const float* emb, const float* pe,
                    float scale, int d, int n, float* x, hipStream_t s);
int attn_self_step(const float* qkv, int d, int heads, int n, float* cache, int step,
                   const int* path, int max_len, float* out, hipStream_t s);
int attn_beam_init(int BN, int N, int max_len, int sos, float* score, int* end, int* tok,
                   int* path, int* last_tok, hipStream_t s);
int attn_beam_update(int B, int N, int step, int max_len, int eos, int V, const float* topv,
                     const int* topi, const float* score_in, const int* end_in,
                     const int* tok_in, const int* path_in, float* score_out, int* end_out,
                     int* tok_out, int* path_out, int* last_tok, int* n_done, hipStream_t s,
                     bool shared_row = false);
int attn_beam_finish(int B, int N, int len, int max_len, int eos, float length_penalty,
                     const float* score, const int* tok, int* out_tok, int* out_len,
                     hipStream_t s, int prefix = 1);
// the prompted search: rows that start as the (B, P) prompts; the prefill's K | V into the cache
int attn_beam_init_prompt(int BN, int N, int max_len, const int* prompt, int P, float* score,
                          int* end, int* tok, int* path, int* last_tok, hipStream_t s);
int attn_prompt_cache_store(const float* qkv, int d, int B, int P, int N, float* cache,
                            hipStream_t s);

// rows scatter/gather helpers
// forward_chunk cache plumbing (see encoder_kernels.hip), one descriptor per streaming
// session of the call.  The cache tensors keep the reference's per-session layouts:
// att (n_layers, heads, t1, 128), cnn (n_layers, 1, d, lorder).
struct ChunkSess {
  const float* att_cache;   // null iff t1 == 0
  float* new_att;           // (n_layers, heads, nt, 128)
  const float* cnn_cache;   // null: zeros (first chunk)
  float* new_cnn;
  int t1, next_start, nt, kv_off;   // kv_off: first row of this session in the K|V buffer
};
int chunk_kv_assemble(const ChunkSess* sess, int n_sess, int layer, int max_tk,
                      const float* qkv, int R, int H, float* kv, hipStream_t s);
int chunk_conv_input(const ChunkSess* sess, int n_sess, int layer, const float* x, int R,
                     int d, int lorder, float* xext, hipStream_t s);
int copy_rows(const float* src, int lds, const int* src_rows, float* dst,
              int ldd, const int* dst_rows, int n_rows, int D, hipStream_t s);
int fill_zero(void* p, size_t bytes, hipStream_t s);

// RNN-T greedy search with frame lookahead (transducer.hip), fp32
// y[b, :N] = W1 x1[b] + b1 (+ W2 x2[b] + b2) for the rows with advance[b] != 0 (null: all rows)
struct RnntLinearArgs {
  const float* x1 = nullptr; int ldx1 = 0;
  const int* x1_rows = nullptr;     // row b of the input is x1[x1_rows[b]] (embedding lookup)
  const float* W1 = nullptr; int K1 = 0;   // [N][K1]
  const float* b1 = nullptr;
  const float* x2 = nullptr; int ldx2 = 0;  // optional second term (the recurrent one)
  const float* W2 = nullptr; int K2 = 0;
  const float* b2 = nullptr;
  float* y = nullptr; int ldy = 0;
  int N = 0, B = 0;
  const int* advance = nullptr;
  const int* n_active = nullptr;    // device flag: 0 = the batch is finished, return at once
};
int rnnt_linear(const RnntLinearArgs& a, hipStream_t s);
// LSTM cell on gates [B][4H] (i | f | g | o), h / c [B][H] in place on the advancing rows
int rnnt_cell(const float* gates, float* h, float* c, const int* advance, int B, int H,
              const int* n_active, hipStream_t s);
// per row m: arg-max over V of tanh(enc_proj[row_enc[m]] + pred_proj[row_pred[m]]) W^T + bias as
// one (max, index) per 128-column block: part_*[m][rnnt_joint_col_blocks(V)]; row_enc[m] < 0:
// an inert row (-inf, -1)
struct RnntJointArgs {
  const float* enc_proj = nullptr; int lde = 0;
  const float* pred_proj = nullptr; int ldp = 0;
  const int* row_enc = nullptr; const int* row_pred = nullptr;
  const float* W = nullptr; const float* bias = nullptr;   // [V][J], [V]
  int M = 0, J = 0, V = 0;
  float* part_max = nullptr; int* part_idx = nullptr;
  const int* n_active = nullptr;
  float* logits = nullptr; int ldl = 0;   // rnnt_joint_rows: the (M, V) logits of the live rows
};
int rnnt_joint_col_blocks(int V);
int rnnt_joint_argmax(const RnntJointArgs& a, hipStream_t s);
// the same GEMM with a full-row epilogue: logits[m][:V] of every row with row_enc[m] >= 0 (the
// others are left as they are); part_* are not used
int rnnt_joint_rows(const RnntJointArgs& a, hipStream_t s);
// search state of a batch, device arrays of B entries unless noted
struct RnntState {
  int* t; int* cnt; int* last_tok; int* advance; int* done; int* n_tok;
  int* tokens; int max_tok;         // [B][max_tok]
  int* row_enc; int* row_pred;      // [B x F] rows of the next joint launch
  int* n_active; int* steps;        // [1]: unfinished utterances, steps taken
  const int* off; const int* len;   // encoder-output rows of each utterance
};
int rnnt_init(const RnntState& st, int B, int F, int blank, hipStream_t s);
int rnnt_advance(const float* part_max, const int* part_idx, int ncb, int V, const RnntState& st,
                 int B, int F, int blank, int n_steps, hipStream_t s);
// the advance kernel's reduction of the column-block partials alone: out_*[m] of M rows
int rnnt_reduce_partials(const float* part_max, const int* part_idx, int ncb, int M,
                         float* out_max, int* out_idx, hipStream_t s);

// One advance of a stateless predictor (transducer_stateless.hip), fp32: for the rows with
// advance[m] != 0 (null: all rows) out[m][:J] = joint.pred_ffn(act(LayerNorm(mix(window of m)))).
// kind 1 (EmbeddingPredictor): w[h][c] = sum_e x[c][e] pos[h][e][c], mix[e] = sum_c (sum_h w[h][c])
// x[c][e] / (heads C), then ffn.  kind 2 (ConvPredictor): mix[e] = sum_c x[c][e] conv_w[e][c]
// (+ conv_b[e]).  x[c] = embed[id[c]], the zero vector for an id outside [0, V).  The window of
// row m, oldest first: ctx[m][:C], or (ctx == null) the last C entries of
// [-1, ..., -1, blank, tokens[tr][0 .. tok_len[tr])] with tr = tok_row ? tok_row[m] : m; a
// position at or past ld_tok reads as -1.  The other rows of `out` are left as they are.
struct RnntStatelessArgs {
  int kind = 0, E = 0, C = 0, heads = 1, J = 0, V = 0;
  int act = 0;                      // 0 swish, 1 relu
  float eps = 1e-5f;
  const float* embed = nullptr;     // [V][E]
  const float* pos = nullptr;       // [heads][E][C]
  const float* ffn_w = nullptr; const float* ffn_b = nullptr;     // [E][E], [E]
  const float* conv_w = nullptr; const float* conv_b = nullptr;   // [E][C], [E] or null
  const float* norm_w = nullptr; const float* norm_b = nullptr;   // [E]
  const float* pj_w = nullptr; const float* pj_b = nullptr;       // joint.pred_ffn [J][E], [J]
  const int* ctx = nullptr;         // [M][C], or null: the token rows
  const int* tokens = nullptr; int ld_tok = 0;
  const int* tok_len = nullptr; const int* tok_row = nullptr;
  int blank = 0;
  float* out = nullptr; int ldo = 0;
  int M = 0;
  const int* advance = nullptr;
  const int* n_active = nullptr;    // device flag: 0 = the batch is finished, return at once
};
int rnnt_stateless_step(const RnntStatelessArgs& a, hipStream_t s);

// Resumable RNN-T greedy search (transducer_stream.hip): the state of a set of sessions, one
// slot each, that stays in HBM between calls.  Arrays of n_slots entries unless noted.
struct RnntStreamSlots {
  float* h; float* c;               // [n_slots][L][H]
  float* pred_proj;                 // [n_slots][J]
  int* last_tok; int* stale;        // stale: pred_proj does not belong to last_tok yet
  int* n_tok; int* frames;          // tokens emitted (counts on past max_tok), frames consumed
  int* trailing_blank;              // frames consumed behind the frame of the last token
  int* last_time;                   // the absolute frame of the last token, -1: none
  int* tokens; int* times; int max_tok;   // [n_slots][max_tok]
  int L, H, J;
};
// The compact batch of one call over n sessions: what rnnt_linear / rnnt_cell / rnnt_joint_argmax
// run on unchanged.  Device arrays of n entries unless noted.
struct RnntStreamCall {
  const int* slot; const int* n_t;  // the call's sessions and the frames each consumes
  float* h; float* c;               // [L][n][H]
  float* pred_proj;                 // [n][J]
  int* last_tok; int* advance; int* done; int* t; int* cnt;
  int* row_enc; int* row_pred;      // [n x F] rows of the next joint launch (enc row i chunk + t)
  int* n_active; int* steps;        // [1]
  // results of the call, compact: n_tok | frames | trailing_blank [3][n], tokens | times
  // [2][n][ld_out], of each row the first min(n_tok, max_tok) entries
  int* out_stat; int* out_tok; int ld_out;
};
// gather the sessions' state into the compact batch; advance = stale && n_t > 0, done = n_t <= 0,
// the first row map, n_active, steps = 0
int rnnt_stream_begin(const RnntStreamSlots& sl, const RnntStreamCall& c, int n, int chunk, int F,
                      hipStream_t s);
// rnnt_advance's rule on the call's frames; tokens and their absolute frames go to the slot's
// own buffers; a token that the n_steps cap emits on the call's last frame sets `stale`
int rnnt_stream_advance(const float* part_max, const int* part_idx, int ncb, int V,
                        const RnntStreamSlots& sl, const RnntStreamCall& c, int n, int chunk,
                        int F, int blank, int n_steps, hipStream_t s);
// scatter the compact state back, frames += n_t, the call's results into out_*
int rnnt_stream_end(const RnntStreamSlots& sl, const RnntStreamCall& c, int n, hipStream_t s);
// zero state, last_tok = blank, stale = 1, counters 0 for the n slots in `slot` (device)
int rnnt_stream_reset(const RnntStreamSlots& sl, const int* slot, int n, int blank, hipStream_t s);

// RNN-T prefix beam search (transducer_beam.hip), fp32 rows and fp64 scores.
// Per live row (row_enc[m] >= 0): lse of the logits, f[v] = log(tw exp(l[v] - lse) +
// cw exp(ctc[row_enc[m]][v])) (fp64 exp / log, one rounding to fp32) and the k largest (value, index), larger value first, the lower
// index on equal values, a NaN as -inf.  Inert rows answer (-inf, -1).  cw == 0: ctc is not read.
struct RnntFuseArgs {
  const float* logits = nullptr; int ldl = 0;   // [M][V]
  const int* row_enc = nullptr;
  const float* ctc = nullptr; int ldc = 0;      // CTC log-probs by encoder row, or null
  const int* row_ctc = nullptr;                 // the CTC row of joint row m (null: row_enc[m])
  float cw = 0.f, tw = 1.f;
  int M = 0, V = 0, k = 0;
  float* val = nullptr; int* idx = nullptr;     // [M][k]
  float* fused = nullptr; int ldf = 0;          // optional: the fused rows [M][V]
};
int rnnt_fuse_topk(const RnntFuseArgs& a, hipStream_t s);
// the slots of a batch: beam per utterance, the first n_live[b] of them live, in rank order
struct RnntBeamSlots {
  int* n_live = nullptr;       // [B]
  double* score = nullptr;     // [B x beam]
  int* tok_len = nullptr;      // [B x beam]
  int* tokens = nullptr;       // [B x beam][max_tok], without the leading blank
};
struct RnntBeamStepArgs {
  RnntBeamSlots in, out;
  int max_tok = 0;
  const float* top_val = nullptr; const int* top_idx = nullptr;   // [B x beam][beam]
  const int* off = nullptr; const int* len = nullptr;             // [B] encoder rows
  int frame = 0, B = 0, beam = 0, blank = 0, V = 0;
  // of the new slots, [B x beam]: the slot (of the whole batch) whose predictor state the slot
  // takes (-1: none), the token it appended (else blank), whether the predictor steps on it,
  // and its joint row of the next frame (-1: inert)
  int* src = nullptr; int* last_tok = nullptr; int* advance = nullptr; int* row_enc = nullptr;
  int* n_advance = nullptr;    // optional [1]: += the new slots that set `advance`
  // Carry mode (pending != nullptr; the resumable search, transducer_beam_stream.hip): `len` is
  // the frames of this CALL and another call may follow.  On an utterance's last frame of the
  // call `src` is written as on any other frame (the gather carries the state), a token-appending
  // slot's owed predictor step goes to pending[g] (advance stays 0) and row_enc stays -1.  On a
  // later step (frame >= len) the utterance's slots move on as they are with src[g] = g: both
  // buffer parities hold them, last_tok and pending are left alone.  last_time_out[g]: frame0[b]
  // + frame if the new slot appended a token, else last_time_in of its source slot.  All null:
  // the kernel does exactly what the one-shot search needs.
  int* pending = nullptr;                      // [B x beam]
  const int* last_time_in = nullptr; int* last_time_out = nullptr;   // [B x beam]
  const int* frame0 = nullptr;                 // [B] frames consumed before this call
};
// one hypothesis [blank], score 0.0, per utterance; row_pred[g] = g
int rnnt_beam_init(const RnntBeamSlots& st, int* last_tok, int* advance, int* row_enc,
                   int* row_pred, const int* off, const int* len, int B, int beam, int blank, hipStream_t s);
int rnnt_beam_step(const RnntBeamStepArgs& a, hipStream_t s);
// rows src[g] of h_in / c_in [L][M][H] and pp_in [M][J] into rows g of the out buffers (src < 0: skip)
int rnnt_beam_gather(const int* src, const float* h_in, const float* c_in, const float* pp_in,
                     float* h_out, float* c_out, float* pp_out, int M, int L, int H, int J,
                     hipStream_t s);

// Resumable RNN-T prefix beam search (transducer_beam_stream.hip): the state of n_slots sessions
// of `beam` slots each that stays in HBM between calls.  Slot q = session * beam + j.
struct RnntBeamStreamSlots {
  int* n_live; int* frames;         // [n_slots]: live hypotheses, frames consumed
  double* score;                    // [n_slots x beam]
  int* tok_len; int* last_tok;      // [n_slots x beam]
  int* pending;                     // the predictor step on last_tok is still owed
  int* last_time;                   // the absolute frame of the slot's last token, -1: none
  int* tokens; int max_tok;         // [n_slots x beam][max_tok = max_frames]; -1 behind tok_len
  float* h; float* c;               // [n_slots x beam][L][H]
  float* pred_proj;                 // [n_slots x beam][J]
  int beam, L, H, J;
};
// The compact batch of one call over n sessions, M = n x beam rows: what predictor_step,
// rnnt_linear, rnnt_joint_rows, rnnt_fuse_topk, rnnt_beam_step (carry mode) and rnnt_beam_gather
// run on.  `st`, h, c, pred_proj, last_time: the buffer of one parity.
struct RnntBeamStreamCall {
  const int* slot; const int* n_t;  // [n] the call's sessions and the frames each consumes
  RnntBeamSlots st; int max_tok;    // token rows [M][max_tok]
  float* h; float* c;               // [L][M][H]
  float* pred_proj;                 // [M][J]
  int* last_time;                   // [M]
  int* last_tok; int* pending; int* advance; int* row_enc; int* row_pred;   // [M]
  int* off; int* len; int* frame0;  // [n]: i * chunk, n_t[i], frames before the call
  // results (rnnt_beam_stream_end): n_live | frames | trailing_blank [3][n], tok_len [M],
  // score [M], token rows [M][ld_out] (the first tok_len entries of each)
  int* out_stat; int* out_len; double* out_score; int* out_tok; int ld_out;
};
// slots -> the compact batch (parity 0): advance = pending && n_t > 0 (pending is consumed then),
// row_enc = i * chunk for the live slots of a session with n_t > 0, else -1
int rnnt_beam_stream_begin(const RnntBeamStreamSlots& sl, const RnntBeamStreamCall& c, int n,
                           int chunk, hipStream_t s);
// the compact batch (the parity the call ended in) -> slots, frames += n_t, the call's results.
// Dead slots are stored in one canonical form (zero state, -inf, blank, -1).
int rnnt_beam_stream_end(const RnntBeamStreamSlots& sl, const RnntBeamStreamCall& c, int n,
                         int blank, hipStream_t s);
// the state rnnt_beam_init gives an utterance, for the n sessions in `slot` (device)
int rnnt_beam_stream_reset(const RnntBeamStreamSlots& sl, const int* slot, int n, int blank,
                           hipStream_t s);

// Teacher-forced transducer score (transducer_score.hip): fp32 rows, fp64 lattice.
// Per row m with row_enc[m] >= 0, for every entry e of its column list
// [col_off[m], col_off[m + 1]): logp[e] = logit[cols[e]] - logsumexp(row), the logits of
// rnnt_joint_kernel (its own A tile and k loop, rnnt_joint_tile.h: the same bits).  Inert rows write nothing.  ent_row[e] is
// the row that entry e belongs to.  Nothing of size (M, V) is written.
struct RnntGatherArgs {
  const float* enc_proj = nullptr; int lde = 0;
  const float* pred_proj = nullptr; int ldp = 0;
  const int* row_enc = nullptr; const int* row_pred = nullptr;
  const float* W = nullptr; const float* bias = nullptr;   // [V][J], [V]
  int M = 0, J = 0, V = 0;
  const int* col_off = nullptr;     // [M + 1]
  const int* cols = nullptr; const int* ent_row = nullptr;   // [col_off[M]]
  float* logp = nullptr;            // [col_off[M]]
};
int rnnt_joint_logp_gather(const RnntGatherArgs& a, hipStream_t s);
// rows r0 .. r0 + n of h / c [L][stride / H][H] take the rows parent[r0 + i] (< 0: left alone)
int rnnt_trie_gather(const int* parent, float* h, float* c, int r0, int n, int L,
                     int64_t layer_stride, int H, hipStream_t s);
// N lattices: score[n] = log P(y | x) by the forward algorithm, fp64.  lp_blank(t, u) =
// blank[blank_base[n] + t blank_stride[n] + ub[u_off[n] + u]] (u <= U), lp_label(t, u) =
// label[label_base[n] + t label_stride[n] + ul[u_off[n] + u]] (u < U).  T[n] <= 0: -inf.
struct RnntLatticeArgs {
  const float* blank = nullptr; const float* label = nullptr;
  const int* T = nullptr; const int* U = nullptr;
  const int64_t* blank_base = nullptr; const int64_t* label_base = nullptr;
  const int* blank_stride = nullptr; const int* label_stride = nullptr;
  const int* u_off = nullptr; const int* ub = nullptr; const int* ul = nullptr;
  double* score = nullptr;
  int N = 0, max_U = 0;
};
int rnnt_lattice(const RnntLatticeArgs& a, hipStream_t s);

// ---- Paraformer (attention_d128.hip, paraformer.hip), fp32 ---------------------------------
// attention() for heads of d_k = 128 (n_heads * 128 columns): mask_mode 0, no position term,
// separate Q and K / V layouts (self and cross attention).  attention() itself stays d_k = 64.
int attention_d128(const AttnArgs& a, hipStream_t s);

// ---- decoders with heads of 32 (attention_d32.hip), fp32 -----------------------------------
// attention() for heads of d_k = 32 (n_heads * 32 columns): mask_mode 0 (cross attention) or 1
// (causal, kv_len < q_len allowed: the padded batches of wn_decoder_forward), no position term,
// no kbias, no block list.  Always fp32: it does not go through attention_form().
int attention_d32(const AttnArgs& a, hipStream_t s);

// LFR front end (paraformer/layers.py:24-92 on ONE utterance, paraformer.py:329-350): output row
// t of utterance b stacks the m frames n t - (m - 1) / 2 + f, f < m, each index clamped to
// [0, len[b] - 1]; then GlobalCMVN over the m F columns, x * xscale + pe[t + 1], and the
// LayerNorm (ln_w, ln_b; statistics over m F columns) of the first encoder layer.  Rows are
// written ldo wide with zeros in columns m F .. ldo - 1.  One wave per row.
constexpr int LFR_MAX_D = 576;     // m F at most (9 columns per lane)
struct LfrFrontArgs {
  const float* feats;     // (B, T, F) padded
  const float* mean;      // [m F] or null (no CMVN)
  const float* istd;      // [m F]
  const float* pe;        // [pe_rows][m F]: row p = the encoding of position p
  const float* ln_w; const float* ln_b;   // [m F]
  float* out; int ldo;    // [sum rows][ldo]
  const int* len;         // [B] frames of the utterance (> 0)
  const int* off;         // [B] first output row; utterance b owns ceil(len[b] / n) rows
  int B, T, F, m, n, max_rows;   // max_rows: output rows of the longest utterance
  float xscale, eps;
};
int lfr_front(const LfrFrontArgs& a, hipStream_t s);

// SenseVoice front end (sensevoice/sensevoice_small_model.py:249-290 on ONE utterance;
// sensevoice.hip): utterance b owns SV_QUERY + ceil(len[b] / n) rows (none with len[b] == 0).
// Row t < SV_QUERY is embed[qid[b][t]] (no CMVN); row t >= SV_QUERY is LFR row t - SV_QUERY as in
// lfr_front, with GlobalCMVN.  Every row then takes x * xscale + pe[t + 1] -- the positions run
// over the concatenated sequence -- and the LayerNorm of the first encoder layer; written ldo
// wide with zeros behind m F.  One wave per row.
constexpr int SV_QUERY = 4;       // lid | event | emotion | text norm
constexpr int SV_EMBED = 16;      // rows of embed.weight
struct SvFrontArgs {
  const float* feats;     // (B, T, F) padded
  const float* mean;      // [m F] or null (no CMVN)
  const float* istd;      // [m F]
  const float* embed;     // [SV_EMBED][m F]
  const float* pe;        // [pe_rows][m F]: row p = the encoding of position p
  const float* ln_w; const float* ln_b;   // [m F]
  float* out; int ldo;    // [sum rows][ldo]
  const int* len;         // [B] frames of the utterance
  const int* off;         // [B] first output row
  const int* qid;         // [B][SV_QUERY], each in [0, SV_EMBED): validated on the host
  int B, T, F, m, n, max_rows;   // max_rows: output rows of the longest utterance (queries included)
  float xscale, eps;
};
int sv_front(const SvFrontArgs& a, hipStream_t s);

// LayerNorm for rows the one-wave-per-row kernels of layernorm() do not cover: D up to 2048, any
// multiple of 4 (the statistics divide by D); columns D .. Dpad - 1 of y are written as zeros.
int layernorm_wide(const float* x, int ldx, const float* w, const float* b, float* y, int ldy,
                   int M, int D, int Dpad, float eps, hipStream_t s);

// CIF predictor (paraformer/cif.py:55-142, 250-293; cnn_groups 1, residual false).
// cif_stage3: img[r] = [h[t - 1] | h[t] | h[t + 1]] (3 d columns) of every owned row, zeros past
// the utterance's own ends: the A operand of the 3-tap dense conv as ONE GEMM with K = 3 d.
int cif_stage3(const float* h, int ldh, float* img, const int* row_utt, const int* off,
               const int* len, int M, int d, hipStream_t s);
// alpha[r] = relu(sigmoid(y[r] . w + b[0]) * smooth - noise) of every owned row (row_utt[r] >= 0),
// one wave per row
int cif_alpha_rows(const float* y, int ldy, const float* w, const float* b, float smooth,
                   float noise, float* alpha, const int* row_utt, int M, int d, hipStream_t s);
// The integrate-and-fire scan, one workgroup per utterance, len[b] + 1 steps (the last one is the
// tail: alpha = tail, a zero hidden row), threshold 1.0; the scalar chain is the reference's fp32
// operations in its order.  Embedding k of utterance b goes to emb row emb_off[b] + k and the
// frame it fired on to fire_t[emb_off[b] + k], k < emb_cap[b]; n_fire[b] counts every fire;
// token_num[b] = floor(sum alpha) (fp64, index order); rows n_fire .. token_num - 1 are zeros.
struct CifFireArgs {
  const float* h; int ldh;          // [rows][ldh] encoder output
  const float* alpha;               // [rows]
  const int* off; const int* len;   // [B] first row / frames
  const int* emb_off; const int* emb_cap;   // [B]
  float* emb; int lde;              // [sum emb_cap][lde]
  int* fire_t; int* n_fire; int* token_num;
  int B, d; float tail;
};
constexpr int CIF_MAX_D = 1024;
int cif_fire(const CifFireArgs& a, hipStream_t s);

}  // namespace wn
