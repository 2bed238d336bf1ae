// C ABI (include/wenet_amd.h): the operator hooks (wn_op_*) the tests and tools call kernels
// through.
#include "model_state.h"

// ===========================================================================
extern "C" {

int wn_op_gemm(const float* A, const float* W, const float* bias,
               const float* resid, float* C, int32_t M, int32_t N, int32_t K,
               float alpha, int32_t act, void* stream) {
  GemmArgs g;
  g.A = A; g.W = W; g.bias = bias; g.resid = resid; g.C = C;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N;
  g.alpha = alpha; g.act = act;
  return gemm_f32(g, (hipStream_t)stream);
}

int wn_op_gemm_bf16(const float* A, const float* W, const float* bias,
                    const float* resid, float* C, int32_t M, int32_t N, int32_t K,
                    float alpha, int32_t act, void* stream) {
  const int saved = t_gemm_prec;
  t_gemm_prec = PREC_BF16;
  const int r = wn_op_gemm(A, W, bias, resid, C, M, N, K, alpha, act, stream);
  t_gemm_prec = saved;
  return r;
}

int wn_op_gemm_bf16_stored(const float* A, const float* W, const float* bias,
                           const float* resid, void* C, int32_t M, int32_t N, int32_t K,
                           float alpha, int32_t act, int32_t c_bf16, void* stream) {
  // test hook of the bf16-storage GEMM: A and W are converted to bf16 images in
  // scratch buffers first (the model path gets them from its producers / the
  // converted weight slab)
  WN_CHECK(A && W && C && M > 0 && N > 0 && K > 0, "gemm(bf16 stored): null / empty");
  WN_CHECK(K % 32 == 0, "gemm: K must be a multiple of 32");
  static thread_local DevBuf a16, w16;
  hipStream_t s = (hipStream_t)stream;
  WN_TRY(a16.ensure((size_t)M * K * 2));
  WN_TRY(w16.ensure((size_t)N * K * 2));
  WN_TRY(convert_f32_to_bf16(A, a16.p, (int64_t)M * K, s));
  WN_TRY(convert_f32_to_bf16(W, w16.p, (int64_t)N * K, s));
  GemmArgs g;
  g.A = a16.as<float>(); g.W = W; g.bias = bias; g.resid = resid;
  g.C = reinterpret_cast<float*>(C);
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N;
  g.alpha = alpha; g.act = act; g.a_bf16 = true; g.c_bf16 = c_bf16 != 0;
  return gemm_bf16_stored(g, w16.p, s);
}

int wn_op_gemm_lowp(const void* A, const void* W, const void* a_scale, const void* w_scale,
                    const float* bias, const float* resid, void* C, void* c_scale,
                    int32_t M, int32_t N, int32_t K, float alpha, int32_t act,
                    int32_t c_mode, int32_t dtype, void* stream) {
  WN_CHECK(A && W && C && M > 0 && N > 0 && K > 0, "gemm(lowp): null / empty");
  WN_CHECK(K % 32 == 0, "gemm: K must be a multiple of 32");
  GemmArgs g;
  g.A = reinterpret_cast<const float*>(A); g.W = nullptr; g.bias = bias; g.resid = resid;
  g.C = reinterpret_cast<float*>(C);
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N;
  g.alpha = alpha; g.act = act;
  if (dtype == 1) {
    WN_CHECK(c_mode == 0 || c_mode == 1, "gemm(lowp): bf16 operands give fp32 / bf16 C");
    g.a_bf16 = true; g.c_bf16 = c_mode == 1;
    return gemm_bf16_stored(g, W, (hipStream_t)stream);
  }
  if (dtype == 2) {
    WN_CHECK(c_mode == 0 || c_mode == 2, "gemm(lowp): MXFP8 operands give fp32 / MXFP8 C");
    g.fp8 = true; g.c_mx = c_mode == 2;
    g.a_scale = reinterpret_cast<const unsigned*>(a_scale); g.a_scale_pitch = M;
    g.w_scale = reinterpret_cast<const unsigned*>(w_scale); g.w_scale_pitch = N;
    g.c_scale = reinterpret_cast<unsigned*>(c_scale); g.c_scale_pitch = M;
    return gemm_mxfp8(g, W, (hipStream_t)stream);
  }
  set_error("gemm(lowp): unknown dtype");
  return -1;
}

int wn_op_mx_quantize(const float* x, int32_t rows, int32_t K, void* q, void* scale,
                      void* stream) {
  WN_CHECK(x && q && scale && rows > 0 && K > 0 && K % 128 == 0,
           "mx_quantize: null / empty / K % 128");
  return mx_quantize(x, K, rows, K, q, reinterpret_cast<unsigned*>(scale), rows,
                     (hipStream_t)stream);
}

int wn_op_ffn_fused(const float* X, const float* W1, const float* b1, const float* W2,
                    const float* b2, float* x, const float* ln_w, const float* ln_b,
                    float* y, int32_t M, int32_t D, int32_t F, int32_t act, float alpha,
                    float eps, void* stream) {
  WN_CHECK(X && W1 && b1 && W2 && b2 && x && ln_w && ln_b && y, "ffn_fused: null argument");
  WN_CHECK(M > 0 && (D == 256 || D == 512) && F > 0 && F % 64 == 0, "ffn_fused: shape");
  const int S = ffn_fused_split(M, D, F);
  WN_CHECK(S > 0, "ffn_fused: hidden size cannot be split for this M");
  static thread_local DevBuf part;
  WN_TRY(part.ensure((size_t)S * M * D * sizeof(float)));
  FfnArgs a;
  a.X = X; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.P = part.as<float>();
  a.M = M; a.D = D; a.F = F; a.S = S; a.act = act;
  WN_TRY(ffn_fused(a, (hipStream_t)stream));
  return ffn_reduce_ln(x, part.as<float>(), S, b2, alpha, ln_w, ln_b, nullptr, nullptr, y, M,
                       D, eps, 0, (hipStream_t)stream);
}

int wn_op_gemm_x6(const float* A, const float* W, const float* bias, const float* resid,
                  float* C, int32_t M, int32_t N, int32_t K, float alpha, int32_t act,
                  int32_t bm, int32_t reps, void* stream) {
  WN_CHECK(A && W && C && M > 0 && N > 0 && K > 0 && K % 16 == 0 && N % 4 == 0,
           "gemm_x6: shape");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf a3, w3;
  WN_TRY(w3.ensure(x6_bytes(N, K)));
  WN_TRY(x6_split(W, N, K, K, w3.as<char>(), s));
  X6Args a;
  if (tune().x6_af32 != 0 && (int64_t)M * K * 4 < ((int64_t)1 << 31)) {
    a.A = A; a.lda = K; a.a_bytes = (int64_t)M * K * 4;      // split in registers
  } else {
    WN_TRY(a3.ensure(x6_bytes(M, K)));
    WN_TRY(x6_split(A, M, K, K, a3.as<char>(), s));
    a.A3 = a3.as<char>();
  }
  a.B3 = w3.as<char>(); a.M = M; a.N = N; a.K = K; a.bm = bm;
  if (bm == 120) { a.bm = 128; a.nw = 8; }   // micro-benchmark: the 8-wave 128-row tile
  if (bm == 129) { a.bm = 128; a.nw = 4; }   // ... the 4-wave form
  a.bias = bias; a.resid = resid; a.ldr = N; a.alpha = alpha; a.act = act; a.C = C; a.ldc = N;
  for (int r = 0; r < (reps > 0 ? reps : 1); ++r) WN_TRY(gemm_x6(a, s));
  return 0;
}

int wn_op_ffn_x6(const float* X, const float* W1, const float* b1, const float* W2,
                 const float* b2, float* x, const float* ln_w, const float* ln_b, float* y,
                 int32_t M, int32_t D, int32_t F, int32_t act, float alpha, float eps,
                 int32_t reps, void* stream) {
  WN_CHECK(X && W1 && b1 && W2 && b2 && x && ln_w && ln_b && y, "ffn_x6: null argument");
  WN_CHECK(M > 0 && (D == 256 || D == 512) && F > 0 && F % 64 == 0, "ffn_x6: shape");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf x3, w13, w23, h3, part;
  if (tune().ffn_x6f != 0 && tune().x6_af32 == 0 && ffn_x6f_supported(M, D, F, act)) {
    // hidden tensor on chip (ffn_x6f.hip)
    FfnX6Args a;
    a.S = ffn_x6f_split(M, F);
    WN_TRY(w13.ensure(x6_bytes(F, D)));
    WN_TRY(w23.ensure(x6_bytes(D, F)));
    WN_TRY(part.ensure((size_t)a.S * M * D * sizeof(float)));
    WN_TRY(x6_split(W1, F, D, D, w13.as<char>(), s));
    WN_TRY(x6_split_perm(W2, D, F, F, w23.as<char>(), s));
    a.X = X; a.ldx = D; a.W13 = w13.as<char>(); a.W2p = w23.as<char>(); a.b1 = b1;
    a.P = part.as<float>(); a.M = M; a.D = D; a.F = F; a.act = act;
    if (tune().ffn_ximg == 2) {     // tests / tools: X handed over as its plane image
      WN_TRY(x3.ensure(x6_bytes(M, D)));
      WN_TRY(x6_split(X, M, D, D, x3.as<char>(), s));
      a.X3 = x3.as<char>(); a.X = nullptr;
    }
    for (int r = 0; r < (reps > 0 ? reps : 1); ++r) WN_TRY(ffn_x6f(a, s));
    return ffn_reduce_ln(x, part.as<float>(), a.S, b2, alpha, ln_w, ln_b, nullptr, nullptr, y, M,
                         D, eps, 0, s);
  }
  const int S = ffn_x6_split(M, F);
  WN_TRY(x3.ensure(x6_bytes(M, D)));
  WN_TRY(w13.ensure(x6_bytes(F, D)));
  WN_TRY(w23.ensure(x6_bytes(D, F)));
  WN_TRY(h3.ensure(x6_bytes(M, F)));
  WN_TRY(part.ensure((size_t)S * M * D * sizeof(float)));
  WN_TRY(x6_split(W1, F, D, D, w13.as<char>(), s));
  WN_TRY(x6_split(W2, D, F, F, w23.as<char>(), s));
  const bool af32 = tune().x6_af32 != 0 && (int64_t)M * F * 4 < ((int64_t)1 << 31);
  static thread_local DevBuf hf;
  if (af32) WN_TRY(hf.ensure((size_t)M * F * sizeof(float)));
  for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
    X6Args g1, g2;
    g1.B3 = w13.as<char>(); g1.M = M; g1.N = F; g1.K = D; g1.bias = b1; g1.act = act;
    g2.B3 = w23.as<char>(); g2.M = M; g2.N = D; g2.K = F;
    g2.epi = 1; g2.ksplit = S; g2.C = part.as<float>();
    if (af32) {
      g1.A = X; g1.lda = D; g1.a_bytes = (int64_t)M * D * 4;
      g1.epi = 0; g1.C = hf.as<float>(); g1.ldc = F;
      g2.A = hf.as<float>(); g2.lda = F; g2.a_bytes = (int64_t)M * F * 4;
    } else {
      WN_TRY(x6_split(X, M, D, D, x3.as<char>(), s));
      g1.A3 = x3.as<char>(); g1.epi = 2; g1.C3 = h3.as<char>();
      g2.A3 = h3.as<char>();
    }
    WN_TRY(gemm_x6(g1, s));
    WN_TRY(gemm_x6(g2, s));
    if (r + 1 < reps) continue;      // timing loops: the residual update only once
    WN_TRY(ffn_reduce_ln(x, part.as<float>(), S, b2, alpha, ln_w, ln_b, nullptr, nullptr, y,
                         M, D, eps, 0, s));
  }
  return 0;
}

int wn_op_gemm_x6r(const float* A, const float* W, const float* bias, float* x_inout,
                   const float* ln_w, const float* ln_b, float* y, float* C, int32_t M,
                   int32_t N, int32_t epi, float alpha, float eps, int32_t reps, void* stream) {
  WN_CHECK(A && W && M > 0 && gemm_x6r_supported(M, N, 256, epi), "gemm_x6r: shape");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf w3;
  WN_TRY(w3.ensure(x6_bytes(N, 256)));
  WN_TRY(x6_split(W, N, 256, 256, w3.as<char>(), s));
  X6RArgs a;
  a.A = A; a.lda = 256; a.W3 = w3.as<char>(); a.bias = bias; a.M = M; a.N = N; a.epi = epi;
  a.C = C; a.ldc = N; a.resid = x_inout; a.ldr = N; a.alpha = alpha; a.x_out = x_inout;
  a.ldx = N; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.y = y; a.ldy = N;
  for (int r = 0; r < (reps > 0 ? reps : 1); ++r) WN_TRY(gemm_x6r(a, s));
  return 0;
}

int wn_op_gemm_x6r512(const float* A, const float* W, const float* bias, float* x_inout,
                      const float* ln_w, const float* ln_b, float* y, const float* W2,
                      const float* bias2, float* C, int32_t M, int32_t N, int32_t epi, float alpha,
                      float eps, int32_t reps, void* stream) {
  WN_CHECK(A && W && M > 0 && gemm_x6r512_supported(M, N, epi), "gemm_x6r512: shape");
  WN_CHECK(epi != 3 || (W2 && C), "gemm_x6r512: the chained epilogue needs W2 and C");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf w3, w3b;
  WN_TRY(w3.ensure(x6_bytes(N, 512)));
  WN_TRY(x6_split(W, N, 512, 512, w3.as<char>(), s));
  X6RArgs a;
  a.A = A; a.lda = 512; a.K = 512; a.W3 = w3.as<char>(); a.bias = bias; a.M = M; a.N = N;
  a.epi = epi; a.C = C; a.ldc = epi == 3 ? 512 : N; a.resid = x_inout; a.ldr = N; a.alpha = alpha;
  a.x_out = x_inout; a.ldx = N; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.y = y; a.ldy = N;
  if (epi == 3) {
    WN_TRY(w3b.ensure(x6_bytes(1024, 512)));
    WN_TRY(x6_split(W2, 1024, 512, 512, w3b.as<char>(), s));
    a.W3b = w3b.as<char>(); a.bias2 = bias2;
  }
  for (int r = 0; r < (reps > 0 ? reps : 1); ++r) WN_TRY(gemm_x6r(a, s));
  return 0;
}

int wn_op_log_add(const double* a_dev, const double* b_dev, double* out_dev,
                  int32_t n, void* stream) {
  return log_add_pairs(a_dev, b_dev, out_dev, n, (hipStream_t)stream);
}

int wn_op_layernorm(const float* x, const float* w, const float* b, float* y,
                    int32_t M, int32_t D, float eps, void* stream) {
  return layernorm(x, D, w, b, y, D, M, D, eps, (hipStream_t)stream);
}

}  // extern "C"
