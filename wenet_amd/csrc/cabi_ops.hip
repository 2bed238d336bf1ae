// C ABI (include/wenet_amd.h): the operator hooks (wn_op_*) the tests and tools call kernels
// through.
#include "model_state.h"
#include "x6.h"

namespace wn {
namespace {

// wn_op_conv1: the plane image cmvn_conv1_x3_kernel wrote (one image row per pixel, even f1
// first) back to fp32 h0 + h1 + h2 in the [frame][F1][C] layout; one thread per (pixel, 8 channels)
__global__ __launch_bounds__(256) void conv1_image_unpack_kernel(
    const char* __restrict__ img, int tiles, const int* __restrict__ t1_off,
    const int* __restrict__ t1_len, int F1, int C, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int n = t1_len[b] * F1 * (C / 8);
  const int ne = (F1 + 1) / 2;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int cg = i % (C / 8), px = i / (C / 8);
    const int fr = px / F1, pos = px - fr * F1;
    const int f1 = pos < ne ? 2 * pos : 2 * (pos - ne) + 1;
    const int row = (t1_off[b] + fr) * F1;
    const char* src = img + x3_piece(cg >> 1, tiles, row + pos, cg & 1);
    const bf16x8 p0 = *reinterpret_cast<const bf16x8*>(src);
    const bf16x8 p1 = *reinterpret_cast<const bf16x8*>(src + X3_REC);
    const bf16x8 p2 = *reinterpret_cast<const bf16x8*>(src + 2 * X3_REC);
    float* o = out + ((int64_t)row + f1) * C + cg * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ((float)p0[e] + (float)p1[e]) + (float)p2[e];
  }
}

// host descriptor arrays of a hook call -> one device buffer (the copy is complete on return)
int upload_ints(DevBuf& buf, const std::vector<int>& v, hipStream_t s) {
  WN_TRY(buf.ensure(v.size() * sizeof(int)));
  WN_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

// offsets / lengths of a packed ragged batch: inside [0, rows), ascending, disjoint
bool packed_ok(const int32_t* off, const int32_t* len, int n, int rows) {
  int64_t end = 0;
  for (int i = 0; i < n; ++i) {
    if (len[i] < 0 || off[i] < end || (int64_t)off[i] + len[i] > rows) return false;
    end = (int64_t)off[i] + len[i];
  }
  return true;
}

// a device index array of a hook call that a kernel dereferences (path rows, token ids): read
// back and checked on the host, columns [0, cols) of every row inside [0, hi), before any launch
int device_ints_in_range(const int32_t* dev, int rows, int ld, int cols, int hi, hipStream_t s,
                         bool* ok) {
  std::vector<int> h((size_t)rows * ld);
  WN_HIP(hipMemcpyAsync(h.data(), dev, h.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  *ok = true;
  for (int r = 0; r < rows; ++r)
    for (int j = 0; j < cols; ++j) {
      const int v = h[(size_t)r * ld + j];
      if (v < 0 || v >= hi) *ok = false;
    }
  return 0;
}

// the widths a row kernel's launcher has a case for
bool width_in(int D, std::initializer_list<int> widths) {
  return std::find(widths.begin(), widths.end(), D) != widths.end();
}

}  // namespace
}  // namespace wn

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

int wn_op_gemm_ex(const wn_gemm_op* op, int32_t* route_out, void* stream) {
  WN_CHECK(op && route_out, "gemm_ex: null argument");
  const wn_gemm_op& o = *op;
  WN_CHECK(o.A && o.W && o.C, "gemm_ex: null operand");
  WN_CHECK(o.M > 0 && o.N > 0 && o.K > 0, "gemm_ex: empty problem");
  WN_CHECK(o.precision == PREC_F32 || o.precision == PREC_BF16, "gemm_ex: precision");
  WN_CHECK(o.act >= ACT_NONE && o.act <= ACT_GELU, "gemm_ex: activation");
  WN_CHECK(o.glu == 0 || o.glu == 1, "gemm_ex: glu is 0 or 1");
  WN_CHECK(o.K % 32 == 0, "gemm_ex: K must be a multiple of 32");
  WN_CHECK(reinterpret_cast<uintptr_t>(o.A) % 16 == 0 && reinterpret_cast<uintptr_t>(o.W) % 16 == 0,
           "gemm_ex: A and W must be 16-byte aligned");
  const bool conv = o.a_row_off != nullptr;
  if (o.glu) {
    WN_CHECK(o.N % 64 == 0, "gemm_ex(GLU): N must be a multiple of 64");
    // (an activation, a residual or alpha with it: gemm_f32's own refusal)
    WN_CHECK(!conv, "gemm_ex(GLU): no gathered A with the GLU epilogue");
  }
  WN_CHECK(o.ldc >= (o.glu ? o.N / 2 : o.N), "gemm_ex: ldc is smaller than the output row");
  WN_CHECK(o.resid == nullptr || o.ldr >= o.N, "gemm_ex: ldr is smaller than N");
  WN_CHECK(o.a_elems > 0, "gemm_ex: a_elems");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf rows;
  if (conv) {
    WN_CHECK(o.act != ACT_SILU, "gemm_ex: no SiLU epilogue with a gathered A");
    WN_CHECK(o.conv_C > 0 && o.conv_C % 32 == 0 && (o.K == 9 * o.conv_C || o.K == o.conv_C),
             "gemm_ex(conv): K must be 9*C (3x3 taps) or C (gathered rows), C % 32 == 0");
    WN_CHECK(o.conv_sy >= 0 && o.conv_sx >= 0 && o.conv_sy % 4 == 0 && o.conv_sx % 4 == 0,
             "gemm_ex(conv): tap strides must be non-negative multiples of 4 floats");
    const int64_t last_tap = o.K == o.conv_C ? 0 : 2 * o.conv_sy + 2 * o.conv_sx;
    WN_CHECK(last_tap + o.conv_C <= o.a_elems, "gemm_ex(conv): a gathered read past a_elems");
    for (int r = 0; r < o.M; ++r) {
      WN_CHECK(o.a_row_off[r] >= 0 && o.a_row_off[r] % 4 == 0,
               "gemm_ex(conv): a row offset is negative or not a multiple of 4 floats");
      WN_CHECK(o.a_row_off[r] <= o.a_elems - last_tap - o.conv_C,
               "gemm_ex(conv): a gathered read past a_elems");
    }
    WN_TRY(rows.ensure((size_t)o.M * sizeof(int64_t)));
    WN_HIP(hipMemcpyAsync(rows.p, o.a_row_off, (size_t)o.M * sizeof(int64_t),
                          hipMemcpyHostToDevice, s));
    WN_HIP(hipStreamSynchronize(s));
  } else {
    WN_CHECK(o.lda % 4 == 0, "gemm_ex: lda must be a multiple of 4 floats");
    WN_CHECK(o.lda >= o.K, "gemm_ex: lda is smaller than K");
    WN_CHECK((int64_t)(o.M - 1) * o.lda + o.K <= o.a_elems, "gemm_ex: a read past a_elems");
  }
  GemmArgs g;
  g.A = o.A; g.W = o.W; g.bias = o.bias; g.resid = o.resid; g.C = o.C;
  g.M = o.M; g.N = o.N; g.K = o.K; g.lda = o.lda; g.ldc = o.ldc; g.ldr = o.ldr;
  g.alpha = o.alpha; g.act = o.act; g.glu = o.glu != 0;
  if (conv) {
    g.a_row_off = rows.as<int64_t>(); g.conv_C = o.conv_C;
    g.conv_sy = o.conv_sy; g.conv_sx = o.conv_sx;
  }
  const int saved = t_gemm_prec;
  t_gemm_prec = o.precision;
  t_gemm_route = 0;
  const int r = gemm_f32(g, s);
  t_gemm_prec = saved;
  *route_out = t_gemm_route;
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

int wn_op_gemm_skinny(const float* A, const float* W, const float* bias, const float* resid,
                      float* C, int32_t M, int32_t N, int32_t K, int32_t act, int32_t w_bf16,
                      int32_t split_k, void* stream) {
  // test hook of the decoder step's GEMM: with w_bf16 the weights are converted to a bf16 image
  // in a scratch buffer first (the model path reads the handle's converted weight slab)
  WN_CHECK(A && W && C && M > 0 && N > 0 && K > 0, "gemm_skinny: null / empty");
  WN_CHECK(M <= 256, "gemm_skinny: M must be in [1, 256]");
  WN_CHECK(K % 32 == 0 && split_k >= 0, "gemm_skinny: K must be a multiple of 32, split_k >= 0");
  static thread_local DevBuf w16, part;
  hipStream_t s = (hipStream_t)stream;
  SkinnyArgs g;
  g.A = A; g.lda = K; g.bias = bias; g.resid = resid; g.ldr = N; g.C = C; g.ldc = N;
  g.M = M; g.N = N; g.K = K; g.act = act;
  if (w_bf16) {
    WN_TRY(w16.ensure((size_t)N * K * 2));
    WN_TRY(convert_f32_to_bf16(W, w16.p, (int64_t)N * K, s));
    g.Wh = w16.p;
  } else {
    g.W = W;
  }
  const int tiles = w_bf16 ? cdiv(K, 64) : K / 32;
  g.split_k = std::min(split_k > 0 ? split_k : gemm_skinny_split(N, K, w_bf16 != 0), tiles);
  WN_TRY(part.ensure(gemm_skinny_ws_bytes(M, N, g.split_k)));
  g.part = part.as<float>(); g.part_bytes = part.cap;
  return gemm_skinny(g, s);
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

int wn_op_gemm_lowp_ex(const wn_gemm_lowp_op* op, int32_t* route_out, void* stream) {
  WN_CHECK(op && route_out, "gemm_lowp_ex: null argument");
  const wn_gemm_lowp_op& o = *op;
  auto al = [](const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
  WN_CHECK(o.A && o.W && o.C, "gemm_lowp_ex: null operand");
  WN_CHECK(o.M > 0 && o.N > 0 && o.K > 0, "gemm_lowp_ex: empty problem");
  WN_CHECK(o.dtype == 1 || o.dtype == 2, "gemm_lowp_ex: dtype is 1 (bf16) or 2 (MXFP8)");
  WN_CHECK(o.c_mode >= 0 && o.c_mode <= 2, "gemm_lowp_ex: c_mode is 0, 1 or 2");
  WN_CHECK(o.act >= ACT_NONE && o.act <= ACT_GELU, "gemm_lowp_ex: activation");
  WN_CHECK(o.glu == 0 || o.glu == 1, "gemm_lowp_ex: glu is 0 or 1");
  const bool fp8 = o.dtype == 2;
  const int esz = fp8 ? 1 : 2;
  WN_CHECK(o.c_mode != 1 || !fp8, "gemm_lowp_ex: a bf16 C needs bf16 operands");
  WN_CHECK(o.c_mode != 2 || fp8, "gemm_lowp_ex: an MXFP8 C needs MXFP8 operands");
  WN_CHECK(o.c_mode == 0 || o.resid == nullptr,
           "gemm_lowp_ex: no residual with a bf16 or MXFP8 C");
  if (o.glu) {
    WN_CHECK(!fp8 && o.c_mode == 0, "gemm_lowp_ex(GLU): bf16 operands and an fp32 C only");
    WN_CHECK(o.N % 64 == 0, "gemm_lowp_ex(GLU): N must be a multiple of 64");
    WN_CHECK(o.act == ACT_NONE && o.resid == nullptr && o.alpha == 1.0f,
             "gemm_lowp_ex(GLU): no activation, residual or alpha with the GLU epilogue");
  }
  WN_CHECK(al(o.A, 16) && al(o.W, 16), "gemm_lowp_ex: A and W must be 16-byte aligned");
  WN_CHECK(al(o.C, 16), "gemm_lowp_ex: C must be 16-byte aligned");
  WN_CHECK(al(o.bias, 16) && al(o.resid, 16),
           "gemm_lowp_ex: bias and residual must be 16-byte aligned");
  if (fp8) {
    WN_CHECK(o.K % 128 == 0 && o.K >= 256,
             "gemm_lowp_ex(MXFP8): K must be a multiple of 128, at least 256");
    WN_CHECK(o.N % 8 == 0, "gemm_lowp_ex(MXFP8): N must be a multiple of 8");
    WN_CHECK(o.c_mode != 2 || o.N % 32 == 0,
             "gemm_lowp_ex(MXFP8 C): N must be a multiple of 32");
    WN_CHECK(o.lda % 16 == 0, "gemm_lowp_ex(MXFP8): lda must be a multiple of 16 elements");
  } else {
    WN_CHECK(o.K % 32 == 0, "gemm_lowp_ex: K must be a multiple of 32");
    WN_CHECK(o.lda % 8 == 0, "gemm_lowp_ex: lda must be a multiple of 8 elements");
  }
  WN_CHECK(o.lda >= o.K, "gemm_lowp_ex: lda is smaller than K");
  const int n_out = o.glu ? o.N / 2 : o.N;
  WN_CHECK(o.ldc >= n_out, "gemm_lowp_ex: ldc is smaller than the output row");
  WN_CHECK(o.ldc % (o.c_mode == 2 ? 16 : o.c_mode == 1 ? 8 : 4) == 0,
           "gemm_lowp_ex: ldc must be a multiple of 4 (fp32 C), 8 (bf16 C) or 16 (MXFP8 C)");
  if (o.resid) {
    WN_CHECK(o.ldr >= o.N, "gemm_lowp_ex: ldr is smaller than N");
    WN_CHECK(o.ldr % 4 == 0, "gemm_lowp_ex: ldr must be a multiple of 4 floats");
  }
  WN_CHECK(((int64_t)(o.M - 1) * o.lda + o.K) * esz <= o.a_bytes,
           "gemm_lowp_ex: a read past a_bytes");
  WN_CHECK((int64_t)o.N * o.K * esz <= o.w_bytes, "gemm_lowp_ex: a read past w_bytes");
  if (fp8) {
    const int64_t nk = o.K / 128;
    WN_CHECK(o.a_scale && o.w_scale, "gemm_lowp_ex(MXFP8): null block scales");
    WN_CHECK(al(o.a_scale, 4) && al(o.w_scale, 4) && al(o.c_scale, 4),
             "gemm_lowp_ex(MXFP8): scale arrays must be 4-byte aligned");
    WN_CHECK(o.a_scale_pitch >= o.M, "gemm_lowp_ex(MXFP8): a_scale_pitch is smaller than M");
    WN_CHECK(o.w_scale_pitch >= o.N, "gemm_lowp_ex(MXFP8): w_scale_pitch is smaller than N");
    WN_CHECK(nk * o.a_scale_pitch * 4 <= o.a_scale_bytes,
             "gemm_lowp_ex(MXFP8): a read past a_scale_bytes");
    WN_CHECK(nk * o.w_scale_pitch * 4 <= o.w_scale_bytes,
             "gemm_lowp_ex(MXFP8): a read past w_scale_bytes");
    if (o.c_mode == 2) {
      WN_CHECK(o.c_scale, "gemm_lowp_ex(MXFP8 C): null C scales");
      WN_CHECK(o.c_scale_pitch >= o.M, "gemm_lowp_ex(MXFP8 C): c_scale_pitch is smaller than M");
      WN_CHECK((int64_t)cdiv(o.N, 128) * o.c_scale_pitch * 4 <= o.c_scale_bytes,
               "gemm_lowp_ex(MXFP8 C): a store past c_scale_bytes");
    }
  }
  GemmArgs g;
  g.A = reinterpret_cast<const float*>(o.A); g.W = nullptr; g.bias = o.bias; g.resid = o.resid;
  g.C = reinterpret_cast<float*>(o.C);
  g.M = o.M; g.N = o.N; g.K = o.K; g.lda = o.lda; g.ldc = o.ldc; g.ldr = o.ldr;
  g.alpha = o.alpha; g.act = o.act; g.glu = o.glu != 0;
  t_gemm_route = 0;
  int r;
  if (fp8) {
    g.fp8 = true; g.c_mx = o.c_mode == 2;
    g.a_scale = reinterpret_cast<const unsigned*>(o.a_scale); g.a_scale_pitch = o.a_scale_pitch;
    g.w_scale = reinterpret_cast<const unsigned*>(o.w_scale); g.w_scale_pitch = o.w_scale_pitch;
    g.c_scale = reinterpret_cast<unsigned*>(o.c_scale); g.c_scale_pitch = o.c_scale_pitch;
    WN_CHECK(gemm_bf16p_supported(g),
             "gemm_lowp_ex(MXFP8): a shape the pipelined kernel does not take (operand of 2 GiB?)");
    r = gemm_mxfp8(g, o.W, (hipStream_t)stream);
  } else {
    g.a_bf16 = true; g.c_bf16 = o.c_mode == 1;
    r = gemm_bf16_stored(g, o.W, (hipStream_t)stream);
  }
  *route_out = t_gemm_route;
  return r;
}

int wn_op_mx_quantize_ex(const float* x, int32_t ld, int32_t rows, int32_t K, void* q,
                         void* scale, int32_t pitch, void* stream) {
  WN_CHECK(x && q && scale, "mx_quantize_ex: null argument");
  WN_CHECK(rows > 0 && K > 0, "mx_quantize_ex: empty problem");
  WN_CHECK(K % 32 == 0, "mx_quantize_ex: K must be a multiple of 32");
  WN_CHECK(ld % 4 == 0, "mx_quantize_ex: ld must be a multiple of 4 floats");
  WN_CHECK(ld >= K, "mx_quantize_ex: ld is smaller than K");
  WN_CHECK(pitch >= rows, "mx_quantize_ex: pitch is smaller than rows");
  WN_CHECK(reinterpret_cast<uintptr_t>(x) % 16 == 0, "mx_quantize_ex: x must be 16-byte aligned");
  WN_CHECK(reinterpret_cast<uintptr_t>(q) % 4 == 0 && reinterpret_cast<uintptr_t>(scale) % 4 == 0,
           "mx_quantize_ex: q and scale must be 4-byte aligned");
  return mx_quantize(x, ld, rows, K, q, reinterpret_cast<unsigned*>(scale), pitch,
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

int wn_op_attention(const wn_attention_op* op, int32_t* form_out, void* stream) {
  WN_CHECK(op && form_out, "attention: null argument");
  const wn_attention_op& o = *op;
  WN_CHECK(o.Q && o.K && o.V && o.O && o.q_off && o.q_len && o.kv_off && o.kv_len,
           "attention: null argument");
  WN_CHECK(o.n_seq > 0 && o.n_seq < 32768 && o.n_heads > 0 && o.n_heads < 256,
           "attention: n_seq / n_heads");
  const int H = o.n_heads, d = H * 64;
  WN_CHECK(o.precision == PREC_F32 || o.precision == PREC_BF16, "attention: precision");
  WN_CHECK(o.ldq % 4 == 0 && o.ldk % 4 == 0 && o.ldv % 4 == 0 && o.ldo % 4 == 0,
           "attention: strides must be multiples of 4 elements");
  WN_CHECK(o.ldq >= d && o.ldk >= d && o.ldv >= d && o.ldo >= d,
           "attention: a stride is smaller than n_heads * 64");
  WN_CHECK(o.q_rows > 0 && o.kv_rows > 0, "attention: empty buffers");
  WN_CHECK(o.mask_mode >= 0 && o.mask_mode <= 2, "attention: mask mode");
  WN_CHECK(o.mask_mode != 2 || o.chunk_size > 0, "attention: chunk size");
  WN_CHECK(packed_ok(o.q_off, o.q_len, o.n_seq, o.q_rows),
           "attention: query rows outside the buffer, unordered or overlapping");
  bool self_attn = true;
  int max_q = 0;
  for (int s = 0; s < o.n_seq; ++s) {
    WN_CHECK(o.kv_len[s] >= 0 && o.kv_off[s] >= 0 &&
                 (int64_t)o.kv_off[s] + o.kv_len[s] <= o.kv_rows,
             "attention: key rows outside the buffer");
    WN_CHECK(o.q_len[s] == 0 || o.kv_len[s] > 0, "attention: queries without keys");
    self_attn = self_attn && o.q_off[s] == o.kv_off[s] && o.q_len[s] == o.kv_len[s];
    max_q = std::max(max_q, o.q_len[s]);
  }
  WN_CHECK(max_q > 0, "attention: empty");
  const bool fold = (o.flags & WN_ATTN_FOLD) != 0, prefold = (o.flags & WN_ATTN_PREFOLD) != 0;
  const bool in16 = (o.flags & WN_ATTN_QKV_BF16) != 0, o16 = (o.flags & WN_ATTN_O_BF16) != 0;
  WN_CHECK(!(fold && prefold), "attention: fold and prefold exclude each other");
  WN_CHECK(!((fold || prefold) && !o.P), "attention: folding needs the position table");
  if (o.P) {
    WN_CHECK(o.bias_u && o.bias_v, "attention: rel-pos needs bias_u and bias_v");
    WN_CHECK(o.ldp % 4 == 0 && o.ldp >= d && o.p_rows > 0, "attention: position table stride");
    for (int s = 0; s < o.n_seq; ++s) {
      const int po = o.p_off ? o.p_off[s] : 0;
      WN_CHECK(po >= 0 && (int64_t)po + o.kv_len[s] <= o.p_rows,
               "attention: position rows outside the table");
    }
  }
  WN_CHECK(!(in16 || o16) || o.precision == PREC_BF16,
           "attention: bf16 matrices only with precision 1");
  WN_CHECK(!in16 || (!o.P && o.ldq == d && o.ldk == d && o.ldv == d),
           "attention: bf16 Q/K/V without rel-pos and with dense rows only");
  WN_CHECK(!prefold || (o.precision == PREC_F32 && (d == 256 || d == 512) && self_attn),
           "attention: prefold needs fp32, d = 256 / 512, self attention");
  WN_CHECK(o.x6_galign == 0 || o.x6_galign == 1, "attention: x6_galign");

  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, img, q16, kfold, kb;
  // descriptor block: q_off | q_len | kv_off | kv_len | p_off | row_utt (of the K / V rows)
  const int n = o.n_seq;
  std::vector<int> h((size_t)5 * n + o.kv_rows, -1);
  for (int i = 0; i < n; ++i) {
    h[i] = o.q_off[i]; h[n + i] = o.q_len[i]; h[2 * n + i] = o.kv_off[i];
    h[3 * n + i] = o.kv_len[i]; h[4 * n + i] = o.p_off ? o.p_off[i] : 0;
    for (int t = 0; t < o.kv_len[i]; ++t) h[5 * n + o.kv_off[i] + t] = i;
  }
  WN_TRY(upload_ints(desc, h, s));
  const int* dd = desc.as<int>();
  AttnArgs a;
  a.Q = (const float*)o.Q; a.K = (const float*)o.K; a.V = (const float*)o.V;
  a.ldq = o.ldq; a.ldk = o.ldk; a.ldv = o.ldv;
  a.O = (float*)o.O; a.ldo = o.ldo; a.o_bf16 = o16;
  a.q_off = dd; a.q_len = dd + n;
  // self attention hands the launchers ONE offset / length array, as the encoder does
  a.kv_off = self_attn ? a.q_off : dd + 2 * n;
  a.kv_len = self_attn ? a.q_len : dd + 3 * n;
  a.n_seq = n; a.n_heads = H; a.max_q_len = max_q;
  a.mask_mode = o.mask_mode; a.chunk_size = o.chunk_size; a.left_chunks = o.left_chunks;
  a.scale = o.scale;
  if (o.P && !prefold) {
    a.P = o.P; a.ldp = o.ldp; a.p_off = o.p_off ? dd + 4 * n : nullptr;
    a.bias_u = o.bias_u; a.bias_v = o.bias_v; a.fold = fold;
  }
  if (prefold) {
    // the fold as its own pass over a copy of the key rows (tune attn_fold = 2 in the encoder)
    WN_TRY(kfold.ensure((size_t)o.kv_rows * d * sizeof(float)));
    WN_TRY(kb.ensure((size_t)o.kv_rows * H * sizeof(float)));
    WN_HIP(hipMemcpy2DAsync(kfold.p, (size_t)d * 4, o.K, (size_t)o.ldk * 4, (size_t)d * 4,
                            o.kv_rows, hipMemcpyDeviceToDevice, s));
    WN_TRY(relpos_fold(kfold.as<float>(), d, o.P, o.ldp, o.bias_u, o.bias_v, dd + 5 * n,
                       dd + 2 * n, o.p_off ? dd + 4 * n : nullptr, kb.as<float>(), H, o.kv_rows,
                       d, s));
    a.K = kfold.as<float>(); a.ldk = d; a.kbias = kb.as<float>();
  }
  if (in16) {
    const size_t nq = (size_t)o.q_rows * d, nk = (size_t)o.kv_rows * d;
    WN_TRY(q16.ensure((nq + 2 * nk) * 2));
    char* base = q16.as<char>();
    WN_TRY(convert_f32_to_bf16((const float*)o.Q, base, (int64_t)nq, s));
    WN_TRY(convert_f32_to_bf16((const float*)o.K, base + nq * 2, (int64_t)nk, s));
    WN_TRY(convert_f32_to_bf16((const float*)o.V, base + (nq + nk) * 2, (int64_t)nk, s));
    a.Q = (const float*)base; a.K = (const float*)(base + nq * 2);
    a.V = (const float*)(base + (nq + nk) * 2);
    a.qkv_bf16 = true;
  }
  if (o.precision == PREC_F32 && self_attn && a.P && a.fold) {
    // the six-product form's scratch image (the pack pass of this launch fills it)
    WN_TRY(img.ensure(attention_x6_image_bytes(o.kv_rows, n, H)));
    a.x6_img = img.p; a.x6_img_bytes = img.cap; a.x6_rows = o.kv_rows;
    if (o.x6_galign) { a.x6_galign = 1; a.row_utt = dd + 5 * n; }
  }
  const int saved = t_gemm_prec;
  t_gemm_prec = o.precision;
  *form_out = attention_form(a).code();
  const int r = attention(a, s);
  t_gemm_prec = saved;
  return r;
}

int wn_op_dwconv(const float* x, int32_t ldx, const float* wt, const float* bias,
                 const float* cpad, const float* ln_w, const float* ln_b, int32_t norm_mode,
                 float* y, int32_t ldy, const int32_t* off, const int32_t* len, int32_t B,
                 int32_t M, int32_t D, int32_t K, int32_t causal, int32_t t_max, float eps,
                 void* stream) {
  WN_CHECK(x && wt && bias && cpad && ln_w && ln_b && y && off && len, "dwconv: null argument");
  WN_CHECK(D == 64 || D == 128 || D == 256 || D == 512 || D == 768 || D == 1024 || D == 1280 ||
               D == 2560,
           "dwconv: unsupported width " + std::to_string(D));
  WN_CHECK(M > 0 && B > 0 && K >= 1 && K <= 255, "dwconv: M / B / K");
  WN_CHECK(causal != 0 || K % 2 == 1, "dwconv: a symmetric kernel has an odd size");
  WN_CHECK(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= D && ldy >= D, "dwconv: strides");
  WN_CHECK(norm_mode == 0 || norm_mode == 1, "dwconv: norm mode");
  WN_CHECK(packed_ok(off, len, B, M), "dwconv: rows outside the buffer, unordered or overlapping");
  std::vector<int> h((size_t)2 * B + M, -1);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(len[b] <= t_max, "dwconv: t_max is smaller than a length");
    h[b] = off[b]; h[B + b] = len[b];
    for (int t = 0; t < len[b]; ++t) h[2 * B + off[b] + t] = b;
  }
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(upload_ints(desc, h, s));
  DwConvArgs a;
  a.x = x; a.ldx = ldx; a.wt = wt; a.bias = bias; a.cpad = cpad; a.ln_w = ln_w; a.ln_b = ln_b;
  a.norm_mode = norm_mode; a.y = y; a.ldy = ldy;
  a.off = desc.as<int>(); a.len = a.off + B; a.row_utt = a.off + 2 * B;
  a.M = M; a.D = D; a.K = K; a.causal = causal != 0; a.t_max = t_max; a.eps = eps;
  return dwconv_ln_silu(a, s);
}

int wn_op_conv1(const float* feats, const float* mean, const float* istd, const float* w,
                const float* bias, float* out, const int32_t* t1_off, const int32_t* t1_len,
                int32_t B, int32_t T, int32_t F, int32_t C, int32_t out_rows,
                int32_t plane_image, void* stream) {
  WN_CHECK(feats && w && bias && out && t1_off && t1_len, "conv1: null argument");
  WN_CHECK((mean == nullptr) == (istd == nullptr), "conv1: mean and istd come together");
  WN_CHECK(F >= 3 && F <= 128, "conv1: feature dim outside [3, 128]");
  WN_CHECK(B > 0 && B < 65536 && T >= 3 && C > 0 && out_rows > 0, "conv1: B / T / C");
  const int F1 = (F - 1) / 2;
  WN_CHECK((int64_t)out_rows * F1 < ((int64_t)1 << 30), "conv1: too many pixels");
  WN_CHECK(packed_ok(t1_off, t1_len, B, out_rows),
           "conv1: frames outside the buffer, unordered or overlapping");
  int max_t1 = 0;
  std::vector<int> h((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    WN_CHECK(2 * (int64_t)t1_len[b] + 1 <= T, "conv1: T is too short for t1_len");
    h[b] = t1_off[b]; h[B + b] = t1_len[b];
    max_t1 = std::max(max_t1, t1_len[b]);
  }
  WN_CHECK(max_t1 > 0, "conv1: empty");
  WN_CHECK(!plane_image || (F1 <= 64 && C % 32 == 0), "conv1: plane image shape");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, img;
  WN_TRY(upload_ints(desc, h, s));
  Conv1Args a;
  a.feats = feats; a.mean = mean; a.istd = istd; a.w = w; a.bias = bias; a.out = out;
  a.t1_off = desc.as<int>(); a.t1_len = a.t1_off + B;
  a.B = B; a.T = T; a.F = F; a.F1 = F1; a.C = C; a.max_t1 = max_t1;
  if (plane_image) {
    a.tiles = cdiv(out_rows * F1, 32);
    WN_TRY(img.ensure(x6_bytes(a.tiles * 32, C)));
    a.out3 = img.as<char>();
    WN_TRY(cmvn_conv1_relu(a, s));
    hipLaunchKernelGGL(conv1_image_unpack_kernel, dim3(cdiv(max_t1 * F1 * (C / 8), 256), B),
                       dim3(256), 0, s, a.out3, a.tiles, a.t1_off, a.t1_len, F1, C, out);
    WN_HIP(hipGetLastError());
    return 0;
  }
  return cmvn_conv1_relu(a, s);
}

int wn_op_attention_relshift(const float* Q, const float* K, const float* V, int32_t ldq,
                             int32_t ldk, int32_t ldv, int32_t rows, const float* P,
                             int32_t ldp, int32_t p_rows, int32_t p_center, const float* bias_u,
                             const float* bias_v, float* O, int32_t ldo, const int32_t* off,
                             const int32_t* len, int32_t n_seq, int32_t n_heads, float scale,
                             void* stream) {
  WN_CHECK(Q && K && V && P && bias_u && bias_v && O && off && len,
           "attention_relshift: null argument");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && n_heads > 0 && n_heads < 65536,
           "attention_relshift: n_seq / n_heads");
  const int d = n_heads * 64;
  WN_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ldp % 4 == 0,
           "attention_relshift: strides must be multiples of 4 elements");
  WN_CHECK(ldq >= d && ldk >= d && ldv >= d && ldo >= d && ldp >= d,
           "attention_relshift: a stride is smaller than n_heads * 64");
  WN_CHECK(rows > 0 && p_rows > 0, "attention_relshift: empty buffers");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           "attention_relshift: rows outside the buffer, unordered or overlapping");
  int max_len = 0;
  std::vector<int> h((size_t)2 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i];
    max_len = std::max(max_len, len[i]);
  }
  WN_CHECK(max_len > 0, "attention_relshift: empty");
  WN_CHECK(p_center >= max_len - 1 && (int64_t)p_center + max_len - 1 < p_rows,
           "attention_relshift: a sequence is longer than the position table covers");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(upload_ints(desc, h, s));
  RelShiftAttnArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.P = P; a.ldp = ldp; a.p_center = p_center; a.p_rows = p_rows;
  a.bias_u = bias_u; a.bias_v = bias_v; a.O = O; a.ldo = ldo;
  a.off = desc.as<int>(); a.len = a.off + n_seq;
  a.n_seq = n_seq; a.n_heads = n_heads; a.max_len = max_len; a.scale = scale;
  return attention_relshift(a, s);
}

int wn_op_attention_sqshift(const float* Q, const float* K, const float* V, int32_t ldq,
                            int32_t ldk, int32_t ldv, int32_t rows, const float* P, int32_t ldp,
                            int32_t p_rows, const float* bias_u, const float* bias_v, float* O,
                            int32_t ldo, const int32_t* off, const int32_t* len, int32_t n_seq,
                            int32_t n_heads, float scale, void* stream) {
  WN_CHECK(Q && K && V && P && bias_u && bias_v && O && off && len,
           "attention_sqshift: null argument");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && n_heads > 0 && n_heads < 65536,
           "attention_sqshift: n_seq / n_heads");
  const int d = n_heads * 64;
  WN_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ldp % 4 == 0,
           "attention_sqshift: strides must be multiples of 4 elements");
  WN_CHECK(ldq >= d && ldk >= d && ldv >= d && ldo >= d && ldp >= d,
           "attention_sqshift: a stride is smaller than n_heads * 64");
  WN_CHECK(rows > 0 && p_rows > 0, "attention_sqshift: empty buffers");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           "attention_sqshift: rows outside the buffer, unordered or overlapping");
  int max_len = 0;
  std::vector<int> h((size_t)2 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i];
    max_len = std::max(max_len, len[i]);
  }
  WN_CHECK(max_len > 0, "attention_sqshift: empty");
  WN_CHECK(p_rows >= max_len,
           "attention_sqshift: a sequence is longer than the position table covers");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(upload_ints(desc, h, s));
  SqShiftAttnArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.P = P; a.ldp = ldp; a.p_rows = p_rows;
  a.bias_u = bias_u; a.bias_v = bias_v; a.O = O; a.ldo = ldo;
  a.off = desc.as<int>(); a.len = a.off + n_seq;
  a.n_seq = n_seq; a.n_heads = n_heads; a.max_len = max_len; a.scale = scale;
  return attention_sqshift(a, s);
}

// the layouts both time hooks share: off | len | half-rate off on the device; the half-rate rows
// (len + 1) / 2 from off2 must lie inside rows2, ascending and disjoint
static int time_hook_layout(const int32_t* off, const int32_t* len, const int32_t* off2, int n_seq,
                            int rows, int rows2, DevBuf& desc, int* max_len, hipStream_t s,
                            const char* who) {
  const std::string w(who);
  WN_CHECK(off && len && off2, w + ": null argument");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && rows > 0 && rows2 > 0, w + ": n_seq / rows");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           w + ": rows outside the buffer, unordered or overlapping");
  std::vector<int> h((size_t)3 * n_seq), len2(n_seq);
  *max_len = 0;
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i]; h[2 * n_seq + i] = off2[i];
    len2[i] = (len[i] + 1) / 2;
    *max_len = std::max(*max_len, len[i]);
  }
  WN_CHECK(packed_ok(off2, len2.data(), n_seq, rows2),
           w + ": half-rate rows outside the buffer, unordered or overlapping");
  WN_CHECK(*max_len > 0, w + ": empty");
  return upload_ints(desc, h, s);
}

int wn_op_time_reduce(const float* x, int32_t ldx, int32_t rows, int32_t C, const float* wt,
                      const float* bias, int32_t K, int32_t pad, float* y, int32_t ldy,
                      int32_t out_rows, const int32_t* off, const int32_t* len,
                      const int32_t* out_off, int32_t n_seq, void* stream) {
  WN_CHECK(x && wt && bias && y, "time_reduce: null argument");
  WN_CHECK(C > 0 && C % 64 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0,
           "time_reduce: C must be a multiple of 64, strides multiples of 4 elements, >= C");
  WN_CHECK((K == 5 && pad == 3) || (K == 1 && pad == 0),
           "time_reduce: 5 taps with padding 3 (conv1d) or 1 tap without padding (stream)");
  WN_CHECK(rows > 0 && out_rows > 0, "time_reduce: empty buffers");
  WN_CHECK(y + (int64_t)out_rows * ldy <= x || x + (int64_t)rows * ldx <= y,
           "time_reduce: y overlaps x");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  int max_len = 0;
  WN_TRY(time_hook_layout(off, len, out_off, n_seq, rows, out_rows, desc, &max_len, s,
                          "time_reduce"));
  TimeReduceArgs a;
  a.x = x; a.ldx = ldx; a.wt = wt; a.bias = bias; a.y = y; a.ldy = ldy;
  a.off = desc.as<int>(); a.len = a.off + n_seq; a.off2 = a.off + 2 * n_seq;
  a.B = n_seq; a.C = C; a.K = K; a.pad = pad; a.max_len = max_len;
  return time_reduce_dwconv(a, s);
}

int wn_op_time_recover(const float* skip, int32_t lds, const float* z, int32_t ldz, int32_t z_rows,
                       float* y, int32_t ldy, int32_t rows, int32_t C, const int32_t* off,
                       const int32_t* len, const int32_t* z_off, int32_t n_seq, void* stream) {
  WN_CHECK(skip && z && y, "time_recover: null argument");
  WN_CHECK(C > 0 && C % 64 == 0 && lds >= C && ldz >= C && ldy >= C && lds % 4 == 0 &&
               ldz % 4 == 0 && ldy % 4 == 0,
           "time_recover: C must be a multiple of 64, strides multiples of 4 elements, >= C");
  WN_CHECK(rows > 0 && z_rows > 0, "time_recover: empty buffers");
  WN_CHECK(y + (int64_t)rows * ldy <= z || z + (int64_t)z_rows * ldz <= y,
           "time_recover: z overlaps y");
  WN_CHECK(y == skip || y + (int64_t)rows * ldy <= skip || skip + (int64_t)rows * lds <= y,
           "time_recover: y overlaps skip without being it");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  int max_len = 0;
  WN_TRY(time_hook_layout(off, len, z_off, n_seq, rows, z_rows, desc, &max_len, s,
                          "time_recover"));
  TimeRecoverArgs a;
  a.skip = skip; a.lds = lds; a.z = z; a.ldz = ldz; a.y = y; a.ldy = ldy;
  a.off = desc.as<int>(); a.len = a.off + n_seq; a.off2 = a.off + 2 * n_seq;
  a.B = n_seq; a.C = C; a.max_len = max_len;
  return time_recover_add(a, s);
}

int wn_op_attention_grouped(const float* Q, const float* K, const float* V, int32_t ldq,
                            int32_t ldk, int32_t ldv, int32_t rows, const float* P, int32_t ldp,
                            int32_t p_rows, const int32_t* p_off, const float* bias_u,
                            const float* bias_v, float* O, int32_t ldo, const int32_t* off,
                            const int32_t* len, int32_t n_seq, int32_t n_heads, int32_t group,
                            int32_t width, int32_t mask_step, int32_t chunk_size,
                            int32_t left_chunks, float scale, void* stream) {
  WN_CHECK(Q && K && V && P && bias_u && bias_v && O && off && len,
           "attention_grouped: null argument");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && n_heads > 0 && n_heads < 65536,
           "attention_grouped: n_seq / n_heads");
  WN_CHECK(width == 96 || width == 192,
           "attention_grouped: width = " + std::to_string(width) +
               " (group * d_k) has no kernel: 96 and 192 have");
  WN_CHECK(group >= 1 && group <= 16 && (n_heads * width) % group == 0,
           "attention_grouped: group must be in [1, 16] and divide n_heads * width");
  const int D = n_heads * width / group;
  WN_CHECK(D % 4 == 0, "attention_grouped: n_heads * width / group must be a multiple of 4");
  WN_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ldp % 4 == 0,
           "attention_grouped: strides must be multiples of 4 elements");
  WN_CHECK(ldq >= D && ldk >= D && ldv >= D && ldo >= D && ldp >= D,
           "attention_grouped: a stride is smaller than n_heads * width / group");
  WN_CHECK(rows > 0 && p_rows > 0, "attention_grouped: empty buffers");
  WN_CHECK(mask_step >= 1 && mask_step <= 4096, "attention_grouped: mask_step must be in [1, 4096]");
  WN_CHECK(chunk_size >= 0 && chunk_size <= (1 << 20),
           "attention_grouped: chunk_size must be in [0, 2^20] (0: full context)");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           "attention_grouped: rows outside the buffer, unordered or overlapping");
  int max_len = 0;
  std::vector<int> h((size_t)3 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i]; h[2 * n_seq + i] = p_off ? p_off[i] : 0;
    WN_CHECK(h[2 * n_seq + i] >= 0 && (int64_t)h[2 * n_seq + i] + len[i] <= p_rows,
             "attention_grouped: a sequence's position rows lie outside the table (p_off, p_rows)");
    max_len = std::max(max_len, len[i]);
  }
  WN_CHECK(max_len > 0 && max_len <= (1 << 18), "attention_grouped: empty, or a sequence too long");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  WN_TRY(upload_ints(desc, h, s));
  GroupedAttnArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.P = P; a.ldp = ldp; a.bias_u = bias_u; a.bias_v = bias_v; a.O = O; a.ldo = ldo;
  a.off = desc.as<int>(); a.len = a.off + n_seq; a.p_off = a.off + 2 * n_seq;
  a.n_seq = n_seq; a.n_heads = n_heads; a.group = group; a.width = width; a.D = D;
  a.max_len = max_len; a.mask_step = mask_step; a.chunk_size = chunk_size;
  a.left_chunks = left_chunks; a.scale = scale;
  return attention_grouped(a, s);
}

// the layouts both stride hooks share: off | len | outgoing-rate off on the device; the outgoing
// rows (len + 1) / 2 from off2 must lie inside rows2, ascending and disjoint
static int stride_hook_layout(const int32_t* off, const int32_t* len, const int32_t* off2,
                              int n_seq, int rows, int rows2, int stride, DevBuf& desc,
                              int* max_len, hipStream_t s, const char* who) {
  const std::string w(who);
  WN_CHECK(off && len && off2, w + ": null argument");
  WN_CHECK(stride == 2, w + ": stride = " + std::to_string(stride) + " has no kernel: 2 has");
  WN_CHECK(n_seq > 0 && n_seq < 65536 && rows > 0 && rows2 > 0, w + ": n_seq / rows");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           w + ": rows outside the buffer, unordered or overlapping");
  std::vector<int> h((size_t)3 * n_seq), len2(n_seq);
  *max_len = 0;
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i]; h[2 * n_seq + i] = off2[i];
    len2[i] = (len[i] + 1) / 2;
    *max_len = std::max(*max_len, len[i]);
  }
  WN_CHECK(packed_ok(off2, len2.data(), n_seq, rows2),
           w + ": outgoing rows outside the buffer, unordered or overlapping");
  WN_CHECK(*max_len > 0, w + ": empty");
  return upload_ints(desc, h, s);
}

int wn_op_stride_dwconv_ln_silu(const float* x, int32_t ldx, int32_t rows, int32_t D,
                                const float* wt, const float* bias, const float* cpad,
                                const float* ln_w, const float* ln_b, int32_t norm_mode,
                                float eps, int32_t K, int32_t causal, int32_t stride, float* y,
                                int32_t ldy, int32_t out_rows, const int32_t* off,
                                const int32_t* len, const int32_t* out_off, int32_t n_seq,
                                void* stream) {
  WN_CHECK(x && wt && bias && ln_w && ln_b && y, "stride_dwconv_ln_silu: null argument");
  WN_CHECK(D >= 64 && D % 64 == 0 && D <= 512 && ldx >= D && ldy >= D,
           "stride_dwconv_ln_silu: D must be a multiple of 64 up to 512, strides >= D");
  WN_CHECK(K >= 1 && K <= 63 && (causal || K % 2 == 1),
           "stride_dwconv_ln_silu: K must be in [1, 63], odd unless causal");
  WN_CHECK(norm_mode == 0 || norm_mode == 1, "stride_dwconv_ln_silu: norm_mode is 0 or 1");
  WN_CHECK(rows > 0 && out_rows > 0, "stride_dwconv_ln_silu: empty buffers");
  WN_CHECK(y + (int64_t)out_rows * ldy <= x || x + (int64_t)rows * ldx <= y,
           "stride_dwconv_ln_silu: y overlaps x");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  int max_len = 0;
  WN_TRY(stride_hook_layout(off, len, out_off, n_seq, rows, out_rows, stride, desc, &max_len, s,
                            "stride_dwconv_ln_silu"));
  StrideDwConvArgs a;
  a.x = x; a.ldx = ldx; a.wt = wt; a.bias = bias; a.cpad = cpad; a.ln_w = ln_w; a.ln_b = ln_b;
  a.norm_mode = norm_mode; a.y = y; a.ldy = ldy;
  a.off = desc.as<int>(); a.len = a.off + n_seq; a.off2 = a.off + 2 * n_seq;
  a.B = n_seq; a.D = D; a.K = K; a.causal = causal; a.stride = stride; a.max_len = max_len;
  a.eps = eps;
  return stride_dwconv_ln_silu(a, s);
}

int wn_op_avgpool_residual_add(const float* x, int32_t ldx, int32_t rows, const float* z,
                               int32_t ldz, float* y, int32_t ldy, int32_t out_rows, int32_t C,
                               int32_t stride, const int32_t* off, const int32_t* len,
                               const int32_t* out_off, int32_t n_seq, void* stream) {
  WN_CHECK(x && z && y, "avgpool_residual_add: null argument");
  WN_CHECK(C >= 4 && C % 4 == 0 && ldx >= C && ldz >= C && ldy >= C && ldx % 4 == 0 &&
               ldz % 4 == 0 && ldy % 4 == 0,
           "avgpool_residual_add: C must be a multiple of 4, strides multiples of 4 elements, >= C");
  WN_CHECK(rows > 0 && out_rows > 0, "avgpool_residual_add: empty buffers");
  WN_CHECK(y + (int64_t)out_rows * ldy <= x || x + (int64_t)rows * ldx <= y,
           "avgpool_residual_add: y overlaps x");
  WN_CHECK(y == z || y + (int64_t)out_rows * ldy <= z || z + (int64_t)out_rows * ldz <= y,
           "avgpool_residual_add: y overlaps z without being it");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  int max_len = 0;
  WN_TRY(stride_hook_layout(off, len, out_off, n_seq, rows, out_rows, stride, desc, &max_len, s,
                            "avgpool_residual_add"));
  AvgPoolResidArgs a;
  a.x = x; a.ldx = ldx; a.z = z; a.ldz = ldz; a.y = y; a.ldy = ldy;
  a.off = desc.as<int>(); a.len = a.off + n_seq; a.off2 = a.off + 2 * n_seq;
  a.B = n_seq; a.C = C; a.stride = stride; a.max_len = max_len;
  return avgpool_residual_add(a, s);
}

int wn_op_firered_frontend(const float* feats, const float* mean, const float* istd,
                           const float* w1, const float* b1, const float* w2, const float* b2,
                           float* out, int32_t ldo, int32_t out_rows, const int32_t* lens,
                           const int32_t* out_off, int32_t* out_len, int32_t B, int32_t T,
                           int32_t F, int32_t C, void* stream) {
  WN_CHECK(feats && w1 && b1 && w2 && b2 && out && lens && out_off && out_len,
           "firered_frontend: null argument");
  WN_CHECK((mean == nullptr) == (istd == nullptr), "firered_frontend: mean and istd come together");
  WN_CHECK(F >= 7 && F <= 128 && B > 0 && B < 65536 && T > 0 && C > 0 && C <= 256 && out_rows > 0,
           "firered_frontend: B / T / F / C");
  const int F1 = (F - 3) / 2 + 1, F2 = (F1 - 3) / 2 + 1;
  WN_CHECK(ldo >= C * F2, "firered_frontend: output stride");
  std::vector<int> h((size_t)5 * B);
  int max_t2 = 0, at1 = 0;
  for (int b = 0; b < B; ++b) {
    WN_CHECK(lens[b] >= 0 && lens[b] <= T, "firered_frontend: a length outside [0, T]");
    // alone semantics: six zero frames behind the utterance's OWN last frame
    const int t2 = lens[b] > 0 ? ((lens[b] + 6 - 3) / 2 + 1 - 3) / 2 + 1 : 0;
    const int t1 = t2 > 0 ? 2 * t2 + 1 : 0;
    out_len[b] = t2;
    h[b] = lens[b]; h[B + b] = at1; h[2 * B + b] = t1; h[3 * B + b] = out_off[b];
    h[4 * B + b] = t2;
    at1 += t1;
    max_t2 = std::max(max_t2, t2);
  }
  WN_CHECK(packed_ok(out_off, out_len, B, out_rows),
           "firered_frontend: frames outside the buffer, unordered or overlapping");
  WN_CHECK(max_t2 > 0, "firered_frontend: empty");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, h1;
  WN_TRY(upload_ints(desc, h, s));
  WN_TRY(h1.ensure((size_t)at1 * F1 * C * sizeof(float)));
  FireRedFrontArgs a;
  a.feats = feats; a.mean = mean; a.istd = istd; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.h1 = h1.as<float>(); a.out = out; a.ldo = ldo;
  a.len = desc.as<int>(); a.t1_off = a.len + B; a.t1_len = a.len + 2 * B;
  a.t2_off = a.len + 3 * B; a.t2_len = a.len + 4 * B;
  a.B = B; a.T = T; a.F = F; a.F1 = F1; a.F2 = F2; a.C = C; a.max_t2 = max_t2;
  return firered_frontend(a, s);
}

// the descriptors both Branchformer hooks share: off | len on the device, the longest length
static int dwt_hook_layout(const int32_t* off, const int32_t* len, int n_seq, int rows,
                           DevBuf& desc, DwTileArgs* a, hipStream_t s, const char* who) {
  const std::string w(who);
  WN_CHECK(off && len && n_seq > 0 && n_seq < 65536 && rows > 0, w + ": n_seq / rows");
  WN_CHECK(packed_ok(off, len, n_seq, rows),
           w + ": rows outside the buffer, unordered or overlapping");
  std::vector<int> h((size_t)2 * n_seq);
  int max_len = 0;
  for (int i = 0; i < n_seq; ++i) {
    h[i] = off[i]; h[n_seq + i] = len[i];
    max_len = std::max(max_len, len[i]);
  }
  WN_CHECK(max_len > 0, w + ": empty");
  WN_TRY(upload_ints(desc, h, s));
  a->off = desc.as<int>(); a->len = a->off + n_seq; a->B = n_seq; a->max_len = max_len;
  return 0;
}

int wn_op_csgu_gate(const float* h, int32_t ldh, int32_t rows, int32_t C, const float* ln_w,
                    const float* ln_b, const float* wt, const float* bias, int32_t K,
                    int32_t causal, int32_t gate, float* y, int32_t ldy, const int32_t* off,
                    const int32_t* len, int32_t n_seq, void* stream) {
  WN_CHECK(h && ln_w && ln_b && wt && bias && y, "csgu_gate: null argument");
  WN_CHECK(C > 0 && C <= CSGU_MAX_C && ldh >= 2 * C && ldy >= C, "csgu_gate: C / strides");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc, stats;
  DwTileArgs a;
  WN_TRY(dwt_hook_layout(off, len, n_seq, rows, desc, &a, s, "csgu_gate"));
  WN_TRY(stats.ensure((size_t)rows * sizeof(float2)));
  a.x = h + C; a.ldx = ldh; a.wt = wt; a.bias = bias; a.y = y; a.ldy = ldy;
  a.C = C; a.K = K; a.causal = causal != 0;
  a.ln_w = ln_w; a.ln_b = ln_b; a.stats = stats.as<float2>(); a.M = rows; a.eps = 1e-5f;
  if (gate) { a.r = h; a.ldr = ldh; }
  return csgu_gate(a, s);
}

int wn_op_merge_dwconv(const float* c, int32_t ldc, int32_t rows, int32_t C, const float* wt,
                       const float* bias, int32_t K, int32_t causal, float* y, int32_t ldy,
                       const int32_t* off, const int32_t* len, int32_t n_seq, void* stream) {
  WN_CHECK(c && wt && bias && y, "merge_dwconv: null argument");
  WN_CHECK(C > 0 && ldc >= C && ldy >= C, "merge_dwconv: C / strides");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  DwTileArgs a;
  WN_TRY(dwt_hook_layout(off, len, n_seq, rows, desc, &a, s, "merge_dwconv"));
  a.x = c; a.ldx = ldc; a.wt = wt; a.bias = bias; a.y = y; a.ldy = ldy;
  a.C = C; a.K = K; a.causal = causal != 0;
  return merge_dwconv(a, s);
}

int wn_op_conv2d4(wn_model* m, const float* feats_dev, const int32_t* feat_lens_host, int32_t B,
                  int32_t T, float* c1, float* c2, float* x, int32_t* enc_lens_host,
                  int32_t* route_out, void* stream) {
  WN_CHECK(m && feats_dev && feat_lens_host && route_out, "wn_op_conv2d4: null argument");
  WN_ENTER(m);
  // (the encode gate is one-shot, as in wn_encode)
  struct GateDrop { wn_model* m; ~GateDrop() { m->enc_gate = nullptr; } } gate_drop{m};
  m->pb_valid = false;
  PrecisionScope prec_scope(m);
  WN_CHECK(!m->data->layers.empty() && m->cfg.encoder_type == 0 && !m->fr.on,
           "wn_op_conv2d4: needs a Conformer encoder");
  WN_CHECK(B > 0, "wn_encode: empty batch");
  WN_CHECK(B < 65536, "wn_op_conv2d4: more than 65535 utterances");
  WN_CHECK(T >= 7, "wn_encode: at least 7 frames are needed by Conv2dSubsampling4");
  hipStream_t s = (hipStream_t)stream;
  WN_HIP(hipSetDevice(m->device));
  WN_TRY(subsample_conv2d4(m, feats_dev, feat_lens_host, B, T, enc_lens_host, 0, s));
  WN_TRY(encode_gate_wait(m, s));
  *route_out = m->front_route;
  const int M = m->rows, d = m->cfg.d_model, F1 = m->F1(), F2 = m->F2();
  if (M > 0) {
    int M1 = 0, max_t1 = 0;
    for (int b = 0; b < B; ++b) {
      const int l1 = m->len[b] > 0 ? 2 * m->len[b] + 1 : 0;
      M1 += l1;
      max_t1 = std::max(max_t1, l1);
    }
    if (c1 && (m->front_route & 15) == CONV2_X6_PLANES) {
      hipLaunchKernelGGL(conv1_image_unpack_kernel, dim3(cdiv(max_t1 * F1 * (d / 8), 256), B),
                         dim3(256), 0, s, m->c1.as<char>(), cdiv(M1 * F1, 32),
                         m->d_off1.as<int>(), m->d_len1.as<int>(), F1, d, c1);
      WN_HIP(hipGetLastError());
    } else if (c1) {
      WN_HIP(hipMemcpyAsync(c1, m->c1.p, (size_t)M1 * F1 * d * sizeof(float),
                            hipMemcpyDeviceToDevice, s));
    }
    if (c2)
      WN_HIP(hipMemcpyAsync(c2, m->c2.p, (size_t)M * F2 * d * sizeof(float),
                            hipMemcpyDeviceToDevice, s));
    if (x)
      WN_HIP(hipMemcpyAsync(x, m->x.p, (size_t)M * d * sizeof(float), hipMemcpyDeviceToDevice,
                            s));
  }
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_ctc_rows(const float* logits, int32_t ld, int32_t M, int32_t V, int32_t k,
                   int32_t blank, float blank_penalty, float* topk_val, int32_t* topk_idx,
                   float* logp, int32_t ld_out, void* stream) {
  WN_CHECK(logits && topk_val && topk_idx, "ctc_rows: null argument");
  WN_CHECK(M > 0 && V > 0 && ld >= V, "ctc_rows: M / V / ld");
  WN_CHECK(k >= 1 && k <= V, "ctc: top-k must be in [1, vocab]");
  WN_CHECK(blank >= 0 && blank < V, "ctc_rows: blank outside the vocabulary");
  WN_CHECK(logp == nullptr || ld_out >= V, "ctc_rows: ld_out");
  CtcRowArgs a;
  a.logits = logits; a.ld = ld; a.M = M; a.V = V; a.k = k; a.blank = blank;
  a.blank_penalty = blank_penalty; a.topk_val = topk_val; a.topk_idx = topk_idx;
  a.logp = logp; a.ld_out = ld_out;
  return ctc_logsoftmax_topk(a, (hipStream_t)stream);
}

// ---- attention for decoder heads of 32 (attention_d32.hip) ------------------------------------

int wn_op_attention_d32(const float* Q, const float* K, const float* V, int32_t ldq, int32_t ldk,
                        int32_t ldv, int32_t q_rows, int32_t kv_rows, float* O, int32_t ldo,
                        const int32_t* q_off, const int32_t* q_len, const int32_t* kv_off,
                        const int32_t* kv_len, int32_t n_seq, int32_t n_heads, float scale,
                        int32_t mask_mode, void* stream) {
  WN_CHECK(Q && K && V && O && q_off && q_len && kv_off && kv_len,
           "attention_d32: null argument");
  WN_CHECK(mask_mode == 0 || mask_mode == 1,
           "attention_d32: mask_mode must be 0 (keys < kv_len) or 1 (causal), not 2 (chunk window)");
  WN_CHECK(n_seq > 0 && n_seq < 32768 && n_heads > 0 && n_heads < 256,
           "attention_d32: n_seq / n_heads");
  const int d = n_heads * 32;
  WN_CHECK(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0,
           "attention_d32: strides must be multiples of 4 elements");
  WN_CHECK(ldq >= d && ldk >= d && ldv >= d && ldo >= d,
           "attention_d32: a stride is smaller than n_heads * 32");
  WN_CHECK(q_rows > 0 && kv_rows > 0, "attention_d32: empty buffers");
  WN_CHECK(((uintptr_t)Q & 15) == 0 && ((uintptr_t)K & 15) == 0 && ((uintptr_t)V & 15) == 0,
           "attention_d32: Q, K and V must be 16-byte aligned");
  WN_CHECK(packed_ok(q_off, q_len, n_seq, q_rows),
           "attention_d32: query rows outside the buffer, unordered or overlapping");
  int max_q = 0;
  for (int i = 0; i < n_seq; ++i) {
    WN_CHECK(kv_len[i] >= 0 && kv_off[i] >= 0 && (int64_t)kv_off[i] + kv_len[i] <= kv_rows,
             "attention_d32: key rows outside the buffer");
    WN_CHECK(q_len[i] == 0 || kv_len[i] > 0, "attention_d32: queries without keys");
    max_q = std::max(max_q, q_len[i]);
  }
  WN_CHECK(max_q > 0, "attention_d32: empty");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf desc;
  std::vector<int> h((size_t)4 * n_seq);
  for (int i = 0; i < n_seq; ++i) {
    h[i] = q_off[i]; h[n_seq + i] = q_len[i];
    h[2 * n_seq + i] = kv_off[i]; h[3 * n_seq + i] = kv_len[i];
  }
  WN_TRY(upload_ints(desc, h, s));
  const int* dd = desc.as<int>();
  AttnArgs a;
  a.Q = Q; a.K = K; a.V = V; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.O = O; a.ldo = ldo;
  a.q_off = dd; a.q_len = dd + n_seq; a.kv_off = dd + 2 * n_seq; a.kv_len = dd + 3 * n_seq;
  a.n_seq = n_seq; a.n_heads = n_heads; a.max_q_len = max_q;
  a.mask_mode = mask_mode; a.scale = scale;
  return attention_d32(a, s);
}

// ---- the `attention` decode mode's kernels (attn_search.hip), one launcher per hook ----------

int wn_op_attn_self_step(const float* qkv, int32_t d, int32_t heads, int32_t n, float* cache,
                         int32_t step, const int32_t* path, int32_t max_len, float* out,
                         void* stream) {
  WN_CHECK(qkv && cache && path && out, "attn_self_step: null argument");
  WN_CHECK(heads >= 1 && heads < 256 && (d == heads * 64 || d == heads * 32),
           "attn_self_step: d must be heads * 64 or heads * 32");
  WN_CHECK(n >= 1 && n <= 4096, "attn_self_step: n outside [1, 4096]");
  WN_CHECK(step >= 0 && step + 1 <= max_len && max_len <= 65536,
           "attn_self_step: step outside [0, max_len)");
  hipStream_t s = (hipStream_t)stream;
  bool ok = false;
  WN_TRY(device_ints_in_range(path, n, max_len, step + 1, n, s, &ok));
  WN_CHECK(ok, "attn_self_step: a path entry outside [0, n)");
  return attn_self_step(qkv, d, heads, n, cache, step, path, max_len, out, s);
}

int wn_op_attn_step_embed(const int32_t* last_tok, int32_t pos, const float* emb, int32_t V,
                          const float* pe, int32_t max_pos, float scale, int32_t d, int32_t n,
                          float* x, void* stream) {
  WN_CHECK(last_tok && emb && pe && x, "attn_step_embed: null argument");
  WN_CHECK(d >= 4 && d % 4 == 0 && n >= 1 && n <= 65536 && V >= 1, "attn_step_embed: d / n / V");
  WN_CHECK(pos >= 0 && pos < max_pos, "attn_step_embed: position outside the table");
  hipStream_t s = (hipStream_t)stream;
  bool ok = false;
  WN_TRY(device_ints_in_range(last_tok, n, 1, 1, V, s, &ok));
  WN_CHECK(ok, "attn_step_embed: a token outside [0, V)");
  return attn_step_embed(last_tok, pos, emb, pe, scale, d, n, x, s);
}

int wn_op_attn_prompt_cache(const float* qkv, int32_t d, int32_t B, int32_t P, int32_t N,
                            float* cache, void* stream) {
  WN_CHECK(qkv && cache, "attn_prompt_cache: null argument");
  WN_CHECK(d >= 4 && d % 4 == 0 && B >= 1 && P >= 1 && (int64_t)B * P <= 65536,
           "attn_prompt_cache: d / B / P");
  WN_CHECK(N >= 1 && N <= 64, "attn_prompt_cache: beam_size must be in [1, 64]");
  return attn_prompt_cache_store(qkv, d, B, P, N, cache, (hipStream_t)stream);
}

int wn_op_beam_init(int32_t B, int32_t N, int32_t max_len, int32_t sos, const int32_t* prompt,
                    int32_t P, float* score, int32_t* end, int32_t* tok, int32_t* path,
                    int32_t* last_tok, void* stream) {
  WN_CHECK(score && end && tok && path && last_tok, "beam_init: null argument");
  WN_CHECK(B >= 1 && B <= 65536, "beam_init: B outside [1, 65536]");
  WN_CHECK(N >= 1 && N <= 64, "beam_init: beam_size must be in [1, 64]");
  WN_CHECK(max_len >= 1, "beam_init: max_len");
  if (prompt) {
    WN_CHECK(P >= 1 && P <= max_len, "beam_init: prompt length outside [1, max_len]");
    return attn_beam_init_prompt(B * N, N, max_len, prompt, P, score, end, tok, path, last_tok,
                                 (hipStream_t)stream);
  }
  return attn_beam_init(B * N, N, max_len, sos, score, end, tok, path, last_tok,
                        (hipStream_t)stream);
}

int wn_op_beam_update(int32_t B, int32_t N, int32_t step, int32_t max_len, int32_t eos,
                      int32_t V, const float* topv, const int32_t* topi, const float* score_in,
                      const int32_t* end_in, const int32_t* tok_in, const int32_t* path_in,
                      float* score_out, int32_t* end_out, int32_t* tok_out, int32_t* path_out,
                      int32_t* last_tok, int32_t shared_row, int32_t* n_done_host, void* stream) {
  WN_CHECK(topv && topi && score_in && end_in && tok_in && path_in && score_out && end_out &&
               tok_out && path_out && last_tok && n_done_host, "beam_update: null argument");
  WN_CHECK(B >= 1 && B <= 65536, "beam_update: B outside [1, 65536]");
  WN_CHECK(N >= 1 && N <= 64, "beam_update: beam_size must be in [1, 64]");
  WN_CHECK(step >= 1 && step + 1 <= max_len, "beam_update: step outside [1, max_len - 1]");
  WN_CHECK(V >= 1 && eos >= 0 && eos < V, "beam_update: eos outside the vocabulary");
  hipStream_t s = (hipStream_t)stream;
  static thread_local DevBuf done;
  WN_TRY(done.ensure(sizeof(int)));
  WN_HIP(hipMemsetAsync(done.p, 0, sizeof(int), s));
  WN_TRY(attn_beam_update(B, N, step, max_len, eos, V, topv, topi, score_in, end_in, tok_in,
                          path_in, score_out, end_out, tok_out, path_out, last_tok,
                          done.as<int>(), s, shared_row != 0));
  WN_HIP(hipMemcpyAsync(n_done_host, done.p, sizeof(int), hipMemcpyDeviceToHost, s));
  WN_HIP(hipStreamSynchronize(s));
  return 0;
}

int wn_op_beam_finish(int32_t B, int32_t N, int32_t len, int32_t max_len, int32_t eos,
                      float length_penalty, const float* score, const int32_t* tok,
                      int32_t* out_tok, int32_t* out_len, int32_t prefix, void* stream) {
  WN_CHECK(score && tok && out_tok && out_len, "beam_finish: null argument");
  WN_CHECK(B >= 1 && B <= 65536, "beam_finish: B outside [1, 65536]");
  WN_CHECK(N >= 1 && N <= 64, "beam_finish: beam_size must be in [1, 64]");
  WN_CHECK(prefix >= 0 && prefix <= len && len <= max_len,
           "beam_finish: need 0 <= prefix <= len <= max_len");
  return attn_beam_finish(B, N, len, max_len, eos, length_penalty, score, tok, out_tok, out_len,
                          (hipStream_t)stream, prefix);
}

// ---- the kernels that own a complete row: LayerNorm family, FFN reduce, row-LN GEMM ----------

int wn_op_layernorm_ex(const float* x, int32_t ldx, const float* w, const float* b, void* y,
                       int32_t ldy, int32_t M, int32_t D, float eps, int32_t y_bf16, void* stream) {
  WN_CHECK(x && w && b && y, "layernorm: null argument");
  WN_CHECK(M > 0, "layernorm: empty");
  WN_CHECK(width_in(D, {64, 128, 192, 256, 384, 512, 640, 768, 1024, 1280}),
           "layernorm: unsupported width " + std::to_string(D));
  WN_CHECK(ldx >= D && ldy >= D && ldx % 4 == 0 && ldy % 4 == 0,
           "layernorm: a row stride is smaller than the width or no multiple of 4");
  return layernorm(x, ldx, w, b, reinterpret_cast<float*>(y), ldy, M, D, eps,
                   (hipStream_t)stream, y_bf16 != 0);
}

int wn_op_layernorm2(const float* x, const float* w1, const float* b1, const float* w2,
                     const float* b2, float* y1, void* y2, int32_t M, int32_t D, float eps,
                     int32_t y2_bf16, void* stream) {
  WN_CHECK(x && w1 && b1 && w2 && b2 && y1 && y2, "layernorm2: null argument");
  WN_CHECK(M > 0, "layernorm2: empty");
  WN_CHECK(width_in(D, {64, 128, 256, 512, 768, 1024, 1280}),
           "layernorm2: unsupported width " + std::to_string(D));
  return layernorm2(x, w1, b1, w2, b2, y1, reinterpret_cast<float*>(y2), M, D, eps,
                    (hipStream_t)stream, y2_bf16 != 0);
}

int wn_op_layernorm_mx(const float* x, int32_t ldx, const float* w, const float* b, void* q,
                       void* scale, int32_t pitch, int32_t M, int32_t D, float eps, void* stream) {
  WN_CHECK(x && w && b && q && scale, "layernorm_mx: null argument");
  WN_CHECK(M > 0, "layernorm_mx: empty");
  WN_CHECK(width_in(D, {256, 512, 768, 1024, 1280}),
           "layernorm_mx: unsupported width " + std::to_string(D));
  WN_CHECK(ldx >= D && ldx % 4 == 0,
           "layernorm_mx: the row stride is smaller than the width or no multiple of 4");
  WN_CHECK(pitch >= M, "layernorm_mx: scale pitch smaller than M");
  return layernorm_mx(x, ldx, w, b, q, reinterpret_cast<unsigned*>(scale), pitch, M, D, eps,
                      (hipStream_t)stream);
}

int wn_op_ffn_reduce_ln(float* x, const float* P, int32_t S, const float* b2, float alpha,
                        const float* w, const float* b, const float* w2, const float* bb2, float* y,
                        void* y3, int64_t y3_bytes, int32_t M, int32_t D, float eps, int32_t mode,
                        void* stream) {
  WN_CHECK(x && P && b2 && w && b, "ffn_reduce_ln: null argument");
  WN_CHECK(M > 0, "ffn_reduce_ln: empty");
  WN_CHECK(D == 256 || D == 512, "ffn_reduce_ln: unsupported width " + std::to_string(D));
  WN_CHECK(S >= 1, "ffn_reduce_ln: S must be at least 1");
  WN_CHECK(mode >= 0 && mode <= 2, "ffn_reduce_ln: mode outside 0..2");
  WN_CHECK(mode != 1 || (w2 && bb2), "ffn_reduce_ln: null argument (mode 1 needs w2 and bb2)");
  if (y3) {
    WN_CHECK(mode == 1, "ffn_reduce_ln: the plane image form is mode 1");
    WN_CHECK(y3_bytes >= 0 && (uint64_t)y3_bytes >= x6_bytes(M, D),
             "ffn_reduce_ln: y3_bytes is smaller than the plane image");
    return ffn_reduce_ln_img(x, P, S, b2, alpha, w, b, w2, bb2, y3, M, D, eps,
                             (hipStream_t)stream);
  }
  WN_CHECK(mode == 2 || y, "ffn_reduce_ln: null argument (modes 0 and 1 write y)");
  return ffn_reduce_ln(x, P, S, b2, alpha, w, b, w2, bb2, y, M, D, eps, mode,
                       (hipStream_t)stream);
}

int wn_op_gemm_rowln(const float* A, int32_t lda, const float* W, const float* bias,
                     const float* resid, int32_t ldr, float alpha, float* x_out, int32_t ldx,
                     const float* ln_w, const float* ln_b, float eps, float* y, int32_t ldy,
                     int32_t M, int32_t K, void* stream) {
  WN_CHECK(A && W && x_out && y && ln_w && ln_b, "gemm_rowln: null argument");
  WN_CHECK(M > 0, "gemm_rowln: empty");
  WN_CHECK(K % 32 == 0 && K >= 96, "gemm_rowln: K must be a multiple of 32, at least 96");
  WN_CHECK(lda >= K && lda % 4 == 0, "gemm_rowln: lda is smaller than K or no multiple of 4");
  WN_CHECK(ldr >= 256 && ldx >= 256 && ldy >= 256, "gemm_rowln: ldr / ldx / ldy below 256");
  // (the kernel addresses A and W with 32-bit byte offsets)
  WN_CHECK((int64_t)M * lda * 4 < ((int64_t)1 << 31) && (int64_t)256 * K * 4 < ((int64_t)1 << 31),
           "gemm_rowln: A or W is 2 GiB or more");
  RowLnArgs a;
  a.A = A; a.lda = lda; a.W = W; a.bias = bias; a.resid = resid; a.ldr = ldr; a.alpha = alpha;
  a.x_out = x_out; a.ldx = ldx; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.y = y; a.ldy = ldy;
  a.M = M; a.N = 256; a.K = K;
  return gemm_rowln(a, (hipStream_t)stream);
}

}  // extern "C"
