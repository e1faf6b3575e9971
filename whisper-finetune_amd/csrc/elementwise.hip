// elementwise.hip — the element-wise bf16 kernels of the training step and the bias-gradient column sums: residual-gradient
// add, the stochastic-depth rescale a*x + b*y (axpby) and its graph-capturable select form (sd_select_fwd / _bwd), dy * gelu'(pre)
// for the conv stem's backward, and colsum / colsum_chunk / colsum_fold.
//
// All kernels are HBM-bound streaming passes.  The element-wise ones move 16 bytes (8 bf16) per lane in a grid-stride loop over
// ew_grid workgroups (bf8_unpack / compute in fp32 / bf8_pack); workgroup 0 finishes the n % 8 tail element by element.  The
// column sums use no atomics and add in a fixed order (bitwise reproducible).
#include "common.h"

__global__ __launch_bounds__(256) void add_bf16_kernel(const unsigned short* a, const unsigned short* b,
                                                        unsigned short* y, long n) {
  const long nv = n >> 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    float x[8], z[8], o[8];
    bf8_unpack(*(const u32x4*)(a + i * 8), x);
    bf8_unpack(*(const u32x4*)(b + i * 8), z);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = x[e] + z[e];
    *(u32x4*)(y + i * 8) = bf8_pack(o);
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) y[t] = f2bf(bf2f(a[t]) + bf2f(b[t]));
  }
}
extern "C" int wft_add_bf16(const wft_bf16* a, const wft_bf16* b, wft_bf16* y, int64_t n, void* stream) {
  WFT_CHECK_ARG(a && b && y && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)a) & 15) == 0 && (((uintptr_t)b) & 15) == 0 && (((uintptr_t)y) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(add_bf16_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, a, b, y, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}


// ----------------------------------------------------------------------------- stochastic-depth rescale
// out = a*x + b*y (y may be NULL: out = a*x).  Forward of StochasticDepthMixin's train-time rescale
// x + (block(x) - x) / (1 - p) = (1 - s) x + s block(x), s = 1/(1-p)  (model/model_utils.py:241-250) in ONE pass instead
// of three element-wise kernels; its backward is two scaled copies.
// (the 8-element body is shared with sd_select_fwd_kernel below)
__device__ __forceinline__ u32x4 axpby8(float a, u32x4 xv, float b, u32x4 yv) {
  float x[8], y[8], o[8];
  bf8_unpack(xv, x);
  bf8_unpack(yv, y);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = a * x[e] + b * y[e];
  return bf8_pack(o);
}
__global__ __launch_bounds__(256) void axpby_bf16_kernel(float a, const unsigned short* x, float b, const unsigned short* y,
                                                          unsigned short* out, long n) {
  const long nv = n >> 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const u32x4 xv = *(const u32x4*)(x + i * 8);
    u32x4 yv = {0u, 0u, 0u, 0u};
    if (y) yv = *(const u32x4*)(y + i * 8);
    *(u32x4*)(out + i * 8) = axpby8(a, xv, b, yv);
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) out[t] = f2bf(a * bf2f(x[t]) + (y ? b * bf2f(y[t]) : 0.f));
  }
}
extern "C" int wft_axpby_bf16(float a, const wft_bf16* x, float b, const wft_bf16* y, wft_bf16* out, int64_t n, void* stream) {
  WFT_CHECK_ARG(x && out && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)x) & 15) == 0 && (((uintptr_t)y) & 15) == 0 && (((uintptr_t)out) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(axpby_bf16_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, a, x, b, y, out, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// Stochastic depth behind a device skip flag (a captured HIP graph: the host writes *skip before each replay).  Kept blocks
// (*skip == 0) run axpby_bf16_kernel's own body, axpby8, in the forward — out = a*x + b*f; the backward repeats its arithmetic
// term for term in the one-operand form a*dy + b0*0 (b0 = 0, runtime) for both outputs, typed out (two axpby8 calls cost two more
// VGPRs) — so that they are bit-identical to ops.SdRescaleFn; a skipped block is a SELECT (out = x, dx = dy, df = 0), never a
// multiply by zero, so that a non-finite value in the discarded block cannot leak.
__global__ __launch_bounds__(256) void sd_select_fwd_kernel(const int* skip, float a, const unsigned short* x, float b,
                                                             const unsigned short* f, unsigned short* out, long n) {
  const bool sk = *skip != 0;
  const long nv = n >> 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const u32x4 xv = *(const u32x4*)(x + i * 8);
    if (sk) {
      *(u32x4*)(out + i * 8) = xv;
      continue;
    }
    *(u32x4*)(out + i * 8) = axpby8(a, xv, b, *(const u32x4*)(f + i * 8));
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) out[t] = sk ? x[t] : f2bf(a * bf2f(x[t]) + b * bf2f(f[t]));
  }
}
__global__ __launch_bounds__(256) void sd_select_bwd_kernel(const int* skip, float a, float s, float b0, const unsigned short* dy,
                                                             unsigned short* dx, unsigned short* df, long n) {
  const bool sk = *skip != 0;
  const long nv = n >> 3;
  const u32x4 zv = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const u32x4 gv = *(const u32x4*)(dy + i * 8);
    if (sk) {
      *(u32x4*)(dx + i * 8) = gv;
      *(u32x4*)(df + i * 8) = zv;
      continue;
    }
    u32x4 o, p;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = bf2f((unsigned short)(gv[e] & 0xffff)), hi = bf2f((unsigned short)(gv[e] >> 16));
      const float zlo = bf2f((unsigned short)(zv[e] & 0xffff)), zhi = bf2f((unsigned short)(zv[e] >> 16));
      o[e] = pack2bf(a * lo + b0 * zlo, a * hi + b0 * zhi);
      p[e] = pack2bf(s * lo + b0 * zlo, s * hi + b0 * zhi);
    }
    *(u32x4*)(dx + i * 8) = o;
    *(u32x4*)(df + i * 8) = p;
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) {
      dx[t] = sk ? dy[t] : f2bf(a * bf2f(dy[t]) + 0.f);
      df[t] = sk ? (unsigned short)0 : f2bf(s * bf2f(dy[t]) + 0.f);
    }
  }
}
extern "C" int wft_sd_select_fwd_bf16(const int32_t* skip, float a, const wft_bf16* x, float b, const wft_bf16* f, wft_bf16* out,
                                      int64_t n, void* stream) {
  WFT_CHECK_ARG(skip && x && f && out && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)x) & 15) == 0 && (((uintptr_t)f) & 15) == 0 && (((uintptr_t)out) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(sd_select_fwd_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, (const int*)skip, a, x, b, f,
                     out, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
extern "C" int wft_sd_select_bwd_bf16(const int32_t* skip, float a, float s, const wft_bf16* dy, wft_bf16* dx, wft_bf16* df, int64_t n,
                                      void* stream) {
  WFT_CHECK_ARG(skip && dy && dx && df && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)dy) & 15) == 0 && (((uintptr_t)dx) & 15) == 0 && (((uintptr_t)df) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(sd_select_bwd_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, (const int*)skip, a, s, 0.f,
                     dy, dx, df, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}


// ----------------------------------------------------------------------------- dGELU
// out = dy * gelu'(pre)   (conv stem backward; the Linear path fuses this in the GEMM epilogue)
__global__ __launch_bounds__(256) void dgelu_mul_kernel(const unsigned short* dy, const unsigned short* pre,
                                                         unsigned short* out, long n) {
  const long nv = n >> 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    float a[8], b[8], o[8];
    bf8_unpack(*(const u32x4*)(dy + i * 8), a);
    bf8_unpack(*(const u32x4*)(pre + i * 8), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = a[e] * dgelu_f(b[e]);
    *(u32x4*)(out + i * 8) = bf8_pack(o);
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) out[t] = f2bf(bf2f(dy[t]) * dgelu_f(bf2f(pre[t])));
  }
}
extern "C" int wft_dgelu_mul_bf16(const wft_bf16* dy, const wft_bf16* pre, wft_bf16* out, int64_t n, void* stream) {
  WFT_CHECK_ARG(dy && pre && out && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)dy) & 15) == 0 && (((uintptr_t)pre) & 15) == 0 && (((uintptr_t)out) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(dgelu_mul_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, dy, pre, out, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- column sums
// out[c] (+)= sum_r x[r, c] without atomics (bitwise reproducible): a workgroup owns 32 columns for ALL rows — 4 column
// threads (16 bytes = 8 columns each, 64-byte row segments) x 64 row lanes — and folds its 64 partial rows in a fixed tree.
// Only reached where no producer kernel has formed the sums already (small models, the conv stem): the bf16 hot path gets
// its bias gradients from the LayerNorm-backward / GEMM / attention epilogues.
__global__ __launch_bounds__(256) void colsum_kernel(const unsigned short* x, long rows, long cols, long ld, float* out,
                                                      int accumulate) {
  __shared__ float red[64][33];
  const int cx = threadIdx.x & 3, ry = threadIdx.x >> 2;
  const long c0 = (long)blockIdx.x * 32 + cx * 8;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c0 < cols) {
    for (long r = ry; r < rows; r += 64) {
      float v[8];
      bf8_unpack(*(const u32x4*)(x + r * ld + c0), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] = s[e];
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if (ry < o) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] += red[ry + o][cx * 8 + e];
    }
    __syncthreads();
  }
  if (threadIdx.x < 32) {
    const long c = (long)blockIdx.x * 32 + threadIdx.x;
    if (c < cols) out[c] = accumulate ? out[c] + red[0][threadIdx.x] : red[0][threadIdx.x];
  }
}
extern "C" int wft_colsum_bf16(const wft_bf16* x, int64_t rows, int64_t cols, int64_t ld, float* out, int accumulate,
                               void* stream) {
  WFT_CHECK_ARG(x && out, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && cols >= 8 && cols % 8 == 0 && ld % 8 == 0, "cols/ld must be multiples of 8");
  WFT_CHECK_ARG((((uintptr_t)x) & 15) == 0, "16-byte alignment");
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((cols + 31) / 32)), dim3(256), 0, (hipStream_t)stream, x, (long)rows, (long)cols,
                     (long)ld, out, accumulate);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// Large inputs (the conv stem's bias gradients: 204 000 x 1280 at 68 clips): cols / 32 workgroups leave 216 of the 256 CUs idle
// (1.2 ms for 522 MB).  With a caller workspace the rows are cut into chunks, one workgroup per (column group, chunk) writes a
// partial row, and a second kernel adds the chunks in index order — the same fixed-order arithmetic at the HBM rate.
__global__ __launch_bounds__(256) void colsum_chunk_kernel(const unsigned short* x, long rows, long cols, long ld, long per, float* part) {
  __shared__ float red[64][33];
  const int cx = threadIdx.x & 3, ry = threadIdx.x >> 2;
  const long c0 = (long)blockIdx.x * 32 + cx * 8;
  const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c0 < cols) {
    for (long r = r0 + ry; r < r1; r += 64) {
      float v[8];
      bf8_unpack(*(const u32x4*)(x + r * ld + c0), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] = s[e];
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if (ry < o) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] += red[ry + o][cx * 8 + e];
    }
    __syncthreads();
  }
  if (threadIdx.x < 32) {
    const long c = (long)blockIdx.x * 32 + threadIdx.x;
    if (c < cols) part[(long)blockIdx.y * cols + c] = red[0][threadIdx.x];
  }
}
__global__ __launch_bounds__(256) void colsum_fold_kernel(const float* part, int nchunk, long cols, float* out, int accumulate) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float t = accumulate ? out[c] : 0.f;
  for (int k = 0; k < nchunk; ++k) t += part[(long)k * cols + c];
  out[c] = t;
}
#define WFT_COLSUM_CHUNKS 64
extern "C" int64_t wft_colsum_workspace_bytes(int64_t rows, int64_t cols) {
  // (round 6: from 8 192 rows on, was 65 536 — the conv stem's bias gradients of a whisper-base step, 24 000 x 512, took 94 us on the
  // 16 workgroups of the one-pass kernel)
  return rows >= 8192 ? (int64_t)WFT_COLSUM_CHUNKS * cols * (int64_t)sizeof(float) : 0;
}
extern "C" int wft_colsum_bf16_ws(const wft_bf16* x, int64_t rows, int64_t cols, int64_t ld, float* out, int accumulate,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  WFT_CHECK_ARG(x && out, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && cols >= 8 && cols % 8 == 0 && ld % 8 == 0, "cols/ld must be multiples of 8");
  WFT_CHECK_ARG((((uintptr_t)x) & 15) == 0, "16-byte alignment");
  const int64_t need = wft_colsum_workspace_bytes(rows, cols);
  if (need == 0 || !workspace || workspace_bytes < need) return wft_colsum_bf16(x, rows, cols, ld, out, accumulate, stream);
  long per = (rows + WFT_COLSUM_CHUNKS - 1) / WFT_COLSUM_CHUNKS;
  if (per < 256) per = 256;  // (four passes of a workgroup's 64 row lanes at least)
  const int nchunk = (int)((rows + per - 1) / per);
  hipLaunchKernelGGL(colsum_chunk_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, x,
                     (long)rows, (long)cols, (long)ld, per, (float*)workspace);
  hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)workspace, nchunk, (long)cols, out, accumulate);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
