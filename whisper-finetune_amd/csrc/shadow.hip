// shadow.hip — the bf16 "shadows" of the fp32 master weights that the GEMMs read: plain casts, the padded and transposed
// shadow of one weight (cast_pad_t), minLoRA's effective weight W + s·B(A⊙mask) as a shadow (lora_merge) with the operands of
// the rank-r adapter-gradient GEMMs (lora_pack), both for every adapter of a model in one launch (lora_refresh_mt), and the
// restack of the fused q/k/v bias vectors that belongs to the same refresh plans (mt_copy_f32).
//
// All kernels are HBM-bound: 4 B read and 2 + 2 B written per weight element, 64x64 tiles through LDS for the transposed side,
// 16-byte loads and 8-byte stores where the layout allows (checked on the host: `fast`).
// Per-element tests, bit for bit on whole buffers: tests/test_shadow_gpu.py (cases and references: tests/_shadow_cases.py).
#include "common.h"

// ----------------------------------------------------------------------------- casts
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* src, unsigned short* dst, long n) {
  const long nv = n >> 3;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
    const f32x4 a = *(const f32x4*)(src + i * 8), b = *(const f32x4*)(src + i * 8 + 4);
    u32x4 o = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
    *(u32x4*)(dst + i * 8) = o;
  }
  if (blockIdx.x == 0) {
    const long t = (nv << 3) + threadIdx.x;
    if (t < n) dst[t] = f2bf(src[t]);
  }
}
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const unsigned short* src, float* dst, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = bf2f(src[i]);
}

extern "C" int wft_cast_f32_bf16(const float* src, wft_bf16* dst, int64_t n, void* stream) {
  WFT_CHECK_ARG(src && dst && n >= 0, "bad args");
  WFT_CHECK_ARG((((uintptr_t)src) & 15) == 0 && (((uintptr_t)dst) & 15) == 0, "16-byte alignment");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(ew_grid(n / 8 + 1)), dim3(256), 0, (hipStream_t)stream, src, dst, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
extern "C" int wft_cast_bf16_f32(const wft_bf16* src, float* dst, int64_t n, void* stream) {
  WFT_CHECK_ARG(src && dst && n >= 0, "bad args");
  if (n == 0) return WFT_OK;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, src, dst, (long)n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// src f32 [rows, cols] -> dst bf16 [rows_pad, cols_pad], dst_t bf16 [cols_pad, rows_pad]; 64x64 tiles via LDS.
// Each thread moves 4 consecutive elements (16-B loads, 8-B stores) on both the straight and the transposed side;
// `fast` = every pointer / leading dimension allows that (checked on the host), otherwise element-wise.
__global__ __launch_bounds__(256) void cast_pad_t_kernel(const float* src, long rows, long cols, unsigned short* dst,
                                                          unsigned short* dst_t, long rows_pad, long cols_pad,
                                                          long ld_dst, long ld_dst_t, int fast, float fs) {
  // fs (fwd_scale): dst = bf16(fs * src) — ONE rounding of the scaled value — while dst_t stays bf16(src): the softmax scale folded
  // into the forward shadow of an attention q projection (wft_attn_args.q_prescaled)
  __shared__ unsigned short tile[64][68];
  const long r0 = (long)blockIdx.y * 64, c0 = (long)blockIdx.x * 64;
  if (fast) {
    const int q = threadIdx.x & 15, rr0 = threadIdx.x >> 4;  // 16 threads x 4 columns per row, 16 rows per pass
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int rr = pass * 16 + rr0;
      const long r = r0 + rr, c = c0 + q * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rows && c + 3 < cols) v = *(const f32x4*)(src + r * cols + c);
      else if (r < rows) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (c + e < cols) ? src[r * cols + c + e] : 0.f;
      }
      const u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *(u32x2*)&tile[rr][q * 4] = pk;
      const u32x2 pf = {pack2bf(v[0] * fs, v[1] * fs), pack2bf(v[2] * fs, v[3] * fs)};
      if (r < rows_pad && c < cols_pad) *(u32x2*)(dst + r * ld_dst + c) = pf;  // cols_pad % 4 == 0 in fast mode
    }
    if (dst_t) {
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int cc = pass * 16 + rr0;  // transposed row = source column
        const long c = c0 + cc, r = r0 + q * 4;
        if (c < cols_pad && r < rows_pad) {
          const u32x2 pk = {(unsigned)tile[q * 4][cc] | ((unsigned)tile[q * 4 + 1][cc] << 16),
                            (unsigned)tile[q * 4 + 2][cc] | ((unsigned)tile[q * 4 + 3][cc] << 16)};
          *(u32x2*)(dst_t + c * ld_dst_t + r) = pk;  // rows_pad % 4 == 0 in fast mode
        }
      }
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const long r = r0 + rr, c = c0 + tx;
    unsigned short v = 0, vf = 0;
    if (r < rows && c < cols) { v = f2bf(src[r * cols + c]); vf = f2bf(src[r * cols + c] * fs); }
    tile[rr][tx] = v;
    if (r < rows_pad && c < cols_pad) dst[r * ld_dst + c] = vf;
  }
  if (dst_t) {
    __syncthreads();
    for (int cc = ty; cc < 64; cc += 4) {
      const long c = c0 + cc, r = r0 + tx;
      if (c < cols_pad && r < rows_pad) dst_t[c * ld_dst_t + r] = tile[tx][cc];
    }
  }
}
extern "C" int wft_cast_pad_transpose_f32_bf16(const float* src, int64_t rows, int64_t cols, wft_bf16* dst,
                                               wft_bf16* dst_t, int64_t rows_pad, int64_t cols_pad, int64_t ld_dst,
                                               int64_t ld_dst_t, float fwd_scale, void* stream) {
  WFT_CHECK_ARG(src && dst, "null pointer");
  if (fwd_scale == 0.f) fwd_scale = 1.f;
  WFT_CHECK_ARG(rows >= 1 && cols >= 1 && rows_pad >= rows && cols_pad >= cols, "bad shape");
  WFT_CHECK_ARG(ld_dst >= cols_pad && (!dst_t || ld_dst_t >= rows_pad), "leading dimensions too small");
  dim3 grid((unsigned)((cols_pad + 63) / 64), (unsigned)((rows_pad + 63) / 64));
  const int fast = cols % 4 == 0 && cols_pad % 4 == 0 && rows_pad % 4 == 0 && ld_dst % 4 == 0 && (!dst_t || ld_dst_t % 4 == 0) &&
                   (((uintptr_t)src) & 15) == 0 && (((uintptr_t)dst) & 7) == 0 && (!dst_t || (((uintptr_t)dst_t) & 7) == 0);
  hipLaunchKernelGGL(cast_pad_t_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, (long)rows, (long)cols, dst, dst_t,
                     (long)rows_pad, (long)cols_pad, (long)ld_dst, (long)ld_dst_t, fast, fwd_scale);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// W_eff = W + scaling * B (A ⊙ mask): minLoRA's parametrized weight (merge: model/lora.py:83-89).
// Written as bf16 [rows_pad, cols_pad] (+ transposed) for the GEMMs and/or as f32 [rows, cols] (merge_lora; may alias W).
// 64x64 tiles; the tile's B rows and (masked, scaled) A columns sit in LDS: r <= 64 FMAs per element, HBM-bound.
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* W, long rows, long cols, const float* Bm, const float* Am,
                                                          const float* mask, int r, float scaling, unsigned short* dst,
                                                          unsigned short* dst_t, long rows_pad, long cols_pad, long ld_dst,
                                                          long ld_dst_t, float* dst_f32, int fast, float fs) {
  __shared__ unsigned short tile[64][68];
  __shared__ float bs[64][65];                                  // bs[i][q] = B[r0 + i][q]
  __shared__ __attribute__((aligned(16))) float as[64][68];     // as[q][j] = scaling * A[q][c0 + j] * mask[c0 + j]
  const long r0 = (long)blockIdx.y * 64, c0 = (long)blockIdx.x * 64;
  for (int i = threadIdx.x; i < 64 * r; i += 256) {
    const int a = i / r, q = i - a * r;
    bs[a][q] = (r0 + a < rows) ? Bm[(r0 + a) * r + q] : 0.f;
  }
  for (int i = threadIdx.x; i < 64 * r; i += 256) {
    const int q = i >> 6, j = i & 63;
    const long c = c0 + j;
    as[q][j] = (c < cols) ? scaling * Am[(long)q * cols + c] * (mask ? mask[c] : 1.f) : 0.f;
  }
  __syncthreads();
  if (fast) {  // 4 consecutive columns per thread: 16-B loads of W / A, 8-B stores both ways (cf. cast_pad_t_kernel)
    const int q4 = threadIdx.x & 15, rr0 = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int rr = pass * 16 + rr0;
      const long rw = r0 + rr, c = c0 + q4 * 4;
      f32x4 w = {0.f, 0.f, 0.f, 0.f};
      const bool in = rw < rows && c + 3 < cols;
      if (in) {
        w = *(const f32x4*)(W + rw * cols + c);
        for (int q = 0; q < r; ++q) {
          const float bq = bs[rr][q];
          const f32x4 a4 = *(const f32x4*)&as[q][q4 * 4];
          w[0] = fmaf(bq, a4[0], w[0]); w[1] = fmaf(bq, a4[1], w[1]); w[2] = fmaf(bq, a4[2], w[2]); w[3] = fmaf(bq, a4[3], w[3]);
        }
        if (dst_f32) *(f32x4*)(dst_f32 + rw * cols + c) = w;
      } else if (rw < rows) {
        for (int e = 0; e < 4; ++e)
          if (c + e < cols) {
            float acc = W[rw * cols + c + e];
            for (int q = 0; q < r; ++q) acc = fmaf(bs[rr][q], as[q][q4 * 4 + e], acc);
            w[e] = acc;
            if (dst_f32) dst_f32[rw * cols + c + e] = acc;
          }
      }
      const u32x2 pk = {pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};
      *(u32x2*)&tile[rr][q4 * 4] = pk;
      const u32x2 pf = {pack2bf(w[0] * fs, w[1] * fs), pack2bf(w[2] * fs, w[3] * fs)};  // (fs: see cast_pad_t_kernel)
      if (dst && rw < rows_pad && c < cols_pad) *(u32x2*)(dst + rw * ld_dst + c) = pf;
    }
    if (dst_t) {
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int cc = pass * 16 + rr0;
        const long c = c0 + cc, rw = r0 + q4 * 4;
        if (c < cols_pad && rw < rows_pad) {
          const u32x2 pk = {(unsigned)tile[q4 * 4][cc] | ((unsigned)tile[q4 * 4 + 1][cc] << 16),
                            (unsigned)tile[q4 * 4 + 2][cc] | ((unsigned)tile[q4 * 4 + 3][cc] << 16)};
          *(u32x2*)(dst_t + c * ld_dst_t + rw) = pk;
        }
      }
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int rr = ty; rr < 64; rr += 4) {
    const long rw = r0 + rr, c = c0 + tx;
    unsigned short v = 0, vf = 0;
    if (rw < rows && c < cols) {
      float acc = W[rw * cols + c];
      for (int q = 0; q < r; ++q) acc = fmaf(bs[rr][q], as[q][tx], acc);
      if (dst_f32) dst_f32[rw * cols + c] = acc;
      v = f2bf(acc);
      vf = f2bf(acc * fs);
    }
    tile[rr][tx] = v;
    if (dst && rw < rows_pad && c < cols_pad) dst[rw * ld_dst + c] = vf;
  }
  if (dst_t) {
    __syncthreads();
    for (int cc = ty; cc < 64; cc += 4) {
      const long c = c0 + cc, rw = r0 + tx;
      if (c < cols_pad && rw < rows_pad) dst_t[c * ld_dst_t + rw] = tile[tx][cc];
    }
  }
}
extern "C" int wft_lora_merge(const float* W, int64_t rows, int64_t cols, const float* B, const float* A, const float* mask,
                              int rank, float scaling, wft_bf16* dst, wft_bf16* dst_t, int64_t rows_pad, int64_t cols_pad,
                              int64_t ld_dst, int64_t ld_dst_t, float* dst_f32, float fwd_scale, void* stream) {
  WFT_CHECK_ARG(W && B && A && (dst || dst_f32), "null pointer");
  if (fwd_scale == 0.f) fwd_scale = 1.f;
  WFT_CHECK_ARG(rows >= 1 && cols >= 1 && rank >= 1 && rank <= 64, "rank must be in 1..64");
  WFT_CHECK_ARG(!dst || (rows_pad >= rows && cols_pad >= cols && ld_dst >= cols_pad), "bad bf16 destination shape");
  WFT_CHECK_ARG(!dst_t || (dst && ld_dst_t >= rows_pad), "transposed destination needs dst and ld_dst_t >= rows_pad");
  if (!dst) { rows_pad = rows; cols_pad = cols; }
  dim3 grid((unsigned)((cols_pad + 63) / 64), (unsigned)((rows_pad + 63) / 64));
  const int fast = cols % 4 == 0 && cols_pad % 4 == 0 && rows_pad % 4 == 0 && (!dst || ld_dst % 4 == 0) && (!dst_t || ld_dst_t % 4 == 0) &&
                   (((uintptr_t)W) & 15) == 0 && (!dst || (((uintptr_t)dst) & 7) == 0) && (!dst_t || (((uintptr_t)dst_t) & 7) == 0) &&
                   (!dst_f32 || (((uintptr_t)dst_f32) & 15) == 0);
  hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, (hipStream_t)stream, W, (long)rows, (long)cols, B, A, mask, rank,
                     scaling, dst, dst_t, (long)rows_pad, (long)cols_pad, (long)ld_dst, (long)ld_dst_t, dst_f32, fast, fwd_scale);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// Operands of the rank-r adapter-gradient GEMMs of ONE adapter inside its Linear group's padded buffers (zero-initialised by
// the caller once; only this adapter's blocks are written):
//   Am [Rpad, K]  rows ro..ro+r  = bf16(scaling * A * mask)      AmT [K, Rpad] its transpose        (u = x Am^T carries s)
//   Bb [Npad, Rpad] block (no..no+n, ro..ro+r) = bf16(scaling * B)   BbT [Rpad, Npad] its transpose (du = dy Bb carries s)
// so dA = (du^T x) * mask and dB = dy^T u need no further scaling.  One launch instead of two element-wise multiplies and two
// cast/transposes per group; the data is a few tens of KB.
__global__ __launch_bounds__(256) void lora_pack_kernel(const float* A, const float* mask, const float* B, int r, long K, long n,
                                                         float scaling, unsigned short* Am, unsigned short* AmT, unsigned short* Bb,
                                                         unsigned short* BbT, long rpad, long npad, long ro, long no) {
  const long na = (long)r * K, nb = n * r;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (long)gridDim.x * 256) {
    if (i < na) {
      const long q = i / K, c = i - q * K;
      const unsigned short v = f2bf(scaling * A[i] * (mask ? mask[c] : 1.f));
      Am[(ro + q) * K + c] = v;
      AmT[c * rpad + ro + q] = v;
    } else {
      const long j = i - na, row = j / r, q = j - row * r;
      const unsigned short v = f2bf(scaling * B[j]);
      Bb[(no + row) * rpad + ro + q] = v;
      BbT[(ro + q) * npad + no + row] = v;
    }
  }
}
extern "C" int wft_lora_pack(const float* A, const float* mask, const float* B, int rank, int64_t K, int64_t n, float scaling,
                             wft_bf16* Am, wft_bf16* AmT, wft_bf16* Bb, wft_bf16* BbT, int64_t rpad, int64_t npad, int64_t ro,
                             int64_t no, void* stream) {
  WFT_CHECK_ARG(A && B && Am && AmT && Bb && BbT, "null pointer");
  WFT_CHECK_ARG(rank >= 1 && K >= 1 && n >= 1 && ro >= 0 && no >= 0 && ro + rank <= rpad && no + n <= npad, "bad shape");
  const int64_t total = (int64_t)rank * K + n * rank;
  hipLaunchKernelGGL(lora_pack_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, A, mask, B, rank, (long)K, (long)n,
                     scaling, Am, AmT, Bb, BbT, (long)rpad, (long)npad, (long)ro, (long)no);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// All adapters of a model in ONE launch: wft_lora_merge (bf16 shadow + transposed shadow) and wft_lora_pack for every row of
// the table — what the 2 x 512 per-Linear launches of a large-v3 LoRA forward/backward do, once per forward, right after the
// dropout masks are drawn.  Row layout (int64 x WFT_LORA_MT_FIELDS): see wft.h.  Blocks are 64x64 tiles of the weights, found by
// bisection over tile_start; the tile in the first row band also writes its 64 columns of Am / AmT, the tile in the first column
// band its 64 rows of Bb / BbT (the values are already in LDS for the merge).  Every value is computed exactly as by the
// per-adapter kernels.
#define WFT_LORA_MT_FIELDS 20
__global__ __launch_bounds__(256) void lora_refresh_mt_kernel(const long* tab, const int* tile_start, int n) {
  __shared__ unsigned short tile[64][68];
  __shared__ float bs[64][65];
  __shared__ __attribute__((aligned(16))) float as[64][68];
  int lo = 0, hi = n - 1;
  const int bid = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  const long* e = tab + (long)lo * WFT_LORA_MT_FIELDS;
  const float* W = (const float*)e[0];
  const long rows = e[1], cols = e[2];
  const float* Bm = (const float*)e[3];
  const float* Am = (const float*)e[4];
  const float* mask = (const float*)e[5];
  const int r = (int)e[6];
  const float scaling = __int_as_float((int)(e[7] & 0xffffffffL));
  const int fsb = (int)(e[7] >> 32);  // bits 32..63: fwd_scale as f32 bits (0 = 1.0): dst = bf16(fs * w), dst_t = bf16(w) — see cast_pad_t_kernel
  const float fs = fsb ? __int_as_float(fsb) : 1.f;
  unsigned short* dst = (unsigned short*)e[8];
  unsigned short* dst_t = (unsigned short*)e[9];
  const long ld_dst = e[10], ld_dst_t = e[11];
  unsigned short* pAm = (unsigned short*)e[12];
  unsigned short* pAmT = (unsigned short*)e[13];
  unsigned short* pBb = (unsigned short*)e[14];
  unsigned short* pBbT = (unsigned short*)e[15];
  const long rpad = e[16], npad = e[17], ro = e[18], no = e[19];
  const int t = bid - tile_start[lo];
  const int tiles_x = (int)(cols >> 6);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const long r0 = (long)ty * 64, c0 = (long)tx * 64;
  for (int i = threadIdx.x; i < 64 * r; i += 256) {
    const int a = i / r, q = i - a * r;
    bs[a][q] = Bm[(r0 + a) * r + q];
  }
  for (int i = threadIdx.x; i < 64 * r; i += 256) {
    const int q = i >> 6, j = i & 63;
    const long c = c0 + j;
    as[q][j] = scaling * Am[(long)q * cols + c] * (mask ? mask[c] : 1.f);
  }
  __syncthreads();
  if (pAm && ty == 0)
    for (int i = threadIdx.x; i < 64 * r; i += 256) {
      const int q = i >> 6, j = i & 63;
      const unsigned short v = f2bf(as[q][j]);
      pAm[(ro + q) * cols + c0 + j] = v;
      pAmT[(c0 + j) * rpad + ro + q] = v;
    }
  if (pBb && tx == 0)
    for (int i = threadIdx.x; i < 64 * r; i += 256) {
      const int a = i / r, q = i - a * r;
      const unsigned short v = f2bf(scaling * bs[a][q]);
      pBb[(no + r0 + a) * rpad + ro + q] = v;
      pBbT[(ro + q) * npad + no + r0 + a] = v;
    }
  const int q4 = threadIdx.x & 15, rr0 = threadIdx.x >> 4;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int rr = pass * 16 + rr0;
    const long rw = r0 + rr, c = c0 + q4 * 4;
    f32x4 w = *(const f32x4*)(W + rw * cols + c);
    for (int q = 0; q < r; ++q) {
      const float bq = bs[rr][q];
      const f32x4 a4 = *(const f32x4*)&as[q][q4 * 4];
      w[0] = fmaf(bq, a4[0], w[0]); w[1] = fmaf(bq, a4[1], w[1]); w[2] = fmaf(bq, a4[2], w[2]); w[3] = fmaf(bq, a4[3], w[3]);
    }
    const u32x2 pk = {pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};
    *(u32x2*)&tile[rr][q4 * 4] = pk;
    const u32x2 pf = {pack2bf(w[0] * fs, w[1] * fs), pack2bf(w[2] * fs, w[3] * fs)};
    *(u32x2*)(dst + rw * ld_dst + c) = pf;
  }
  if (dst_t) {
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int cc = pass * 16 + rr0;
      const long c = c0 + cc, rw = r0 + q4 * 4;
      const u32x2 pk = {(unsigned)tile[q4 * 4][cc] | ((unsigned)tile[q4 * 4 + 1][cc] << 16),
                        (unsigned)tile[q4 * 4 + 2][cc] | ((unsigned)tile[q4 * 4 + 3][cc] << 16)};
      *(u32x2*)(dst_t + c * ld_dst_t + rw) = pk;
    }
  }
}
extern "C" int wft_lora_refresh_mt(const void* tab, const int32_t* tile_start, int n, int total_tiles, void* stream) {
  WFT_CHECK_ARG(tab && tile_start && n >= 0 && total_tiles >= 0, "bad args");
  if (n == 0 || total_tiles == 0) return WFT_OK;
  hipLaunchKernelGGL(lora_refresh_mt_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, (const long*)tab,
                     (const int*)tile_start, n);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// n small f32 copies in one launch (tab: int64 [n][3] = source address, destination address, element count): the stacked bias
// vectors of the fused q/k/v groups after an optimizer step.  160 torch copy_ calls per step did this before, each a blit
// launch of its own with ~40 us between two of them (profiles/r03_headline_gap_analysis.log).
__global__ __launch_bounds__(256) void mt_copy_f32_kernel(const long* tab) {
  const long* row = tab + 3 * (long)blockIdx.x;
  const float* src = (const float*)row[0];
  float* dst = (float*)row[1];
  const long n = row[2] & 0xffffffffL;
  const int fsb = (int)(row[2] >> 32);  // bits 32..63 of the count field: a scale as f32 bits (0 = plain copy): the q slice of a fused bias
  if (fsb) {
    const float fs = __int_as_float(fsb);
    for (long i = threadIdx.x; i < n; i += 256) dst[i] = src[i] * fs;
  } else {
    for (long i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
  }
}
extern "C" int wft_mt_copy_f32(const void* tab, int n, void* stream) {
  WFT_CHECK_ARG(tab && n >= 1, "bad args");
  hipLaunchKernelGGL(mt_copy_f32_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const long*)tab);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- int8 image of a shadow
// Per-row symmetric quantisation (wft.h states the definition): one wave per row, four rows per workgroup; a lane takes 16 columns
// per pass (two 16-byte loads, one 16-byte store).  Two sweeps over the row — amax, then the bytes; the second one hits L2.  Every
// f32 operation is a correctly rounded one of its own (__fdiv_rn / __fmul_rn: nothing for the compiler to contract).
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const unsigned short* __restrict__ W, long rows, int cols, long ldw,
                                                               signed char* __restrict__ Q, long ldq, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const unsigned short* w = W + row * ldw;
  float amax = 0.f;
  for (int c = lane * 16; c < cols; c += 1024) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v[8];
      bf8_unpack(*(const u32x4*)(w + c + 8 * h), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
    }
  }
  amax = wave_max(amax);
  const float inv = amax > 0.f ? __fdiv_rn(127.0f, amax) : 0.0f;
  if (lane == 0) scale[row] = __fdiv_rn(amax, 127.0f);
  signed char* q = Q + row * ldq;
  for (int c = lane * 16; c < cols; c += 1024) {
    u32x4 out;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v[8];
      bf8_unpack(*(const u32x4*)(w + c + 8 * h), v);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        unsigned pk = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = fminf(fmaxf(rintf(__fmul_rn(v[4 * d + e], inv)), -127.0f), 127.0f);
          pk |= ((unsigned)(int)t & 0xffu) << (8 * e);
        }
        out[2 * h + d] = pk;
      }
    }
    *(u32x4*)(q + c) = out;
  }
}
extern "C" int wft_quantize_rows_i8(const wft_bf16* W, int64_t rows, int64_t cols, int64_t ldw, int8_t* Q, int64_t ldq, float* scale,
                                    void* stream) {
  WFT_CHECK_ARG(W && Q && scale, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && cols >= 64 && cols % 64 == 0 && cols < (1ll << 31), "cols must be a multiple of 64");
  WFT_CHECK_ARG(ldw >= cols && ldw % 8 == 0 && ldq >= cols && ldq % 16 == 0, "ldw % 8 == 0 and ldq % 16 == 0");
  WFT_CHECK_ARG((((uintptr_t)W | (uintptr_t)Q) & 15) == 0 && ((uintptr_t)scale & 3) == 0, "W and Q must be 16-byte aligned");
  hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)W,
                     (long)rows, (int)cols, (long)ldw, (signed char*)Q, (long)ldq, scale);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
