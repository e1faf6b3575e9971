// office.hip — the office pipeline's room reverb and bit crush over a ragged batch (include/wft.h "Office effects" is the contract).
//
//   wft_fir_conv_f32   a causal FIR per row, each row with an impulse response of its own length: uniform-partitioned overlap-save in
//                      f32 on the 2048-point LDS FFT of fft2048.h, OF_L = 1024 new outputs per block.
//       pass 1  one workgroup per (partition p, row): taps [p * 1024, (p + 1) * 1024) of the row's IR, zero-padded to 2048 -> FFT ->
//               H[b][p][0..1024] in the workspace.  A partition wholly behind n_taps[b] is not written: pass 2 never reads it.
//       pass 2  one workgroup per (output block k, row): for every live partition p (p < ceil(T / 1024) and p <= k: an earlier segment
//               is all zeros) the segment x[(k - p - 1) * 1024 .. (k - p + 1) * 1024) -> LDS -> FFT, X * H_p accumulated over the
//               one-sided bins in registers in ascending p (thread t owns bins t, t + 256, t + 512, t + 768; thread 0 also 1024);
//               then ONE inverse FFT of the Hermitian extension, the last 1024 reals scaled by 1 / 2048, stored where i < N.
//               The forward FFT of a segment is recomputed per partition: the right trade at the room IRs' P <= 2, and the workspace
//               stays at B * P * 1025 complex numbers.
//       The live partitions depend on T and k only, never on taps_max or B: a row's bits do not depend on them either.
//   wft_bitcrush_f32   audiomentations' BitCrush: rintf(x * q) / q with q = 2^(bits - 1) + 1, one thread per sample, contraction off.
// Side kernels of the loader: plain C++, nothing hand-scheduled.  16 KB of block plus 8 KB of twiddles per workgroup.
#include "common.h"
#include "fft2048.h"

#define OF_L (ST_N / 2)           // new outputs per FFT block
#define OF_TAPS_MAX 8192
#define OF_MAX_N (1 << 30)
#define OF_T 256                  // threads per workgroup of the bit crush
#define OF_TILE 1024              // samples per workgroup of the bit crush

__device__ __forceinline__ int of_clamp(const int* v, int b, int hi) { return v ? min(max(v[b], 0), hi) : hi; }

// ------------------------------------------------------------------------------------------------------------ pass 1: IR spectra
__global__ __launch_bounds__(ST_THREADS) void of_ir_fft_kernel(const float* ir, long ld_ir, const int* n_taps, int taps_max, f32x2* H,
                                                               int P) {
  __shared__ __attribute__((aligned(8))) f32x2 x[ST_N];
  __shared__ __attribute__((aligned(8))) f32x2 tw[ST_N / 2];
  const int tid = threadIdx.x, p = blockIdx.x, b = blockIdx.y;
  const int T = of_clamp(n_taps, b, taps_max);
  if (p * OF_L >= T) return;  // uniform: wholly behind the row's taps
  st_twiddles(tw, tid);
  const float* row = ir + b * ld_ir;
  for (int i = tid; i < ST_N; i += ST_THREADS) {
    const int j = p * OF_L + i;
    const float v = (i < OF_L && j < T) ? row[j] : 0.f;
    x[st_brev(i)] = f32x2{v, 0.f};
  }
  __syncthreads();
  st_fft<false>(x, tw, tid);
  f32x2* h = H + ((long)b * P + p) * ST_BINS;
  for (int k = tid; k < ST_BINS; k += ST_THREADS) h[k] = x[k];
}

// ------------------------------------------------------------------------------------------------------------ pass 2: overlap-save
__global__ __launch_bounds__(ST_THREADS) void of_conv_kernel(const float* in, long ld_in, const int* n, int n_max, const int* n_taps,
                                                             int taps_max, const f32x2* H, int P, float* out, long ld_out) {
  __shared__ __attribute__((aligned(8))) f32x2 x[ST_N];
  __shared__ __attribute__((aligned(8))) f32x2 tw[ST_N / 2];
  const int tid = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
  const int N = of_clamp(n, b, n_max), T = of_clamp(n_taps, b, taps_max);
  const long i0 = (long)k * OF_L;
  const int cnt = (int)min((long)OF_L, (long)n_max - i0);  // >= 1 by the grid
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out + i0;
  if (i0 >= N || T == 0) {  // uniform: zeros behind the row's end, a bit copy without taps
    for (int q = tid; q < cnt; q += ST_THREADS) orow[q] = (T == 0 && i0 + q < N) ? row[i0 + q] : 0.f;
    return;
  }
  st_twiddles(tw, tid);
  const int live = min((T + OF_L - 1) / OF_L, k + 1);
  f32x2 acc[5];
#pragma unroll
  for (int r = 0; r < 5; ++r) acc[r] = f32x2{0.f, 0.f};
#pragma unroll 1
  for (int p = 0; p < live; ++p) {
    __syncthreads();  // the last partition's products have read x; the twiddles are written
    const long j0 = (long)(k - p - 1) * OF_L;
    for (int i = tid; i < ST_N; i += ST_THREADS) {
      const long j = j0 + i;
      const float v = (j >= 0 && j < N) ? row[j] : 0.f;
      x[st_brev(i)] = f32x2{v, 0.f};
    }
    __syncthreads();
    st_fft<false>(x, tw, tid);
    const f32x2* h = H + ((long)b * P + p) * ST_BINS;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int bin = tid + r * ST_THREADS;
      if (r < 4 || tid == 0) {
        const f32x2 X = x[bin], Hp = h[bin];
        acc[r] = f32x2{acc[r][0] + (X[0] * Hp[0] - X[1] * Hp[1]), acc[r][1] + (X[0] * Hp[1] + X[1] * Hp[0])};
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int bin = tid + r * ST_THREADS;
    if (r < 4 || tid == 0) {
      x[st_brev(bin)] = acc[r];
      if (bin >= 1 && bin < ST_N / 2) x[st_brev(ST_N - bin)] = f32x2{acc[r][0], -acc[r][1]};  // Hermitian extension
    }
  }
  __syncthreads();
  st_fft<true>(x, tw, tid);
  for (int q = tid; q < cnt; q += ST_THREADS) orow[q] = i0 + q < N ? x[OF_L + q][0] * (1.0f / ST_N) : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ bit crush
#pragma clang fp contract(off)
__global__ __launch_bounds__(OF_T) void of_bitcrush_kernel(const float* in, long ld_in, const int* n, int n_max, const int* bits, float* out,
                                                           long ld_out) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int N = of_clamp(n, b, n_max);
  const long i0 = (long)blockIdx.x * OF_TILE;
  const int cnt = (int)min((long)OF_TILE, (long)n_max - i0);
  const float* row = in + b * ld_in + i0;
  float* orow = out + b * ld_out + i0;
  const int d = bits[b];
  const bool crush = d >= 1 && d <= 24;           // anything else: the row is a copy
  const float q = ldexpf(1.0f, crush ? d - 1 : 0) + 1.0f;  // exact: 2^23 + 1 has 24 bits
  for (int s = tid; s < cnt; s += OF_T) {
    float v = 0.f;
    if (i0 + s < N) {
      v = row[s];
      if (crush) v = rintf(v * q) / q;
    }
    orow[s] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static inline bool of_disjoint(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)a_bytes, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)b_bytes;
  return a1 <= b0 || b1 <= a0;
}
static inline int64_t of_rows_bytes(int64_t ld, int64_t w, int B) { return ((int64_t)(B - 1) * ld + w) * (int64_t)sizeof(float); }

extern "C" int wft_fir_conv_block(void) { return OF_L; }

extern "C" int64_t wft_fir_conv_workspace_bytes(int B, int taps_max) {
  if (B < 1 || B > 65535 || taps_max < 1 || taps_max > OF_TAPS_MAX) return -1;
  const int64_t P = (taps_max + OF_L - 1) / OF_L;
  return (int64_t)B * P * ST_BINS * (int64_t)sizeof(f32x2);
}

extern "C" int wft_fir_conv_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const float* ir, int64_t ld_ir,
                                const int32_t* n_taps, int taps_max, float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                                int B, void* stream) {
  WFT_CHECK_ARG(in && ir && out && workspace, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= OF_MAX_N && taps_max >= 1 && taps_max <= OF_TAPS_MAX,
                "bad shape (1 <= n_max <= 2^30, 1 <= taps_max <= 8192, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max && ld_ir >= taps_max, "leading dimension smaller than the row");
  const int64_t need = wft_fir_conv_workspace_bytes(B, taps_max);
  WFT_CHECK_ARG(workspace_bytes >= need, "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)ir % 4 == 0 && (uintptr_t)n % 4 == 0 &&
                    (uintptr_t)n_taps % 4 == 0 && (uintptr_t)workspace % 8 == 0,
                "in / out / ir / n / n_taps must be 4-byte, workspace 8-byte aligned");
  const int64_t in_bytes = of_rows_bytes(ld_in, n_max, B), out_bytes = of_rows_bytes(ld_out, n_max, B);
  WFT_CHECK_ARG(of_disjoint(in, in_bytes, out, out_bytes), "in and out overlap (the convolution cannot run in place)");
  WFT_CHECK_ARG(of_disjoint(ir, of_rows_bytes(ld_ir, taps_max, B), out, out_bytes) && of_disjoint(workspace, need, out, out_bytes) &&
                    of_disjoint(workspace, need, in, in_bytes) && of_disjoint(workspace, need, ir, of_rows_bytes(ld_ir, taps_max, B)),
                "ir, workspace, in and out overlap");
  const int P = (taps_max + OF_L - 1) / OF_L;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(of_ir_fft_kernel, dim3(P, B), dim3(ST_THREADS), 0, s, ir, (long)ld_ir, n_taps, taps_max, (f32x2*)workspace, P);
  hipLaunchKernelGGL(of_conv_kernel, dim3((unsigned)cdiv64(n_max, OF_L), B), dim3(ST_THREADS), 0, s, in, (long)ld_in, n, (int)n_max, n_taps,
                     taps_max, (const f32x2*)workspace, P, out, (long)ld_out);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_bitcrush_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const int32_t* bits, float* out,
                                int64_t ld_out, int B, void* stream) {
  WFT_CHECK_ARG(in && bits && out, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= OF_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)bits % 4 == 0,
                "in / out / n / bits must be 4-byte aligned");
  WFT_CHECK_ARG((in == out && ld_in == ld_out) || of_disjoint(in, of_rows_bytes(ld_in, n_max, B), out, of_rows_bytes(ld_out, n_max, B)),
                "in and out overlap without being the same rows");
  hipLaunchKernelGGL(of_bitcrush_kernel, dim3((unsigned)cdiv64(n_max, OF_TILE), B), dim3(OF_T), 0, (hipStream_t)stream, in, (long)ld_in, n,
                     (int)n_max, bits, out, (long)ld_out);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
