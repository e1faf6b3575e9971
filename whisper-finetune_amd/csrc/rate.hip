// rate.hip — resampling at a per-row fractional rate over a ragged batch (include/wft.h "Per-row rate conversion" is the contract).
//
// Two entry points, one launch each, a grid of (tiles, B) workgroups of 256 threads, thread t owning outputs m0 + t + 256 q so that
// neighbouring lanes store neighbouring outputs:
//   wft_sinc_resample_rows_f32   the Hann-windowed sinc of wft_resample_f32 in its continuous form, the ratio a float64 per row.  A
//                                workgroup stages the input span of its outputs in LDS (RS_STAGE floats; the tile is sized by the
//                                host's lower bound of the ratios so that the span fits), then every output sums its taps in ascending
//                                j in fp64.  A tap's weight is evaluated directly: one sinpi, one cospi and one division per tap (the
//                                naive form; 13 taps at a ratio >= 1, 25 at 0.5).
//   wft_alias_f32                audiomentations' Aliasing: np.interp down to a coarser grid and back, fused: an output needs two
//                                intermediate values and each of those two samples, found by a direct index (no search) and read
//                                through the caches (neighbouring outputs share them).
// Side kernels of the loader: plain C++, nothing hand-scheduled.  The fp64 arithmetic is the contract, so contraction is off.
#include "common.h"

#pragma clang fp contract(off)

#define RT_T 256                  // threads per workgroup
#define RS_TILE_MAX 1024          // outputs per workgroup at most
#define RS_STAGE 1600             // floats of the staging buffer
#define RS_HALO 14                // staged samples in front of floor(m0 / ratio): taps reach 13 below floor(t0)
#define RS_SPAN (RS_STAGE - 32)   // tile / ratio_lo may not pass this: (tile - 1) / ratio + 1 + 13 + RS_HALO + 1 <= RS_STAGE
#define AL_TILE 1024              // outputs per workgroup of the alias kernel
#define RT_MAX_N (1 << 30)
#define RT_PI 3.141592653589793

__device__ __forceinline__ int rt_row_len(const int* n, int b, int n_max) { return n ? min(max(n[b], 0), n_max) : n_max; }

// ------------------------------------------------------------------------------------------------------------ sinc resampler
__global__ __launch_bounds__(RT_T) void rt_sinc_kernel(const float* in, long ld_in, const int* n_in, int n_in_max, const double* ratio,
                                                       double ratio_lo, float* out, long ld_out, int n_out, int tile) {
  __shared__ float stage[RS_STAGE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long m0 = (long)blockIdx.x * tile;
  const int cnt = (int)min((long)tile, (long)n_out - m0);  // >= 1 by the grid
  float* orow = out + b * ld_out;
  const double rho = ratio[b];
  const int N = rt_row_len(n_in, b, n_in_max);
  long limit = 0;  // outputs [0, limit) follow the formula, [limit, n_out) are zero (librosa's fix_length)
  if (rho >= ratio_lo && rho <= 2.0) limit = min((long)n_out, (long)ceil((double)N * rho));  // false for NaN
  if (m0 >= limit) {  // uniform
    for (int q = tid; q < cnt; q += RT_T) orow[m0 + q] = 0.f;
    return;
  }
  const float* row = in + b * ld_in;
  const long jb = (long)floor((double)m0 / rho) - RS_HALO;
  const long m_last = min(m0 + cnt, limit) - 1;
  const long need = (long)floor((double)m_last / rho) + RS_HALO + 1 - jb;
  const int span = (int)min(need, (long)RS_STAGE);  // (need <= RS_STAGE whenever rho >= ratio_lo: the tile is sized for it)
  for (int s = tid; s < span; s += RT_T) {
    const long j = jb + s;
    stage[s] = (j >= 0 && j < N) ? row[j] : 0.f;
  }
  __syncthreads();
  const double c = 0.99 * fmin(1.0, rho);
  const int K = (int)(6.0 / c) + 1;  // |c (k - f)| < 6 with 0 <= f < 1 needs -K < k <= K
  for (int q = tid; q < cnt; q += RT_T) {
    const long m = m0 + q;
    float r = 0.f;
    if (m < limit) {
      const double t0 = (double)m / rho;
      const long i0 = (long)floor(t0);
      const int s0 = (int)(i0 - jb);
      double acc = 0.0;
      for (int k = -K; k <= K; ++k) {
        const double t = (double)(i0 + k) - t0;
        const double a = c * t;
        const int s = s0 + k;
        if (fabs(a) < 6.0 && s >= 0 && s < span) {
          const double w = cospi(a / 12.0);
          const double snc = a == 0.0 ? 1.0 : sinpi(a) / (RT_PI * a);
          const double g = (c * snc) * (w * w);
          acc += (double)stage[s] * g;
        }
      }
      r = (float)acc;
    }
    orow[m] = r;
  }
}

// ------------------------------------------------------------------------------------------------------------ alias
// np.linspace(0, n, num): point k is k * step, the last point is n itself
__device__ __forceinline__ double rt_grid(long k, long num, double step, double n_d) { return k == num - 1 ? n_d : (double)k * step; }

// the largest index whose grid point is <= t (0 <= t <= n): floor(t / step), corrected against the formed grid values
__device__ __forceinline__ long rt_locate(double t, long num, double step, double n_d) {
  long k = (long)floor(t / step);
  k = min(max(k, 0l), num - 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (k > 0 && rt_grid(k, num, step, n_d) > t) --k;
    else if (k < num - 1 && rt_grid(k + 1, num, step, n_d) <= t) ++k;
  }
  return k;
}

// np.interp(u_k, x, samples): the intermediate value at point k of the coarse grid
__device__ __forceinline__ double rt_inner(const float* row, long k, long n, long d, double step_x, double step_u, double n_d) {
  const double t = rt_grid(k, d, step_u, n_d);
  const long j = rt_locate(t, n, step_x, n_d);
  const double f0 = (double)row[j];
  const double g0 = rt_grid(j, n, step_x, n_d);
  if (j == n - 1 || g0 == t) return f0;
  const double f1 = (double)row[j + 1];
  const double slope = (f1 - f0) / (rt_grid(j + 1, n, step_x, n_d) - g0);
  return slope * (t - g0) + f0;
}

__global__ __launch_bounds__(RT_T) void rt_alias_kernel(const float* in, long ld_in, const int* n, int n_max, const double* new_rate,
                                                        double sample_rate, float* out, long ld_out) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long nb = rt_row_len(n, b, n_max);
  const long i0 = (long)blockIdx.x * AL_TILE;
  const int cnt = (int)min((long)AL_TILE, (long)n_max - i0);
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const double rate = new_rate[b];
  const double n_d = (double)nb;
  const double dq = rint((n_d * rate) / sample_rate);       // half to even: Python's round of the same two operations
  const bool active = rate != 0.0 && nb >= 2 && dq >= 2.0 && dq <= 4294967296.0;  // false for NaN; otherwise the row is a copy
  if (!active) {  // uniform
    for (int q = tid; q < cnt; q += RT_T) orow[i0 + q] = i0 + q < nb ? row[i0 + q] : 0.f;
    return;
  }
  const long d = (long)dq;
  const double step_x = n_d / (double)(nb - 1), step_u = n_d / (double)(d - 1);
  for (int q = tid; q < cnt; q += RT_T) {
    const long i = i0 + q;
    float r = 0.f;
    if (i < nb) {
      const double t = rt_grid(i, nb, step_x, n_d);
      const long k = rt_locate(t, d, step_u, n_d);
      const double v0 = rt_inner(row, k, nb, d, step_x, step_u, n_d);
      const double g0 = rt_grid(k, d, step_u, n_d);
      double y = v0;
      if (k != d - 1 && g0 != t) {
        const double v1 = rt_inner(row, k + 1, nb, d, step_x, step_u, n_d);
        const double slope = (v1 - v0) / (rt_grid(k + 1, d, step_u, n_d) - g0);
        y = slope * (t - g0) + v0;
      }
      r = (float)y;
    }
    orow[i] = r;
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static inline bool rt_disjoint(const float* in, int64_t ld_in, int64_t w_in, const float* out, int64_t ld_out, int64_t w_out, int B) {
  const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (B - 1) * ld_in + w_in);
  const uintptr_t o0 = (uintptr_t)out, o1 = (uintptr_t)(out + (B - 1) * ld_out + w_out);
  return i1 <= o0 || o1 <= i0;
}

extern "C" int wft_sinc_resample_rows_tile(double ratio_lo) {
  if (!(ratio_lo >= 0.5 && ratio_lo <= 2.0)) return 0;
  const int fit = (int)((double)RS_SPAN * ratio_lo) / 4 * 4;
  return fit < RS_TILE_MAX ? fit : RS_TILE_MAX;
}

extern "C" int wft_sinc_resample_rows_f32(const float* in, int64_t ld_in, const int32_t* n_in, int64_t n_in_max, const double* ratio,
                                          double ratio_lo, float* out, int64_t ld_out, int64_t n_out, int B, void* stream) {
  WFT_CHECK_ARG(in && n_in && ratio && out, "null pointer");
  WFT_CHECK_ARG(ratio_lo >= 0.5 && ratio_lo <= 2.0, "ratio_lo outside [0.5, 2.0]");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_in_max >= 1 && n_in_max <= RT_MAX_N && n_out >= 1 && n_out <= RT_MAX_N,
                "bad shape (1 <= n_in_max, n_out <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_in >= n_in_max && ld_out >= n_out, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n_in % 4 == 0 && (uintptr_t)ratio % 8 == 0,
                "in / out / n_in must be 4-byte, ratio 8-byte aligned");
  WFT_CHECK_ARG(rt_disjoint(in, ld_in, n_in_max, out, ld_out, n_out, B), "in and out overlap");
  const int tile = wft_sinc_resample_rows_tile(ratio_lo);
  WFT_CHECK_ARG(tile >= 4, "no tile for this ratio_lo");
  const dim3 grid((unsigned)cdiv64(n_out, tile), (unsigned)B);
  hipLaunchKernelGGL(rt_sinc_kernel, grid, dim3(RT_T), 0, (hipStream_t)stream, in, (long)ld_in, n_in, (int)n_in_max, ratio, ratio_lo, out,
                     (long)ld_out, (int)n_out, tile);
  WFT_CHECK_LAUNCH_AS("wft_sinc_resample_rows_f32");
  return WFT_OK;
}

extern "C" int wft_alias_tile(void) { return AL_TILE; }

extern "C" int wft_alias_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const double* new_rate, double sample_rate,
                             float* out, int64_t ld_out, int B, void* stream) {
  WFT_CHECK_ARG(in && new_rate && out, "null pointer");
  WFT_CHECK_ARG(sample_rate > 0.0 && sample_rate <= 1e9, "sample_rate must lie in (0, 1e9]");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= RT_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)new_rate % 8 == 0,
                "in / out / n must be 4-byte, new_rate 8-byte aligned");
  WFT_CHECK_ARG(rt_disjoint(in, ld_in, n_max, out, ld_out, n_max, B), "in and out overlap");
  const dim3 grid((unsigned)cdiv64(n_max, AL_TILE), (unsigned)B);
  hipLaunchKernelGGL(rt_alias_kernel, grid, dim3(RT_T), 0, (hipStream_t)stream, in, (long)ld_in, n, (int)n_max, new_rate, sample_rate, out,
                     (long)ld_out);
  WFT_CHECK_LAUNCH_AS("wft_alias_f32");
  return WFT_OK;
}
