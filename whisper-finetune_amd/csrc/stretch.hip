// stretch.hip — time-stretch augmentation: the phase vocoder of include/wft.h "Time stretch" (N = 2048, H = 512).
//
// Three stages on the caller's workspace, every row on its own (the bits of a row depend on its samples, its rate and n_in only):
//   stft     one workgroup per (frame, row): 2048 zero-centred, Hann-windowed samples -> LDS -> radix-2 FFT -> D[b][t][0..1024]
//   vocoder  one thread per (row, bin), a sequential loop over the output frames: t * rate, its floor and alpha in double, the phase
//            a product of unit complex numbers that is renormalised every step                       -> S[b][t][0..1024]
//   istft    one workgroup per (output frame, row): the Hermitian extension of S[b][t] -> LDS -> inverse FFT -> real part * window / N,
//            written IN PLACE over S[b][t] (2048 floats in the 2050 the frame occupies); then one thread per output sample gathers
//            its <= 4 frames in ascending t and divides by the window's sum of squares.  No atomics anywhere.
// The FFT (fft2048.h, shared with office.hip) is a plain in-place decimation-in-time radix-2 over a bit-reversed load.  The stretch
// is a side kernel of the loader (a few tens of MB per clip): nothing here is hand-scheduled.
#include <float.h>
#include "common.h"
#include "fft2048.h"

#define ST_H 512
#define ST_MAX_IN (1 << 26)  // samples per row: keeps every frame count and sample index far inside 32 bits

// periodic Hann 0.5 - 0.5 cos(2 pi i / 2048) as sin^2(pi i / 2048): a few ulp RELATIVE to the window's own value.  (0.5 - 0.5 cos
// is off by an ulp of 1 — a hundredth of the window at its first samples — and the unwindowed synthesis frame is not small there:
// next to silence, where no other frame covers that error, it showed as 90 times the synthesis' allowance.)
__device__ __forceinline__ float st_window(int i) {
  const float sn = sinpif((float)i * (1.0f / ST_N));
  return sn * sn;
}

// frames of the analysis and, for one row, of the synthesis; n_out.  All in double, as the definition states them.
static inline int st_frames(int64_t n_in) { return (int)(1 + n_in / ST_H); }
__host__ __device__ static inline int st_out_frames(int F, double rate) { return (int)ceil((double)F / rate); }
__device__ __forceinline__ bool st_rate_ok(double rate, double rate_lo) { return rate >= rate_lo && rate <= 2.0; }  // false for NaN

// ------------------------------------------------------------------------------------------------------------ stft
__global__ __launch_bounds__(ST_THREADS) void stretch_stft_kernel(const float* in, long ld_in, int n_in, f32x2* D, int F) {
  __shared__ __attribute__((aligned(8))) f32x2 x[ST_N];
  __shared__ __attribute__((aligned(8))) f32x2 tw[ST_N / 2];
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  st_twiddles(tw, tid);
  __syncthreads();
  const float* row = in + b * ld_in;
  for (int i = tid; i < ST_N; i += ST_THREADS) {
    const int j = t * ST_H + i - ST_N / 2;  // zero centre padding
    const float v = (j >= 0 && j < n_in) ? row[j] : 0.f;
    x[st_brev(i)] = f32x2{st_window(i) * v, 0.f};
  }
  __syncthreads();
  st_fft<false>(x, tw, tid);
  f32x2* d = D + ((long)b * F + t) * ST_BINS;
  for (int k = tid; k < ST_BINS; k += ST_THREADS) d[k] = x[k];
}

// ------------------------------------------------------------------------------------------------------------ vocoder
// u(c) = c / |c|, and 1 whenever |c| == 0, whatever the signs of its zeros
__device__ __forceinline__ f32x2 st_unit(f32x2 c, float mag) {
  return mag == 0.f ? f32x2{1.f, 0.f} : f32x2{c[0] / mag, c[1] / mag};
}
__device__ __forceinline__ float st_abs(f32x2 c) { return sqrtf(c[0] * c[0] + c[1] * c[1]); }

__global__ __launch_bounds__(64) void stretch_vocoder_kernel(const f32x2* D, int F, const double* rates, double rate_lo, f32x2* S,
                                                             int T_max) {
  const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  const double rate = rates[b];
  if (k >= ST_BINS || !st_rate_ok(rate, rate_lo)) return;
  const int T = min(st_out_frames(F, rate), T_max);  // (== for an accepted rate; the min keeps every store inside the row's S)
  const f32x2* d = D + (long)b * F * ST_BINS + k;
  f32x2* s = S + (long)b * T_max * ST_BINS + k;
  f32x2 P = f32x2{1.f, 0.f};
  for (int t = 0; t < T; ++t) {
    const double step = (double)t * rate;
    const double fl = floor(step);
    const int i = (int)fl;  // i <= F - 1 because step < F
    const float alpha = (float)(step - fl);
    const f32x2 zero = f32x2{0.f, 0.f};
    const f32x2 d0 = i < F ? d[(long)i * ST_BINS] : zero;          // D is extended by two zero frames
    const f32x2 d1 = i + 1 < F ? d[(long)(i + 1) * ST_BINS] : zero;
    const float m0 = st_abs(d0), m1 = st_abs(d1);
    const f32x2 u0 = st_unit(d0, m0), u1 = st_unit(d1, m1);
    if (t == 0) P = u0;
    const float mag = (1.0f - alpha) * m0 + alpha * m1;
    s[(long)t * ST_BINS] = f32x2{mag * P[0], mag * P[1]};
    // P <- P * u1 * conj(u0), renormalised
    const f32x2 q = f32x2{u1[0] * u0[0] + u1[1] * u0[1], u1[1] * u0[0] - u1[0] * u0[1]};
    const f32x2 p = f32x2{P[0] * q[0] - P[1] * q[1], P[0] * q[1] + P[1] * q[0]};
    const float pm = st_abs(p);
    P = st_unit(p, pm);
  }
}

// ------------------------------------------------------------------------------------------------------------ istft
__global__ __launch_bounds__(ST_THREADS) void stretch_ifft_kernel(f32x2* S, int F, const double* rates, double rate_lo, int T_max) {
  __shared__ __attribute__((aligned(8))) f32x2 x[ST_N];
  __shared__ __attribute__((aligned(8))) f32x2 tw[ST_N / 2];
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const double rate = rates[b];
  if (!st_rate_ok(rate, rate_lo) || t >= min(st_out_frames(F, rate), T_max)) return;  // uniform over the workgroup
  st_twiddles(tw, tid);
  f32x2* s = S + ((long)b * T_max + t) * ST_BINS;
  for (int k = tid; k < ST_BINS; k += ST_THREADS) {
    f32x2 c = s[k];
    if (k == 0 || k == ST_N / 2) c[1] = 0.f;  // a real signal's DC and Nyquist bins are real: their imaginary parts do not count
    x[st_brev(k)] = c;
    if (k >= 1 && k < ST_N / 2) x[st_brev(ST_N - k)] = f32x2{c[0], -c[1]};  // Hermitian extension
  }
  __syncthreads();
  st_fft<true>(x, tw, tid);
  float* frame = (float*)s;  // 2048 floats inside the 2050 of this frame's spectrum: every load of it is behind the barriers above
  for (int i = tid; i < ST_N; i += ST_THREADS) frame[i] = x[i][0] * (1.0f / ST_N) * st_window(i);
}

__global__ __launch_bounds__(256) void stretch_ola_kernel(const float* frames, int n_in, int F, const double* rates, double rate_lo,
                                                          int T_max, float* out, long ld_out, int n_out_max, int* n_out) {
  const int b = blockIdx.y;
  const int m = blockIdx.x * 256 + threadIdx.x;
  const double rate = rates[b];
  const bool ok = st_rate_ok(rate, rate_lo);
  const int n = ok ? min((int)rint((double)n_in / rate), n_out_max) : -1;  // half-to-even
  if (m == 0) n_out[b] = n;
  if (m >= n) return;
  const int T = min(st_out_frames(F, rate), T_max);
  const float* fr = frames + (long)b * T_max * (2 * ST_BINS);
  const int p = m + ST_N / 2;  // position in the centre-padded signal
  const int t_hi = min(p / ST_H, T - 1), t_lo = max(p / ST_H - (ST_N / ST_H - 1), 0);
  float acc = 0.f, wss = 0.f;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int off = p - t * ST_H;  // in [0, 2048)
    acc += fr[(long)t * (2 * ST_BINS) + off];
    const float w = st_window(off);
    wss = fmaf(w, w, wss);
  }
  out[b * ld_out + m] = wss > FLT_MIN ? acc / wss : acc;
}

// ------------------------------------------------------------------------------------------------------------ entry points
static inline bool st_rate_lo_ok(double rate_lo) { return rate_lo >= 0.5 && rate_lo <= 2.0; }
static inline int64_t st_n_out_max(int64_t n_in, double rate_lo) { return (int64_t)rint((double)n_in / rate_lo); }

extern "C" int64_t wft_time_stretch_workspace_bytes(int B, int64_t n_in, double rate_lo) {
  if (B < 1 || n_in < 1 || n_in > ST_MAX_IN || !st_rate_lo_ok(rate_lo)) return -1;
  const int64_t F = st_frames(n_in), T_max = st_out_frames((int)F, rate_lo);
  return (int64_t)B * (F + T_max) * ST_BINS * (int64_t)sizeof(f32x2);
}

#define ST_CHECK_SHAPE()                                                                                  \
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_in >= 1 && n_in <= ST_MAX_IN, "bad shape (1 <= n_in <= 2^26, B <= 65535)")

extern "C" int wft_stretch_stft_f32(const float* in, int64_t ld_in, int64_t n_in, float* D, int B, void* stream) {
  WFT_CHECK_ARG(in && D, "null pointer");
  ST_CHECK_SHAPE();
  WFT_CHECK_ARG(ld_in >= n_in, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)D % 8 == 0, "in must be 4-byte, D 8-byte aligned");
  const int F = st_frames(n_in);
  hipLaunchKernelGGL(stretch_stft_kernel, dim3(F, B), dim3(ST_THREADS), 0, (hipStream_t)stream, in, (long)ld_in, (int)n_in, (f32x2*)D, F);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_stretch_vocoder_f32(const float* D, int64_t n_in, const double* rates, double rate_lo, float* S, int B, void* stream) {
  WFT_CHECK_ARG(D && rates && S, "null pointer");
  ST_CHECK_SHAPE();
  WFT_CHECK_ARG(st_rate_lo_ok(rate_lo), "rate_lo must lie in [0.5, 2.0]");
  WFT_CHECK_ARG((uintptr_t)D % 8 == 0 && (uintptr_t)S % 8 == 0 && (uintptr_t)rates % 8 == 0, "D, S and rates must be 8-byte aligned");
  const int F = st_frames(n_in), T_max = st_out_frames(F, rate_lo);
  hipLaunchKernelGGL(stretch_vocoder_kernel, dim3((ST_BINS + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, (const f32x2*)D, F, rates,
                     rate_lo, (f32x2*)S, T_max);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_stretch_istft_f32(float* S, int64_t n_in, const double* rates, double rate_lo, float* out, int64_t ld_out,
                                     int32_t* n_out, int B, void* stream) {
  WFT_CHECK_ARG(S && rates && out && n_out, "null pointer");
  ST_CHECK_SHAPE();
  WFT_CHECK_ARG(st_rate_lo_ok(rate_lo), "rate_lo must lie in [0.5, 2.0]");
  WFT_CHECK_ARG(ld_out >= st_n_out_max(n_in, rate_lo), "ld_out smaller than round(n_in / rate_lo)");
  WFT_CHECK_ARG((uintptr_t)S % 8 == 0 && (uintptr_t)rates % 8 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n_out % 4 == 0,
                "S and rates must be 8-byte, out and n_out 4-byte aligned");
  const int F = st_frames(n_in), T_max = st_out_frames(F, rate_lo);
  const int n_max = (int)st_n_out_max(n_in, rate_lo);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(stretch_ifft_kernel, dim3(T_max, B), dim3(ST_THREADS), 0, s, (f32x2*)S, F, rates, rate_lo, T_max);
  hipLaunchKernelGGL(stretch_ola_kernel, dim3((n_max + 255) / 256, B), dim3(256), 0, s, (const float*)S, (int)n_in, F, rates, rate_lo,
                     T_max, out, (long)ld_out, n_max, n_out);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_time_stretch_f32(const float* in, int64_t ld_in, int64_t n_in, const double* rates, double rate_lo, float* out,
                                    int64_t ld_out, int32_t* n_out, void* workspace, int64_t workspace_bytes, int B, void* stream) {
  WFT_CHECK_ARG(in && rates && out && n_out && workspace, "null pointer");
  ST_CHECK_SHAPE();
  WFT_CHECK_ARG(st_rate_lo_ok(rate_lo), "rate_lo must lie in [0.5, 2.0]");
  WFT_CHECK_ARG(ld_in >= n_in, "leading dimension smaller than the row");
  WFT_CHECK_ARG(ld_out >= st_n_out_max(n_in, rate_lo), "ld_out smaller than round(n_in / rate_lo)");
  WFT_CHECK_ARG(workspace_bytes >= wft_time_stretch_workspace_bytes(B, n_in, rate_lo), "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n_out % 4 == 0 && (uintptr_t)rates % 8 == 0 &&
                    (uintptr_t)workspace % 8 == 0,
                "in / out / n_out must be 4-byte, rates / workspace 8-byte aligned");
  float* D = (float*)workspace;
  float* S = D + (int64_t)B * st_frames(n_in) * ST_BINS * 2;
  int rc = wft_stretch_stft_f32(in, ld_in, n_in, D, B, stream);
  if (rc == WFT_OK) rc = wft_stretch_vocoder_f32(D, n_in, rates, rate_lo, S, B, stream);
  if (rc == WFT_OK) rc = wft_stretch_istft_f32(S, n_in, rates, rate_lo, out, ld_out, n_out, B, stream);
  return rc;
}
