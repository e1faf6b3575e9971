// audio.hip — log-mel front end and SpecAugment on the GPU.
//
// logmel: one 256-thread workgroup per (clip, 16 frames): the 2800-sample reflect-padded
// audio span is staged once in LDS, Hann-windowed frames are written to LDS and folded on the DFT's
// symmetry (x[n] +- x[400 - n]: half the multiply-adds), the 400-point DFT is evaluated directly in fp32
// from a 400-entry twiddle table in LDS (exact periodic index k*n mod 400, no trig in the loop), then the [16 x 201] power tile is multiplied by
// the mel filterbank and log10'd.  Algorithmic HBM bytes per clip: 1.92 MB read +
// n_mels*3000*4 B written twice (the clip-max floor needs a second pass).
// specaug: one pass, bilinear time-warp gather + time/frequency/extremes masks.
#include "common.h"

#define NFFT 400
#define HOP 160
#define NBIN 201
#define FPB 16  // frames per block

// One workgroup's 16 frames of one clip `a` of n_samples samples (reflect padding at both ends of THOSE samples).  Frames
// fr < n_store are written (log10, not yet normalised) to orow[mI * ld_row + fr]; frames fr < n_max enter the clip maximum.
// RAGGED (wft_logmel_ragged): also the minimum over the frames fr < n_keep, kept as an order-preserving key of the float's bits.
// wft_logmel is the instantiation with n_store == n_max == n_frames: both entry points run this one body, so equal samples
// give equal bits.
__device__ __forceinline__ unsigned int f32_order_key(float f) {
  const unsigned int u = __builtin_bit_cast(unsigned int, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_order_key(unsigned int k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
template <bool RAGGED>
__device__ __forceinline__ void logmel_block(const float* a, const float* filters, float* orow, long ld_row, unsigned int* clipmax,
                                             unsigned int* clipmin, int n_samples, int n_mels, int n_store, int n_max, int n_keep,
                                             int f0) {
  __shared__ float span[(FPB - 1) * HOP + NFFT];  // 2800
  __shared__ __attribute__((aligned(16))) float frames[FPB][NFFT];  // windowed
  __shared__ __attribute__((aligned(8))) float tw[NFFT][2];         // (cos, sin)(2 pi i / 400)
  __shared__ float power[FPB][NBIN + 3];
  __shared__ float wmax[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < (FPB - 1) * HOP + NFFT; i += 256) {
    int idx = f0 * HOP + i - NFFT / 2;  // position in the un-padded clip
    if (idx < 0) idx = -idx;
    if (idx >= n_samples) idx = 2 * (n_samples - 1) - idx;
    idx = idx < 0 ? 0 : (idx >= n_samples ? n_samples - 1 : idx);
    span[i] = a[idx];
  }
  for (int i = tid; i < NFFT; i += 256) {
    // sincospi keeps the table accurate to 1 ulp: angle = 2*pi*i/400
    float sn, cs;
    sincospif((float)i / 200.0f, &sn, &cs);
    tw[i][0] = cs;
    tw[i][1] = sn;
  }
  __syncthreads();
  for (int i = tid; i < FPB * NFFT; i += 256) {
    const int f = i / NFFT, n = i - f * NFFT;
    const float w = 0.5f - 0.5f * tw[n][0];  // periodic Hann
    frames[f][n] = w * span[f * HOP + n];
  }
  __syncthreads();
  // Fold every windowed frame on the DFT's symmetry (round 5: half the multiply-adds).  cos(2 pi k (400 - n) / 400) =
  // cos(2 pi k n / 400) and sin(...) = -sin(...), so with s[n] = x[n] + x[400 - n], d[n] = x[n] - x[400 - n] (n = 1..199):
  //   Re X[k] = x[0] + (-1)^k x[200] + sum_n s[n] cos(2 pi k n / 400),   Im X[k] = -sum_n d[n] sin(2 pi k n / 400)
  // In place: [f][0] = x[0], [f][1..199] = s, [f][200] = x[200], [f][201..399] = d[1..199] (so that both 4-sample reads of the loop
  // below are 16-byte aligned); two phases around a barrier because d[n] lands in another pair's input.
  {
    constexpr int PAIRS = FPB * 199, PER = (PAIRS + 255) / 256;
    float pa[PER], pb[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * 256;
      if (i < PAIRS) {
        const int f = i / 199, n = 1 + (i - f * 199);
        pa[j] = frames[f][n];
        pb[j] = frames[f][NFFT - n];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = tid + j * 256;
      if (i < PAIRS) {
        const int f = i / 199, n = 1 + (i - f * 199);
        frames[f][n] = pa[j] + pb[j];
        frames[f][200 + n] = pa[j] - pb[j];
      }
    }
    __syncthreads();
  }
  // DFT, register-blocked: thread = one bin k for all FPB frames.  Per 4 samples: 4 twiddle pairs (ds_read_b64) + 2 FPB
  // broadcast float4 frame reads feed 8*FPB FMAs: VALU-bound.  (The sample at offset 200 of the first d read is x[200], multiplied
  // by sin(0) = 0: an exact zero.)
  if (tid < NBIN) {
    const int k = tid;
    float re[FPB], im[FPB];
#pragma unroll
    for (int f = 0; f < FPB; ++f) { re[f] = 0.f; im[f] = 0.f; }
    int idx = 0;
    for (int n = 0; n < 200; n += 4) {
      f32x2 t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        t[j] = *(const f32x2*)tw[idx];
        idx += k;
        idx = idx >= NFFT ? idx - NFFT : idx;
      }
#pragma unroll
      for (int f = 0; f < FPB; ++f) {
        const f32x4 xs = *(const f32x4*)&frames[f][n];
        const f32x4 xd = *(const f32x4*)&frames[f][200 + n];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          re[f] = fmaf(xs[j], t[j][0], re[f]);
          im[f] = fmaf(xd[j], t[j][1], im[f]);
        }
      }
    }
    const float sgn = (k & 1) ? -1.f : 1.f;  // cos(pi k)
#pragma unroll
    for (int f = 0; f < FPB; ++f) {
      re[f] = fmaf(frames[f][200], sgn, re[f]);
      power[f][k] = re[f] * re[f] + im[f] * im[f];
    }
  }
  // The mel filters are triangles: 2-30 non-zero bins out of 201 per filter.  Each filter's non-zero range is found once per
  // workgroup (one thread per filter; skipping exact zeros leaves every sum bit-identical to the dense loop).
  __shared__ short mlo[256], mhi[256];
  if (tid < n_mels && tid < 256) {
    const float* fl = filters + (long)tid * NBIN;
    int lo = NBIN, hi = 0;
    for (int k = 0; k < NBIN; ++k)
      if (fl[k] != 0.f) { lo = lo < k ? lo : k; hi = k + 1; }
    mlo[tid] = (short)(lo < hi ? lo : 0);
    mhi[tid] = (short)hi;
  }
  __syncthreads();
  float lmax = -1.0e30f, lmin = 3.0e38f;
  for (int o = tid; o < n_mels * FPB; o += 256) {
    const int mI = o / FPB, f = o - mI * FPB;
    const float* fl = filters + (long)mI * NBIN;
    float acc = 0.f;
    const int k0 = mI < 256 ? mlo[mI] : 0, k1 = mI < 256 ? mhi[mI] : NBIN;
    for (int k = k0; k < k1; ++k) acc = fmaf(fl[k], power[f][k], acc);
    const float lg = log10f(fmaxf(acc, 1.0e-10f));
    const int fr = f0 + f;
    if (fr < n_store) orow[mI * ld_row + fr] = lg;
    if (fr < n_max) lmax = fmaxf(lmax, lg);
    if (RAGGED && fr < n_keep) lmin = fminf(lmin, lg);
  }
  lmax = wave_max(lmax);
  if ((tid & 63) == 0) wmax[tid >> 6] = lmax;
  __syncthreads();
  if (tid == 0) {
    const float mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    // log10 values are >= -10, so (mx + 20) is a positive float: its bit pattern orders like an int
    atomicMax(clipmax, __builtin_bit_cast(unsigned int, mx + 20.0f));
  }
  if (RAGGED) {
    lmin = -wave_max(-lmin);
    __syncthreads();
    if ((tid & 63) == 0) wmax[tid >> 6] = lmin;
    __syncthreads();
    if (tid == 0) atomicMin(clipmin, f32_order_key(fminf(fminf(wmax[0], wmax[1]), fminf(wmax[2], wmax[3]))));
  }
}

__global__ __launch_bounds__(256) void logmel_kernel(const float* audio, const float* filters, float* out,
                                                      unsigned int* clipmax, int n_samples, int n_mels, int n_frames) {
  const int b = blockIdx.y;
  logmel_block<false>(audio + (long)b * n_samples, filters, out + (long)b * n_mels * n_frames, n_frames, clipmax + b, nullptr,
                      n_samples, n_mels, n_frames, n_frames, 0, blockIdx.x * FPB);
}

__global__ __launch_bounds__(256) void logmel_norm_kernel(float* out, const unsigned int* clipmax, long per_clip, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / per_clip);
    const float mx = __builtin_bit_cast(float, clipmax[b]) - 20.0f;
    const float v = fmaxf(out[i], mx - 8.0f);
    out[i] = (v + 4.0f) / 4.0f;
  }
}

extern "C" int wft_logmel(const float* audio, const float* filters, float* out, float* clipmax, int B, int n_samples,
                          int n_mels, int n_frames, void* stream) {
  WFT_CHECK_ARG(audio && filters && out && clipmax, "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_mels >= 1 && n_frames >= 1 && n_samples == n_frames * HOP, "n_samples must be 160*n_frames");
  WFT_CHECK_ARG(n_samples > NFFT, "clip too short");
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(clipmax, 0, B * sizeof(float), s);
  dim3 grid((n_frames + FPB - 1) / FPB, B);
  hipLaunchKernelGGL(logmel_kernel, grid, dim3(256), 0, s, audio, filters, out, (unsigned int*)clipmax, n_samples, n_mels,
                     n_frames);
  const long per_clip = (long)n_mels * n_frames, total = per_clip * B;
  hipLaunchKernelGGL(logmel_norm_kernel, dim3(ew_grid(total)), dim3(256), 0, s, out, (const unsigned int*)clipmax, per_clip,
                     total);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// --------------------------------------------------------------------------------- ragged log-mel
// Row b has n_samples[b] samples (clamped to [0, max_samples]) and frames_b = n_samples[b] / 160 frames; kept = min(keep_frames[b],
// frames_b, T_out) columns hold its normalised log-mel, the columns behind them the minimum of the kept ones (of none kept: 0).
// stats u32 [2 B]: {clip maximum over ALL frames_b frames as wft_logmel keeps it, order key of the minimum over the kept frames}.
__device__ __forceinline__ void ragged_row(const int* n_samples, const int* keep_frames, int b, int max_samples, int T_out, int& ns,
                                           int& frames, int& kept) {
  ns = min(max(n_samples[b], 0), max_samples);
  frames = ns / HOP;
  kept = min(min(max(keep_frames[b], 0), frames), T_out);
}
__global__ __launch_bounds__(256) void logmel_ragged_kernel(const float* audio, long ld_audio, const int* n_samples, const int* keep_frames,
                                                             const float* filters, float* out, unsigned int* stats, int max_samples,
                                                             int n_mels, int T_out) {
  const int b = blockIdx.y, f0 = blockIdx.x * FPB;
  int ns, frames, kept;
  ragged_row(n_samples, keep_frames, b, max_samples, T_out, ns, frames, kept);
  if (f0 >= frames) return;  // uniform over the workgroup, in front of every barrier
  logmel_block<true>(audio + b * ld_audio, filters, out + (long)b * n_mels * T_out, T_out, stats + 2 * b, stats + 2 * b + 1, ns, n_mels,
                     min(frames, T_out), frames, kept, f0);
}
__global__ __launch_bounds__(256) void logmel_ragged_norm_kernel(float* out, const unsigned int* stats, const int* n_samples,
                                                                  const int* keep_frames, int max_samples, int T_out, long per_clip,
                                                                  long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / per_clip);
    const int t = (int)((i - b * per_clip) % T_out);
    int ns, frames, kept;
    ragged_row(n_samples, keep_frames, b, max_samples, T_out, ns, frames, kept);
    if (kept == 0) { out[i] = 0.f; continue; }
    const float mx = __builtin_bit_cast(float, stats[2 * b]) - 20.0f;
    const float v = fmaxf(t < kept ? out[i] : f32_from_order_key(stats[2 * b + 1]), mx - 8.0f);
    out[i] = (v + 4.0f) / 4.0f;
  }
}

extern "C" int wft_logmel_ragged(const float* audio, int64_t ld_audio, const int32_t* n_samples, const int32_t* keep_frames,
                                 const float* filters, float* out, float* stats, int B, int max_samples, int n_mels, int T_out,
                                 void* stream) {
  WFT_CHECK_ARG(audio && n_samples && keep_frames && filters && out && stats, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_mels >= 1 && T_out >= 1, "bad shape");
  WFT_CHECK_ARG(max_samples > NFFT && ld_audio >= max_samples, "max_samples must exceed 400 and fit the row");
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(stats, 0, 2 * B * sizeof(float), s);
  (void)hipMemset2DAsync(stats + 1, 2 * sizeof(float), 0xff, sizeof(float), B, s);  // the minimum's key starts at the largest
  dim3 grid((max_samples / HOP + FPB - 1) / FPB, B);
  hipLaunchKernelGGL(logmel_ragged_kernel, grid, dim3(256), 0, s, audio, (long)ld_audio, n_samples, keep_frames, filters, out,
                     (unsigned int*)stats, max_samples, n_mels, T_out);
  const long per_clip = (long)n_mels * T_out, total = per_clip * B;
  hipLaunchKernelGGL(logmel_ragged_norm_kernel, dim3(ew_grid(total)), dim3(256), 0, s, out, (const unsigned int*)stats, n_samples,
                     keep_frames, max_samples, T_out, per_clip, total);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// --------------------------------------------------------------------------------- SpecAugment
// params per clip: {apply_warp, warp_p, warp_d, t0, t1, f0, f1, unused}; extremes: {low_len, high_len}
__global__ __launch_bounds__(256) void specaug_kernel(const float* in, float* out, const int* params, const int* extremes,
                                                       int n_mels, int T) {
  const int b = blockIdx.z, mI = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int* pr = params + b * 8;
  const int apply_warp = pr[0], wp = pr[1], wd = pr[2], t0 = pr[3], t1 = pr[4], f0 = pr[5], f1 = pr[6];
  const int lo = extremes ? extremes[b * 2] : 0, hi = extremes ? extremes[b * 2 + 1] : 0;
  const float* row = in + ((long)b * n_mels + mI) * T;
  float v;
  if (apply_warp) {
    // cubic Hermite spline through (0,-1), (wp, y1), (T-1, 1)  (data/utils.py:66-85,110-136)
    const float L1 = (float)(T - 1);
    const float y1 = (float)(wp - wd) * 2.0f / L1 - 1.0f;
    const float sa = (y1 + 1.0f) / (float)wp;           // secant of segment 0
    const float sb = (1.0f - y1) / (float)(T - 1 - wp);  // secant of segment 1
    const float mmid = (sa + sb) * 0.5f;
    const float xs = (float)t;
    float xl, dx, yl, yr, ml, mr;
    if (t <= wp) { xl = 0.f; dx = (float)wp; yl = -1.0f; yr = y1; ml = sa; mr = mmid; }
    else { xl = (float)wp; dx = (float)(T - 1 - wp); yl = y1; yr = 1.0f; ml = mmid; mr = sb; }
    const float u = (xs - xl) / dx;
    const float u2 = u * u, u3 = u2 * u;
    const float h0 = 1.0f - 3.0f * u2 + 2.0f * u3;
    const float h1 = u - 2.0f * u2 + u3;
    const float h2 = 3.0f * u2 - 2.0f * u3;
    const float h3 = -u2 + u3;
    const float ys = h0 * yl + h1 * ml * dx + h2 * yr + h3 * mr * dx;
    // grid_sample, bilinear, align_corners=True, zero padding; the row coordinate is exact
    const float ix = (ys + 1.0f) * 0.5f * L1;
    const float fx = floorf(ix);
    const int x0 = (int)fx, x1 = x0 + 1;
    const float w1 = ix - fx, w0 = 1.0f - w1;
    const float a0 = (x0 >= 0 && x0 < T) ? row[x0] : 0.f;
    const float a1 = (x1 >= 0 && x1 < T) ? row[x1] : 0.f;
    v = a0 * w0 + a1 * w1;
  } else {
    v = row[t];
  }
  if (t >= t0 && t < t1) v = 0.f;
  if (mI >= f0 && mI < f1) v = 0.f;
  if (mI < lo || mI >= n_mels - hi) v = 0.f;
  out[((long)b * n_mels + mI) * T + t] = v;
}
extern "C" int wft_specaug(const float* in, float* out, const int32_t* params, const int32_t* extremes, int B, int n_mels,
                           int T, void* stream) {
  WFT_CHECK_ARG(in && out && params && in != out, "bad pointers (in and out must differ)");
  WFT_CHECK_ARG(B >= 1 && n_mels >= 1 && T >= 2, "bad shape");
  dim3 grid((T + 255) / 256, n_mels, B);
  hipLaunchKernelGGL(specaug_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, params, extremes, n_mels, T);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// --------------------------------------------------------------------------------- layout for the conv stem
// mel f32 [B, n_mels, T] -> bf16 [B, T+2, c_pad], rows 0 and T+1 zero, channels >= n_mels zero
__global__ __launch_bounds__(256) void mel_tmajor_kernel(const float* mel, unsigned short* out, int n_mels, int T, int c_pad) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z;
  const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int cc = ty; cc < 64; cc += 4) {
    const int c = c0 + cc, t = t0 + tx;
    tile[cc][tx] = (c < n_mels && t < T) ? mel[((long)b * n_mels + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int tt = ty; tt < 64; tt += 4) {
    const int t = t0 + tt, c = c0 + tx;
    if (t < T && c < c_pad) out[((long)b * (T + 2) + t + 1) * c_pad + c] = f2bf(tile[tx][tt]);
  }
  // halo rows
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < 64; c += 256) {
      const int cg = c0 + c;
      if (cg < c_pad) {
        out[((long)b * (T + 2)) * c_pad + cg] = 0;
        out[((long)b * (T + 2) + T + 1) * c_pad + cg] = 0;
      }
    }
  }
}
extern "C" int wft_mel_to_tmajor_bf16(const float* mel, wft_bf16* out, int B, int n_mels, int T, int c_pad, void* stream) {
  WFT_CHECK_ARG(mel && out, "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_mels >= 1 && T >= 1 && c_pad >= n_mels, "bad shape");
  dim3 grid((T + 63) / 64, (c_pad + 63) / 64, B);
  hipLaunchKernelGGL(mel_tmajor_kernel, grid, dim3(256), 0, (hipStream_t)stream, mel, out, n_mels, T, c_pad);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// --------------------------------------------------------------------------------- resampling
// Polyphase windowed-sinc FIR (include/wft.h "wft_resample_f32"): out[m] = sum_k taps[r][k + width - 1] * x[j0 + k] over
// k = -width + 1 .. width, with m * orig = j0 * new_rate + r.  One workgroup per (tile of outputs, row): the tile's input span
// [j0(first) - width + 1, j0(last) + width] is staged once in LDS with 16-byte loads (the span start is moved back to the row's
// 16-byte grid; a chunk that crosses 0 or n_in is read element by element, zero outside), then a thread computes up to four outputs
// of one phase r — each one f32 fma chain in ascending k, so its bits do not depend on the tiling.  The table goes through the
// cache: 8 bytes (two taps) per load, one row per thread, shared by its outputs; neighbouring lanes hold neighbouring outputs.
// m * orig is formed in 64 bits once per workgroup (the tile's first output); inside a tile the phase advances in 32 bits,
// r0 + i * orig < new_rate + tile * orig < 2^31 (checked by the entry point).
#define RS_THREADS 256
#define RS_PER 4                          // outputs per thread (of one phase)
#define RS_TILE_MAX (RS_THREADS * RS_PER)  // outputs per workgroup
#define RS_SPAN 8192                      // floats of LDS for the input span (32 KiB)

// outputs per workgroup for a rate pair: the largest multiple of 4, at most RS_TILE_MAX, whose input span fits RS_SPAN floats
//   span <= floor((new_rate - 1 + (tile - 1) * orig) / new_rate) + 2 * width   (first to last tap)
//           + 3 (alignment in front) + 3 (the last chunk rounded up);  0: not even four outputs fit.
extern "C" int wft_resample_tile(int orig, int new_rate, int width) {
  if (orig < 1 || new_rate < 1 || width < 1) return 0;
  const int64_t room = (int64_t)RS_SPAN - 2 * (int64_t)width - 6;
  if (room < 0) return 0;
  int64_t t = room * new_rate / orig + 1;  // (tile - 1) * orig <= room * new_rate
  if (t > RS_TILE_MAX) t = RS_TILE_MAX;
  t &= ~(int64_t)3;
  if (t * orig + new_rate >= ((int64_t)1 << 31)) return 0;
  return (int)t;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* in, long ld_in, long n_in, const float* taps, int o, int n,
                                                              int width, float* out, long ld_out, long n_out, int tile) {
  __shared__ __attribute__((aligned(16))) float xs[RS_SPAN];
  const int tid = threadIdx.x;
  const long m0 = (long)blockIdx.x * tile;
  const int cnt = (int)min((long)tile, n_out - m0);  // outputs of this tile, >= 1
  const unsigned long p0 = (unsigned long)m0 * (unsigned long)o;
  const long j0t = (long)(p0 / (unsigned long)n);
  const unsigned r0 = (unsigned)(p0 % (unsigned long)n);
  const float* x = in + blockIdx.y * ld_in;
  const long js = j0t - width + 1;                                   // first input element any output of the tile reads
  const int mis = (int)(((long)((uintptr_t)x >> 2) + js) & 3);       // its distance behind the row's 16-byte grid
  const long ja = js - mis;                                          // xs[i] = x[ja + i]
  const long je = j0t + (r0 + (unsigned)(cnt - 1) * (unsigned)o) / (unsigned)n + width;  // last one (inclusive)
  const int n_chunk = (int)((je - ja) / 4) + 1;                      // 4 * n_chunk <= RS_SPAN by the choice of `tile`
  for (int c = tid; c < n_chunk; c += RS_THREADS) {
    const long j = ja + 4 * c;
    f32x4 v;
    if (j >= 0 && j + 3 < n_in) {
      v = *(const f32x4*)(x + j);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (j + e >= 0 && j + e < n_in) ? x[j + e] : 0.f;
    }
    *(f32x4*)&xs[4 * c] = v;
  }
  __syncthreads();
  // Outputs of one phase share a table row: a thread takes up to four outputs i = c + n * q of phase c (q = qb, qb + QB, qb + 2 QB,
  // qb + 3 QB), loads each pair of taps once for all of them, and neighbouring lanes hold neighbouring phases c, so their LDS windows
  // start o / n floats apart and their stores are neighbours.  For n = 1 that is outputs tid, tid + 256, ... with a wave-uniform row.
  const int nt = 2 * width;
  const int C = min(n, tile);                  // phases that occur in a tile
  const int Q = (tile + n - 1) / n;            // outputs per phase, at most
  const int QB = (Q + RS_PER - 1) / RS_PER;    // groups per phase
  float* orow = out + blockIdx.y * ld_out + m0;
  for (int g = tid; g < C * QB; g += RS_THREADS) {
    const int qb = g / C, c = g - qb * C;
    const int i0 = c + n * qb;                 // the group's first output; >= cnt: the whole group lies behind the tile's end
    if (i0 >= cnt) continue;
    const unsigned t = r0 + (unsigned)i0 * (unsigned)o;
    const int dj = (int)(t / (unsigned)n);     // j0 of output m0 + i0, relative to the tile's
    const int r = (int)(t - (unsigned)dj * (unsigned)n);
    const float* tp = taps + (long)r * nt;     // the phase's table row
    const int step = QB * o;                   // i grows by n * QB from one output of the group to the next: j0 by QB * o, r stays
    const float* xp[RS_PER];                   // &x[j0 - width + 1] in LDS
    bool live[RS_PER];
#pragma unroll
    for (int e = 0; e < RS_PER; ++e) {
      live[e] = (long)i0 + (long)e * n * QB < cnt;         // an output behind the tile's end repeats the group's first one and is not stored
      xp[e] = xs + mis + dj + (live[e] ? e * step : 0);
    }
    // four independent fma chains, each in ascending k from 0.0f; two taps (8 bytes) per table load
    float acc[RS_PER] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k = 0; k < nt; k += 2) {
      const f32x2 w = *(const f32x2*)(tp + k);
#pragma unroll
      for (int e = 0; e < RS_PER; ++e) {
        acc[e] = fmaf(w[0], xp[e][k], acc[e]);
        acc[e] = fmaf(w[1], xp[e][k + 1], acc[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < RS_PER; ++e)
      if (live[e]) orow[i0 + e * n * QB] = acc[e];
  }
}

extern "C" int wft_resample_f32(const float* in, int64_t ld_in, int64_t n_in, const float* taps, int orig, int new_rate, int width,
                                float* out, int64_t ld_out, int64_t n_out, int B, void* stream) {
  WFT_CHECK_ARG(in && taps && out, "null pointer");
  WFT_CHECK_ARG(orig >= 1 && new_rate >= 1 && width >= 1 && B >= 1 && B <= 65535 && n_in >= 1, "bad shape");
  int a = orig, b = new_rate;
  while (b) { const int t = a % b; a = b; b = t; }
  WFT_CHECK_ARG(a == 1, "orig and new_rate must be reduced (coprime)");
  WFT_CHECK_ARG(n_in <= (INT64_MAX - orig) / new_rate, "n_in * new_rate overflows");
  WFT_CHECK_ARG(n_out == (n_in * new_rate + orig - 1) / orig, "n_out must be ceil(n_in * new_rate / orig)");
  WFT_CHECK_ARG(ld_in >= n_in && ld_out >= n_out, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)taps % 8 == 0, "in / out must be 4-byte, taps 8-byte aligned");
  const int tile = wft_resample_tile(orig, new_rate, width);
  WFT_CHECK_ARG(tile >= 4, "rate pair not supported: the input span of four outputs does not fit the staging buffer");
  const int64_t n_tiles = cdiv64(n_out, tile);
  WFT_CHECK_ARG(n_tiles <= 0x7fffffff, "too many output tiles");
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)n_tiles, B), dim3(RS_THREADS), 0, (hipStream_t)stream, in, (long)ld_in, (long)n_in,
                     taps, orig, new_rate, width, out, (long)ld_out, (long)n_out, tile);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
