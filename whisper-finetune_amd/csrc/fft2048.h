// fft2048.h — the 2048-point radix-2 FFT in LDS that the time stretch (stretch.hip) and the FIR convolution (office.hip) share.
//
// A plain in-place decimation-in-time radix-2 over a bit-reversed load, 11 stages of 1024 butterflies on 256 threads with a barrier
// between them; twiddles exp(-2 pi i m / 2048), m < 1024, from a sincospif table built once per workgroup.
#pragma once
#include "common.h"

#define ST_N 2048
#define ST_BINS 1025   // one-sided
#define ST_LOGN 11
#define ST_THREADS 256

__device__ __forceinline__ void st_twiddles(f32x2* tw, int tid) {
  for (int i = tid; i < ST_N / 2; i += ST_THREADS) {
    float sn, cs;
    sincospif((float)i / (float)(ST_N / 2), &sn, &cs);  // angle = 2 pi i / 2048
    tw[i] = f32x2{cs, -sn};
  }
}
__device__ __forceinline__ int st_brev(int i) { return (int)(__brev((unsigned)i) >> (32 - ST_LOGN)); }

// x holds the input in bit-reversed order; on return x[k] is the DFT (inverse: the unscaled inverse DFT) in natural order.
template <bool INVERSE>
__device__ __forceinline__ void st_fft(f32x2* x, const f32x2* tw, int tid) {
#pragma unroll 1
  for (int s = 0; s < ST_LOGN; ++s) {
    const int half = 1 << s;
#pragma unroll
    for (int r = 0; r < ST_N / 2 / ST_THREADS; ++r) {
      const int j = tid + r * ST_THREADS;
      const int pos = j & (half - 1);
      const int i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
      f32x2 w = tw[pos << (ST_LOGN - 1 - s)];
      if (INVERSE) w[1] = -w[1];
      const f32x2 a = x[i0], b = x[i1];
      const float tr = w[0] * b[0] - w[1] * b[1];
      const float ti = w[0] * b[1] + w[1] * b[0];
      x[i0] = f32x2{a[0] + tr, a[1] + ti};
      x[i1] = f32x2{a[0] - tr, a[1] - ti};
    }
    __syncthreads();
  }
}
