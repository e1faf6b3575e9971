// loss.hip — the loss head over the bf16 logits [rows, V]: label-smoothed cross entropy forward (per-row loss, log-sum-exp and
// the teacher-forced argmax), its fixed-order reduction to {loss sum, valid rows}, the backward that writes dlogits, and the
// one-pass evaluation statistics per token (token_stats).
//
// HBM-bound: the forward reads rows·V·2 B once, the backward reads and writes them once.  One 256-thread workgroup per row,
// 16-byte loads, an online (max, sum-exp) pair per thread merged over the wave and then over the four waves in a fixed order.
#include "common.h"

// ----------------------------------------------------------------------------- cross entropy
// one 256-thread block per row; online (max, sum-exp), sum of logits, target logit, argmax.
__global__ __launch_bounds__(256) void ce_fwd_kernel(const unsigned short* logits, long ld, const long* targets, long V,
                                                      float eps, float* row_loss, float* row_lse, long* argmax) {
  __shared__ float sm[4], ss[4], sx[4], sbv[4];
  __shared__ int sbi[4];
  const long row = blockIdx.x;
  const unsigned short* x = logits + row * ld;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float m = -3.0e38f, s = 0.f, sumx = 0.f, bv = -3.0e38f;
  int bi = 0x7fffffff;
  const long nv = V >> 3;
  for (long i = tid; i < nv; i += 256) {
    const u32x4 r = *(const u32x4*)(x + i * 8);
    float v[8];
    bf8_unpack(r, v);
    float cm = v[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) cm = fmaxf(cm, v[e]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (v[e] > bv) { bv = v[e]; bi = (int)(i * 8 + e); }
      sumx += v[e];
    }
    if (cm > m) { s *= __expf(m - cm); m = cm; }
#pragma unroll
    for (int e = 0; e < 8; ++e) s += __expf(v[e] - m);
  }
  for (long c = (nv << 3) + tid; c < V; c += 256) {
    const float v = bf2f(x[c]);
    if (v > bv) { bv = v; bi = (int)c; }
    sumx += v;
    if (v > m) { s *= __expf(m - v); m = v; }
    s += __expf(v - m);
  }
  // wave reduce
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float nm = fmaxf(m, om);
    s = s * __expf(m - nm) + os * __expf(om - nm);
    m = nm;
    sumx += __shfl_xor(sumx, o, 64);
    const float obv = __shfl_xor(bv, o, 64);
    const int obi = __shfl_xor(bi, o, 64);
    if (obv > bv || (obv == bv && obi < bi)) { bv = obv; bi = obi; }
  }
  if (lane == 0) { sm[wv] = m; ss[wv] = s; sx[wv] = sumx; sbv[wv] = bv; sbi[wv] = bi; }
  __syncthreads();
  if (tid == 0) {
    float M = sm[0], S = ss[0], X = sx[0], BV = sbv[0];
    int BI = sbi[0];
    for (int w = 1; w < 4; ++w) {
      const float nm = fmaxf(M, sm[w]);
      S = S * __expf(M - nm) + ss[w] * __expf(sm[w] - nm);
      M = nm;
      X += sx[w];
      if (sbv[w] > BV || (sbv[w] == BV && sbi[w] < BI)) { BV = sbv[w]; BI = sbi[w]; }
    }
    const float lse = M + __logf(S);
    const long t = targets[row];
    float loss = 0.f;
    if (t >= 0 && t < V) {
      const float xt = bf2f(x[t]);
      loss = (1.f - eps) * (lse - xt) + eps * (lse - X / (float)V);
    }
    row_loss[row] = loss;
    row_lse[row] = lse;
    if (argmax) argmax[row] = BI;
  }
}
// deterministic reduction of the row losses (single block)
__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* row_loss, const long* targets, long rows, long V,
                                                         float* stats) {
  __shared__ float sl[256], sc[256];
  float l = 0.f, c = 0.f;
  for (long r = threadIdx.x; r < rows; r += 256) {
    const long t = targets[r];
    if (t >= 0 && t < V) { l += row_loss[r]; c += 1.f; }
  }
  sl[threadIdx.x] = l;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { stats[0] = sl[0]; stats[1] = sc[0]; }
}
extern "C" int wft_ce_fwd(const wft_bf16* logits, int64_t ld, const int64_t* targets, int64_t rows, int64_t V,
                          float label_smoothing, float* row_loss, float* row_lse, float* stats, int64_t* argmax,
                          void* stream) {
  WFT_CHECK_ARG(logits && targets && row_loss && row_lse && stats, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && V >= 1 && ld >= V && ld % 8 == 0, "bad shape (ld must be a multiple of 8, >= V)");
  WFT_CHECK_ARG((((uintptr_t)logits) & 15) == 0, "16-byte alignment");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, (long)ld, (const long*)targets, (long)V,
                     label_smoothing, row_loss, row_lse, (long*)argmax);
  hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss, (const long*)targets, (long)rows, (long)V, stats);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const unsigned short* logits, long ld, const long* targets, long V,
                                                      float eps, const float* row_lse, const float* stats,
                                                      const float* gscale, unsigned short* dlogits) {
  const long row = blockIdx.x;
  const unsigned short* x = logits + row * ld;
  unsigned short* dx = dlogits + row * ld;
  const long t = targets[row];
  const bool valid = t >= 0 && t < V;
  const float coef = valid ? gscale[0] / fmaxf(stats[1], 1.f) : 0.f;
  const float lse = row_lse[row];
  const float sm = eps / (float)V;
  const long nv = ld >> 3;
  for (long i = threadIdx.x; i < nv; i += 256) {
    const u32x4 r = *(const u32x4*)(x + i * 8);
    float v[8];
    bf8_unpack(r, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long c = i * 8 + e;
      float g = 0.f;
      if (c < V) {
        g = __expf(v[e] - lse) - sm;
        if (c == t) g -= (1.f - eps);
        g *= coef;
      }
      v[e] = g;
    }
    *(u32x4*)(dx + i * 8) = bf8_pack(v);
  }
}
extern "C" int wft_ce_bwd(const wft_bf16* logits, int64_t ld, const int64_t* targets, int64_t rows, int64_t V,
                          float label_smoothing, const float* row_lse, const float* stats, const float* gscale,
                          wft_bf16* dlogits, void* stream) {
  WFT_CHECK_ARG(logits && targets && row_lse && stats && gscale && dlogits, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && V >= 1 && ld >= V && ld % 8 == 0, "bad shape (ld must be a multiple of 8, >= V)");
  WFT_CHECK_ARG((((uintptr_t)logits) & 15) == 0 && (((uintptr_t)dlogits) & 15) == 0, "16-byte alignment");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                     (const long*)targets, (long)V, label_smoothing, row_lse, stats, gscale, dlogits);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- eval token statistics
// One pass over the V logits of every token (eval/metrics.py:106-137 computes log_softmax, softmax, CE,
// entropy and max-prob as five separate [S, V] passes): per row
//   out[row] = { lse, max logit, sum_c p_c * x_c, x_target (0 if ignored) },  argmax[row] (lowest index on ties)
// from which nll = lse - x_t, log p(pred) = max - lse, confidence = exp(max - lse), entropy = lse - E_p[x].
__global__ __launch_bounds__(256) void token_stats_kernel(const unsigned short* logits, long ld, const long* targets, long V,
                                                           float* out4, long* argmax) {
  __shared__ float sm[4], ss[4], sw[4], sbv[4];
  __shared__ int sbi[4];
  const long row = blockIdx.x;
  const unsigned short* x = logits + row * ld;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float m = -3.0e38f, s = 0.f, w = 0.f, bv = -3.0e38f;  // w = sum exp(x - m) * x
  int bi = 0x7fffffff;
  auto push = [&](float v, int idx) {
    if (v > bv) { bv = v; bi = idx; }
    if (v > m) { const float f = __expf(m - v); s *= f; w *= f; m = v; }
    const float e = __expf(v - m);
    s += e;
    w += e * v;
  };
  const long nv = V >> 3;
  for (long i = tid; i < nv; i += 256) {
    float v[8];
    bf8_unpack(*(const u32x4*)(x + i * 8), v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      push(v[2 * e], (int)(i * 8 + 2 * e));
      push(v[2 * e + 1], (int)(i * 8 + 2 * e + 1));
    }
  }
  for (long c = (nv << 3) + tid; c < V; c += 256) push(bf2f(x[c]), (int)c);
  auto merge = [&](float om, float os, float ow, float obv, int obi) {
    const float nm = fmaxf(m, om);
    const float f0 = __expf(m - nm), f1 = __expf(om - nm);
    s = s * f0 + os * f1;
    w = w * f0 + ow * f1;
    m = nm;
    if (obv > bv || (obv == bv && obi < bi)) { bv = obv; bi = obi; }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    merge(__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(w, o, 64), __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) { sm[wv] = m; ss[wv] = s; sw[wv] = w; sbv[wv] = bv; sbi[wv] = bi; }
  __syncthreads();
  if (tid == 0) {
    m = sm[0]; s = ss[0]; w = sw[0]; bv = sbv[0]; bi = sbi[0];
    for (int k = 1; k < 4; ++k) merge(sm[k], ss[k], sw[k], sbv[k], sbi[k]);
    const long t = targets ? targets[row] : -100;
    out4[row * 4 + 0] = m + __logf(s);
    out4[row * 4 + 1] = bv;
    out4[row * 4 + 2] = w / s;
    out4[row * 4 + 3] = (t >= 0 && t < V) ? bf2f(x[t]) : 0.f;
    argmax[row] = bi;
  }
}
extern "C" int wft_token_stats(const wft_bf16* logits, int64_t ld, const int64_t* targets, int64_t rows, int64_t V,
                               float* out4, int64_t* argmax, void* stream) {
  WFT_CHECK_ARG(logits && out4 && argmax, "null pointer");
  WFT_CHECK_ARG(rows >= 1 && V >= 1 && ld >= V && ld % 8 == 0, "bad shape (ld must be a multiple of 8, >= V)");
  WFT_CHECK_ARG((((uintptr_t)logits) & 15) == 0, "16-byte alignment");
  hipLaunchKernelGGL(token_stats_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ld,
                     (const long*)targets, (long)V, out4, (long*)argmax);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
