// wavefx.hip — noise, clipping and level augmentation over a ragged batch (include/wft.h "Wave effects" is the contract).
//
// One entry point, one stage per call.  Every stage ends in an APPLY pass: a grid of (spans, B) workgroups, 256 threads, a thread
// owning 4 consecutive samples per trip (one 16-byte access when the row is 16-byte aligned, scalar accesses otherwise), WF_TRIPS
// trips per workgroup.  Two stages need a per-row statistic first:
//   NOISE / gaussian_snr   the row's sum of squares: fp64, per chunk of WF_CHUNK samples in a fixed tree, the chunks added in order
//   CLIP                   four order statistics of the row, EXACT: a radix select over the order-preserving u32 keys in three
//                          passes (11, 11, 10 bits).  A pass histograms the keys that match each rank's prefix so far (LDS integer
//                          atomics per chunk, flushed with global integer atomics: order-independent), then one workgroup per row
//                          walks the histogram to the bin that holds each rank.  The four ranks (j and j + 1 of both percentiles)
//                          ride side by side: ranks with the same prefix share one histogram slot.
// The records live in device memory, so which rows need a statistic is found on the device: a one-workgroup PLAN launch writes the
// list of those rows, and the statistic launches are a FIXED grid of WF_GRID workgroups looping over (listed row, chunk) items, so
// their cost follows the listed rows (about 5 % of a batch clip at the default rates), not B.  An empty list costs idle launches.
// Bits never depend on the order of the list or on the grid: sums are stored per (row, chunk), counts are integers.
// Side kernels of the loader: plain C++, nothing hand-scheduled.  The fp64 arithmetic is the contract, so contraction is off.
#include "common.h"

#pragma clang fp contract(off)

#define WF_T 256                      // threads per workgroup
#define WF_TILE (4 * WF_T)            // samples per workgroup trip of the apply pass
#define WF_TRIPS 4
#define WF_SPAN (WF_TILE * WF_TRIPS)  // samples per workgroup of the apply pass
#define WF_CHUNK 4096                 // samples per item of the statistic passes
#define WF_GRID 1024                  // workgroups of a statistic launch
#define WF_BINS 2048
#define WF_SLOTS 4
#define WF_SEL 16                     // u32 per row: prefix[4], rank[4], slot[4], pad
#define WF_MAX_N (1 << 30)

__device__ __forceinline__ int wf_row_len(const int* n, int b, int n_max) { return n ? min(max(n[b], 0), n_max) : n_max; }

// ------------------------------------------------------------------------------------------------------------ 4-sample access
__device__ __forceinline__ void wf_load4(const float* row, bool vec, int i, int n_b, float (&v)[4]) {
  if (vec && i + 4 <= n_b) {
    const float4 q = *reinterpret_cast<const float4*>(row + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n_b ? row[i + k] : 0.f;
  }
}
__device__ __forceinline__ void wf_store4(float* row, bool vec, int i, int hi, const float (&v)[4]) {
  if (vec && i + 4 <= hi) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < hi) row[i + k] = v[k];
  }
}
__device__ __forceinline__ bool wf_vec_ok(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------ plan
// list of the rows that need the stage's statistic: gaussian_snr rows (NOISE), clipping rows with n[b] >= 1 (CLIP)
__global__ __launch_bounds__(WF_T) void wf_plan_kernel(const wft_wave_fx* fx, const int* n, int n_max, int B, int stage, int* count,
                                                       int* list) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += WF_T) {
    const bool want = stage == WFT_FX_NOISE ? fx[b].noise_kind == WFT_FX_GAUSSIAN_SNR
                                            : (fx[b].clip_kind == WFT_FX_CLIPPING && wf_row_len(n, b, n_max) >= 1);
    if (want) list[atomicAdd(&cnt, 1)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) *count = cnt;
}

// ------------------------------------------------------------------------------------------------------------ NOISE
__global__ __launch_bounds__(WF_T) void wf_sumsq_kernel(const float* in, long ld_in, const int* n, int n_max, const int* count,
                                                        const int* list, double* partial, int C) {
  __shared__ double s[WF_T];
  const int tid = threadIdx.x;
  const long items = (long)*count * C;
  for (long w = blockIdx.x; w < items; w += gridDim.x) {
    const int b = list[w / C], c = (int)(w % C);
    const int n_b = wf_row_len(n, b, n_max), base = c * WF_CHUNK;
    if (base >= n_b) continue;  // uniform
    const float* row = in + b * ld_in;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < WF_CHUNK / WF_T; ++k) {
      const int i = base + k * WF_T + tid;
      if (i < n_b) {
        const double v = (double)row[i];
        acc += v * v;
      }
    }
    s[tid] = acc;
    __syncthreads();
    for (int h = WF_T / 2; h >= 1; h >>= 1) {
      if (tid < h) s[tid] += s[tid + h];
      __syncthreads();
    }
    if (tid == 0) partial[(long)b * C + c] = s[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(WF_T) void wf_sigma_kernel(const wft_wave_fx* fx, const int* n, int n_max, const int* count, const int* list,
                                                        const double* partial, int C, double* sigma) {
  const int cnt = *count;
  for (int k = blockIdx.x * WF_T + threadIdx.x; k < cnt; k += gridDim.x * WF_T) {
    const int b = list[k];
    const int n_b = wf_row_len(n, b, n_max);
    const int nc = (n_b + WF_CHUNK - 1) / WF_CHUNK;
    double sum = 0.0;
    for (int c = 0; c < nc; ++c) sum += partial[(long)b * C + c];
    double sg = 0.0;
    if (n_b > 0 && sum > 0.0) sg = sqrt(sum / (double)n_b) / exp10(fx[b].noise_value / 20.0);
    sigma[b] = sg;
  }
}

__device__ __forceinline__ unsigned wf_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

// Philox4x32-10 (Salmon et al. 2011), the generator of wft_decode_sample
__device__ __forceinline__ void wf_philox(unsigned c0, unsigned k0, unsigned k1, unsigned (&w)[4]) {
  unsigned c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = wf_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = wf_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the Box-Muller pair of words (wa, wb): z for the even and for the odd sample
__device__ __forceinline__ void wf_normal_pair(unsigned wa, unsigned wb, double& ze, double& zo) {
  const double u1 = (double)(2u * (wa >> 9) + 1u) * 5.9604644775390625e-08;
  const double u2 = (double)(2u * (wb >> 9) + 1u) * 5.9604644775390625e-08;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  ze = r * cs;
  zo = r * sn;
}

__global__ __launch_bounds__(WF_T) void wf_noise_kernel(const float* in, long ld_in, const int* n, int n_max, const wft_wave_fx* fx,
                                                        const double* sigma, float* out, long ld_out, int inplace) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n_b = wf_row_len(n, b, n_max);
  const int kind = fx[b].noise_kind;
  double sg = 0.0;
  if (kind == WFT_FX_GAUSSIAN_NOISE) sg = fx[b].noise_value;
  else if (kind == WFT_FX_GAUSSIAN_SNR) sg = sigma[b];
  const bool active = sg != 0.0;
  if (inplace && !active) return;  // uniform
  const int hi = inplace ? n_b : n_max;
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const bool vin = wf_vec_ok(row), vout = wf_vec_ok(orow);
  const unsigned long long seed = fx[b].seed;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll 1
  for (int t = 0; t < WF_TRIPS; ++t) {
    const int i = blockIdx.x * WF_SPAN + t * WF_TILE + 4 * tid;
    if (i >= hi) break;
    float v[4];
    wf_load4(row, vin, i, n_b, v);
    if (active && i < n_b) {
      unsigned w[4];
      wf_philox((unsigned)(i >> 2), k0, k1, w);
      double z[4];
      wf_normal_pair(w[0], w[1], z[0], z[1]);
      wf_normal_pair(w[2], w[3], z[2], z[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < n_b) v[k] = (float)((double)v[k] + sg * z[k]);
    }
    wf_store4(orow, vout, i, hi, v);
  }
}

// ------------------------------------------------------------------------------------------------------------ CLIP
__device__ __forceinline__ unsigned wf_key(float x) {
  const unsigned u = __float_as_uint(x);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float wf_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// one count into an LDS histogram; the lanes that share the first live lane's bin are counted by ONE atomic (a zero-padded row puts
// most of a wave into one bin, and same-address LDS atomics serialise)
__device__ __forceinline__ void wf_hist_add(unsigned* h, unsigned bin, bool valid) {
  const unsigned long long act = __ballot(valid);
  if (act == 0ull) return;  // uniform
  const int leader = __ffsll((long long)act) - 1;
  const unsigned fb = (unsigned)__shfl((int)bin, leader);
  const bool same = valid && bin == fb;
  const unsigned long long m = __ballot(same);
  if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[fb], (unsigned)__popcll(m));
  if (valid && !same) atomicAdd(&h[bin], 1u);
}

// pass 0: bits 31..21 of every key into slot 0; pass 1: bits 20..10 of the keys whose bits 31..21 match a rank's prefix, into that
// rank's slot; pass 2: bits 9..0 of the keys whose bits 31..10 match
__global__ __launch_bounds__(WF_T) void wf_hist_kernel(const float* in, long ld_in, const int* n, int n_max, const int* count,
                                                       const int* list, const unsigned* sel, unsigned* hist, int C, int pass) {
  __shared__ unsigned h[WF_SLOTS * WF_BINS];
  const int tid = threadIdx.x;
  const long items = (long)*count * C;
  const int nh = pass == 0 ? WF_BINS : WF_SLOTS * WF_BINS;
  for (long w = blockIdx.x; w < items; w += gridDim.x) {
    const int b = list[w / C], c = (int)(w % C);
    const int n_b = wf_row_len(n, b, n_max), base = c * WF_CHUNK;
    if (base >= n_b) continue;  // uniform
    for (int j = tid; j < nh; j += WF_T) h[j] = 0u;
    unsigned pre[WF_SLOTS];
    bool own[WF_SLOTS];
#pragma unroll
    for (int r = 0; r < WF_SLOTS; ++r) {
      pre[r] = pass ? sel[b * WF_SEL + r] : 0u;
      own[r] = pass ? sel[b * WF_SEL + 8 + r] == (unsigned)r : r == 0;  // a rank whose prefix an earlier rank has shares that slot
    }
    __syncthreads();
    const float* row = in + b * ld_in;
#pragma unroll 1
    for (int k = 0; k < WF_CHUNK / WF_T; ++k) {
      const int i = base + k * WF_T + tid;
      const bool valid = i < n_b;
      const unsigned key = valid ? wf_key(row[i]) : 0u;
      if (pass == 0) {
        wf_hist_add(h, key >> 21, valid);
      } else {
        const unsigned top = pass == 1 ? key >> 21 : key >> 10;
        const unsigned bin = pass == 1 ? (key >> 10) & 2047u : key & 1023u;
#pragma unroll
        for (int r = 0; r < WF_SLOTS; ++r)
          if (own[r]) wf_hist_add(h + r * WF_BINS, bin, valid && top == pre[r]);  // own[] is uniform
      }
    }
    __syncthreads();
    unsigned* g = hist + (long)b * (WF_SLOTS * WF_BINS);
    for (int j = tid; j < nh; j += WF_T) {
      const unsigned v = h[j];
      if (v) atomicAdd(&g[j], v);
    }
    __syncthreads();
  }
}

// one workgroup per listed row: the bin that holds each rank, the rank inside it, and after the last pass the thresholds
__global__ __launch_bounds__(WF_T) void wf_select_kernel(const wft_wave_fx* fx, const int* n, int n_max, const int* count, const int* list,
                                                         unsigned* sel, unsigned* hist, float* thr, int pass) {
  __shared__ unsigned part[WF_T];
  __shared__ unsigned found[2 * WF_SLOTS];  // bin, rank inside the bin
  const int tid = threadIdx.x, cnt = *count;
  constexpr int PER = WF_BINS / WF_T;
  for (int k = blockIdx.x; k < cnt; k += gridDim.x) {
    const int b = list[k];
    const int n_b = wf_row_len(n, b, n_max);  // >= 1 (plan)
    const int q = min(max(fx[b].clip_q, 0), 50);
    const long m_lo = (long)q * (n_b - 1), m_hi = (long)(100 - q) * (n_b - 1);
    const int j_lo = (int)(m_lo / 100), r_lo = (int)(m_lo % 100), j_hi = (int)(m_hi / 100), r_hi = (int)(m_hi % 100);
    unsigned pre[WF_SLOTS], rank[WF_SLOTS], slot[WF_SLOTS];
    if (pass == 0) {
      rank[0] = j_lo; rank[1] = r_lo ? j_lo + 1 : j_lo; rank[2] = j_hi; rank[3] = r_hi ? j_hi + 1 : j_hi;  // (j + 1 <= n_b - 1 when g != 0)
#pragma unroll
      for (int r = 0; r < WF_SLOTS; ++r) { pre[r] = 0u; slot[r] = 0u; }
    } else {
#pragma unroll
      for (int r = 0; r < WF_SLOTS; ++r) { pre[r] = sel[b * WF_SEL + r]; rank[r] = sel[b * WF_SEL + 4 + r]; slot[r] = sel[b * WF_SEL + 8 + r]; }
    }
    unsigned* g = hist + (long)b * (WF_SLOTS * WF_BINS);
#pragma unroll 1
    for (int r = 0; r < WF_SLOTS; ++r) {
      const unsigned* hr = g + slot[r] * WF_BINS;
      unsigned loc[PER], sum = 0u;
#pragma unroll
      for (int j = 0; j < PER; ++j) { loc[j] = hr[tid * PER + j]; sum += loc[j]; }
      part[tid] = sum;
      __syncthreads();
      unsigned before = 0u;
      for (int t = 0; t < tid; ++t) before += part[t];
      if (rank[r] >= before && rank[r] < before + sum) {  // exactly one thread: the counts of the slot add up to more than the rank
        unsigned cum = before;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (rank[r] >= cum && rank[r] < cum + loc[j]) { found[2 * r] = tid * PER + j; found[2 * r + 1] = rank[r] - cum; }
          cum += loc[j];
        }
      }
      __syncthreads();
    }
    const int bits = pass == 2 ? 10 : 11;
#pragma unroll
    for (int r = 0; r < WF_SLOTS; ++r) { pre[r] = (pre[r] << bits) | found[2 * r]; rank[r] = found[2 * r + 1]; }
    __syncthreads();  // found[] is read; the histogram is read
    if (pass < 2) {
      for (int j = tid; j < WF_SLOTS * WF_BINS; j += WF_T) g[j] = 0u;
      if (tid == 0) {
#pragma unroll
        for (int r = 0; r < WF_SLOTS; ++r) {
          unsigned s = r;
          for (int e = r - 1; e >= 0; --e)
            if (pre[e] == pre[r]) s = e;
          sel[b * WF_SEL + r] = pre[r]; sel[b * WF_SEL + 4 + r] = rank[r]; sel[b * WF_SEL + 8 + r] = s;
        }
      }
    } else if (tid == 0) {
      const float a_lo = wf_unkey(pre[0]), b_lo = wf_unkey(pre[1]), a_hi = wf_unkey(pre[2]), b_hi = wf_unkey(pre[3]);
      const double g_lo = (double)r_lo / 100.0, g_hi = (double)r_hi / 100.0;
      thr[2 * b] = r_lo ? (float)((double)a_lo + g_lo * ((double)b_lo - (double)a_lo)) : a_lo;
      thr[2 * b + 1] = r_hi ? (float)((double)a_hi + g_hi * ((double)b_hi - (double)a_hi)) : a_hi;
    }
  }
}

__global__ __launch_bounds__(WF_T) void wf_clip_kernel(const float* in, long ld_in, const int* n, int n_max, const wft_wave_fx* fx,
                                                       const float* thr, float* out, long ld_out, int inplace) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n_b = wf_row_len(n, b, n_max);
  const bool active = fx[b].clip_kind == WFT_FX_CLIPPING && n_b >= 1;
  if (inplace && !active) return;  // uniform
  const int hi = inplace ? n_b : n_max;
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const bool vin = wf_vec_ok(row), vout = wf_vec_ok(orow);
  const float lo = active ? thr[2 * b] : 0.f, up = active ? thr[2 * b + 1] : 0.f;
#pragma unroll 1
  for (int t = 0; t < WF_TRIPS; ++t) {
    const int i = blockIdx.x * WF_SPAN + t * WF_TILE + 4 * tid;
    if (i >= hi) break;
    float v[4];
    wf_load4(row, vin, i, n_b, v);
    if (active) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < n_b) v[k] = v[k] < lo ? lo : (v[k] > up ? up : v[k]);
    }
    wf_store4(orow, vout, i, hi, v);
  }
}

// ------------------------------------------------------------------------------------------------------------ LEVEL
__global__ __launch_bounds__(WF_T) void wf_level_kernel(const float* in, long ld_in, const int* n, int n_max, const wft_wave_fx* fx,
                                                        float* out, long ld_out, int inplace) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n_b = wf_row_len(n, b, n_max);
  const int kind = fx[b].level_kind;
  const bool active = kind == WFT_FX_GAIN || kind == WFT_FX_GAIN_TRANSITION || kind == WFT_FX_SHIFT;
  if (inplace && !active) return;  // uniform
  const int hi = inplace ? n_b : n_max;
  const float* row = in + b * ld_in;
  float* orow = out + b * ld_out;
  const bool vin = wf_vec_ok(row), vout = wf_vec_ok(orow);
  const float ratio = fx[b].gain_ratio;
  const double d0 = fx[b].db_start, dd = fx[b].db_end - fx[b].db_start;
  const long long t0 = fx[b].t0;
  const int64_t rl = fx[b].ramp_len - 1;
  const double den = (double)(rl > 1 ? rl : 1);
  long long s = 0;
  int F = 0;
  if (kind == WFT_FX_SHIFT && n_b > 0) {
    s = (long long)rint(fx[b].shift_fraction * (double)n_b) % n_b;  // rint: to nearest, ties to even
    if (s < 0) s += n_b;
    const int64_t fl = fx[b].fade_len;
    F = fl < 0 ? 0 : (fl > n_b / 2 ? n_b / 2 : (int)fl);
    if (s == 0) F = 0;
  }
  const double fden = (double)max(F - 1, 1);
#pragma unroll 1
  for (int t = 0; t < WF_TRIPS; ++t) {
    const int i = blockIdx.x * WF_SPAN + t * WF_TILE + 4 * tid;
    if (i >= hi) break;
    float v[4];
    if (kind == WFT_FX_SHIFT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = 0.f;
        if (i + k < n_b) {
          int d = i + k - (int)s;
          if (d < 0) d += n_b;
          const float x = row[d];
          const int e = n_b - 1 - d;
          if (d < F) v[k] = (float)((double)x * ((double)d / fden));
          else if (e < F) v[k] = (float)((double)x * ((double)e / fden));
          else v[k] = x;
        }
      }
    } else {
      wf_load4(row, vin, i, n_b, v);
      if (kind == WFT_FX_GAIN) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i + k < n_b) v[k] = v[k] * ratio;
      } else if (kind == WFT_FX_GAIN_TRANSITION) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (i + k < n_b) {
            const long long rel = (long long)((unsigned long long)(i + k) - (unsigned long long)t0);
            const double u = fmin(fmax((double)rel / den, 0.0), 1.0);
            v[k] = (float)((double)v[k] * exp10((d0 + dd * u) / 20.0));
          }
        }
      }
    }
    wf_store4(orow, vout, i, hi, v);
  }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static inline int64_t wf_head_bytes(int B) { return 8 + 4 * (int64_t)((B + 1) / 2 * 2) + 8 * (int64_t)B; }  // count, list, sigma | lo hi

extern "C" int wft_wave_fx_tile(void) { return WF_TILE; }

extern "C" int64_t wft_wave_fx_workspace_bytes(int B, int64_t n_max, int stage) {
  if (B < 1 || B > 65535 || n_max < 1 || n_max > WF_MAX_N) return -1;
  const int64_t C = cdiv64(n_max, WF_CHUNK);
  switch (stage) {
    case WFT_FX_NOISE: return wf_head_bytes(B) + (int64_t)B * C * (int64_t)sizeof(double);
    case WFT_FX_CLIP: return wf_head_bytes(B) + (int64_t)B * (WF_SEL + WF_SLOTS * WF_BINS) * (int64_t)sizeof(unsigned);
    case WFT_FX_LEVEL: return 8;
    default: return -1;
  }
}

extern "C" int wft_wave_fx_f32(const float* in, int64_t ld_in, const int32_t* n, int64_t n_max, const wft_wave_fx* fx, int stage,
                               float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes, int B, void* stream) {
  WFT_CHECK_ARG(in && fx && out && workspace, "null pointer");
  const bool known_stage = stage == WFT_FX_NOISE || stage == WFT_FX_CLIP || stage == WFT_FX_LEVEL;  // (the message quotes the condition)
  WFT_CHECK_ARG(known_stage, "unknown stage (0 noise, 1 clip, 2 level)");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= WF_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_in >= n_max && ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG(workspace_bytes >= wft_wave_fx_workspace_bytes(B, n_max, stage), "workspace too small");
  WFT_CHECK_ARG((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)n % 4 == 0 && (uintptr_t)fx % 8 == 0 &&
                    (uintptr_t)workspace % 8 == 0,
                "in / out / n must be 4-byte, fx / workspace 8-byte aligned");
  const bool inplace = in == out && ld_in == ld_out;
  if (!inplace) {  // in place is the same pointer and the same stride; anything else must not overlap
    const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (B - 1) * ld_in + n_max);
    const uintptr_t o0 = (uintptr_t)out, o1 = (uintptr_t)(out + (B - 1) * ld_out + n_max);
    WFT_CHECK_ARG(i1 <= o0 || o1 <= i0, "in and out overlap partially");
  }
  hipStream_t st = (hipStream_t)stream;
  const int nm = (int)n_max, C = (int)cdiv64(n_max, WF_CHUNK);
  const dim3 agrid((unsigned)cdiv64(n_max, WF_SPAN), (unsigned)B);
  char* ws = (char*)workspace;
  int* count = (int*)ws;
  int* list = (int*)(ws + 8);
  char* row8 = ws + 8 + 4 * (int64_t)((B + 1) / 2 * 2);  // sigma f64 [B] | lo, hi f32 [B][2]
  char* tail = ws + wf_head_bytes(B);
  if (stage == WFT_FX_NOISE) {
    double* sigma = (double*)row8;
    double* partial = (double*)tail;
    hipLaunchKernelGGL(wf_plan_kernel, dim3(1), dim3(WF_T), 0, st, fx, n, nm, B, stage, count, list);
    hipLaunchKernelGGL(wf_sumsq_kernel, dim3(WF_GRID), dim3(WF_T), 0, st, in, (long)ld_in, n, nm, (const int*)count, (const int*)list,
                       partial, C);
    hipLaunchKernelGGL(wf_sigma_kernel, dim3((unsigned)(cdiv64(B, WF_T) < 64 ? cdiv64(B, WF_T) : 64)), dim3(WF_T), 0, st, fx, n, nm,
                       (const int*)count, (const int*)list, (const double*)partial, C, sigma);
    hipLaunchKernelGGL(wf_noise_kernel, agrid, dim3(WF_T), 0, st, in, (long)ld_in, n, nm, fx, (const double*)sigma, out, (long)ld_out,
                       (int)inplace);
  } else if (stage == WFT_FX_CLIP) {
    float* thr = (float*)row8;
    unsigned* sel = (unsigned*)tail;
    unsigned* hist = sel + (int64_t)B * WF_SEL;
    hipLaunchKernelGGL(wf_plan_kernel, dim3(1), dim3(WF_T), 0, st, fx, n, nm, B, stage, count, list);
    if (hipMemsetAsync(hist, 0, (size_t)B * WF_SLOTS * WF_BINS * sizeof(unsigned), st) != hipSuccess) {
      wft_set_error("wft_wave_fx_f32: clearing the histograms failed");
      return WFT_ERR_LAUNCH;
    }
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(wf_hist_kernel, dim3(WF_GRID), dim3(WF_T), 0, st, in, (long)ld_in, n, nm, (const int*)count, (const int*)list,
                         (const unsigned*)sel, hist, C, pass);
      hipLaunchKernelGGL(wf_select_kernel, dim3(256), dim3(WF_T), 0, st, fx, n, nm, (const int*)count, (const int*)list, sel, hist, thr,
                         pass);
    }
    hipLaunchKernelGGL(wf_clip_kernel, agrid, dim3(WF_T), 0, st, in, (long)ld_in, n, nm, fx, (const float*)thr, out, (long)ld_out,
                       (int)inplace);
  } else {
    hipLaunchKernelGGL(wf_level_kernel, agrid, dim3(WF_T), 0, st, in, (long)ld_in, n, nm, fx, out, (long)ld_out, (int)inplace);
  }
  WFT_CHECK_LAUNCH_AS("wft_wave_fx_f32");
  return WFT_OK;
}
