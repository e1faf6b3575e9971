// align.hip — word-level alignment (include/wft.h "Word-level alignment"): the device stages of upstream's
// `whisper/timing.py: find_alignment` behind the softmax scores of the alignment heads.
//  attn_probs_kernel    row softmax of the scaled cross-attention scores of a head list, written out in fp32
//  align_matrix_kernel  standardise over the tokens, median-filter along the frames, average the heads
//  dtw_kernel           dynamic time warping over one audio's cost matrix, anti-diagonal sweep + backtrace in one launch
//  word_spans_kernel    the first frame of every path row, then per word its two boundary frames and its mean token probability
// Per-audio lengths are device int32 arrays; every kernel clamps them to its static extents before it forms an address.
#include <math.h>

#include "common.h"

// ----------------------------------------------------------------------------- a. alignment-head probabilities
// One workgroup = 32 query rows of one (audio, selected head); its four waves take the 32-key tiles in turn.  Scores are
// mfma_f32_32x32x16_bf16 products (A = the query tile, B = a key tile, both read from global memory in fragment order: lane l
// holds 8 consecutive d of row / key l & 31 at d = 16 ks + 8 (l >> 5)), so an accumulator register is one query row and its lane
// one key.  Pass 1 keeps a running (max, sum) per lane and row and merges them once, through the wave and then LDS; pass 2
// recomputes the tile and makes the one normalised write — the scores never leave the chip, the output is written once.
#define AP_THREADS 256
#define AP_WAVES 4
#define AP_NEG -1.0e30f  // "no key yet": exp2(AP_NEG - m) is 0 without an inf - inf

__device__ __forceinline__ int ap_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ f32x16 ap_scores(const bf16x8* qa, const unsigned short* kb, long ldk, int key, int Tk, int lane) {
  const int kr = min(key + (lane & 31), Tk - 1);  // a key behind the buffer is read as the last one and masked by the caller
  const unsigned short* kp = kb + (long)kr * ldk + (lane >> 5) * 8;
  f32x16 acc = f32x16{0};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[ks], *(const bf16x8*)(kp + ks * 16), acc, 0, 0, 0);
  return acc;
}

__global__ __launch_bounds__(AP_THREADS) void attn_probs_kernel(const unsigned short* q, long ldq, long q_bs, const unsigned short* k,
                                                                long ldk, long k_bs, const int* heads, const int* n_tok,
                                                                const int* n_key, float* probs, long p_bs, long p_hs, long ldp, int H,
                                                                int Tq, int Tk, float alpha) {
  __shared__ float s_m[AP_WAVES][32], s_l[AP_WAVES][32];
  const int b = blockIdx.z, s = blockIdx.y, t0 = blockIdx.x * 32;
  const int nt = min(max(n_tok[b], 0), Tq), nk = min(max(n_key[b], 0), Tk);
  if (t0 >= nt || nk <= 0) return;  // (the whole workgroup)
  const int h = min(max(heads[s], 0), H - 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned short* qp = q + b * q_bs + (long)min(t0 + (lane & 31), Tq - 1) * ldq + h * 64 + (lane >> 5) * 8;
  const unsigned short* kb = k + b * k_bs + h * 64;
  bf16x8 qa[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qa[ks] = *(const bf16x8*)(qp + ks * 16);
  const int ntiles = (nk + 31) / 32;

  float m[16], l[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) { m[e] = AP_NEG; l[e] = 0.f; }
  for (int kt = wave; kt < ntiles; kt += AP_WAVES) {
    const f32x16 acc = ap_scores(qa, kb, ldk, kt * 32, Tk, lane);
    const bool live = kt * 32 + (lane & 31) < nk;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float x = live ? acc[e] * alpha : AP_NEG;
      const float mn = fmaxf(m[e], x);
      l[e] = l[e] * __builtin_amdgcn_exp2f(m[e] - mn) + (live ? __builtin_amdgcn_exp2f(x - mn) : 0.f);
      m[e] = mn;
    }
  }
  // merge the 32 lanes that share a row (xor 16 .. 1 stays inside a half wave), then the waves
#pragma unroll
  for (int e = 0; e < 16; ++e) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float om = __shfl_xor(m[e], o, 64), ol = __shfl_xor(l[e], o, 64);
      const float mn = fmaxf(m[e], om);
      l[e] = l[e] * __builtin_amdgcn_exp2f(m[e] - mn) + ol * __builtin_amdgcn_exp2f(om - mn);
      m[e] = mn;
    }
    if ((lane & 31) == 0) {
      s_m[wave][ap_row(e, lane)] = m[e];
      s_l[wave][ap_row(e, lane)] = l[e];
    }
  }
  __syncthreads();
  float inv[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int r = ap_row(e, lane);
    float mm = s_m[0][r];
#pragma unroll
    for (int w = 1; w < AP_WAVES; ++w) mm = fmaxf(mm, s_m[w][r]);
    float ll = 0.f;
#pragma unroll
    for (int w = 0; w < AP_WAVES; ++w) ll += s_l[w][r] * __builtin_amdgcn_exp2f(s_m[w][r] - mm);
    m[e] = mm;
    inv[e] = 1.0f / ll;  // (nk >= 1: ll >= 1)
  }
  float* pb = probs + b * p_bs + s * p_hs;
  for (int kt = wave; kt < ntiles; kt += AP_WAVES) {
    const f32x16 acc = ap_scores(qa, kb, ldk, kt * 32, Tk, lane);
    const int key = kt * 32 + (lane & 31);
    if (key < nk) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int t = t0 + ap_row(e, lane);
        if (t < nt) pb[(long)t * ldp + key] = __builtin_amdgcn_exp2f(acc[e] * alpha - m[e]) * inv[e];
      }
    }
  }
}

extern "C" int wft_attn_probs_bf16(const wft_attn_args* a, const int32_t* heads, int n_heads, const int32_t* n_tok, const int32_t* n_key,
                                   float* probs, int64_t p_bs, int64_t p_hs, int64_t ldp, void* stream) {
  WFT_CHECK_ARG(a && a->q && a->k && heads && n_tok && n_key && probs, "null pointer");
  WFT_CHECK_ARG(a->B >= 1 && a->B <= 65535 && a->H >= 1 && a->Tq >= 1 && a->Tk >= 1, "bad shape");
  WFT_CHECK_ARG(n_heads >= 1 && n_heads <= 65535, "n_heads must lie in 1..65535");
  WFT_CHECK_ARG(a->ldq % 8 == 0 && a->ldk % 8 == 0 && a->q_bs % 8 == 0 && a->k_bs % 8 == 0 && ((uintptr_t)a->q | (uintptr_t)a->k) % 16 == 0,
                "q / k rows must be 16-byte aligned");
  WFT_CHECK_ARG(a->ldq >= (int64_t)a->H * 64 && a->ldk >= (int64_t)a->H * 64, "row strides below H * 64");
  WFT_CHECK_ARG(ldp >= a->Tk && p_hs >= (int64_t)a->Tq * ldp && p_bs >= 0, "probs strides do not hold [n_heads, Tq, Tk]");
  WFT_CHECK_ARG(a->scale > 0.f, "scale must be positive");
  WFT_CHECK_ARG(!a->q_prescaled, "cross-attention q is never prescaled");
  const dim3 grid((a->Tq + 31) / 32, n_heads, a->B);
  hipLaunchKernelGGL(attn_probs_kernel, grid, dim3(AP_THREADS), 0, (hipStream_t)stream, a->q, (long)a->ldq, (long)a->q_bs, a->k, (long)a->ldk,
                     (long)a->k_bs, heads, n_tok, n_key, probs, (long)p_bs, (long)p_hs, (long)ldp, a->H, a->Tq, a->Tk,
                     a->scale * 1.4426950408889634f);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- b. standardise, median-filter, average the heads
// One workgroup = 32 output columns of one audio plus a halo of width / 2 on each side (64 LDS columns), all token rows, every head
// in turn.  LDS column c stands for source column reflect(c0 - halo + c) — the reflection is resolved per column, so the strip
// edges need no special case.  Per head every thread loads its 28 rows of one LDS column into registers (all loads in flight at
// once: every probability is read once), the column mean and the biased deviation are reduced through LDS in a fixed order (the
// thread's rows ascending, then the 16 row groups in order), and the rows go through a 64 x 64 LDS tile in chunks: z = (p - mean)
// / std in, the median of every thread's two windows out, into its 14 accumulators.  The median is the classic 13-exchange
// selection network at the default width 7 (min / max pairs on registers) and a rank count at any other width — the element
// with exactly width / 2 others below it, equal values ordered by position.
#define AM_THREADS 1024
#define AM_COLS 32
#define AM_LDS_COLS 64
#define AM_CHUNK 64
#define AM_MAX_TQ 448
#define AM_MAX_WIDTH 31
#define AM_ROWS_PER_THREAD (AM_MAX_TQ / 16)

__device__ __forceinline__ int am_reflect(int j, int n) {
  if (j < 0) j = -j;
  if (j >= n) j = 2 * (n - 1) - j;
  return min(max(j, 0), n - 1);  // (a column past the reflected range is not part of any written window: any valid address)
}

__device__ __forceinline__ void am_exchange(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// the median of z[0 .. 6]
__device__ __forceinline__ float am_median7(const float* z) {
  float p0 = z[0], p1 = z[1], p2 = z[2], p3 = z[3], p4 = z[4], p5 = z[5], p6 = z[6];
  am_exchange(p0, p5); am_exchange(p0, p3); am_exchange(p1, p6); am_exchange(p2, p4); am_exchange(p0, p1);
  am_exchange(p3, p5); am_exchange(p2, p6); am_exchange(p2, p3); am_exchange(p3, p6); am_exchange(p4, p5);
  am_exchange(p1, p4); am_exchange(p1, p3); am_exchange(p3, p4);
  return p3;
}

// the median of z[0 .. 2 hw] by rank count
__device__ __forceinline__ float am_median(const float* z, int hw) {
  float med = z[hw];
  for (int x = 0; x <= 2 * hw; ++x) {
    const float vx = z[x];
    int rank = 0;
    for (int y = 0; y <= 2 * hw; ++y) {
      const float vy = z[y];
      rank += (vy < vx || (vy == vx && y < x)) ? 1 : 0;
    }
    if (rank == hw) med = vx;
  }
  return med;
}

__global__ __launch_bounds__(AM_THREADS) void align_matrix_kernel(const float* probs, long p_bs, long p_hs, long ldp, const int* n_tok,
                                                                  const int* n_key, float* out, long m_bs, long ldm, int n_sel, int Tq,
                                                                  int Tk, int width) {
  __shared__ float s_z[AM_CHUNK][AM_LDS_COLS];
  __shared__ float s_red[AM_THREADS / AM_LDS_COLS][AM_LDS_COLS];
  __shared__ float s_mean[AM_LDS_COLS], s_std[AM_LDS_COLS];
  const int b = blockIdx.y, c0 = blockIdx.x * AM_COLS;
  const int nt = min(max(n_tok[b], 0), min(Tq, AM_MAX_TQ)), nk = min(max(n_key[b], 0), Tk);
  if (c0 >= nk || nt <= 0) return;  // (the whole workgroup)
  const int hw = nk <= width / 2 ? 0 : width / 2;  // upstream's early return: no filter for that audio
  const int tid = threadIdx.x;
  const int lc = tid & 63, lg = tid >> 6;  // loader: LDS column, row group (16)
  const int oc = tid & 31, og = tid >> 5;  // output: column of the strip, row group (32)
  const int src = am_reflect(c0 - hw + lc, nk);
  const bool out_live = c0 + oc < nk;
  const unsigned off = (unsigned)(lg * ldp + src);  // row lg of the thread's source column inside a head's [Tq, ldp] slice
  float acc[AM_MAX_TQ / 32];
#pragma unroll
  for (int i = 0; i < AM_MAX_TQ / 32; ++i) acc[i] = 0.f;

  for (int s = 0; s < n_sel; ++s) {
    const float* hb = probs + b * p_bs + s * p_hs;  // (uniform: the loads take a scalar base and one 32-bit lane offset)
    float p[AM_ROWS_PER_THREAD];                    // rows lg + 16 i of the column; 0 behind the audio's tokens
#pragma unroll
    for (int i = 0; i < AM_ROWS_PER_THREAD; ++i) p[i] = lg + 16 * i < nt ? (hb + (long)i * 16 * ldp)[off] : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < AM_ROWS_PER_THREAD; ++i) sum += p[i];
    s_red[lg][lc] = sum;
    __syncthreads();
    if (tid < 64) {
      float tot = 0.f;
      for (int g = 0; g < 16; ++g) tot += s_red[g][tid];
      s_mean[tid] = tot / (float)nt;
    }
    __syncthreads();
    const float mean = s_mean[lc];
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < AM_ROWS_PER_THREAD; ++i) {
      const float d = lg + 16 * i < nt ? p[i] - mean : 0.f;
      sq += d * d;
    }
    s_red[lg][lc] = sq;
    __syncthreads();
    if (tid < 64) {
      float tot = 0.f;
      for (int g = 0; g < 16; ++g) tot += s_red[g][tid];
      s_std[tid] = sqrtf(tot / (float)nt);
    }
    __syncthreads();
    const float sd = s_std[lc];
#pragma unroll
    for (int ch = 0; ch < AM_MAX_TQ / AM_CHUNK; ++ch) {
      if (ch * AM_CHUNK < nt) {  // (the whole workgroup)
#pragma unroll
        for (int i = 0; i < AM_CHUNK / 16; ++i) {
          const int r = lg + 16 * i;
          s_z[r][lc] = ch * AM_CHUNK + r < nt ? (p[ch * (AM_CHUNK / 16) + i] - mean) / sd : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float* zr = &s_z[og + 32 * i][oc];  // the window is zr[0 .. 2 hw], its centre zr[hw]
          acc[2 * ch + i] += hw == 3 ? am_median7(zr) : am_median(zr, hw);
        }
        __syncthreads();
      }
    }
  }
  float* ob = out + b * m_bs + c0 + oc;
  const float ns = (float)n_sel;
#pragma unroll
  for (int ch = 0; ch < AM_MAX_TQ / AM_CHUNK; ++ch)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = ch * AM_CHUNK + og + 32 * i;
      if (out_live && t < nt) ob[(long)t * ldm] = acc[2 * ch + i] / ns;
    }
}

extern "C" int wft_align_matrix(const float* probs, int64_t p_bs, int64_t p_hs, int64_t ldp, const int32_t* n_tok, const int32_t* n_key,
                                float* matrix, int64_t m_bs, int64_t ldm, int B, int n_sel, int Tq, int Tk, int width, void* stream) {
  WFT_CHECK_ARG(probs && n_tok && n_key && matrix, "null pointer");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_sel >= 1 && Tk >= 1, "bad shape");
  WFT_CHECK_ARG(Tq >= 1 && Tq <= AM_MAX_TQ, "Tq must lie in 1..448 (n_text_ctx)");
  WFT_CHECK_ARG(width >= 1 && width <= AM_MAX_WIDTH && (width & 1), "width must be odd and lie in 1..31");
  WFT_CHECK_ARG(ldp <= (1 << 24), "ldp above 2^24 (row offsets inside a head's slice are 32-bit)");
  WFT_CHECK_ARG(ldp >= Tk && p_hs >= (int64_t)Tq * ldp && p_bs >= 0 && ldm >= Tk && m_bs >= (int64_t)Tq * ldm,
                "strides do not hold [n_sel, Tq, Tk] / [Tq, Tk]");
  const dim3 grid((Tk + AM_COLS - 1) / AM_COLS, B);
  hipLaunchKernelGGL(align_matrix_kernel, grid, dim3(AM_THREADS), 0, (hipStream_t)stream, probs, (long)p_bs, (long)p_hs, (long)ldp, n_tok,
                     n_key, matrix, (long)m_bs, (long)ldm, n_sel, Tq, Tk, width);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- c. dynamic time warping
// One workgroup per audio, thread r = token row r.  At step s thread r fills cell (r, j = s - r): its own previous value is the
// horizontal predecessor, the value thread r - 1 wrote to LDS at step s - 1 the vertical one, and what it read there a step earlier
// the diagonal one.  Two LDS rows alternate, one barrier per step.  The cost row of a thread is read eight columns ahead into
// registers, so no load sits on the dependent chain.  Trace bytes go to the workspace in anti-diagonal order ([s][r]: one
// coalesced store per step); after the sweep thread 0 walks them back, writing the path reversed, and the workgroup turns it round.
#define DTW_MAX_ROWS 448
#define DTW_AHEAD 8

__global__ __launch_bounds__(DTW_MAX_ROWS) void dtw_kernel(const float* matrix, long m_bs, long ldm, int row0, const int* n_rows,
                                                           const int* n_cols, int negate, unsigned char* trace, long t_bs,
                                                           int n_rows_max, int n_cols_max, int* path_text, int* path_time, long ld_path,
                                                           int* path_len) {
  __shared__ float s_val[2][DTW_MAX_ROWS];
  __shared__ int s_len;
  const int b = blockIdx.x, r = threadIdx.x;
  const int N = min(max(n_rows[b], 0), n_rows_max), M = min(max(n_cols[b], 0), n_cols_max);
  if (N == 0 || M == 0) {  // (the whole workgroup)
    if (r == 0) path_len[b] = 0;
    return;
  }
  const bool mine = r < N;
  s_val[0][r] = s_val[1][r] = INFINITY;  // what a thread reads of its upper neighbour before that one has started: column -1
  __syncthreads();
  const float* xr = matrix + b * m_bs + (long)(row0 + (mine ? r : 0)) * ldm;
  unsigned char* tr = trace + b * t_bs;
  const float sign = negate ? -1.f : 1.f;
  const float inf = INFINITY;
  float prev = inf;                  // cost[r][j - 1]
  float up_old = r == 0 ? 0.f : inf; // cost[r - 1][j - 1]: row -1 is inf but for the corner
  const int S = N + M - 1;
  float nxt[DTW_AHEAD];
#pragma unroll
  for (int i = 0; i < DTW_AHEAD; ++i) {
    const int j = i - r;
    nxt[i] = (mine && j >= 0 && j < M) ? xr[j] : 0.f;
  }
  for (int sb = 0; sb < S; sb += DTW_AHEAD) {
    float cur[DTW_AHEAD];
#pragma unroll
    for (int i = 0; i < DTW_AHEAD; ++i) {
      cur[i] = nxt[i];
      const int j = sb + DTW_AHEAD + i - r;
      nxt[i] = (mine && j >= 0 && j < M) ? xr[j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < DTW_AHEAD; ++i) {
      const int s = sb + i;
      if (s < S) {  // (the whole workgroup)
        const int j = s - r;
        const float up = r == 0 ? inf : s_val[s & 1][r - 1];  // cost[r - 1][j], written at step s - 1 (step 0: unused, j < 0)
        if (mine && j >= 0 && j < M) {
          const float c0 = up_old, c1 = up, c2 = prev;
          float c;
          unsigned char t;
          if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
          else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
          else { c = c2; t = 2; }
          prev = sign * cur[i] + c;
          tr[(long)s * n_rows_max + r] = t;
          s_val[(s + 1) & 1][r] = prev;
        }
        up_old = up;
        __syncthreads();
      }
    }
  }
  // (the barrier of the last step also orders the trace stores of this workgroup before thread 0's loads)
  int* pt = path_text + b * ld_path;
  int* pj = path_time + b * ld_path;
  if (r == 0) {
    int i = N - 1, j = M - 1, n = 0;
    while (i >= 0 && j >= 0 && n < ld_path) {
      pt[n] = i;
      pj[n] = j;
      ++n;
      const unsigned char t = tr[(long)(i + j) * n_rows_max + i];
      if (t == 0) { --i; --j; }
      else if (t == 1) --i;
      else --j;
    }
    s_len = n;
    path_len[b] = n;
  }
  __syncthreads();
  const int n = s_len;
  for (int x = r; x < n / 2; x += blockDim.x) {
    const int y = n - 1 - x;
    const int a0 = pt[x], a1 = pj[x];
    pt[x] = pt[y];
    pj[x] = pj[y];
    pt[y] = a0;
    pj[y] = a1;
  }
}

extern "C" int64_t wft_dtw_workspace_bytes(int B, int n_rows_max, int n_cols_max) {
  if (B < 1 || n_rows_max < 1 || n_cols_max < 1) return 0;
  const int64_t per = (int64_t)(n_rows_max + n_cols_max - 1) * n_rows_max;
  return B * ((per + 255) / 256 * 256);
}

extern "C" int wft_dtw_f32(const float* matrix, int64_t m_bs, int64_t ldm, int matrix_rows, int row0, const int32_t* n_rows,
                           const int32_t* n_cols, int B, int n_rows_max, int n_cols_max, int negate, int32_t* path_text,
                           int32_t* path_time, int64_t ld_path, int32_t* path_len, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  WFT_CHECK_ARG(matrix && n_rows && n_cols && path_text && path_time && path_len && workspace, "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_cols_max >= 1, "bad shape");
  WFT_CHECK_ARG(n_rows_max >= 1 && n_rows_max <= DTW_MAX_ROWS, "n_rows_max must lie in 1..448 (one thread per token row)");
  WFT_CHECK_ARG(row0 >= 0 && (int64_t)row0 + n_rows_max <= matrix_rows, "row0 + n_rows_max exceeds the matrix rows");
  WFT_CHECK_ARG(ldm >= n_cols_max && m_bs >= (int64_t)matrix_rows * ldm, "matrix strides do not hold [matrix_rows, n_cols_max]");
  WFT_CHECK_ARG(ld_path >= (int64_t)n_rows_max + n_cols_max - 1, "ld_path below n_rows_max + n_cols_max - 1");
  WFT_CHECK_ARG(workspace_bytes >= wft_dtw_workspace_bytes(B, n_rows_max, n_cols_max), "workspace too small");
  const int threads = (n_rows_max + 63) / 64 * 64;
  hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, matrix, (long)m_bs, (long)ldm, row0, n_rows, n_cols, negate,
                     (unsigned char*)workspace, (long)(wft_dtw_workspace_bytes(B, n_rows_max, n_cols_max) / B), n_rows_max, n_cols_max,
                     path_text, path_time, (long)ld_path, path_len);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- d. word spans
// One workgroup per audio.  The path's text rows go through LDS in chunks of WS_CHUNK entries; thread r looks for the lowest
// position that holds row r (16-byte LDS reads, the same address in every lane: a broadcast) and reads that position's frame once.
// Every row has one owner, so no two threads write the same word of s_first.  Then thread w forms word w: two lookups and a serial
// fp32 sum over its tokens, in ascending order.
#define WS_THREADS 512  // >= DTW_MAX_ROWS: one thread per path row
#define WS_CHUNK 2048

__global__ __launch_bounds__(WS_THREADS) void word_spans_kernel(const int* path_text, const int* path_time, int ld_path, const int* path_len,
                                                               const int* bounds, long ld_bounds, const int* n_words,
                                                               const float* token_probs, long n_probs, const int* tok_off, int* start_frame,
                                                               int* end_frame, float* prob, long ld_words, int n_words_max, int n_rows_max) {
  __shared__ __attribute__((aligned(16))) int s_text[WS_CHUNK];
  __shared__ int s_first[WS_THREADS];
  const int b = blockIdx.x, r = threadIdx.x;
  const int L = min(max(path_len[b], 0), ld_path), nw = min(max(n_words[b], 0), n_words_max);
  if (L == 0 || nw == 0) return;  // (the whole workgroup)
  const int* pt = path_text + (long)b * ld_path;
  int found = -1;  // the lowest position of row r
  for (int c0 = 0; c0 < L; c0 += WS_CHUNK) {
    const int n = min(WS_CHUNK, L - c0);
    for (int x = r; x < WS_CHUNK; x += WS_THREADS) s_text[x] = x < n ? pt[c0 + x] : -1;  // (-1 is no row)
    __syncthreads();
    if (found < 0 && r < n_rows_max) {
      for (int x = 0; x < n; x += 4) {
        const int4 v = *(const int4*)(s_text + x);
        const int hit = v.x == r ? 0 : v.y == r ? 1 : v.z == r ? 2 : v.w == r ? 3 : -1;
        if (hit >= 0) {
          found = c0 + x + hit;
          break;
        }
      }
    }
    __syncthreads();
  }
  s_first[r] = found >= 0 ? path_time[(long)b * ld_path + found] : -1;
  __syncthreads();
  const int* bd = bounds + b * ld_bounds;
  const long off = min(max((long)tok_off[b], 0L), n_probs);
  for (int w = r; w < nw; w += WS_THREADS) {
    const int lo = min(max(bd[w], 0), n_rows_max - 1), hi = min(max(bd[w + 1], 0), n_rows_max - 1);
    float sum = 0.f;
    for (int i = lo; i < hi; ++i) sum += off + i < n_probs ? token_probs[off + i] : 0.f;
    start_frame[b * ld_words + w] = s_first[lo];
    end_frame[b * ld_words + w] = s_first[hi];
    prob[b * ld_words + w] = hi > lo ? sum / (float)(hi - lo) : 0.f;
  }
}

extern "C" int wft_word_spans(const int32_t* path_text, const int32_t* path_time, int64_t ld_path, const int32_t* path_len,
                              const int32_t* bounds, int64_t ld_bounds, const int32_t* n_words, const float* token_probs, int64_t n_probs,
                              const int32_t* tok_off, int32_t* start_frame, int32_t* end_frame, float* prob, int64_t ld_words, int B,
                              int n_rows_max, void* stream) {
  WFT_CHECK_ARG(path_text && path_time && path_len && bounds && n_words && token_probs && tok_off && start_frame && end_frame && prob,
                "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_rows_max >= 1 && n_rows_max <= DTW_MAX_ROWS, "B >= 1 and n_rows_max in 1..448 (one thread per path row)");
  WFT_CHECK_ARG(ld_path >= 1 && ld_path <= (1 << 30), "ld_path must lie in 1..2^30");
  WFT_CHECK_ARG(ld_bounds >= 2 && ld_words >= 1 && n_probs >= 1, "bounds rows hold at least 2 entries, word rows and token_probs at least 1");
  int64_t n_words_max = n_rows_max;  // a word has at least one row: more words than rows cannot be
  if (ld_bounds - 1 < n_words_max) n_words_max = ld_bounds - 1;
  if (ld_words < n_words_max) n_words_max = ld_words;
  hipLaunchKernelGGL(word_spans_kernel, dim3(B), dim3(WS_THREADS), 0, (hipStream_t)stream, path_text, path_time, (int)ld_path, path_len, bounds,
                     (long)ld_bounds, n_words, token_probs, (long)n_probs, tok_off, start_frame, end_frame, prob, (long)ld_words, (int)n_words_max,
                     n_rows_max);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
