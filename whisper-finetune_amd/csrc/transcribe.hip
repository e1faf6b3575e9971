// transcribe.hip — language detection and long-form windows (include/wft.h "Language detection and long-form windows").
//  lang_probs_kernel    upstream's `detect_language` tail: softmax and argmax over the language columns of one logits row
//  mel_windows_kernel   upstream's `pad_or_trim(mel[:, seek : seek + segment_size], N_FRAMES)` for a batch of rows, every row with
//                       its own recording and its own seek, all of them read from device memory
// Both clamp what they read from device memory before they form an address.
#include <limits.h>
#include <math.h>

#include "common.h"

// ----------------------------------------------------------------------------- a. language probabilities
// One workgroup per row; thread t holds the language columns j = t, t + 256, ... (at most four: n_lang <= 1024) in registers, so
// every logit is gathered once.  Maximum with the lowest j on ties, then exp(x - max) summed in a fixed order (the thread's own
// values ascending, the xor butterfly of the wave, the four waves in order), ocml's expf / logf: the same arguments give the same bits.
#define LP_THREADS 256
#define LP_WAVES 4
#define LP_PER 4
#define LP_MAX_LANG (LP_THREADS * LP_PER)

__global__ __launch_bounds__(LP_THREADS) void lang_probs_kernel(const unsigned short* logits, long ld, int V, const int* lang_ids,
                                                                int n_lang, float* probs, long ld_probs, long* best) {
  __shared__ float s_max[LP_WAVES], s_sum[LP_WAVES];
  __shared__ int s_arg[LP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned short* row = logits + b * ld;
  float x[LP_PER];
  float m = -INFINITY;
  int mj = INT_MAX;
#pragma unroll
  for (int i = 0; i < LP_PER; ++i) {
    const int j = tid + LP_THREADS * i;
    x[i] = -INFINITY;
    if (j < n_lang) {
      x[i] = bf2f(row[min(max(lang_ids[j], 0), V - 1)]);
      if (x[i] > m) {  // (j ascends: the first of equal values stays)
        m = x[i];
        mj = j;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oj = __shfl_xor(mj, o, 64);
    if (om > m || (om == m && oj < mj)) {
      m = om;
      mj = oj;
    }
  }
  if (lane == 0) {
    s_max[wave] = m;
    s_arg[wave] = mj;
  }
  __syncthreads();
  m = s_max[0];
  mj = s_arg[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w)
    if (s_max[w] > m || (s_max[w] == m && s_arg[w] < mj)) {
      m = s_max[w];
      mj = s_arg[w];
    }
  float d[LP_PER], part = 0.f;
#pragma unroll
  for (int i = 0; i < LP_PER; ++i) {
    d[i] = x[i] - m;
    if (tid + LP_THREADS * i < n_lang) part += expf(d[i]);
  }
  part = wave_sum(part);
  if (lane == 0) s_sum[wave] = part;
  __syncthreads();
  float total = s_sum[0];
#pragma unroll
  for (int w = 1; w < LP_WAVES; ++w) total += s_sum[w];
  const float lg = logf(total);
#pragma unroll
  for (int i = 0; i < LP_PER; ++i) {
    const int j = tid + LP_THREADS * i;
    if (j < n_lang) probs[b * ld_probs + j] = expf(d[i] - lg);
  }
  if (tid == 0) best[b] = min(max(lang_ids[mj < n_lang ? mj : 0], 0), V - 1);  // (no finite language logit at all: the first id)
}

extern "C" int wft_lang_probs(const wft_bf16* logits, int64_t ld, int64_t V, const int32_t* lang_ids, int n_lang, float* probs,
                              int64_t ld_probs, int64_t* best, int B, void* stream) {
  WFT_CHECK_ARG(logits && lang_ids && probs && best, "null pointer");
  WFT_CHECK_ARG(B >= 1 && V >= 1 && V <= INT_MAX && ld >= V, "bad shape (ld must be >= V)");
  WFT_CHECK_ARG(n_lang >= 1 && n_lang <= LP_MAX_LANG, "n_lang must lie in 1..1024");
  WFT_CHECK_ARG(ld_probs >= n_lang, "ld_probs below n_lang");
  hipLaunchKernelGGL(lang_probs_kernel, dim3(B), dim3(LP_THREADS), 0, (hipStream_t)stream, (const unsigned short*)logits, (long)ld, (int)V,
                     lang_ids, n_lang, probs, (long)ld_probs, (long*)best);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- b. windows of the long log-mels
// One workgroup = 1024 output frames of one (row, mel bin); a thread writes four frames with one 16-byte store (out rows are 16-byte
// aligned: n_win % 4 == 0).  The source start mel_off + m * ld + seek has any alignment, the same one for the whole workgroup: k =
// its element address mod 4.  A thread loads the aligned 16-byte chunk that holds its first frame and, for k != 0, the one behind it,
// and takes its four frames out of the eight (a switch on the uniform k: no dynamic register indexing).  Neighbouring lanes read
// neighbouring chunks, so the loads are as coalesced as the stores; the second chunk of a lane is the first of the next one and
// comes from the cache, HBM sees every byte once.  A chunk that crosses either end of its recording is read element by element,
// the elements outside as 0 — nothing outside [mel_off, mel_off + n_mels * ld) is ever addressed.  Frames at or beyond
// min(n_win, content_frames - seek) are written as 0.0f whatever the source holds there (a select, no arithmetic).
#define MW_THREADS 256

__device__ __forceinline__ f32x4 mw_load4(const float* rec, long c, long n_rec) {
  if (c >= 0 && c + 4 <= n_rec) return *(const f32x4*)(rec + c);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (c + e >= 0 && c + e < n_rec) ? rec[c + e] : 0.f;
  return v;
}

__global__ __launch_bounds__(MW_THREADS) void mel_windows_kernel(const float* mel, const long* mel_off, const int* ld_frames,
                                                                 const int* content_frames, const int* audio, const int* seek, float* out,
                                                                 int A, int n_mels, int n_win) {
  const int row = blockIdx.x, r = row / n_mels, m = row - r * n_mels;
  const int v = blockIdx.y * MW_THREADS + threadIdx.x;
  if (v >= n_win / 4) return;
  const int a = min(max(audio[r], 0), A - 1);
  const int ld = max(ld_frames[a], 0);
  const int cf = min(max(content_frames[a], 0), ld);
  const int sk = min(max(seek[r], 0), cf);
  const int t0 = 4 * v;
  const int n = min(n_win, cf - sk) - t0;  // this thread's frames that hold audio (<= 0: none, >= 4: all)
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (n > 0) {
    const long off = mel_off[a], n_rec = (long)n_mels * ld;
    const float* rec = mel + off;
    const long s = (long)m * ld + sk + t0;  // the first frame, as an element of the recording
    const int k = (int)((off + s) & 3);
    const f32x4 lo = mw_load4(rec, s - k, n_rec);
    if (k == 0) {
      o = lo;
    } else {
      const f32x4 hi = mw_load4(rec, s - k + 4, n_rec);
      switch (k) {
        case 1: o = f32x4{lo[1], lo[2], lo[3], hi[0]}; break;
        case 2: o = f32x4{lo[2], lo[3], hi[0], hi[1]}; break;
        default: o = f32x4{lo[3], hi[0], hi[1], hi[2]}; break;
      }
    }
#pragma unroll
    for (int e = 1; e < 4; ++e) o[e] = e < n ? o[e] : 0.f;
  }
  *(f32x4*)(out + ((long)row * n_win + t0)) = o;
}

extern "C" int wft_mel_windows(const float* mel, const int64_t* mel_off, const int32_t* ld_frames, const int32_t* content_frames,
                               const int32_t* audio, const int32_t* seek, float* out, int R, int A, int n_mels, int n_win, void* stream) {
  WFT_CHECK_ARG(mel && mel_off && ld_frames && content_frames && audio && seek && out, "null pointer");
  WFT_CHECK_ARG(R >= 1 && A >= 1 && n_mels >= 1 && (int64_t)R * n_mels <= INT_MAX, "bad shape");
  WFT_CHECK_ARG(n_win >= 4 && n_win % 4 == 0, "n_win must be a positive multiple of 4 (16-byte output rows)");
  WFT_CHECK_ARG(((uintptr_t)mel | (uintptr_t)out) % 16 == 0, "mel and out must be 16-byte aligned");
  const dim3 grid(R * n_mels, (n_win / 4 + MW_THREADS - 1) / MW_THREADS);
  hipLaunchKernelGGL(mel_windows_kernel, grid, dim3(MW_THREADS), 0, (hipStream_t)stream, mel, (const long*)mel_off, ld_frames, content_frames,
                     audio, seek, out, A, n_mels, n_win);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
