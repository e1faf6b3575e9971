// pcm.hip — file bytes to mono f32 samples over a ragged batch of recordings (include/wft.h "PCM decode" is the contract).
//
// wft_pcm_decode_f32: one launch, grid (ceil(n_max / PCM_T), B), one workgroup per tile of PCM_T output frames of one row.  A row's
// bytes start at ANY byte offset and a frame is 1 .. 64 bytes (3- and 9-byte frames included), so no thread loads its frame from
// global memory: the workgroup stages the 16-byte granules that cover its frames into LDS with aligned dwordx4 loads (at most
// PCM_STAGE bytes of frames per pass, so a tile of wide frames takes several passes), and every thread then assembles its samples
// from two or three LDS words with a byte shift.  A granule is loaded only if it holds a byte of the pass's frames, and those lie
// inside [raw, raw + raw_bytes) because the row was checked against raw_bytes first; a row that fails a check decodes as frames = 0.
// The table is device memory, so that check is the kernel's own and is uniform over the workgroup.
// Each channel sample becomes an exact fp64 value, the mean is an fp64 sum in channel order and a true fp64 division, and the one
// rounding is fp64 -> f32.  A side kernel of the loaders: plain C++, nothing hand-scheduled, no fast-math flag on this file.
#include "common.h"

#pragma clang fp contract(off)

#define PCM_T 1024                         // output frames per workgroup
#define PCM_THREADS 256
#define PCM_STAGE 16384                    // bytes of frames staged per pass (>= 64 * PCM_THREADS: a pass holds >= 256 frames)
#define PCM_GRAN (PCM_STAGE / 16 + 1)      // granules of a pass: its frames plus a lead of at most 15 bytes
#define PCM_MAX_N (1 << 30)
#define PCM_MAX_CH 8

__device__ __forceinline__ int pcm_sample_bytes(int format) {
  switch (format) {
    case WFT_PCM_U8: case WFT_PCM_ALAW: case WFT_PCM_ULAW: return 1;
    case WFT_PCM_S16LE: return 2;
    case WFT_PCM_S24LE: return 3;
    case WFT_PCM_S32LE: case WFT_PCM_F32LE: return 4;
    case WFT_PCM_F64LE: return 8;
    default: return 0;
  }
}

// G.711, expanded to the 16-bit integer in integer arithmetic (the CCITT reference expansion, as Python's audioop has it)
__device__ __forceinline__ int pcm_ulaw(unsigned u) {
  u = ~u & 0xffu;
  const int t = ((int)((u & 0x0fu) << 3) + 0x84) << ((u & 0x70u) >> 4);
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ int pcm_alaw(unsigned a) {
  a = (a ^ 0x55u) & 0xffu;
  const int seg = (int)((a & 0x70u) >> 4);
  int t = (int)((a & 0x0fu) << 4);
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
  return (a & 0x80u) ? t : -t;
}

// the little-endian bytes [o, o + 8) of the staged span (only the sample's own bytes are used by the caller)
__device__ __forceinline__ unsigned long long pcm_lds_bytes(const unsigned* w, int o, bool wide) {
  const int i = o >> 2, s = (o & 3) * 8;
  const unsigned w0 = w[i], w1 = w[i + 1];
  const unsigned long long lo = ((unsigned long long)w1 << 32) | w0;
  if (!wide) return lo >> s;
  const unsigned w2 = w[i + 2];
  return s ? (lo >> s) | ((unsigned long long)w2 << (64 - s)) : lo;
}

__device__ __forceinline__ double pcm_value(int format, unsigned long long v) {
  switch (format) {
    case WFT_PCM_U8: return (double)((int)(v & 0xffu) - 128) * 0x1p-7;
    case WFT_PCM_S16LE: return (double)(int)(short)(v & 0xffffu) * 0x1p-15;
    case WFT_PCM_S24LE: return (double)((int)((unsigned)v << 8) >> 8) * 0x1p-23;
    case WFT_PCM_S32LE: return (double)(int)(unsigned)v * 0x1p-31;
    case WFT_PCM_F32LE: return (double)__builtin_bit_cast(float, (unsigned)v);
    case WFT_PCM_F64LE: return __builtin_bit_cast(double, v);
    case WFT_PCM_ALAW: return (double)pcm_alaw((unsigned)v) * 0x1p-15;
    default: return (double)pcm_ulaw((unsigned)v) * 0x1p-15;  // WFT_PCM_ULAW: the format was checked
  }
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_decode_kernel(const uint8_t* raw, long long raw_bytes, const wft_pcm_row* rows, float* out,
                                                                 long long ld_out, int n_max) {
  __shared__ uint4 stage[PCM_GRAN + 1];  // one granule more: the word reads behind a pass's last sample stay inside the array
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile0 = blockIdx.x * PCM_T, tile1 = min(tile0 + PCM_T, n_max);
  const wft_pcm_row r = rows[b];
  const int sb = pcm_sample_bytes(r.format);
  const int C = r.channels;
  int frames = r.frames;
  // the clamp: everything below is uniform over the workgroup
  bool ok = sb > 0 && C >= 1 && C <= PCM_MAX_CH && r.channel >= -1 && r.channel < C && frames >= 0 && frames <= n_max && r.byte_off >= 0;
  const int fb = ok ? C * sb : 1;
  if (ok) {
    const long long need = (long long)frames * fb;  // <= 2^36
    ok = need <= raw_bytes && r.byte_off <= raw_bytes - need;
  }
  if (!ok) frames = 0;
  float* orow = out + (long long)b * ld_out;
  const int dec1 = min(tile1, frames);  // frames of this tile that are decoded: [tile0, dec1)
  const int per_pass = min(PCM_STAGE / fb, PCM_T);
  const unsigned* words = reinterpret_cast<const unsigned*>(stage);
  const bool wide = sb == 8;
  const double cd = (double)C;
#pragma unroll 1
  for (int f0 = tile0; f0 < dec1; f0 += per_pass) {
    const int P = min(per_pass, dec1 - f0);
    const uintptr_t first = (uintptr_t)raw + (uintptr_t)r.byte_off + (uintptr_t)((long long)f0 * fb);
    const int lead = (int)(first & 15);
    const uint4* src = reinterpret_cast<const uint4*>(first - lead);
    const int gran = (lead + P * fb + 15) >> 4;  // <= PCM_GRAN; granule g holds a byte of the pass: 16 g < lead + P fb, 16 g + 15 >= lead
    __syncthreads();  // the previous pass has been read
    for (int g = tid; g < gran; g += PCM_THREADS) stage[g] = src[g];
    __syncthreads();
    for (int j = tid; j < P; j += PCM_THREADS) {
      const int o = lead + j * fb;
      double v;
      if (r.channel >= 0) {
        v = pcm_value(r.format, pcm_lds_bytes(words, o + r.channel * sb, wide));
      } else {
        v = pcm_value(r.format, pcm_lds_bytes(words, o, wide));
        for (int c = 1; c < C; ++c) v = v + pcm_value(r.format, pcm_lds_bytes(words, o + c * sb, wide));
        v = v / cd;
      }
      orow[f0 + j] = (float)v;
    }
  }
  for (int j = max(tile0, frames) + tid; j < tile1; j += PCM_THREADS) orow[j] = 0.f;
}

extern "C" int wft_pcm_decode_tile(void) { return PCM_T; }

extern "C" int wft_pcm_decode_f32(const uint8_t* raw, int64_t raw_bytes, const wft_pcm_row* rows, float* out, int64_t ld_out, int64_t n_max,
                                  int B, void* stream) {
  WFT_CHECK_ARG(raw && rows && out, "null pointer");
  WFT_CHECK_ARG(raw_bytes >= 1, "raw_bytes must be at least 1");
  WFT_CHECK_ARG(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= PCM_MAX_N, "bad shape (1 <= n_max <= 2^30, 1 <= B <= 65535)");
  WFT_CHECK_ARG(ld_out >= n_max, "leading dimension smaller than the row");
  WFT_CHECK_ARG((uintptr_t)rows % 8 == 0 && (uintptr_t)out % 4 == 0, "rows must be 8-byte, out 4-byte aligned");
  static_assert(sizeof(wft_pcm_row) == 32, "wft_pcm_row is 32 bytes");
  hipLaunchKernelGGL(pcm_decode_kernel, dim3((unsigned)cdiv64(n_max, PCM_T), (unsigned)B), dim3(PCM_THREADS), 0, (hipStream_t)stream, raw,
                     (long long)raw_bytes, rows, out, (long long)ld_out, (int)n_max);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
