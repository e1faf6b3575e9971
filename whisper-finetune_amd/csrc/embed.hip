// embed.hip — token embedding: out = bf16(emb[token] + pos[position]) forward (one fp32 add, one rounding; decode_embed_kernel
// in decode_pick.hip repeats this arithmetic), and the backward into the fp32 gradients of both tables.
//
// HBM-bound.  The backward uses no atomics: a token id usually occurs at several positions, and every table row is added in
// position order by the one workgroup that owns it (bitwise reproducible).
#include "common.h"

// ----------------------------------------------------------------------------- embedding
__global__ __launch_bounds__(256) void embed_fwd_kernel(const long* tokens, const float* emb, const float* pos,
                                                         unsigned short* out, long n_tok, long S, int d, long V) {
  const int dv = d >> 3;
  const long total = n_tok * dv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long t = i / dv;
    const int c = (int)(i - t * dv) * 8;
    long tok = tokens[t];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    const float* e = emb + tok * d + c;
    const float* pp = pos + (t % S) * d + c;
    const f32x4 a0 = *(const f32x4*)e, a1 = *(const f32x4*)(e + 4);
    const f32x4 b0 = *(const f32x4*)pp, b1 = *(const f32x4*)(pp + 4);
    u32x4 o = {pack2bf(a0[0] + b0[0], a0[1] + b0[1]), pack2bf(a0[2] + b0[2], a0[3] + b0[3]),
               pack2bf(a1[0] + b1[0], a1[1] + b1[1]), pack2bf(a1[2] + b1[2], a1[3] + b1[3])};
    *(u32x4*)(out + t * d + c) = o;
  }
}
extern "C" int wft_embed_fwd(const int64_t* tokens, const float* emb, const float* pos, wft_bf16* out, int64_t B,
                             int64_t S, int d, int64_t V, void* stream) {
  WFT_CHECK_ARG(tokens && emb && pos && out, "null pointer");
  WFT_CHECK_ARG(B >= 1 && S >= 1 && d >= 8 && d % 8 == 0 && V >= 1, "bad shape");
  const long total = B * S * (d / 8);
  hipLaunchKernelGGL(embed_fwd_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, (const long*)tokens, emb,
                     pos, out, (long)(B * S), (long)S, d, (long)V);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// demb[tok] += dout[position] for every position holding `tok`, WITHOUT atomics (a token id usually occurs at several
// positions — the special tokens at every clip's start — and fp32 atomics would add them in a run-dependent order): a
// workgroup owns 16 consecutive vocabulary rows, scans the token list in chunks of 256 and adds the positions that fall
// into its rows in position order (read-modify-write of rows nobody else touches).  ~V/16 blocks x n_tok/256 chunk scans of
// an L2-resident list.
__global__ __launch_bounds__(256) void embed_bwd_tok_kernel(const long* tokens, const unsigned short* dout, float* demb,
                                                             long n_tok, int d, long V) {
  __shared__ int hit[256];
  const long row0 = (long)blockIdx.x * 16;
  for (long base = 0; base < n_tok; base += 256) {
    const long j = base + threadIdx.x;
    const long tok = j < n_tok ? tokens[j] : -1;
    const bool mine = tok >= row0 && tok < row0 + 16 && tok < V;
    if (!__syncthreads_or(mine)) continue;  // block-uniform
    hit[threadIdx.x] = mine ? (int)(tok - row0) : -1;
    __syncthreads();
    for (int t = 0; t < 256; ++t) {
      const int r = hit[t];  // LDS broadcast: uniform
      if (r < 0) continue;
      const unsigned short* src = dout + (base + t) * d;
      float* dst = demb + (row0 + r) * d;
      for (int c = threadIdx.x; c < d; c += 256) dst[c] += bf2f(src[c]);
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void embed_bwd_pos_kernel(const unsigned short* dout, float* dpos, long B, long S, int d) {
  const long total = S * d;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    float s = 0.f;
    for (long b = 0; b < B; ++b) s += bf2f(dout[b * S * d + i]);
    dpos[i] += s;
  }
}
extern "C" int wft_embed_bwd(const int64_t* tokens, const wft_bf16* dout, float* demb, float* dpos, int64_t B, int64_t S,
                             int d, int64_t V, void* stream) {
  WFT_CHECK_ARG(tokens && dout && demb && dpos, "null pointer");
  WFT_CHECK_ARG(B >= 1 && S >= 1 && d >= 1 && V >= 1, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(embed_bwd_tok_kernel, dim3((unsigned)((V + 15) / 16)), dim3(256), 0, s, (const long*)tokens, dout, demb,
                     (long)(B * S), d, (long)V);
  hipLaunchKernelGGL(embed_bwd_pos_kernel, dim3(ew_grid(S * d)), dim3(256), 0, s, dout, dpos, (long)B, (long)S, d);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
