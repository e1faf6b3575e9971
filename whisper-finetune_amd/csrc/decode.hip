// decode.hip — the single-token kernels of KV-cached greedy decoding (include/wft.h "Greedy decoding").
//
// A cached decoding step runs ONE query row per (sequence, head) against a key/value cache that grows by one row per step.  Nothing
// here depends on the step: the position of every sequence lives in device memory (`len`), so a step is a fixed launch sequence.
//
//  attn_decode_kernel / attn_decode_merge_kernel   softmax(q K^T) V for one query row, HBM-bound K/V read
//  decode_embed_kernel                             token + positional embedding at the device-side position
//  decode_pick_kernel / decode_count_kernel        suppress, arg-max, log-probability, state update, unfinished-row count
#include "common.h"

// ----------------------------------------------------------------------------- single-token attention
// Work split.  A key row of one head is 64 bf16 = 128 bytes = 8 lanes x 16 bytes, so a wave reads 8 keys per load instruction: lane l
// holds dims 8(l & 7) .. +7 of key sub-index l >> 3.  Every group of 8 lanes runs its OWN online softmax (m, l, o[8 dims per lane]) over
// the keys it sees, so the loop needs only the 3-step butterfly inside the group that completes the dot product; the 8 groups of a
// wave, the 4 waves of a workgroup and the `nsplit` workgroups of a (sequence, head) are merged once at the end, each level in a fixed
// order (no atomics: reruns are bit-identical).  K and V go straight from global memory to VGPRs in 16-byte loads, two blocks of 4 keys
// per lane in flight for each (the data is used once; an LDS round trip would only add latency).
// Keys are dealt in blocks of 32 (8 groups x 4 in flight) round-robin over (split, wave): block j belongs to wave j % 4 of split
// (j / 4) % nsplit — ragged lengths balance themselves and a split whose first block lies beyond the row's length writes an empty partial.
// Measured choices (tools/dev/decode_bench.py): 4 waves per workgroup (8: -1 to -12 %); ONE launch wherever B * H
// workgroups cover the chip's 256 CUs, and never a split of fewer than 512 keys — the second launch costs more than a short split
// saves (a 448-key self-attention cache is never split; 1 500 cross-attention keys are cut in at most 3).
#define DEC_WAVES 4
#define DEC_TARGET_WGS 256
#define DEC_MIN_SPLIT_KEYS 512
#define DEC_BLOCK_KEYS 32
#define DEC_PART 66  // floats per partial: m, l, o[64]
#define DEC_NEG (-1.0e30f)

struct dec_state {
  float m, l;
  float o[8];
};

__device__ __forceinline__ void dec_merge(dec_state& a, float bm, float bl, const float* bo) {
  const float M = fmaxf(a.m, bm);
  const float wa = __builtin_amdgcn_exp2f(a.m - M), wb = __builtin_amdgcn_exp2f(bm - M);
  a.l = a.l * wa + bl * wb;
#pragma unroll
  for (int i = 0; i < 8; ++i) a.o[i] = a.o[i] * wa + bo[i] * wb;
  a.m = M;
}

__device__ __forceinline__ void dec_unpack8(const u32x4 r, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __builtin_bit_cast(float, r[i] << 16);
    f[2 * i + 1] = __builtin_bit_cast(float, r[i] & 0xffff0000u);
  }
}

__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kernel(wft_attn_decode_args a, int nsplit, float qk_alpha) {
  __shared__ float red[DEC_WAVES][DEC_PART];
  const int bh = blockIdx.x, sp = blockIdx.y;
  const int b = bh / a.H, h = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 3, c = lane & 7;

  int n = a.Tk;          // keys this row attends over
  int p_new = -1;        // self form: the position whose k / v are this step's rows
  if (a.len) {
    n = a.len[b];
    n = n < 1 ? 1 : (n > a.Tk ? a.Tk : n);
    p_new = n - 1;
  }
  const unsigned short* kc = a.k_cache + (long)b * a.cache_bs + h * 64 + c * 8;
  const unsigned short* vc = a.v_cache + (long)b * a.cache_bs + h * 64 + c * 8;
  const unsigned short* kn = a.len ? a.k_new + (long)b * a.ld_new + h * 64 + c * 8 : kc;
  const unsigned short* vn = a.len ? a.v_new + (long)b * a.ld_new + h * 64 + c * 8 : vc;

  if (a.len && sp == 0 && wave == 0 && lane < 16) {
    // the append: this step's k row (lanes 0-7) and v row (lanes 8-15) into the cache.  No lane of this launch READS cache row
    // p_new (the lane that owns key p_new takes it from k_new / v_new below), so there is nothing to order.
    const u32x4 r = *(const u32x4*)(g == 0 ? kn : vn);
    unsigned short* dst = (g == 0 ? a.k_cache : a.v_cache) + (long)b * a.cache_bs + (long)p_new * a.ld_cache + h * 64 + c * 8;
    *(u32x4*)dst = r;
  }

  float q[8];
  dec_unpack8(*(const u32x4*)(a.q + (long)b * a.ldq + h * 64 + c * 8), q);

  dec_state st;
  st.m = DEC_NEG;
  st.l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) st.o[i] = 0.f;

  // One block of 32 keys: 4 K and 4 V loads of 16 bytes per lane.  The loads of the NEXT block are issued before the current one is
  // used (two named register sets, no branch around a load: a block index beyond the row's end reads the clamped last key and is
  // never used), so a wave keeps 16 KiB in flight.
  auto load = [&](int blk, u32x4* kr, u32x4* vr) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int t = blk * DEC_BLOCK_KEYS + g + u * 8;
      t = t < n ? t : n - 1;  // (a clamped, in-bounds address; the value is discarded)
      const bool fresh = t == p_new;
      kr[u] = *(const u32x4*)(fresh ? kn : kc + (long)t * a.ld_cache);
      vr[u] = *(const u32x4*)(fresh ? vn : vc + (long)t * a.ld_cache);
    }
  };
  auto consume = [&](int blk, const u32x4* kr, const u32x4* vr) {
    float s[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ok[u] = blk * DEC_BLOCK_KEYS + g + u * 8 < n;
      float kf[8];
      dec_unpack8(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d = fmaf(q[i], kf[i], d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      s[u] = ok[u] ? d * qk_alpha : DEC_NEG;
    }
    const float mn = fmaxf(fmaxf(st.m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
    const float resc = __builtin_amdgcn_exp2f(st.m - mn);
    st.m = mn;
    st.l *= resc;
#pragma unroll
    for (int i = 0; i < 8; ++i) st.o[i] *= resc;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
      float vf[8];
      dec_unpack8(vr[u], vf);
      st.l += p;
#pragma unroll
      for (int i = 0; i < 8; ++i) st.o[i] = fmaf(p, vf[i], st.o[i]);
    }
  };
  const int stride = nsplit * DEC_WAVES;
  int blk = sp * DEC_WAVES + wave;
  u32x4 kA[4], vA[4], kB[4], vB[4];
  load(blk, kA, vA);
  while (blk * DEC_BLOCK_KEYS < n) {
    load(blk + stride, kB, vB);
    consume(blk, kA, vA);
    blk += stride;
    if (!(blk * DEC_BLOCK_KEYS < n)) break;
    load(blk + stride, kA, vA);
    consume(blk, kB, vB);
    blk += stride;
  }

  // the 8 key groups of the wave (butterfly over lane bits 3..5; group 0's copy is the one used)
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    const float bm = __shfl_xor(st.m, off, 64), bl = __shfl_xor(st.l, off, 64);
    float bo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bo[i] = __shfl_xor(st.o[i], off, 64);
    dec_merge(st, bm, bl, bo);
  }
  if (g == 0) {
    if (c == 0) {
      red[wave][0] = st.m;
      red[wave][1] = st.l;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave][2 + c * 8 + i] = st.o[i];
  }
  __syncthreads();
  if (wave == 0 && g == 0) {
    // the 4 waves, in wave order
    for (int w = 1; w < DEC_WAVES; ++w) {
      float bo[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) bo[i] = red[w][2 + c * 8 + i];
      dec_merge(st, red[w][0], red[w][1], bo);
    }
    if (nsplit == 1) {
      const float inv = 1.0f / st.l;  // (n >= 1: at least one key)
      u32x4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = pack2bf(st.o[2 * i] * inv, st.o[2 * i + 1] * inv);
      *(u32x4*)(a.o + (long)b * a.ldo + h * 64 + c * 8) = r;
    } else {
      float* part = (float*)a.workspace + ((long)bh * nsplit + sp) * DEC_PART;
      if (c == 0) {
        part[0] = st.m;
        part[1] = st.l;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) part[2 + c * 8 + i] = st.o[i];
    }
  }
}

// the `nsplit` partials of one (sequence, head), in split order: one wave, one lane per output dim
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(const float* ws, int nsplit, unsigned short* o, long ldo, int H) {
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, i = threadIdx.x;
  const float* part = ws + (long)bh * nsplit * DEC_PART;
  float m = part[0], l = part[1], acc = part[2 + i];
  for (int s = 1; s < nsplit; ++s) {
    const float* q = part + (long)s * DEC_PART;
    const float M = fmaxf(m, q[0]);
    const float wa = __builtin_amdgcn_exp2f(m - M), wb = __builtin_amdgcn_exp2f(q[0] - M);
    l = l * wa + q[1] * wb;
    acc = acc * wa + q[2 + i] * wb;
    m = M;
  }
  o[(long)b * ldo + h * 64 + i] = f2bf(acc / l);
}

static int dec_nsplit(const wft_attn_decode_args* a) {
  // enough workgroups to cover the chip when B * H alone does not, in splits of about DEC_MIN_SPLIT_KEYS keys or more
  const long bh = (long)a->B * a->H;
  long want = (DEC_TARGET_WGS + bh - 1) / bh;
  const long most = (a->Tk + DEC_MIN_SPLIT_KEYS - 1) / DEC_MIN_SPLIT_KEYS;
  if (want > most) want = most;
  if (want > 16) want = 16;
  return want < 1 ? 1 : (int)want;
}

extern "C" int64_t wft_attn_decode_workspace_bytes(const wft_attn_decode_args* a) {
  if (!a || a->B < 1 || a->H < 1 || a->Tk < 1) return 0;
  const int ns = dec_nsplit(a);
  return ns == 1 ? 0 : (int64_t)a->B * a->H * ns * DEC_PART * (int64_t)sizeof(float);
}

extern "C" int wft_attn_decode_bf16(const wft_attn_decode_args* a, void* stream) {
  WFT_CHECK_ARG(a && a->q && a->k_cache && a->v_cache && a->o, "null pointer");
  WFT_CHECK_ARG(a->B >= 1 && a->H >= 1 && a->Tk >= 1 && (long)a->B * a->H <= 0x7fffffffL, "bad shape");
  const long d = (long)a->H * 64;
  WFT_CHECK_ARG(a->ldq >= d && a->ldo >= d && a->ld_cache >= d, "leading dimensions must cover H * 64 = d");
  WFT_CHECK_ARG(a->ldq % 8 == 0 && a->ldo % 8 == 0 && a->ld_cache % 8 == 0 && a->cache_bs % 8 == 0, "ld / batch strides must be multiples of 8");
  WFT_CHECK_ARG(a->cache_bs >= (int64_t)(a->Tk - 1) * a->ld_cache + d, "cache capacity: a sequence's Tk rows must fit its batch stride");
  WFT_CHECK_ARG(((((uintptr_t)a->q) | ((uintptr_t)a->k_cache) | ((uintptr_t)a->v_cache) | ((uintptr_t)a->o)) & 15) == 0, "16-byte alignment");
  if (a->len) {
    WFT_CHECK_ARG(a->k_new && a->v_new, "self-attention form (len given) needs the step's k / v rows");
    WFT_CHECK_ARG(a->ld_new >= d && a->ld_new % 8 == 0 && ((((uintptr_t)a->k_new) | ((uintptr_t)a->v_new)) & 15) == 0, "k_new / v_new layout");
  }
  WFT_CHECK_ARG(a->scale > 0.f, "scale");
  const int ns = dec_nsplit(a);
  if (ns > 1)
    WFT_CHECK_ARG(a->workspace && a->workspace_bytes >= wft_attn_decode_workspace_bytes(a) && (((uintptr_t)a->workspace) & 15) == 0,
                  "workspace of wft_attn_decode_workspace_bytes(args) bytes");
  const float alpha = a->q_prescaled ? 1.0f : a->scale * 1.4426950408889634f;
  hipLaunchKernelGGL(attn_decode_kernel, dim3((unsigned)(a->B * a->H), (unsigned)ns), dim3(DEC_WAVES * 64), 0, (hipStream_t)stream, *a, ns, alpha);
  if (ns > 1)
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3((unsigned)(a->B * a->H)), dim3(64), 0, (hipStream_t)stream, (const float*)a->workspace,
                       ns, a->o, (long)a->ldo, a->H);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- embedding at the device-side position
// out[b] = emb[tokens[b, len[b] - 1]] + pos[len[b] - 1]: the arithmetic of embed_fwd_kernel (misc.hip), one fp32 add and one rounding.
__global__ __launch_bounds__(256) void decode_embed_kernel(const long* tokens, long ld_tokens, const int* len, const float* emb,
                                                            const float* pos, unsigned short* out, int B, int n_ctx, int d, long V) {
  const int dv = d >> 3;
  const long total = (long)B * dv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / dv);
    const int c = (int)(i - (long)b * dv) * 8;
    int p = len[b] - 1;
    p = p < 0 ? 0 : (p >= n_ctx ? n_ctx - 1 : p);
    long tok = tokens[(long)b * ld_tokens + p];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    const float* e = emb + tok * d + c;
    const float* pp = pos + (long)p * d + c;
    const f32x4 a0 = *(const f32x4*)e, a1 = *(const f32x4*)(e + 4);
    const f32x4 b0 = *(const f32x4*)pp, b1 = *(const f32x4*)(pp + 4);
    u32x4 o = {pack2bf(a0[0] + b0[0], a0[1] + b0[1]), pack2bf(a0[2] + b0[2], a0[3] + b0[3]),
               pack2bf(a1[0] + b1[0], a1[1] + b1[1]), pack2bf(a1[2] + b1[2], a1[3] + b1[3])};
    *(u32x4*)(out + (long)b * d + c) = o;
  }
}

extern "C" int wft_decode_embed(const int64_t* tokens, int64_t ld_tokens, const int32_t* len, const float* emb, const float* pos,
                                wft_bf16* out, int B, int n_ctx, int d, int64_t V, void* stream) {
  WFT_CHECK_ARG(tokens && len && emb && pos && out, "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_ctx >= 1 && ld_tokens >= n_ctx && d >= 8 && d % 8 == 0 && V >= 1, "bad shape");
  WFT_CHECK_ARG(((((uintptr_t)emb) | ((uintptr_t)pos) | ((uintptr_t)out)) & 15) == 0, "16-byte alignment");
  const long total = (long)B * (d / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
  hipLaunchKernelGGL(decode_embed_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const long*)tokens, (long)ld_tokens, len, emb, pos,
                     out, B, n_ctx, d, (long)V);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- greedy pick
// One workgroup per sequence.  Pass 1: maximum of the un-suppressed logits with its LOWEST index (each thread scans its columns in
// ascending order with a strict compare; the tree compares (value, index) pairs).  Pass 2 (the row is L2-resident): sum of
// exp(x - max) over the same columns, so log p(pick) = -log(sum).  Thread 0 then advances the row's state unless it is finished.
#define PICK_THREADS 256

__device__ __forceinline__ bool pick_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ __launch_bounds__(PICK_THREADS) void decode_pick_kernel(wft_decode_pick_args a) {
  __shared__ float s_v[PICK_THREADS / 64];
  __shared__ int s_i[PICK_THREADS / 64];
  __shared__ float s_sum[PICK_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned short* row = a.logits + (long)b * a.ld;
  const int V = (int)a.V;
  const int L = a.len[b];
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && L == a.first_len[b]) ? a.suppress_first : nullptr;

  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c0 = tid * 8; c0 < V; c0 += PICK_THREADS * 8) {
    float f[8];
    dec_unpack8(*(const u32x4*)(row + c0), f);  // (ld % 8 == 0 and ld >= V rounded up to 8: in bounds)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c0 + j;
      const bool live = col < V && !(m1 && m1[col]) && !(m2 && m2[col]);
      if (live && f[j] > best) {
        best = f[j];
        bi = col;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (pick_better(ov, oi, best, bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    s_v[wave] = best;
    s_i[wave] = bi;
  }
  __syncthreads();
  best = s_v[0];
  bi = s_i[0];
  for (int w = 1; w < PICK_THREADS / 64; ++w)
    if (pick_better(s_v[w], s_i[w], best, bi)) {
      best = s_v[w];
      bi = s_i[w];
    }
  const bool any = bi != 0x7fffffff;

  float sum = 0.f;
  if (any) {
    for (int c0 = tid * 8; c0 < V; c0 += PICK_THREADS * 8) {
      float f[8];
      dec_unpack8(*(const u32x4*)(row + c0), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = c0 + j;
        const bool live = col < V && !(m1 && m1[col]) && !(m2 && m2[col]);
        sum += live ? __expf(f[j] - best) : 0.f;
      }
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = s_sum[0];
    for (int w = 1; w < PICK_THREADS / 64; ++w) tot += s_sum[w];
    const long pick = any ? bi : a.eot;  // (every column suppressed: the row ends)
    const float lp = any ? -__logf(tot) : 0.f;
    if (a.pick_out) a.pick_out[b] = pick;
    if (a.logprob_out) a.logprob_out[b] = lp;
    if (!a.finished[b]) {  // a finished row is frozen
      if (L >= 0 && L < a.max_len) {
        a.tokens[(long)b * a.ld_tokens + L] = pick;
        a.sum_logprob[b] += lp;
        a.len[b] = L + 1;
      }
      a.finished[b] = (pick == a.eot || L + 1 >= a.max_len) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void decode_count_kernel(const int* finished, int B, int* unfinished) {
  __shared__ int s[4];
  int n = 0;
  for (int i = threadIdx.x; i < B; i += 256) n += finished[i] ? 0 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) unfinished[0] = s[0] + s[1] + s[2] + s[3];
}

extern "C" int wft_decode_pick(const wft_decode_pick_args* a, void* stream) {
  WFT_CHECK_ARG(a && a->logits && a->tokens && a->len && a->finished && a->sum_logprob && a->unfinished, "null pointer");
  WFT_CHECK_ARG(a->B >= 1 && a->V >= 1 && a->V <= 0x7ffffff0L, "bad shape");
  WFT_CHECK_ARG(a->ld % 8 == 0 && a->ld >= (a->V + 7) / 8 * 8 && (((uintptr_t)a->logits) & 15) == 0, "logits rows: 16-byte aligned, ld >= V rounded up to 8");
  WFT_CHECK_ARG(a->max_len >= 1 && a->max_len <= a->ld_tokens, "max_len must fit the token buffer");
  WFT_CHECK_ARG(a->eot >= 0 && a->eot < a->V, "eot outside the vocabulary");
  WFT_CHECK_ARG(!a->suppress_first || a->first_len, "suppress_first needs first_len");
  hipLaunchKernelGGL(decode_pick_kernel, dim3((unsigned)a->B), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->finished, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
