// decode.hip — the single-token kernels of KV-cached greedy and beam-search decoding (include/wft.h "Greedy decoding", "Beam search").
//
// A cached decoding step runs ONE query row per (sequence, head) against a key/value cache that grows by one row per step.  Nothing
// here depends on the step: the position of every sequence lives in device memory (`len`), so a step is a fixed launch sequence.
//
//  attn_decode_kernel / attn_decode_merge_kernel   softmax(q K^T) V for one query row, HBM-bound K/V read
//  attn_decode_beam_kernel<W, SELF>                the same attention for beams: self keys through the ancestry table, cross keys
//                                                  read once per audio for all of its beams.  Kept apart from attn_decode_kernel on
//                                                  purpose (see the note above it); the host side of the two entry points is one.
//  decode_embed_kernel                             token + positional embedding at the device-side position
//  decode_pick_kernel / decode_count_kernel        suppress, arg-max, log-probability, state update, unfinished-row count
//  decode_topk_kernel / beam_update_kernel         the W + 1 best continuations per hypothesis; one beam-search step per audio
//  decode_pick_kernel<true> / decode_topk_kernel<true>   the same two under upstream's timestamp rules (ts_row_rules, ts_decide)
//  decode_sample_kernel<TS>                         the pick with a temperature per row: Gumbel-max over Philox noise (include/wft.h "Sampled decoding")
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

// ----------------------------------------------------------------------------- single-token attention for beams
// attn_decode_kernel's work split, key-to-lane dealing, two-blocks-in-flight loads and merge order, for two new shapes.
//  SELF (W = 1): hypothesis r reads key t at cache slot anc[r, t] — keys are never copied when beams are reordered, only rows of
//    `anc` are.  The 4 slot indices of a block are fetched ONE BLOCK AHEAD of its keys (iA / iB below: when the K / V loads of block
//    j + 1 are issued their indices are already in registers, and the indices of block j + 2 are in flight), so the indirection adds
//    one dependent load at the head of a row and none to the K / V stream.
//  cross (W = group): one workgroup per (audio, head, split) loads each K / V block ONCE and runs the online softmax of the audio's W
//    query rows against it: W states per lane, the arithmetic of one query exactly that of attn_decode_kernel.
// Why this template is not also the greedy kernel.  A three-mode form of it (own slot / ancestry / cross) compiles without scratch, but
// hipcc does not give its W = 1 instantiations attn_decode_kernel's schedule: there the next block's 8 loads are issued before the
// current block is consumed under s_waitcnt vmcnt(14) .. (8); in the template's instantiations they sink below the loop's exit test
// and are waited for at once (vmcnt(6) .. (0)), about one block in flight; dropping the index plumbing outside the ancestry mode
// does not bring it back (checked from the ISA).  Greedy decoding runs every step; it keeps the kernel with the measured schedule.
template <int W, bool SELF>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_beam_kernel(wft_attn_decode_beam_args a, int nsplit, float qk_alpha) {
  __shared__ float red[DEC_WAVES][W][DEC_PART];
  const int ah = blockIdx.x, sp = blockIdx.y;
  const int au = ah / a.H, h = ah - au * a.H;  // au: the slot row (SELF) or the audio
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 3, c = lane & 7;
  const int r0 = au * W;  // first query row

  int n = a.Tk;
  int p_new = -1;
  if (SELF) {
    n = a.len[au];
    n = n < 1 ? 1 : (n > a.Tk ? a.Tk : n);
    p_new = n - 1;
  }
  const long hoff = h * 64 + c * 8;
  const unsigned short* kc = a.k_cache + hoff + (SELF ? 0 : (long)au * a.cache_bs);
  const unsigned short* vc = a.v_cache + hoff + (SELF ? 0 : (long)au * a.cache_bs);
  const unsigned short* kn = SELF ? a.k_new + (long)au * a.ld_new + hoff : kc;
  const unsigned short* vn = SELF ? a.v_new + (long)au * a.ld_new + hoff : vc;
  const int* anc = SELF ? a.anc + (long)au * a.ld_anc : nullptr;

  if (SELF && sp == 0 && wave == 0 && lane < 16) {
    // the append into the row's OWN slot at position p_new.  No lane of this launch reads position p_new of any slot (whoever owns
    // key p_new takes it from k_new / v_new), and no `anc` entry of an earlier position points at it: nothing to order.
    const u32x4 r = *(const u32x4*)(g == 0 ? kn : vn);
    unsigned short* dst = (g == 0 ? a.k_cache : a.v_cache) + (long)au * a.cache_bs + (long)p_new * a.ld_cache + hoff;
    *(u32x4*)dst = r;
  }

  float q[W][8];
#pragma unroll
  for (int j = 0; j < W; ++j) dec_unpack8(*(const u32x4*)(a.q + (long)(r0 + j) * a.ldq + hoff), q[j]);

  dec_state st[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    st[j].m = DEC_NEG;
    st[j].l = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) st[j].o[i] = 0.f;
  }

  auto ldidx = [&](int blk, int* ix) {
    if (SELF) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int t = blk * DEC_BLOCK_KEYS + g + u * 8;
        t = t < n ? t : n - 1;
        int s = au;
        if (t != p_new) s = anc[t];
        ix[u] = (unsigned)s < (unsigned)a.R ? s : au;  // (an in-bounds slot whatever the table holds)
      }
    }
  };
  auto load = [&](int blk, const int* ix, u32x4* kr, u32x4* vr) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int t = blk * DEC_BLOCK_KEYS + g + u * 8;
      t = t < n ? t : n - 1;  // (a clamped, in-bounds address; the value is discarded)
      const bool fresh = t == p_new;
      const long off = (SELF ? (long)ix[u] * a.cache_bs : 0) + (long)t * a.ld_cache;
      kr[u] = *(const u32x4*)(fresh ? kn : kc + off);
      vr[u] = *(const u32x4*)(fresh ? vn : vc + off);
    }
  };
  auto consume = [&](int blk, const u32x4* kr, const u32x4* vr) {
    bool ok[4];
    float kf[4][8], vf[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ok[u] = blk * DEC_BLOCK_KEYS + g + u * 8 < n;
      dec_unpack8(kr[u], kf[u]);
      dec_unpack8(vr[u], vf[u]);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(q[j][i], kf[u][i], d);
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        s[u] = ok[u] ? d * qk_alpha : DEC_NEG;
      }
      const float mn = fmaxf(fmaxf(st[j].m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
      const float resc = __builtin_amdgcn_exp2f(st[j].m - mn);
      st[j].m = mn;
      st[j].l *= resc;
#pragma unroll
      for (int i = 0; i < 8; ++i) st[j].o[i] *= resc;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
        st[j].l += p;
#pragma unroll
        for (int i = 0; i < 8; ++i) st[j].o[i] = fmaf(p, vf[u][i], st[j].o[i]);
      }
    }
  };
  const int stride = nsplit * DEC_WAVES;
  int blk = sp * DEC_WAVES + wave;
  u32x4 kA[4], vA[4], kB[4], vB[4];
  int iA[4] = {0, 0, 0, 0}, iB[4] = {0, 0, 0, 0};
  ldidx(blk, iA);
  ldidx(blk + stride, iB);
  load(blk, iA, kA, vA);
  while (blk * DEC_BLOCK_KEYS < n) {
    ldidx(blk + 2 * stride, iA);
    load(blk + stride, iB, kB, vB);
    consume(blk, kA, vA);
    blk += stride;
    if (!(blk * DEC_BLOCK_KEYS < n)) break;
    ldidx(blk + 2 * stride, iB);
    load(blk + stride, iA, kA, vA);
    consume(blk, kB, vB);
    blk += stride;
  }

#pragma unroll
  for (int j = 0; j < W; ++j) {
    // the 8 key groups of the wave (butterfly over lane bits 3..5; group 0's copy is the one used)
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
      const float bm = __shfl_xor(st[j].m, off, 64), bl = __shfl_xor(st[j].l, off, 64);
      float bo[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) bo[i] = __shfl_xor(st[j].o[i], off, 64);
      dec_merge(st[j], bm, bl, bo);
    }
    if (g == 0) {
      if (c == 0) {
        red[wave][j][0] = st[j].m;
        red[wave][j][1] = st[j].l;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][j][2 + c * 8 + i] = st[j].o[i];
    }
  }
  __syncthreads();
  if (wave == 0 && g == 0) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      // the 4 waves, in wave order
      for (int w = 1; w < DEC_WAVES; ++w) {
        float bo[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) bo[i] = red[w][j][2 + c * 8 + i];
        dec_merge(st[j], red[w][j][0], red[w][j][1], bo);
      }
      const long rh = (long)(r0 + j) * a.H + h;
      if (nsplit == 1) {
        const float inv = 1.0f / st[j].l;
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = pack2bf(st[j].o[2 * i] * inv, st[j].o[2 * i + 1] * inv);
        *(u32x4*)(a.o + (long)(r0 + j) * a.ldo + hoff) = r;
      } else {
        float* part = (float*)a.workspace + (rh * nsplit + sp) * DEC_PART;  // the layout attn_decode_merge_kernel reads, per query row
        if (c == 0) {
          part[0] = st[j].m;
          part[1] = st[j].l;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) part[2 + c * 8 + i] = st[j].o[i];
      }
    }
  }
}

// the `nsplit` partials of one (query row, head), in split order: one wave, one lane per output dim
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

// Host side.  Both entry points work on the beam struct: greedy decoding is its group = 1 case without an ancestry table.
static wft_attn_decode_beam_args dec_from_greedy(const wft_attn_decode_args* a) {
  wft_attn_decode_beam_args b = {};
  b.q = a->q, b.ldq = a->ldq, b.k_new = a->k_new, b.v_new = a->v_new, b.ld_new = a->ld_new;
  b.k_cache = a->k_cache, b.v_cache = a->v_cache, b.ld_cache = a->ld_cache, b.cache_bs = a->cache_bs;
  b.o = a->o, b.ldo = a->ldo, b.len = a->len;
  b.R = a->B, b.H = a->H, b.Tk = a->Tk, b.group = 1, b.scale = a->scale, b.q_prescaled = a->q_prescaled;
  b.workspace = a->workspace, b.workspace_bytes = a->workspace_bytes;
  return b;
}

static int dec_nsplit(const wft_attn_decode_beam_args& a) {
  // enough workgroups to cover the chip when the (sequence, head) or — cross form — (audio, head) pairs alone do not, in splits of
  // about DEC_MIN_SPLIT_KEYS keys or more (the rule stated in wft.h)
  const long bh = (long)(a.len ? a.R : a.R / a.group) * a.H;
  long want = (DEC_TARGET_WGS + bh - 1) / bh;
  const long most = ((long)a.Tk + DEC_MIN_SPLIT_KEYS - 1) / DEC_MIN_SPLIT_KEYS;
  if (want > most) want = most;
  if (want > 16) want = 16;
  return want < 1 ? 1 : (int)want;
}

static int64_t dec_workspace_bytes(const wft_attn_decode_beam_args& a) {
  if (a.R < 1 || a.H < 1 || a.Tk < 1 || a.group < 1 || a.group > 8 || a.R % a.group != 0 || (a.len && a.group != 1)) return 0;
  const int ns = dec_nsplit(a);
  return ns == 1 ? 0 : (int64_t)a.R * a.H * ns * DEC_PART * (int64_t)sizeof(float);
}

// the argument checks of both entry points (`who`: the one that reports); use_anc: the self form reads keys through `anc`
static int dec_check(const wft_attn_decode_beam_args& a, bool use_anc, const char* who) {
  WFT_CHECK_ARG_AS(who, a.q && a.k_cache && a.v_cache && a.o, "null pointer");
  WFT_CHECK_ARG_AS(who, a.R >= 1 && a.H >= 1 && a.Tk >= 1 && (long)a.R * a.H <= 0x7fffffffL, "bad shape");
  WFT_CHECK_ARG_AS(who, a.group >= 1 && a.group <= 8 && a.R % a.group == 0, "group must lie in 1..8 and divide the rows");
  const long d = (long)a.H * 64;
  WFT_CHECK_ARG_AS(who, a.ldq >= d && a.ldo >= d && a.ld_cache >= d, "leading dimensions must cover H * 64 = d");
  WFT_CHECK_ARG_AS(who, a.ldq % 8 == 0 && a.ldo % 8 == 0 && a.ld_cache % 8 == 0 && a.cache_bs % 8 == 0, "ld / batch strides must be multiples of 8");
  WFT_CHECK_ARG_AS(who, a.cache_bs >= (int64_t)(a.Tk - 1) * a.ld_cache + d, "cache capacity: the Tk rows of a sequence or slot must fit its batch stride");
  WFT_CHECK_ARG_AS(who, ((((uintptr_t)a.q) | ((uintptr_t)a.k_cache) | ((uintptr_t)a.v_cache) | ((uintptr_t)a.o)) & 15) == 0, "16-byte alignment");
  if (a.len) {
    WFT_CHECK_ARG_AS(who, a.group == 1, "the self form (len given) takes group = 1");
    WFT_CHECK_ARG_AS(who, !use_anc || (a.anc && a.ld_anc >= a.Tk), "the self form needs the ancestry table, ld_anc >= Tk");
    WFT_CHECK_ARG_AS(who, a.k_new && a.v_new, "self-attention form (len given) needs the step's k / v rows");
    WFT_CHECK_ARG_AS(who, a.ld_new >= d && a.ld_new % 8 == 0 && ((((uintptr_t)a.k_new) | ((uintptr_t)a.v_new)) & 15) == 0, "k_new / v_new layout");
  }
  WFT_CHECK_ARG_AS(who, a.scale > 0.f, "scale");
  if (dec_nsplit(a) > 1)
    WFT_CHECK_ARG_AS(who, a.workspace && a.workspace_bytes >= dec_workspace_bytes(a) && (((uintptr_t)a.workspace) & 15) == 0,
              "workspace of as many bytes as the entry point's _workspace_bytes function returns");
  return WFT_OK;
}

// the main kernel the (checked) arguments select — `greedy`: the caller's own struct when it is wft_attn_decode_bf16 — and the merge
static int dec_launch(const wft_attn_decode_beam_args& a, const wft_attn_decode_args* greedy, hipStream_t s) {
  const int ns = dec_nsplit(a);
  const float alpha = a.q_prescaled ? 1.0f : a.scale * 1.4426950408889634f;
  const dim3 grid((unsigned)((a.R / a.group) * a.H), (unsigned)ns), block(DEC_WAVES * 64);
#define BEAM_LAUNCH(W_, SELF_) hipLaunchKernelGGL((attn_decode_beam_kernel<W_, SELF_>), grid, block, 0, s, a, ns, alpha)
  if (greedy) {
    hipLaunchKernelGGL(attn_decode_kernel, grid, block, 0, s, *greedy, ns, alpha);
  } else if (a.len) {
    BEAM_LAUNCH(1, true);
  } else {
    switch (a.group) {
      case 1: BEAM_LAUNCH(1, false); break;
      case 2: BEAM_LAUNCH(2, false); break;
      case 3: BEAM_LAUNCH(3, false); break;
      case 4: BEAM_LAUNCH(4, false); break;
      case 5: BEAM_LAUNCH(5, false); break;
      case 6: BEAM_LAUNCH(6, false); break;
      case 7: BEAM_LAUNCH(7, false); break;
      default: BEAM_LAUNCH(8, false); break;
    }
  }
#undef BEAM_LAUNCH
  if (ns > 1)
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3((unsigned)(a.R * a.H)), dim3(64), 0, s, (const float*)a.workspace, ns, a.o, (long)a.ldo,
                       a.H);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int64_t wft_attn_decode_workspace_bytes(const wft_attn_decode_args* a) { return a ? dec_workspace_bytes(dec_from_greedy(a)) : 0; }
extern "C" int64_t wft_attn_decode_beam_workspace_bytes(const wft_attn_decode_beam_args* a) { return a ? dec_workspace_bytes(*a) : 0; }

extern "C" int wft_attn_decode_bf16(const wft_attn_decode_args* a, void* stream) {
  WFT_CHECK_ARG(a, "null pointer");
  const wft_attn_decode_beam_args b = dec_from_greedy(a);
  const int rc = dec_check(b, false, __func__);
  return rc != WFT_OK ? rc : dec_launch(b, a, (hipStream_t)stream);
}

extern "C" int wft_attn_decode_beam_bf16(const wft_attn_decode_beam_args* a, void* stream) {
  WFT_CHECK_ARG(a, "null pointer");
  const int rc = dec_check(*a, true, __func__);
  return rc != WFT_OK ? rc : dec_launch(*a, nullptr, (hipStream_t)stream);
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
// The row scan, the arg-best reduce and the sum pass are shared with decode_topk_kernel below.
#define PICK_THREADS 256
#define PICK_WAVES (PICK_THREADS / 64)
#define PICK_NONE 0x7fffffff

__device__ __forceinline__ bool pick_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// f(x, col) for the live columns of a logits row — col < V, live(col), neither mask set — that this thread owns: 16-byte reads,
// ascending columns.  live: the per-row column predicate of the timestamp rules (ts_live below), pick_all where there are none.
struct pick_all {
  __device__ __forceinline__ bool operator()(int) const { return true; }
};

template <typename P, typename F>
__device__ __forceinline__ void pick_scan(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, P live, F f) {
  for (int c0 = threadIdx.x * 8; c0 < V; c0 += PICK_THREADS * 8) {
    float x[8];
    dec_unpack8(*(const u32x4*)(row + c0), x);  // (ld % 8 == 0 and ld >= V rounded up to 8: in bounds)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c0 + j;
      if (col < V && live(col) && !(m1 && m1[col]) && !(m2 && m2[col])) f(x[j], col);
    }
  }
}

// the workgroup's best (value, lowest index) in every thread: the wave butterfly, then the waves in wave order.  s_v / s_i: one
// entry per wave; the caller puts a barrier between two calls.
__device__ __forceinline__ void pick_wg_best(float& best, int& bi, float* s_v, int* s_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (pick_better(ov, oi, best, bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_v[threadIdx.x >> 6] = best;
    s_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  best = s_v[0];
  bi = s_i[0];
  for (int w = 1; w < PICK_WAVES; ++w)
    if (pick_better(s_v[w], s_i[w], best, bi)) {
      best = s_v[w];
      bi = s_i[w];
    }
}

// the workgroup's sum of `sum` in every thread: the wave butterfly, then the waves in wave order.  s_sum: one entry per wave, not
// reused without a barrier in between.
__device__ __forceinline__ float pick_wg_sum(float sum, float* s_sum) {
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  float tot = s_sum[0];
  for (int w = 1; w < PICK_WAVES; ++w) tot += s_sum[w];
  return tot;
}

// sum of exp(x - top) over the live columns of the row (0 when `any` is false), in every thread: per thread in column order, then
// pick_wg_sum
__device__ __forceinline__ float pick_wg_sumexp(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, float top,
                                                bool any, float* s_sum) {
  float sum = 0.f;
  if (any) pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int) { sum += __expf(x - top); });
  return pick_wg_sum(sum, s_sum);
}

// ----------------------------------------------------------------------------- the timestamp rules (include/wft.h "Timestamp rules")
// Upstream's `ApplyTimestampRules`, restated.  Rules 1-4 remove column RANGES that follow from three facts about the row's sampled
// tokens tokens[r, F..L) — the last one, the one before it, the last timestamp among them — so they become four per-row scalars and
// a live column is `col != no_ts && (col < ts_begin ? col >= text_lo : ts_lo <= col <= ts_hi)`:
//   1  no_ts is removed                                                                       (no_ts = -1: nothing)
//   2  last_ts && pen_ts: every timestamp is removed (ts_lo = V); last_ts && !pen_ts: columns 0..eot-1 are (text_lo = eot)
//   3  t = the last sampled timestamp: ts_begin..t-1 are removed, and t itself unless last_ts && !pen_ts  (ts_lo = t or t + 1)
//   4  no sampled token yet: all text is removed (text_lo = ts_begin), and timestamps above ts_begin + max_initial (ts_hi)
// Rule 5 (the probability rule) needs the row's values and lives in the kernels: ts_decide below.
// The facts are read from `tokens` by the workgroup itself — at most n_text_ctx i64 values, one strided read and a max-index
// reduce — so there is no per-row rule state to keep, permute or reset, and nothing on the host depends on the step.
struct ts_row {
  int no_ts, ts_begin, text_lo, ts_lo, ts_hi;
};

__device__ __forceinline__ bool ts_live(const ts_row& t, int col) {
  return col != t.no_ts && (col < t.ts_begin ? col >= t.text_lo : (col >= t.ts_lo && col <= t.ts_hi));
}

// the same ts_row in every thread.  tok: the row's tokens (ld_tokens of them are addressable), F / L: first_len / len of the row;
// s_ts: one entry per wave, used by nothing else.
__device__ __forceinline__ ts_row ts_row_rules(const wft_ts_rules& ru, const long* tok, long ld_tokens, int F, int L, int V, int eot,
                                               int* s_ts) {
  L = (int)min((long)max(L, 0), ld_tokens);
  F = min(max(F, 0), L);
  const int n = L - F;  // sampled tokens
  int idx = -1;         // position of the last sampled timestamp (ascending positions per thread: the last hit is its largest)
  for (int i = F + (int)threadIdx.x; i < L; i += PICK_THREADS)
    if (tok[i] >= ru.ts_begin) idx = i;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) idx = max(idx, __shfl_xor(idx, o, 64));
  if ((threadIdx.x & 63) == 0) s_ts[threadIdx.x >> 6] = idx;
  __syncthreads();
  idx = s_ts[0];
  for (int w = 1; w < PICK_WAVES; ++w) idx = max(idx, s_ts[w]);
  const bool last_ts = n >= 1 && tok[L - 1] >= ru.ts_begin;
  const bool pen_ts = n < 2 || tok[L - 2] >= ru.ts_begin;
  ts_row t;
  t.no_ts = ru.no_timestamps;
  t.ts_begin = ru.ts_begin;
  t.text_lo = 0;
  t.ts_lo = ru.ts_begin;
  t.ts_hi = V - 1;
  if (last_ts && pen_ts) t.ts_lo = V;
  if (last_ts && !pen_ts) t.text_lo = eot;
  if (idx >= 0) {
    const long last = min(tok[idx], (long)V - 1);
    t.ts_lo = max(t.ts_lo, (int)last + ((last_ts && !pen_ts) ? 0 : 1));
  }
  if (n == 0) {
    t.text_lo = ru.ts_begin;
    if (ru.max_initial >= 0) t.ts_hi = (int)min((long)V - 1, (long)ru.ts_begin + ru.max_initial);
  }
  return t;
}

// Rule 5 rides the two passes the kernels make anyway.  Pass 1 keeps TWO arg-best pairs, the best live text column (bt, it) and the
// best live timestamp column (bs, is); pass 2 keeps two sums of exp(x - m), m = max(bt, bs), per thread in column order and reduced
// by pick_wg_sum.  Both log-probabilities share the normaliser, so "logsumexp of the timestamps > the best text log-probability"
// is log(sum_ts) > bt - m (an empty side is -inf: 0 timestamps never win, 0 text columns always lose to a live timestamp).
struct ts_pass {
  float bt, bs, m, st, ss;
  int it, is;
  bool wins;  // the timestamps win: every text column is removed
};

template <typename P>
__device__ __forceinline__ ts_pass ts_decide(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, int ts_begin,
                                             P live, float* s_v, int* s_i, float* s_sum, float* s_sum2) {
  ts_pass p;
  p.bt = p.bs = -INFINITY;
  p.it = p.is = PICK_NONE;
  pick_scan(row, V, m1, m2, live, [&](float x, int col) {
    if (col < ts_begin) {
      if (x > p.bt) {
        p.bt = x;
        p.it = col;
      }
    } else if (x > p.bs) {
      p.bs = x;
      p.is = col;
    }
  });
  pick_wg_best(p.bt, p.it, s_v, s_i);
  __syncthreads();
  pick_wg_best(p.bs, p.is, s_v, s_i);
  p.m = fmaxf(p.bt, p.bs);
  p.st = p.ss = 0.f;
  if (p.it != PICK_NONE || p.is != PICK_NONE) {
    const float m = p.m;
    pick_scan(row, V, m1, m2, live, [&](float x, int col) {
      const float e = __expf(x - m);
      if (col < ts_begin) p.st += e;
      else p.ss += e;
    });
  }
  p.st = pick_wg_sum(p.st, s_sum);
  p.ss = pick_wg_sum(p.ss, s_sum2);
  p.wins = __logf(p.ss) > p.bt - p.m;
  return p;
}

// TS: the timestamp-rule form (wft_decode_pick_ts).  The timestamps win -> the best timestamp column under the normaliser sum_ts;
// otherwise the better of the two pairs (value descending, the lower column on ties) under sum_ts + sum_text.
template <bool TS>
__global__ __launch_bounds__(PICK_THREADS) void decode_pick_kernel(wft_decode_pick_args a, wft_ts_rules ru) {
  __shared__ float s_v[PICK_WAVES];
  __shared__ int s_i[PICK_WAVES];
  __shared__ float s_sum[PICK_WAVES];
  const int b = blockIdx.x;
  const unsigned short* row = a.logits + (long)b * a.ld;
  const int V = (int)a.V;
  const int L = a.len[b];
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && L == a.first_len[b]) ? a.suppress_first : nullptr;

  float best = -INFINITY;
  int bi = PICK_NONE;
  float lp;
  if constexpr (TS) {
    __shared__ int s_ts[PICK_WAVES];
    __shared__ float s_sum2[PICK_WAVES];
    const ts_row t = ts_row_rules(ru, a.tokens + (long)b * a.ld_tokens, a.ld_tokens, a.first_len[b], L, V, a.eot, s_ts);
    const ts_pass p = ts_decide(row, V, m1, m2, t.ts_begin, [&](int col) { return ts_live(t, col); }, s_v, s_i, s_sum, s_sum2);
    const bool ts = p.wins || pick_better(p.bs, p.is, p.bt, p.it);
    best = ts ? p.bs : p.bt;
    bi = ts ? p.is : p.it;
    lp = p.wins ? (p.bs - p.m) - __logf(p.ss) : -__logf(p.st + p.ss);
  } else {
    pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int col) {
      if (x > best) {
        best = x;
        bi = col;
      }
    });
    pick_wg_best(best, bi, s_v, s_i);
    lp = -__logf(pick_wg_sumexp(row, V, m1, m2, best, bi != PICK_NONE, s_sum));
  }
  const bool any = bi != PICK_NONE;
  if (threadIdx.x == 0) {
    const long pick = any ? bi : a.eot;  // (every column suppressed: the row ends)
    if (!any) lp = 0.f;
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

static int pick_check(const wft_decode_pick_args* a, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->logits && a->tokens && a->len && a->finished && a->sum_logprob && a->unfinished, "null pointer");
  WFT_CHECK_ARG_AS(who, a->B >= 1 && a->V >= 1 && a->V <= 0x7ffffff0L, "bad shape");
  WFT_CHECK_ARG_AS(who, a->ld % 8 == 0 && a->ld >= (a->V + 7) / 8 * 8 && (((uintptr_t)a->logits) & 15) == 0, "logits rows: 16-byte aligned, ld >= V rounded up to 8");
  WFT_CHECK_ARG_AS(who, a->max_len >= 1 && a->max_len <= a->ld_tokens, "max_len must fit the token buffer");
  WFT_CHECK_ARG_AS(who, a->eot >= 0 && a->eot < a->V, "eot outside the vocabulary");
  WFT_CHECK_ARG_AS(who, !a->suppress_first || a->first_len, "suppress_first needs first_len");
  return WFT_OK;
}

static int ts_check(const wft_ts_rules* ru, int eot, int64_t V, const char* who) {
  WFT_CHECK_ARG_AS(who, ru, "null pointer");
  WFT_CHECK_ARG_AS(who, ru->ts_begin > eot && ru->ts_begin < V, "ts_begin must lie in (eot, V)");
  WFT_CHECK_ARG_AS(who, ru->no_timestamps >= -1 && ru->no_timestamps < V, "no_timestamps is -1 or a column");
  return WFT_OK;
}

extern "C" int wft_decode_pick(const wft_decode_pick_args* a, void* stream) {
  if (int rc = pick_check(a, __func__)) return rc;
  hipLaunchKernelGGL(decode_pick_kernel<false>, dim3((unsigned)a->B), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, wft_ts_rules{});
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->finished, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_decode_pick_ts(const wft_decode_pick_args* a, const wft_ts_rules* ru, void* stream) {
  if (int rc = pick_check(a, __func__)) return rc;
  if (int rc = ts_check(ru, a->eot, a->V, __func__)) return rc;
  WFT_CHECK_ARG(a->first_len, "the timestamp rules need first_len");
  hipLaunchKernelGGL(decode_pick_kernel<true>, dim3((unsigned)a->B), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, *ru);
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->finished, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- sampled pick (include/wft.h "Sampled decoding")
// decode_pick_kernel with one more question per row: t = temperature[r] > 0 draws the token by the Gumbel-max rule — the arg-max of
// key(col) = x[col] / t + g(col) over the live columns is a draw from softmax(x / t) — and t <= 0 is decode_pick_kernel's own code,
// statement for statement (same scans, same reduction order: same bits).  The noise is a pure function of (seed[r], len[r], col):
// Philox4x32-10 keyed by the seed, counter (col >> 2, len, 0, 0), output word col & 3; one block serves the 4 columns of a lane's
// 16-byte read half, so a lane runs 2 blocks per 8 columns (kept in registers across the calls of pick_scan's f).
struct philox4 {
  unsigned w[4];
};

__host__ __device__ __forceinline__ unsigned philox_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

__host__ __device__ __forceinline__ philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = philox_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = philox_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return philox4{{c0, c1, c2, c3}};
}

// g = -log(-log(v)), v = (2k + 1) * 2^-24 with k the word's top 23 bits: an odd 24-bit integer scaled, exact in fp32 and inside
// (0, 1).  The accurate logf: the winners are the columns with v near 1, where -log(v) ~ 1 - v is tiny and __logf's absolute error
// would be a large relative one.
__device__ __forceinline__ float gumbel_of(unsigned word) {
  const float v = (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;
  return -logf(-logf(v));
}

// the per-row noise source: g(col), one Philox block per 4 columns, the last block kept
struct gumbel_row {
  unsigned k0, k1, pos;
  int blk;
  philox4 cur;
  __device__ __forceinline__ float operator()(int col) {
    if ((col >> 2) != blk) {
      blk = col >> 2;
      cur = philox4x32_10((unsigned)blk, pos, 0u, 0u, k0, k1);
    }
    const int j = col & 3;
    const unsigned w = j == 0 ? cur.w[0] : (j == 1 ? cur.w[1] : (j == 2 ? cur.w[2] : cur.w[3]));
    return gumbel_of(w);
  }
};

// the logit of the workgroup's winning key column `bi` in every thread: the thread that brought (mine_i == bi) publishes the logit
// it carried.  s_x: used by nothing else.
__device__ __forceinline__ float sample_wg_logit(int bi, int mine_i, float mine_x, float* s_x) {
  if (bi != PICK_NONE && mine_i == bi) *s_x = mine_x;
  __syncthreads();
  return bi != PICK_NONE ? *s_x : -INFINITY;
}

// Plain form: the key scan rides the max pass (one HBM read of the row), the sum pass is decode_pick_kernel's.  TS form: ts_decide's
// two passes on the UNTEMPERED row (upstream filters before GreedyDecoder.update divides by the temperature), then — t > 0 only — one
// more scan of the L2-resident row under the final predicate, as decode_topk_kernel<true> does; the log-probability reuses
// ts_decide's maximum and sums.  Either way it is the pick's log-softmax at temperature 1 over the live columns.
template <bool TS>
__global__ __launch_bounds__(PICK_THREADS) void decode_sample_kernel(wft_decode_pick_args a, wft_ts_rules ru, const float* temperature,
                                                                     const unsigned long long* seed, int group) {
  __shared__ float s_v[PICK_WAVES];
  __shared__ int s_i[PICK_WAVES];
  __shared__ float s_sum[PICK_WAVES];
  __shared__ float s_x;
  const int b = blockIdx.x;
  const unsigned short* row = a.logits + (long)(b / group) * a.ld;
  const int V = (int)a.V;
  const int L = a.len[b];
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && L == a.first_len[b]) ? a.suppress_first : nullptr;
  const float temp = temperature[b];
  const bool draw = temp > 0.f;
  const float inv_t = draw ? 1.0f / temp : 0.f;
  const unsigned long long sd = seed[b];
  gumbel_row g = {(unsigned)sd, (unsigned)(sd >> 32), (unsigned)L, -1, {}};

  float best = -INFINITY;
  int bi = PICK_NONE;
  float lp;
  float kbest = -INFINITY, kx = -INFINITY;  // the best key of this thread's columns, its column and its logit
  int ki = PICK_NONE;
  auto key = [&](float x, int col) {
    const float k = x * inv_t + g(col);
    if (k > kbest) {  // (strict, ascending columns: a tie stays with the lower column; a -inf logit never enters)
      kbest = k;
      ki = col;
      kx = x;
    }
  };
  if constexpr (TS) {
    __shared__ int s_ts[PICK_WAVES];
    __shared__ float s_sum2[PICK_WAVES];
    ts_row t = ts_row_rules(ru, a.tokens + (long)b * a.ld_tokens, a.ld_tokens, a.first_len[b], L, V, a.eot, s_ts);
    const ts_pass p = ts_decide(row, V, m1, m2, t.ts_begin, [&](int col) { return ts_live(t, col); }, s_v, s_i, s_sum, s_sum2);
    if (draw) {
      if (p.wins) t.text_lo = t.ts_begin;
      pick_scan(row, V, m1, m2, [&](int col) { return ts_live(t, col); }, key);
      const int mine = ki;
      __syncthreads();
      pick_wg_best(kbest, ki, s_v, s_i);
      bi = ki;
      best = sample_wg_logit(bi, mine, kx, &s_x);
      lp = (best - p.m) - __logf(p.wins ? p.ss : p.st + p.ss);
    } else {
      const bool ts = p.wins || pick_better(p.bs, p.is, p.bt, p.it);
      best = ts ? p.bs : p.bt;
      bi = ts ? p.is : p.it;
      lp = p.wins ? (p.bs - p.m) - __logf(p.ss) : -__logf(p.st + p.ss);
    }
  } else {
    if (draw) {
      pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int col) {
        if (x > best) {
          best = x;
          bi = col;
        }
        key(x, col);
      });
    } else {
      pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int col) {
        if (x > best) {
          best = x;
          bi = col;
        }
      });
    }
    pick_wg_best(best, bi, s_v, s_i);
    if (draw) {
      const int mine = ki;
      __syncthreads();
      pick_wg_best(kbest, ki, s_v, s_i);
      const float x = sample_wg_logit(ki, mine, kx, &s_x);
      const float sum = pick_wg_sumexp(row, V, m1, m2, best, bi != PICK_NONE, s_sum);
      lp = (x - best) - __logf(sum);
      bi = ki;
    } else {
      lp = -__logf(pick_wg_sumexp(row, V, m1, m2, best, bi != PICK_NONE, s_sum));
    }
  }
  const bool any = bi != PICK_NONE;
  if (threadIdx.x == 0) {
    const long pick = any ? bi : a.eot;  // (every column suppressed: the row ends)
    if (!any) lp = 0.f;
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

static int sample_check(const wft_decode_pick_args* a, const wft_sample_rules* s, const char* who) {
  if (int rc = pick_check(a, who)) return rc;
  WFT_CHECK_ARG_AS(who, s && s->temperature && s->seed, "null pointer (temperature / seed)");
  WFT_CHECK_ARG_AS(who, s->group >= 1 && a->B % s->group == 0, "group must be >= 1 and divide the state rows");
  return WFT_OK;
}

extern "C" int wft_decode_sample(const wft_decode_pick_args* a, const wft_sample_rules* s, void* stream) {
  if (int rc = sample_check(a, s, __func__)) return rc;
  hipLaunchKernelGGL(decode_sample_kernel<false>, dim3((unsigned)a->B), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, wft_ts_rules{},
                     s->temperature, (const unsigned long long*)s->seed, s->group);
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->finished, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_decode_sample_ts(const wft_decode_pick_args* a, const wft_sample_rules* s, const wft_ts_rules* ru, void* stream) {
  if (int rc = sample_check(a, s, __func__)) return rc;
  if (int rc = ts_check(ru, a->eot, a->V, __func__)) return rc;
  WFT_CHECK_ARG(a->first_len, "the timestamp rules need first_len");
  hipLaunchKernelGGL(decode_sample_kernel<true>, dim3((unsigned)a->B), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, *ru, s->temperature,
                     (const unsigned long long*)s->seed, s->group);
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->finished, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- the W + 1 best continuations of a row
// One workgroup per logits row, decode_pick_kernel's 16-byte row reads and masks.  Pass 1: every thread keeps the TOPK_MAX best
// (value, column) of ITS columns as a sorted list in registers (columns come in ascending order, so a tie stays behind the lower
// column).  Merge: k rounds, each the workgroup's best list head under (value desc, column asc) — a fixed-order tree, no atomics —
// after which the one thread that owns that column pops it.  Pass 2 (the row is L2-resident): decode_pick_kernel's sum of
// exp(x - max), in its order; log p = (x - max) - log(sum).  A live column whose logit is -inf can never be a candidate.
#define TOPK_MAX 9

// TS: the timestamp-rule form (wft_decode_topk_ts).  Rule 5 decides which columns are live, so it must precede the candidate
// merge: ts_decide's two passes run first (the first one reads HBM, the second the L2-resident row), then the list pass above runs
// unchanged under the FINAL predicate — a third scan, of a row that is still L2-resident — and the log-probabilities reuse
// ts_decide's maximum and sums.  Chosen over two register lists per thread (text / timestamp, merged by rule 5's outcome): the
// list insertion, the merge rounds and the pop stay the code of the plain kernel and 2 x 9 more (value, column) registers are not
// held through the scan.  Neither form has been timed (DESIGN.md §3 "Timestamp rules").
template <bool TS>
__global__ __launch_bounds__(PICK_THREADS) void decode_topk_kernel(wft_decode_topk_args a, wft_ts_rules ru, const long* tokens, long ld_tokens,
                                                                   int eot) {
  __shared__ float s_v[PICK_WAVES];
  __shared__ int s_i[PICK_WAVES];
  __shared__ float s_sum[PICK_WAVES];
  __shared__ float s_wv[TOPK_MAX];
  __shared__ int s_wi[TOPK_MAX];
  const int tid = threadIdx.x;
  const long r = (long)blockIdx.x * a.row_step;
  const unsigned short* row = a.logits + (long)blockIdx.x * a.ld;
  const int V = (int)a.V;
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && a.len && a.len[r] == a.first_len[r]) ? a.suppress_first : nullptr;

  ts_row t = {};
  float top = 0.f, tot = 0.f;
  auto live = [&](int col) {
    if constexpr (TS) return ts_live(t, col);
    else return true;
  };
  if constexpr (TS) {
    __shared__ int s_ts[PICK_WAVES];
    __shared__ float s_sum2[PICK_WAVES];
    t = ts_row_rules(ru, tokens + r * ld_tokens, ld_tokens, a.first_len[r], a.len[r], V, eot, s_ts);
    const ts_pass p = ts_decide(row, V, m1, m2, t.ts_begin, live, s_v, s_i, s_sum, s_sum2);
    if (p.wins) t.text_lo = t.ts_begin;
    top = p.m;
    tot = p.wins ? p.ss : p.st + p.ss;
  }

  float lv[TOPK_MAX];
  int li[TOPK_MAX];
#pragma unroll
  for (int p = 0; p < TOPK_MAX; ++p) {
    lv[p] = -INFINITY;
    li[p] = PICK_NONE;
  }
  pick_scan(row, V, m1, m2, live, [&](float x, int col) {
    if (x > lv[TOPK_MAX - 1]) {
      lv[TOPK_MAX - 1] = x;
      li[TOPK_MAX - 1] = col;
#pragma unroll
      for (int p = TOPK_MAX - 1; p > 0; --p) {
        if (lv[p] > lv[p - 1]) {  // strict: an equal value stays behind the earlier (lower) column
          const float tv = lv[p]; lv[p] = lv[p - 1]; lv[p - 1] = tv;
          const int ti = li[p]; li[p] = li[p - 1]; li[p - 1] = ti;
        }
      }
    }
  });

  for (int rnd = 0; rnd < a.k; ++rnd) {
    float best = lv[0];
    int bi = li[0];
    pick_wg_best(best, bi, s_v, s_i);
    if (bi != PICK_NONE && li[0] == bi) {  // the owner of that column pops it
#pragma unroll
      for (int p = 0; p < TOPK_MAX - 1; ++p) {
        lv[p] = lv[p + 1];
        li[p] = li[p + 1];
      }
      lv[TOPK_MAX - 1] = -INFINITY;
      li[TOPK_MAX - 1] = PICK_NONE;
    }
    if (tid == 0) {
      s_wv[rnd] = best;
      s_wi[rnd] = bi;
    }
    __syncthreads();
  }
  if constexpr (!TS) {
    top = s_wv[0];
    tot = pick_wg_sumexp(row, V, m1, m2, top, s_wi[0] != PICK_NONE, s_sum);
  }
  if (tid < a.k) {
    const bool have = s_wi[tid] != PICK_NONE;
    a.cand_tok[r * a.k + tid] = have ? s_wi[tid] : -1;
    a.cand_logp[r * a.k + tid] = have ? (s_wv[tid] - top) - __logf(tot) : -INFINITY;
  }
}

static int topk_check(const wft_decode_topk_args* a, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->logits && a->cand_tok && a->cand_logp, "null pointer");
  WFT_CHECK_ARG_AS(who, a->rows >= 1 && a->row_step >= 1 && a->V >= 1 && a->V <= 0x7ffffff0L, "bad shape");
  WFT_CHECK_ARG_AS(who, a->k >= 2 && a->k <= TOPK_MAX, "k = beam size + 1 must lie in 2..9");
  WFT_CHECK_ARG_AS(who, a->ld % 8 == 0 && a->ld >= (a->V + 7) / 8 * 8 && (((uintptr_t)a->logits) & 15) == 0, "logits rows: 16-byte aligned, ld >= V rounded up to 8");
  WFT_CHECK_ARG_AS(who, !a->suppress_first || (a->first_len && a->len), "suppress_first needs len and first_len");
  return WFT_OK;
}

extern "C" int wft_decode_topk(const wft_decode_topk_args* a, void* stream) {
  if (int rc = topk_check(a, __func__)) return rc;
  hipLaunchKernelGGL(decode_topk_kernel<false>, dim3((unsigned)a->rows), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, wft_ts_rules{},
                     (const long*)nullptr, 0L, 0);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_decode_topk_ts(const wft_decode_topk_args* a, const wft_ts_rules* ru, const int64_t* tokens, int64_t ld_tokens, int eot,
                                  void* stream) {
  if (int rc = topk_check(a, __func__)) return rc;
  WFT_CHECK_ARG(eot >= 0 && eot < a->V, "eot outside the vocabulary");
  if (int rc = ts_check(ru, eot, a->V, __func__)) return rc;
  WFT_CHECK_ARG(a->first_len && a->len, "the timestamp rules need len and first_len");
  WFT_CHECK_ARG(tokens && ld_tokens >= 1, "the timestamp rules need the token rows");
  hipLaunchKernelGGL(decode_topk_kernel<true>, dim3((unsigned)a->rows), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, *ru,
                     (const long*)tokens, (long)ld_tokens, eot);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- one beam-search step per audio
// One workgroup per audio (include/wft.h wft_beam_update).  The <= 72 candidates are ranked by counting, thread 0 walks the order,
// then the rows of `tokens` and `anc` are permuted in place: a permutation of rows touches one column at a time, so the thread that
// owns column t reads its W values into registers and writes them back permuted — no scratch copy, nothing to order between threads.
#define BEAM_MAX_W 8
#define BEAM_THREADS 256
#define BEAM_MAX_CAND (BEAM_MAX_W * (BEAM_MAX_W + 1))

template <typename T>
__device__ __forceinline__ T beam_sel(const T* v, int j) {
  T out = v[0];
#pragma unroll
  for (int i = 1; i < BEAM_MAX_W; ++i) out = j == i ? v[i] : out;
  return out;
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_update_kernel(wft_beam_update_args a) {
  __shared__ float s_score[BEAM_MAX_CAND];
  __shared__ int s_tok[BEAM_MAX_CAND];
  __shared__ int s_order[BEAM_MAX_CAND];
  __shared__ int s_src[BEAM_MAX_W], s_ntok[BEAM_MAX_W], s_fsrc[BEAM_MAX_W];
  __shared__ float s_nscore[BEAM_MAX_W], s_fscore[BEAM_MAX_W];
  __shared__ int s_nfin;
  const int au = blockIdx.x, tid = threadIdx.x, W = a.W, k = W + 1;
  if (a.done[au]) return;  // a done audio is frozen
  const int r0 = au * W;
  const int L = a.len[r0];
  const int have = a.fin_n[au];
  if (L < 1 || L >= a.max_len || have < 0 || have >= a.C) {  // (nothing can be appended: the audio ends here)
    if (tid == 0) a.done[au] = 1;
    return;
  }
  const int nc = (a.first ? 1 : W) * k;
  if (tid < nc) {
    const int j = tid / k, i = tid - j * k;
    const int tok = a.cand_tok[(long)(r0 + j) * k + i];
    float sc = __fadd_rn(a.sum_logprob[r0 + j], a.cand_logp[(long)(r0 + j) * k + i]);
    sc = (tok >= 0 && sc == sc) ? sc : -INFINITY;
    s_tok[tid] = tok;
    s_score[tid] = sc;
  }
  __syncthreads();
  if (tid < nc) {
    const float sc = s_score[tid];
    int rank = 0;
    for (int o = 0; o < nc; ++o) {
      const float so = s_score[o];
      rank += (so > sc || (so == sc && o < tid)) ? 1 : 0;
    }
    s_order[rank] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int ns = 0, nf = 0;
    for (int p = 0; p < nc && ns < W; ++p) {
      const int cnd = s_order[p], tok = s_tok[cnd], j = cnd / k;
      if (tok < 0) continue;
      if (tok == a.eot) {
        if (have + nf < a.C) {
          s_fsrc[nf] = j;
          s_fscore[nf] = s_score[cnd];
          ++nf;
        }
      } else {
        s_src[ns] = j;
        s_ntok[ns] = tok;
        s_nscore[ns] = s_score[cnd];
        ++ns;
      }
    }
    for (; ns < W; ++ns) {  // (not reached while W non-eot candidates exist, which the host checks)
      s_src[ns] = ns;
      s_ntok[ns] = a.eot;
      s_nscore[ns] = -INFINITY;
    }
    s_nfin = nf;
  }
  __syncthreads();
  const int nf = s_nfin;
  for (int t = tid; t < (int)a.ld_tokens; t += BEAM_THREADS) {
    long v[BEAM_MAX_W];
    int w[BEAM_MAX_W];
#pragma unroll
    for (int j = 0; j < BEAM_MAX_W; ++j) {
      v[j] = (j < W && t < L) ? a.tokens[(long)(r0 + j) * a.ld_tokens + t] : 0;
      w[j] = (j < W && t < L - 1) ? a.anc[(long)(r0 + j) * a.ld_anc + t] : 0;
    }
    for (int e = 0; e < nf; ++e)
      a.fin_tokens[((long)au * a.C + have + e) * a.ld_tokens + t] = t < L ? beam_sel(v, s_fsrc[e]) : (long)a.eot;
    if (t <= L) {
      for (int s = 0; s < W; ++s) {
        const int j = s_src[s];
        a.tokens[(long)(r0 + s) * a.ld_tokens + t] = t < L ? beam_sel(v, j) : (long)s_ntok[s];
        if (t < L) a.anc[(long)(r0 + s) * a.ld_anc + t] = t < L - 1 ? beam_sel(w, j) : r0 + j;
      }
    }
  }
  if (tid < W) {
    a.sum_logprob[r0 + tid] = s_nscore[tid];
    a.len[r0 + tid] = L + 1;
    if (a.src_out) a.src_out[r0 + tid] = s_src[tid];
  }
  if (tid == 0) {
    for (int e = 0; e < nf; ++e) {
      a.fin_len[(long)au * a.C + have + e] = L + 1;
      a.fin_score[(long)au * a.C + have + e] = s_fscore[e];
    }
    a.fin_n[au] = have + nf;
    a.done[au] = (have + nf >= a.C || L + 1 >= a.max_len) ? 1 : 0;
  }
}

extern "C" int wft_beam_update(const wft_beam_update_args* a, void* stream) {
  WFT_CHECK_ARG(a && a->cand_tok && a->cand_logp && a->tokens && a->anc && a->len && a->sum_logprob && a->done && a->unfinished, "null pointer");
  WFT_CHECK_ARG(a->fin_tokens && a->fin_len && a->fin_score && a->fin_n, "null pointer (finished lists)");
  WFT_CHECK_ARG(a->B >= 1 && a->W >= 1 && a->W <= BEAM_MAX_W, "beam size must lie in 1..8");
  WFT_CHECK_ARG(a->C >= 1, "the finished lists hold C >= 1 entries");
  WFT_CHECK_ARG(a->max_len >= 1 && a->max_len <= a->ld_tokens && a->max_len <= a->ld_anc, "max_len must fit the token buffer and the ancestry table");
  WFT_CHECK_ARG(a->eot >= 0, "eot outside the vocabulary");
  hipLaunchKernelGGL(beam_update_kernel, dim3((unsigned)a->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)a->done, a->B, a->unfinished);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
