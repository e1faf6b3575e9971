// decode_attn.hip — single-token attention of KV-cached decoding (include/wft.h "Greedy decoding", "Beam search"): one query row per
// (sequence, head) against a key/value cache that grows by one row per step.  Nothing here depends on the step: the position of
// every sequence lives in device memory (`len`), so a step is a fixed launch sequence.
//
//  attn_decode_kernel / attn_decode_merge_kernel   softmax(q K^T) V for one query row, HBM-bound K/V read
//  attn_decode_beam_kernel<W, SELF>                the same attention for beams: self keys through the ancestry table, cross keys
//                                                  read once per audio for all of its beams.  Kept apart from attn_decode_kernel on
//                                                  purpose (see the note above it); the host side of the two entry points is one.
#include "decode_common.h"

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
// Sharing __device__ __forceinline__ helpers between the two does not work either (same check).  All four — the per-query block
// update, the 8-group butterfly, the LDS put, the wave merge and store — shared: attn_decode_kernel goes from 114 to 144 VGPRs,
// attn_decode_beam_kernel<1, true> from 126 to 138, and all ten beam streams change.  Only the merge / store tail shared: the VGPR
// counts stay, but attn_decode_kernel's stream (1 143 -> 1 140 lines) and all ten beam streams still change.
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
