// attn_common.h — what the attention files share (kernels: attn_fwd.hip, attn_bwd.hip, attn_dq4w.hip, attn_dkdv4w.hip; host: attn.hip).
// Fused attention for head_dim 64 (every Whisper size): forward with online
// softmax, and a two-kernel recompute backward (dQ sweep over keys; dK/dV sweep over
// queries) — no atomics, bitwise reproducible.
//
// MFMA plan (v_mfma_f32_32x32x16_bf16, one wave = 32 queries (fwd, dq) or 32 keys (dkdv)):
//   fwd : S^T = K·Q^T (key rows from LDS, Q in registers; the query sits on the LANE, so
//         the row max / row sum of softmax are in-lane reductions + one xor-32 shuffle),
//         O^T += V^T·P^T with P^T taken straight from the S^T accumulators
//         (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand")
//         and V^T fragments read with ds_read_b64_tr_b16.
//   dq  : same orientation; dP^T = V·dO^T, dS^T = P^T ⊙ (dP^T − δ), dQ^T += K^T·dS^T.
//   dkdv: key on the lane: S = Q·K^T, dP = dO·V^T (K, V rows in registers, Q/dO tiles in
//         LDS), dV^T += dO^T·P, dK^T += Q^T·dS.
// LDS tiles are [64 rows][64 bf16] (128-byte rows) filled by global_load_lds_dwordx4 with
// ONE source-side swizzle (chunk ^= F(row)) that is conflict-free for both the 32-row
// ds_read_b128 operand reads and the 4-row transposed reads.
#pragma once
#include "common.h"
#include "gemm_common.h"  // wft_num_cus, wft_launch_lds
#include <stdlib.h>
#include <string.h>
#define ATT_NEG (-1.0e30f)
#define ATT_TAU 8.0f  // lazy-rescale threshold (log2 units)
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

struct AttnP {
  const unsigned short* q; long ldq, q_bs;
  const unsigned short* k; long ldk, k_bs;
  const unsigned short* v; long ldv, v_bs;
  unsigned short* o; long ldo, o_bs;
  float* lse;
  int B, H, Tq, Tk, causal;
  float scale;
  const unsigned short* d_o; long lddo, do_bs;
  float* delta;
  unsigned short* dq; long lddq, dq_bs;
  unsigned short* dk; long lddk, dk_bs;
  unsigned short* dv; long lddv, dv_bs;
  float* cs_q;  // [B * ceil(Tq/32)][H*64] per-wave column sums of dq (or NULL)
  float* cs_v;  // [B * ceil(Tk/32)][H*64] per-wave column sums of dv (or NULL)
  int xcd;      // XCD-aware block placement on (WFT_ATTN_XCD=0 switches it off for A/B runs)
  // q_prescaled (wft.h): q already carries scale * log2(e) (folded into the forward weight shadow of the q projection in fp32, one
  // bf16 rounding), so the scores ARE the exponent of exp2 and no kernel multiplies them by c.  c: factor between the q.k
  // accumulators and log2 units (1 when prescaled); ls: factor between them and natural-log units (lse = m * ls + log l; the
  // row constant that enters the S chains of the backward kernels is -lse / ls; dK = dS^T q * ls).  dQ keeps `scale`: the kernels
  // return the gradient w.r.t. the UNSCALED projection output, which is what the projection's backward GEMMs consume.
  int qpre;
  float c, ls;
};

__device__ __forceinline__ int att_F(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// Stage one [64][64] bf16 tile (rows row0.. of a [nrows, ld] matrix, 64 columns at `base`).
// 8 wave-instructions of 8 rows x 128 B; wave w issues instructions 2w, 2w+1.
// The per-lane part of the source address (row-in-tile * ld + swizzled chunk) is computed ONCE per kernel
// (AttStage); a full tile then costs no vector arithmetic at all: the tile origin is a wave-uniform 64-bit
// base (SALU) and the load uses the saddr + 32-bit-voffset form.  (Before: 16 v_mul_lo_u32 + 8 v_mad_u64_u32
// per tile, ~25 % of the forward kernel's VALU cycles.)  Only the ragged last tile clamps rows per lane.
struct AttStage {
  unsigned off[2];  // byte offset of this lane's 16 bytes inside a tile whose row 0 is the base
  int row[2];
};
__device__ __forceinline__ AttStage att_stage_init(long ld, int wave, int lane) {
  AttStage st;
  const int rr = lane >> 3, cp = lane & 7;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 8 * (wave * 2 + j) + rr;
    st.row[j] = row;
    st.off[j] = (unsigned)(row * (int)ld + ((cp ^ att_F(row)) << 3)) * 2u;
  }
  return st;
}
template <bool RAGGED>
__device__ __forceinline__ void att_stage1(const AttStage& st, const unsigned short* base, long ld, int row0, int nrows,
                                           char* tile, int wave, int lane) {
  const char* tb = (const char*)base + (long)row0 * ld * 2;  // wave-uniform
  if (!RAGGED) {  // scalar base + constant per-lane offset: the saddr form, no vector instruction per piece
    const unsigned long long b64 = (unsigned long long)tb;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b64), hi = __builtin_amdgcn_readfirstlane((unsigned)(b64 >> 32));
    const unsigned long long sb = ((unsigned long long)hi << 32) | lo;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr_of(tile) + wave * 2048);
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16_saddr(st.off[j], sb, dst + j * 1024);
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int rl = st.row[j];
    rl = row0 + rl < nrows ? rl : nrows - 1 - row0;
    const unsigned off = (unsigned)(rl * (int)ld + (((lane & 7) ^ att_F(st.row[j])) << 3)) * 2u;
    glds16(tb + off, tile + (wave * 2 + j) * 1024);
  }
}
__device__ __forceinline__ void att_stage(const AttStage& st, const unsigned short* base, long ld, int row0, int nrows,
                                          char* tile, int wave, int lane) {
  if (row0 + 64 <= nrows) att_stage1<false>(st, base, ld, row0, nrows, tile, wave, lane);
  else att_stage1<true>(st, base, ld, row0, nrows, tile, wave, lane);
}
// two tiles that share row0 / nrows (K and V, or Q and dO): ONE wave-uniform branch for both
__device__ __forceinline__ void att_stage2(const AttStage& sa, const unsigned short* a, long lda, char* ta,
                                           const AttStage& sb, const unsigned short* b, long ldb, char* tb,
                                           int row0, int nrows, int wave, int lane) {
  if (row0 + 64 <= nrows) {
    att_stage1<false>(sa, a, lda, row0, nrows, ta, wave, lane);
    att_stage1<false>(sb, b, ldb, row0, nrows, tb, wave, lane);
  } else {
    att_stage1<true>(sa, a, lda, row0, nrows, ta, wave, lane);
    att_stage1<true>(sb, b, ldb, row0, nrows, tb, wave, lane);
  }
}

// The attention files are compiled with -ffinite-math-only (Makefile): without it hipcc canonicalises (v_max_f32 x,x,x) every MFMA
// result in front of fmaxf, ~25 extra VALU instructions per tile.  Scores are finite by construction (masked entries
// are -1e30, never -inf).  Plain builtins (not inline asm) so the compiler's MFMA->VALU hazard handling still applies.
__device__ __forceinline__ float att_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float att_max2(float a, float b) { return __builtin_fmaxf(a, b); }
// max over the 32 scores a lane holds for its query (two 32x32 accumulator blocks)
__device__ __forceinline__ float att_max32(const f32x16& a, const f32x16& b) {
  float t0 = att_max3(a[0], a[1], a[2]), t1 = att_max3(a[3], a[4], a[5]);
  float t2 = att_max3(b[0], b[1], b[2]), t3 = att_max3(b[3], b[4], b[5]);
  t0 = att_max3(t0, a[6], a[7]);   t1 = att_max3(t1, a[8], a[9]);
  t2 = att_max3(t2, b[6], b[7]);   t3 = att_max3(t3, b[8], b[9]);
  t0 = att_max3(t0, a[10], a[11]); t1 = att_max3(t1, a[12], a[13]);
  t2 = att_max3(t2, b[10], b[11]); t3 = att_max3(t3, b[12], b[13]);
  t0 = att_max3(t0, a[14], a[15]); t2 = att_max3(t2, b[14], b[15]);
  return att_max3(att_max2(t0, t1), t2, t3);
}

// Per-lane LDS byte offsets of every fragment read, computed ONCE per kernel: with the tile base a
// compile-time constant (loops are unrolled by two over the LDS buffers) every ds_read in the tile loop is
// base-VGPR + immediate — the address arithmetic that used to be ~1/3 of the VALU stream is gone.
//   row[s]      : 32x32x16 A-operand row read, lane (r = lane&31, h = lane>>5) gets tile[blk*32 + r][16s + 8h .. +8]
//                 (+ blk*4096 immediate)
//   tr[db][t]   : transposed read t (rows 8t + 4h + (i>>2)) of the "accumulator as B operand" k-order:
//                 element j of lane (r, h) = tile[16*ks + 8*(j>>2) + 4h + (j&3)][32*db + r]   (+ ks*2048 immediate)
struct AttOffs {
  int row[4];
  int tr[2][2];
};
__device__ __forceinline__ AttOffs att_offsets(int lane) {
  AttOffs o;
  const int r = lane & 31, h = lane >> 5, g = lane >> 4, i = lane & 15;
#pragma unroll
  for (int s = 0; s < 4; ++s) o.row[s] = r * 128 + (((2 * s + h) ^ att_F(r)) << 4);
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int rowt = 8 * t + 4 * h + (i >> 2);
      const int col = 32 * db + 16 * (g & 1) + 4 * (i & 3);
      o.tr[db][t] = rowt * 128 + (((col >> 3) ^ att_F(rowt)) << 4) + ((col & 7) << 1);
    }
  return o;
}
__device__ __forceinline__ bf16x8 att_row_frag(const char* tile, const AttOffs& o, int blk, int s) {
  return *(const bf16x8*)(tile + blk * 4096 + o.row[s]);
}
__device__ __forceinline__ bf16x8 att_tr_frag(const char* tile, const AttOffs& o, int ks, int db) {
  s16x8 out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const s16x4 x = lds_read_tr16(tile + ks * 2048 + o.tr[db][t]);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[4 * t + e] = x[e];
  }
  return __builtin_bit_cast(bf16x8, out);
}

__device__ __forceinline__ bf16x8 att_pack8(const f32x16& a, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)a[8 * s + j];
  return r;
}

__device__ __forceinline__ bf16x8 att_load_reg_frag(const unsigned short* rowptr, int s, int h) {
  return *(const bf16x8*)(rowptr + 16 * s + 8 * h);
}

// ds_read_b64_tr_b16 from inline asm (the caller owns s_waitcnt lgkmcnt + sched_barrier before first use; see
// common.h lds_read_tr16_asm) with the slot / fragment offset in the instruction's immediate field
template <int IMM>
__device__ __forceinline__ s16x4 att_tr_asm(unsigned lds_byte_addr) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(IMM));
  return r;
}
// ds_read_b128 from inline asm, same contract: hipcc sinks plain LDS loads to just in front of their first use (one LDS round
// trip per MFMA pair in the S / dP loops); issued from asm they stay where they are written — all in one batch.
template <int IMM>
__device__ __forceinline__ f32x4 att_f4_asm(unsigned lds_byte_addr) {
  f32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(IMM));
  return r;
}
template <int IMM>
__device__ __forceinline__ bf16x8 att_row_asm(unsigned lds_byte_addr) {
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(IMM));
  return r;
}
__device__ __forceinline__ bf16x8 att_join(s16x4 a, s16x4 b) {
  s16x8 out;
#pragma unroll
  for (int e = 0; e < 4; ++e) { out[e] = a[e]; out[4 + e] = b[e]; }
  return __builtin_bit_cast(bf16x8, out);
}
// lanes l and l^32 hold the two halves of one query's row: combine them with v_permlane32_swap (VALU) instead of
// a ds_bpermute round trip through the LDS pipe.  (Inline asm: hipcc folds the builtin's two results into one value
// when both inputs are the same variable.  s_nop 1 covers the VALU-write -> permlane-read hazard.)
__device__ __forceinline__ void att_xhalf(float v, float& a, float& b) {
  a = v;
  b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float att_xhalf_max(float v) {
  float a, b;
  att_xhalf(v, a, b);
  return att_max2(a, b);
}
__device__ __forceinline__ float att_xhalf_sum(float v) {
  float a, b;
  att_xhalf(v, a, b);
  return a + b;
}

// Column sums (over the 32 rows = lanes of one half-wave pair) of a [64 d][32 rows] accumulator pair whose values were
// just rounded to bf16 for the store: acc[db][4a+e] belongs to column d = 32 db + 8 a + 4 h + e.  Rows >= nvalid are
// excluded.  Result: lanes r == 0 (h = 0, 1) write 32 floats each to dst[d].
__device__ __forceinline__ void att_colsum_store(const f32x16 (&acc)[2], float mul, bool row_valid, int r, int h, float* dst) {
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = row_valid ? bf2f(f2bf(acc[db][i] * mul)) : 0.f;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // xor masks < 32 stay inside the half-wave
      if (r == 0) dst[32 * db + 8 * (i >> 2) + 4 * h + (i & 3)] = v;
    }
}

// XCD-aware block placement.  The hardware deals consecutive workgroup ids round-robin over the 8 XCDs, each with its
// own 4 MiB L2.  All nx blocks of one (batch, head) re-stream the same K/V (or Q/dO) tiles, so they are mapped onto ONE
// XCD: the i-th workgroup an XCD receives works on group (i / nx) * 8 + xcd, member i % nx.  (PMC before: FETCH_SIZE of
// the backward kernels was ~5x their algorithmic bytes — every XCD pulled every head's tiles through the fabric.)
// Bijective when the number of (batch, head) groups is a multiple of 8; identity order otherwise.
__device__ __forceinline__ void att_block_coords(int nx, int H, int B, int xcd_on, int& bx, int& hd, int& b) {
  const int L = blockIdx.x;
  int g, m;
  if ((((long)H * B) & 7) == 0 && xcd_on) {
    const int xcd = L & 7, i = L >> 3;
    g = (i / nx) * 8 + xcd;
    m = i - (i / nx) * nx;
  } else {
    g = L / nx;
    m = L - g * nx;
  }
  bx = m;
  hd = g % H;
  b = g / H;
}

template <int V>
struct IntC { static constexpr int value = V; };
// f(IntC<0>{}), ..., f(IntC<N-1>{}): loop indices usable as template arguments (immediate offsets of asm reads)
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(IntC<N - 1>{});
  }
}

// ---- shared by the two one-wave-per-SIMD backward kernels: piece stride of their LDS tiles (layout: attn_dkdv4w.hip), clobber lists
#define W4_PIECE 1280
#define W4_KV 20480                      // one wave's K and V (dQ kernel: Q and dO) fragments in transit: two tiles of 10 240 B
#define W4_STR2(x) #x
#define W4_STR(x) W4_STR2(x)
#define W4_A8(x) "a" W4_STR(x##0), "a" W4_STR(x##1), "a" W4_STR(x##2), "a" W4_STR(x##3), "a" W4_STR(x##4), "a" W4_STR(x##5), "a" W4_STR(x##6), "a" W4_STR(x##7), "a" W4_STR(x##8), "a" W4_STR(x##9)
#define W4_V8(x) "v" W4_STR(x##0), "v" W4_STR(x##1), "v" W4_STR(x##2), "v" W4_STR(x##3), "v" W4_STR(x##4), "v" W4_STR(x##5), "v" W4_STR(x##6), "v" W4_STR(x##7), "v" W4_STR(x##8), "v" W4_STR(x##9)
#define W4_S8(x) "s" W4_STR(x##0), "s" W4_STR(x##1), "s" W4_STR(x##2), "s" W4_STR(x##3), "s" W4_STR(x##4), "s" W4_STR(x##5), "s" W4_STR(x##6), "s" W4_STR(x##7), "s" W4_STR(x##8), "s" W4_STR(x##9)
// v24..v255, s40..s79
#define W4_CLOBBER_V "v24", "v25", "v26", "v27", "v28", "v29", W4_V8(3), W4_V8(4), W4_V8(5), W4_V8(6), W4_V8(7), W4_V8(8), W4_V8(9), W4_V8(10), W4_V8(11), W4_V8(12), W4_V8(13), W4_V8(14), W4_V8(15), W4_V8(16), W4_V8(17), W4_V8(18), W4_V8(19), W4_V8(20), W4_V8(21), W4_V8(22), W4_V8(23), W4_V8(24), "v250", "v251", "v252", "v253", "v254", "v255"
#define W4_CLOBBER_S W4_S8(4), W4_S8(5), W4_S8(6), W4_S8(7)

template <int N>
__device__ __forceinline__ float w4_acc() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "i"(N));
  return x;
}
template <int BASE>
__device__ __forceinline__ f32x16 w4_get16() {
  f32x16 v;
  v[0] = w4_acc<BASE>(); v[1] = w4_acc<BASE + 1>(); v[2] = w4_acc<BASE + 2>(); v[3] = w4_acc<BASE + 3>();
  v[4] = w4_acc<BASE + 4>(); v[5] = w4_acc<BASE + 5>(); v[6] = w4_acc<BASE + 6>(); v[7] = w4_acc<BASE + 7>();
  v[8] = w4_acc<BASE + 8>(); v[9] = w4_acc<BASE + 9>(); v[10] = w4_acc<BASE + 10>(); v[11] = w4_acc<BASE + 11>();
  v[12] = w4_acc<BASE + 12>(); v[13] = w4_acc<BASE + 13>(); v[14] = w4_acc<BASE + 14>(); v[15] = w4_acc<BASE + 15>();
  return v;
}

// ---- host side: byte offsets fit the 32-bit buffer addressing of the one-wave-per-SIMD kernels' asm blocks
// (+ 256: the last workgroup's lanes address rows up to 255 past the end; the descriptors return zeros for them)
static inline bool attn_offsets_fit32(const wft_attn_args* a) {
  const long lim = 0x7fffffffL;
  return (long)(a->Tq + 256) * a->ldq * 2 < lim && (long)(a->Tq + 256) * a->lddo * 2 < lim && (long)(a->Tk + 256) * a->ldk * 2 < lim &&
         (long)(a->Tk + 256) * a->ldv * 2 < lim;
}
// What each kernel file offers attn_plan and the entry points (attn.hip): its eligibility rule and the launch on the plan's grid
// (the file knows its kernel's LDS bytes and instantiation; int: WFT_OK or WFT_ERR_LAUNCH from raising the dynamic-LDS limit)
bool wft_fwd_pipe_eligible(const wft_attn_args* a);                        // attn_fwd.hip
void wft_attn_fwd_launch(const AttnP& p, bool pipe, dim3 grid, hipStream_t s);
void wft_attn_dq8w_launch(const AttnP& p, dim3 grid, hipStream_t s);        // attn_bwd.hip
int wft_attn_dkdv8w_launch(const AttnP& p, dim3 grid, hipStream_t s);
bool wft_dq4w_eligible(const wft_attn_args* a);                            // attn_dq4w.hip
int wft_dq4w_launch(const AttnP& p, dim3 grid, hipStream_t s);
bool wft_dkdv4w_eligible(const wft_attn_args* a);                          // attn_dkdv4w.hip
int wft_dkdv4w_launch(const AttnP& p, dim3 grid, hipStream_t s);
