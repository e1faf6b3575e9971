// attn_dkdv4w.hip — dK/dV, one wave per SIMD (round 4): the kernel, its eligibility rule and its launch
#include "attn_common.h"
// The non-causal dK/dV sweep (the encoder's 1500 x 1500 attention and the decoder's cross attention: 85 of a step's 657 ms in
// attn_bwd_dkdv_kernel, matrix pipe 29 % busy) as ONE hand-scheduled stream per SIMD, like gemm_nt4w.hip.  In that kernel a
// wave's chain  S / dP MFMAs -> exp, multiplies, packing -> dV / dK MFMAs  is serial and only the SIMD's other wave fills the
// holes; here a wave owns 64 keys (two 32-key blocks, K / V fragments in a[128:191]) and runs THREE query blocks at once:
//   iteration j:  MFMA  slots  0-15  dV / dK of block j-1   (operands: P, dS packed in v[32:63]; Q^T, dO^T fragments v[96:127])
//                       slots 16-31  S / dP of block j+1    (into the other accumulator generation, which STARTS from the row
//                                                            constants -lse/scale and -delta read from LDS as the C operand)
//                 VALU  4 per slot   block j: slots 0-15  p = exp2(c S')  (2 multiplies + 2 exponentials per slot),
//                                             slots 16-23 dS = p dP',  slots 24-31 the 32 bf16 packs
//                 LDS   slots  0-11  row fragments of Q, dO and the constants of block j+1;  slots 16-31 transposed fragments of j
// so the matrix pipe never waits for the vector stream of the same block (budget per 32-cycle MFMA: 24 issue cycles; 2 exp + 2
// mul = 24).  Q / dO fragments and constants are shared by the wave's two key blocks (half the LDS traffic per MFMA).
// Queries beyond Tq need no masks: their Q / dO rows and constants arrive as ZEROS (buffer descriptors that end at row Tq), so
// they add exp2(0) * 0 = 0 to dV and 0 * finite = 0 to dK; keys beyond Tk are lanes whose results are not stored.
// LDS: three buffers of one 64-query tile {Q, dO: 8 pieces of 8 rows, 1 280 B apart, piece pid at pid * 1280 + 64 (pid & 1) +
// 16 (pid >> 1); -lse/scale, -delta: 256 B each}.  Piece pid holds queries q0 + {0, 2} + 16 m, q0 = (pid & 1) + 4 (pid >> 1): row q sits
// at 64 (q & 3) + 16 ((q >> 2) & 3) modulo 256 B, which makes BOTH the 32-row ds_read_b128 operand reads and the 4-row
// ds_read_b64_tr_b16 reads bank-conflict-free with every fragment address = one base register + an immediate.
#define D4_BUF 20992  // Q at 0, dO at 10240, -lse/scale at 20480, -delta at 20736
#define D4_LDS (3 * D4_BUF + 4 * W4_KV)
#define D4_ASM_MACROS R"ASM(
; registers: S(g,kb) v[g+32kb..+15], dP(g,kb) v[g+16+32kb..+15], g = 128 / 192;  PF(kb) v[32+16kb..+7], DSF(kb) v[40+16kb..+7];
; row constants v[64:79] (-lse/scale), v[80:95] (-delta); Q rows AQ(s) a[192+4s..], dO rows AD(s) a[208+4s..]; TQ(ks,db) v[96+8ks+4db..], TD(ks,db) v[112+8ks+4db..];
; dK(kb,db) a[64kb+16db..+15], dV(kb,db) a[64kb+32+16db..+15]; KF(kb,s) a[128+32kb+4s..+3], VF(kb,s) a[144+32kb+4s..+3]
.macro D4_M2 n
  .if ((\n) %% 2) == 0
    v_mfma_f32_32x32x16_bf16 a[64*((\n)/8)+32+16*(((\n)/2)%%2):64*((\n)/8)+32+16*(((\n)/2)%%2)+15], v[112+8*(((\n)/4)%%2)+4*(((\n)/2)%%2):112+8*(((\n)/4)%%2)+4*(((\n)/2)%%2)+3], v[32+16*((\n)/8)+4*(((\n)/4)%%2):32+16*((\n)/8)+4*(((\n)/4)%%2)+3], a[64*((\n)/8)+32+16*(((\n)/2)%%2):64*((\n)/8)+32+16*(((\n)/2)%%2)+15]
  .else
    v_mfma_f32_32x32x16_bf16 a[64*((\n)/8)+16*(((\n)/2)%%2):64*((\n)/8)+16*(((\n)/2)%%2)+15], v[96+8*(((\n)/4)%%2)+4*(((\n)/2)%%2):96+8*(((\n)/4)%%2)+4*(((\n)/2)%%2)+3], v[40+16*((\n)/8)+4*(((\n)/4)%%2):40+16*((\n)/8)+4*(((\n)/4)%%2)+3], a[64*((\n)/8)+16*(((\n)/2)%%2):64*((\n)/8)+16*(((\n)/2)%%2)+15]
  .endif
.endm
.macro D4_M1 n, g
  ; chain (\n)/4: 0 S kb0, 1 dP kb0, 2 S kb1, 3 dP kb1; k-step (\n)%%4.  The first MFMA of a chain starts from the block's row
  ; constants (v[64:79] -lse/scale for S, v[80:95] -delta for dP), shared by the two key blocks
  .if ((\n) %% 4) == 0
    v_mfma_f32_32x32x16_bf16 v[\g+16*(((\n)/4)%%2)+32*((\n)/8):\g+16*(((\n)/4)%%2)+32*((\n)/8)+15], a[192+16*(((\n)/4)%%2):192+16*(((\n)/4)%%2)+3], a[128+16*(((\n)/4)%%2)+32*((\n)/8):128+16*(((\n)/4)%%2)+32*((\n)/8)+3], v[64+16*(((\n)/4)%%2):64+16*(((\n)/4)%%2)+15]
  .else
    v_mfma_f32_32x32x16_bf16 v[\g+16*(((\n)/4)%%2)+32*((\n)/8):\g+16*(((\n)/4)%%2)+32*((\n)/8)+15], a[192+16*(((\n)/4)%%2)+4*((\n)%%4):192+16*(((\n)/4)%%2)+4*((\n)%%4)+3], a[128+16*(((\n)/4)%%2)+32*((\n)/8)+4*((\n)%%4):128+16*(((\n)/4)%%2)+32*((\n)/8)+4*((\n)%%4)+3], v[\g+16*(((\n)/4)%%2)+32*((\n)/8):\g+16*(((\n)/4)%%2)+32*((\n)/8)+15]
  .endif
.endm
; row read i (0..15) of a block, in the order the S / dP chains need them: 0-3 -lse/scale -> v[64:79], 4-7 Q rows -> a[192:207],
; 8-11 -delta -> v[80:95], 12-15 dO rows -> a[208:223]
.macro D4_RD1 i, rb, cb, qb
  .if (\i) < 4
    ds_read_b128 v[64+4*(\i):64+4*(\i)+3], \cb offset:20480+128*\qb+32*(\i)
  .elseif (\i) < 8
    ds_read_b128 a[192+4*((\i)-4):192+4*((\i)-4)+3], \rb offset:512*\qb+32*((\i)-4)
  .elseif (\i) < 12
    ds_read_b128 v[80+4*((\i)-8):80+4*((\i)-8)+3], \cb offset:20736+128*\qb+32*((\i)-8)
  .else
    ds_read_b128 a[208+4*((\i)-12):208+4*((\i)-12)+3], \rb offset:10240+512*\qb+32*((\i)-12)
  .endif
.endm
; transposed read m (0..15) in the order the dV / dK MFMAs consume them: (ks, db) = (m/8, (m/4)%2); (m/2)%2 = 0 dO^T, 1 Q^T; t = m%2
.macro D4_RD2 m, tb, qb
  ds_read_b64_tr_b16 v[112-16*(((\m)/2)%%2)+8*((\m)/8)+4*(((\m)/4)%%2)+2*((\m)%%2):112-16*(((\m)/2)%%2)+8*((\m)/8)+4*(((\m)/4)%%2)+2*((\m)%%2)+1], \tb offset:10240*(1-((\m)/2)%%2)+5152*((\m)%%2)+128*(4*\qb+2*((\m)/8))+64*(((\m)/4)%%2)
.endm
; next 64-query tile: source bases += 64 rows (Q, dO) / 256 B (constants), bounds shrink with them (not below zero)
.macro D4_ADVANCE
  s_add_u32 s40, s40, s56
  s_addc_u32 s41, s41, 0
  s_sub_u32 s42, s42, s56
  s_cselect_b32 s42, 0, s42
  s_add_u32 s44, s44, s57
  s_addc_u32 s45, s45, 0
  s_sub_u32 s46, s46, s57
  s_cselect_b32 s46, 0, s46
  s_add_u32 s48, s48, 256
  s_addc_u32 s49, s49, 0
  s_sub_u32 s50, s50, 256
  s_cselect_b32 s50, 0, s50
.endm
; step i (0..4) of this wave's share of one tile -> the buffer at LDS offset \boff (an SGPR): pieces 2 wave, 2 wave + 1 of Q (0, 1)
; and dO (2, 3); 4: the constants (even waves -lse/scale, odd waves -delta; waves 2, 3 repeat 0, 1 so that every wave has
; five pieces per tile in flight and the counted waits are uniform)
.macro D4_DMA i, boff
  .if (\i) == 0
    s_add_u32 m0, s58, \boff
    s_nop 0
    buffer_load_dwordx4 %[voQ0], s[40:43], 0 offen lds
  .elseif (\i) == 1
    s_add_u32 m0, s59, \boff
    s_nop 0
    buffer_load_dwordx4 %[voQ1], s[40:43], 0 offen lds
  .elseif (\i) == 2
    s_add_u32 m0, s58, \boff
    s_add_u32 m0, m0, 10240
    s_nop 0
    buffer_load_dwordx4 %[voD0], s[44:47], 0 offen lds
  .elseif (\i) == 3
    s_add_u32 m0, s59, \boff
    s_add_u32 m0, m0, 10240
    s_nop 0
    buffer_load_dwordx4 %[voD1], s[44:47], 0 offen lds
  .else
    s_add_u32 m0, s60, \boff
    s_nop 0
    buffer_load_dword %[voC], s[48:51], 0 offen lds
  .endif
.endm
.macro D4_STAGE boff
  D4_DMA 0, \boff
  D4_DMA 1, \boff
  D4_DMA 2, \boff
  D4_DMA 3, \boff
  D4_DMA 4, \boff
.endm
; one iteration.  gV: generation (128 / 192) whose block is exponentiated here, gM: the other (target of the S / dP MFMAs);
; rb1, cb1, qb1: bases / half of the block whose row fragments are read; tb2, qb2: of the block whose transposed fragments are read;
; dma = 1: this wave's LDS-DMA share of the tile two ahead goes out in slots 16-20 (buffer offset s65), sources advance in slot 21.
; A wave alone on its SIMD issues in order and an MFMA gap hides about 24 issue cycles (measured here: two junk v_mov per gap cost
; 1.4 cycles each, the third and fourth 3.4): every slot carries 20 cycles of vector work and ONE LDS read —
;   slots  0-15  c-multiply of key block 1, both exponentials; row read number slot
;   slots 16-23  four dS multiplies, one pack; transposed read         24-31  three packs, the c-multiplies of the NEXT block's
;                key block 0 (its S chain finished in slot 19); transposed read
; LDS reads are counted, never drained: transposed fragment f (two reads, slots 16 + 2 f, 17 + 2 f) is consumed by slot f of the
; next iteration behind lgkmcnt(14 - f) (the later transposed reads + the f row reads issued since); the row reads behind
; lgkmcnt(8) (slot 16: constants and Q rows) and lgkmcnt(4) (slot 20: -delta, dO rows; four transposed reads are younger).
.macro D4_ITER gV, gM, rb1, cb1, qb1, tb2, qb2, dma
  .set d4_s, 0
  .rept 32
    .if d4_s < 8
      s_waitcnt lgkmcnt(14-d4_s)
    .elseif d4_s == 16
      s_waitcnt lgkmcnt(8)
    .elseif d4_s == 20
      s_waitcnt lgkmcnt(4)
    .endif
    .if d4_s < 16
      D4_M2 d4_s
      .if att_pre == 0
      v_mul_f32 v[\gV+32+d4_s], %[c], v[\gV+32+d4_s]
      .endif
      v_exp_f32 v[\gV+d4_s], v[\gV+d4_s]
      D4_RD1 d4_s, \rb1, \cb1, \qb1
      v_exp_f32 v[\gV+32+d4_s], v[\gV+32+d4_s]
    .else
      D4_M1 d4_s-16, \gM
      .if d4_s < 24
        v_mul_f32 v[\gV+16+2*(d4_s-16)], v[\gV+2*(d4_s-16)], v[\gV+16+2*(d4_s-16)]
        v_mul_f32 v[\gV+16+2*(d4_s-16)+1], v[\gV+2*(d4_s-16)+1], v[\gV+16+2*(d4_s-16)+1]
        D4_RD2 d4_s-16, \tb2, \qb2
        v_mul_f32 v[\gV+48+2*(d4_s-16)], v[\gV+32+2*(d4_s-16)], v[\gV+48+2*(d4_s-16)]
        v_mul_f32 v[\gV+48+2*(d4_s-16)+1], v[\gV+32+2*(d4_s-16)+1], v[\gV+48+2*(d4_s-16)+1]
        v_cvt_pk_bf16_f32 v[32+(d4_s-16)], v[\gV+2*(d4_s-16)], v[\gV+2*(d4_s-16)+1]
        .if \dma && d4_s < 21
          D4_DMA d4_s-16, s65
        .endif
        .if \dma && d4_s == 21
          D4_ADVANCE
        .endif
      .else
        v_cvt_pk_bf16_f32 v[48+(d4_s-24)], v[\gV+32+2*(d4_s-24)], v[\gV+32+2*(d4_s-24)+1]
        v_cvt_pk_bf16_f32 v[40+(d4_s-24)], v[\gV+16+2*(d4_s-24)], v[\gV+16+2*(d4_s-24)+1]
        D4_RD2 d4_s-16, \tb2, \qb2
        v_cvt_pk_bf16_f32 v[56+(d4_s-24)], v[\gV+48+2*(d4_s-24)], v[\gV+48+2*(d4_s-24)+1]
        .if att_pre == 0
        v_mul_f32 v[\gM+2*(d4_s-24)], %[c], v[\gM+2*(d4_s-24)]
        v_mul_f32 v[\gM+2*(d4_s-24)+1], %[c], v[\gM+2*(d4_s-24)+1]
        .endif
      .endif
    .endif
    .set d4_s, d4_s+1
  .endr
.endm
)ASM"

#define D4_ASM_PURGE R"ASM(
.purgem D4_M2
.purgem D4_M1
.purgem D4_RD1
.purgem D4_RD2
.purgem D4_ADVANCE
.purgem D4_DMA
.purgem D4_STAGE
.purgem D4_ITER
)ASM"

// a0..a223
#define D4_CLOBBER_A "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", W4_A8(1), W4_A8(2), W4_A8(3), W4_A8(4), W4_A8(5), W4_A8(6), W4_A8(7), W4_A8(8), W4_A8(9), W4_A8(10), W4_A8(11), W4_A8(12), W4_A8(13), W4_A8(14), W4_A8(15), W4_A8(16), W4_A8(17), W4_A8(18), W4_A8(19), W4_A8(20), W4_A8(21), "a220", "a221", "a222", "a223"

#ifdef D4_STAMPS
#define D4_STAMP_ASM(r) "s_memtime s[" #r ":" #r "+1]\n s_waitcnt lgkmcnt(0)\n"
#else
#define D4_STAMP_ASM(r) ""
#endif
#ifdef D4_STAMPS  // developer build (tools/dev/dkdv4w_stamps.py, make ATTN_DEFS=-DD4_STAMPS): clock-tick sums over workgroups, wave 0
__device__ unsigned long long d4_dbg[16];
extern "C" void wft_dbg_read(unsigned long long* host, int reset) {
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(d4_dbg), z, sizeof z); return; }
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(d4_dbg), 16 * sizeof(unsigned long long));
}
#endif
// descriptors and requests shared by the main block and the prefetch block of attn_bwd_dkdv4w_kernel
#define D4_ASM_MACROS2 R"ASM(
; descriptors: Q s[40:43], dO s[44:47], this wave's constants (-lse/scale or -delta) s[48:51], K s[68:71], V s[72:75];
; tile strides s56, s57; LDS-DMA destinations inside a buffer: piece 2 wave (s58), 2 wave + 1 (s59), this wave's constant row (s60:
; even waves lse, odd delta); buffer offsets: cur (tile T) s63, nxt (T+1) s64, ld (T+2) s65; this wave's K / V transit area s52
.macro D4_SRD_INIT
  s_mov_b64 s[40:41], %[bQ]
  s_lshr_b32 s61, %[stQ], 6
  s_sub_u32 s62, %[tq], 1
  s_mul_i32 s42, s62, s61
  s_add_u32 s42, s42, 128
  s_mov_b32 s43, 0x20000
  s_mov_b64 s[44:45], %[bD]
  s_lshr_b32 s61, %[stD], 6
  s_mul_i32 s46, s62, s61
  s_add_u32 s46, s46, 128
  s_mov_b32 s47, 0x20000
  s_and_b32 s61, %[wave], 1
  s_cmp_eq_u32 s61, 0
  s_cselect_b64 s[48:49], %[bL], %[bT]
  s_lshl_b32 s50, %[tq], 2
  s_mov_b32 s51, 0x20000
  s_mov_b32 s56, %[stQ]
  s_mov_b32 s57, %[stD]
  s_mov_b64 s[68:69], %[bK]
  s_sub_u32 s62, %[tk], 1
  s_mul_i32 s70, s62, %[ldk2]
  s_add_u32 s70, s70, 128
  s_mov_b32 s71, 0x20000
  s_mov_b64 s[72:73], %[bV]
  s_mul_i32 s74, s62, %[ldv2]
  s_add_u32 s74, s74, 128
  s_mov_b32 s75, 0x20000
  s_lshl_b32 s61, %[wave], 1
  s_mul_i32 s58, s61, 1280
  s_lshr_b32 s62, s61, 1
  s_lshl_b32 s62, s62, 4
  s_add_u32 s58, s58, s62
  s_add_u32 s58, s58, %[lds0]
  s_add_u32 s59, s58, 1344
  s_and_b32 s60, %[wave], 1
  s_mul_i32 s60, s60, 256
  s_add_u32 s60, s60, 20480
  s_add_u32 s60, s60, %[lds0]
  s_mov_b32 s63, 0
  s_mov_b32 s64, )ASM" W4_STR(D4_BUF) R"ASM(
  s_mov_b32 s65, 2*)ASM" W4_STR(D4_BUF) R"ASM(
  s_mul_i32 s52, %[wave], )ASM" W4_STR(W4_KV) R"ASM(
  s_add_u32 s52, s52, 3*)ASM" W4_STR(D4_BUF) R"ASM(
  s_add_u32 s52, s52, %[lds0]
.endm
; K / V rows of this wave's 64 keys -> its transit area, as two tiles in the piece layout of the Q / dO tiles (8 + 8 LDS-DMA pieces of
; eight whole 128-byte rows: the row-per-lane fragment loads they replace touched every line four times and cost ~400 cycles of
; issue each).  Piece pid holds keys q0 + {0, 2} + 16 m, q0 = (pid & 1) + 4 (pid >> 1); rows past Tk lie beyond the descriptors: zeros.
.macro D4_KVDMA
  .set d4_i, 0
  .rept 8
    s_mul_i32 s61, %[ldk2], (d4_i%%2)+4*(d4_i/2)
    v_add_u32 v29, s61, %[voKp]
    s_add_u32 m0, s52, d4_i*1280+64*(d4_i%%2)+16*(d4_i/2)
    s_mul_i32 s62, %[ldv2], (d4_i%%2)+4*(d4_i/2)
    buffer_load_dwordx4 v29, s[68:71], 0 offen lds
    v_add_u32 v30, s62, %[voVp]
    s_add_u32 m0, s52, 10240+d4_i*1280+64*(d4_i%%2)+16*(d4_i/2)
    s_nop 0
    buffer_load_dwordx4 v30, s[72:75], 0 offen lds
    .set d4_i, d4_i+1
  .endr
.endm
; ... and from there into a[128:191] as row fragments (lane (r, h): key 32 kb + r, columns 16 s + 8 h .. + 8)
.macro D4_KVRD
  s_sub_u32 s61, s52, %[lds0]
  v_add_u32 v29, s61, %[rb]
  .set d4_i, 0
  .rept 8
    ds_read_b128 a[128+32*(d4_i/4)+4*(d4_i%%4):128+32*(d4_i/4)+4*(d4_i%%4)+3], v29 offset:512*(d4_i/4)+32*(d4_i%%4)
    ds_read_b128 a[144+32*(d4_i/4)+4*(d4_i%%4):144+32*(d4_i/4)+4*(d4_i%%4)+3], v29 offset:10240+512*(d4_i/4)+32*(d4_i%%4)
    .set d4_i, d4_i+1
  .endr
.endm
; first two tiles of an item -> buffers 0, 1 (sources end up two tiles on)
.macro D4_STAGE2
  D4_STAGE s63
  D4_ADVANCE
  s_nop 4
  D4_STAGE s64
  D4_ADVANCE
.endm
)ASM"
#define D4_ASM_PURGE2 R"ASM(
.purgem D4_SRD_INIT
.purgem D4_KVDMA
.purgem D4_KVRD
.purgem D4_STAGE2
)ASM"

template <bool PRE>  // PRE: q_prescaled — the asm loops are assembled without their c-scale multiplies (.set att_pre)
__global__ __launch_bounds__(256) void attn_bwd_dkdv4w_kernel(AttnP p) {
#ifdef D4_STAMPS
  unsigned long long st0 = __builtin_amdgcn_s_memtime();
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // PERSISTENT: one workgroup per CU (it owns the CU: one wave per SIMD, 512 registers) walks work items (batch, head, 256-key
  // block).  The workgroups of one XCD take that XCD's items round-robin, in the order (head group, key block): the ~32 items
  // in flight on an XCD are the key blocks of 5-6 heads, whose Q / dO tiles (384 KB per head) stay in that XCD's L2, exactly
  // as with one workgroup per item (att_block_coords).  The next item's K / V fragments and first three tiles are requested
  // before this item's epilogue, so only a workgroup's first item waits for memory.
  const int nkb = (p.Tk + 255) >> 8;
  const int ngrp = p.H * p.B;
  const bool xcd_mode = ((ngrp & 7) == 0) && p.xcd && ((gridDim.x & 7) == 0);
  const int xcd = xcd_mode ? (int)(blockIdx.x & 7) : 0;
  const int w0 = xcd_mode ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int wstep = xcd_mode ? (int)(gridDim.x >> 3) : (int)gridDim.x;
  const int nitems = (xcd_mode ? ngrp >> 3 : ngrp) * nkb;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
  // fragment read bases (see the layout note above)
  const int c = r & 15, pidr = (c & 1) | ((c >> 2) << 1);
  const unsigned rb = lds0 + pidr * W4_PIECE + 64 * (pidr & 1) + 16 * (pidr >> 1) + (2 * (r >> 4) + ((c >> 1) & 1)) * 128 + h * 16;
  const int g4 = lane >> 4, i16 = lane & 15, pidt = ((i16 >> 2) & 1) | ((g4 >> 1) << 1);
  const unsigned tb = lds0 + pidt * W4_PIECE + 64 * (pidt & 1) + 16 * (pidt >> 1) + ((i16 >> 3) & 1) * 128 + 32 * (g4 & 1) + 8 * (i16 & 3);
  const unsigned cb = lds0 + 16 * h;
  // LDS-DMA share of this wave: pieces 2 wave and 2 wave + 1 of Q and of dO; lane: slot lane >> 3 (query q0 + 2 (slot & 1) + 16 (slot >> 1)), chunk lane & 7
  const int slot = lane >> 3, ch = lane & 7;
  auto qrow = [&](int pid) { return (pid & 1) + 4 * (pid >> 1) + 2 * (slot & 1) + 16 * (slot >> 1); };
  const unsigned voQ0 = (unsigned)(qrow(2 * wave) * (int)p.ldq + ch * 8) * 2u, voQ1 = (unsigned)(qrow(2 * wave + 1) * (int)p.ldq + ch * 8) * 2u;
  const unsigned voD0 = (unsigned)(qrow(2 * wave) * (int)p.lddo + ch * 8) * 2u, voD1 = (unsigned)(qrow(2 * wave + 1) * (int)p.lddo + ch * 8) * 2u;
  const unsigned voC = (unsigned)lane * 4u;
  auto sg64 = [](unsigned long long x) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
  };
  const unsigned tq = __builtin_amdgcn_readfirstlane((unsigned)p.Tq), tk = __builtin_amdgcn_readfirstlane((unsigned)p.Tk);
  const unsigned ldk2 = __builtin_amdgcn_readfirstlane((unsigned)p.ldk * 2u), ldv2 = __builtin_amdgcn_readfirstlane((unsigned)p.ldv * 2u);
  const unsigned stQ = __builtin_amdgcn_readfirstlane((unsigned)p.ldq * 128u), stD = __builtin_amdgcn_readfirstlane((unsigned)p.lddo * 128u);
  const unsigned npair = __builtin_amdgcn_readfirstlane((unsigned)((p.Tq + 63) >> 6));  // 64-query tiles = iteration pairs
  const float cscale = p.c;
  const unsigned cbits = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, cscale));
  const unsigned wv = (unsigned)wave;
  // everything that depends on the work item
  struct Item {
    int b, hd, kw0;
    unsigned long long bQ, bD, bL, bT, bK, bV;
    unsigned voKp, voVp;
  };
  auto item = [&](int t) {
    Item x;
    const int g = xcd_mode ? (t / nkb) * 8 + xcd : t / nkb;
    x.hd = g % p.H;
    x.b = g / p.H;
    x.kw0 = (t % nkb) * 256 + wave * 64;
    const long sbase = ((long)x.b * p.H + x.hd) * p.Tq;
    x.bQ = sg64((unsigned long long)(p.q + (long)x.b * p.q_bs + x.hd * 64));
    x.bD = sg64((unsigned long long)(p.d_o + (long)x.b * p.do_bs + x.hd * 64));
    x.bL = sg64((unsigned long long)(p.delta + (long)p.B * p.H * p.Tq + sbase));  // -lse / scale (written by the dQ kernel)
    x.bT = sg64((unsigned long long)(p.delta + sbase));                            // -delta
    x.bK = sg64((unsigned long long)(p.k + (long)x.b * p.k_bs + x.hd * 64));
    x.bV = sg64((unsigned long long)(p.v + (long)x.b * p.v_bs + x.hd * 64));
    // byte offset of this lane's share of K / V piece 0 of the wave's 64 keys (slot lane >> 3: key 2 (slot & 1) + 16 (slot >> 1),
    // chunk lane & 7), relative to the (batch, head) bases
    x.voKp = (unsigned)((x.kw0 + 2 * (slot & 1) + 16 * (slot >> 1)) * (int)p.ldk + ch * 8) * 2u;
    x.voVp = (unsigned)((x.kw0 + 2 * (slot & 1) + 16 * (slot >> 1)) * (int)p.ldv + ch * 8) * 2u;
    return x;
  };

  for (int t = w0; t < nitems; t += wstep) {
  const Item cur = item(t);
  const int b = cur.b, hd = cur.hd, kw0 = cur.kw0;
  const unsigned first = __builtin_amdgcn_readfirstlane((unsigned)(t == w0));

  asm volatile(".set att_pre, %c[pre]\n" D4_ASM_MACROS D4_ASM_MACROS2 R"ASM(
    D4_SRD_INIT
    s_mov_b32 s66, %[npair]      ; loop counter
    s_cmp_eq_u32 %[first], 0
    s_cbranch_scc1 2f
    ; ---- first item of this workgroup: its K / V rows and tiles 0, 1 are requested here ...
    D4_KVDMA
    D4_STAGE2
    s_branch 3f
2:
    ; ---- ... later ones found them requested by the prefetch block behind the previous item (below): only the descriptors move on
    D4_ADVANCE
    D4_ADVANCE
    s_waitcnt vmcnt(0)
3:
    ; ---- (under the loads) accumulators, packed operands and transposed fragments start from zero: iteration 0 multiplies them
    .set d4_i, 0
    .rept 128
      v_accvgpr_write_b32 a[d4_i], 0
      .set d4_i, d4_i+1
    .endr
    .set d4_i, 32
    .rept 32
      v_mov_b32 v[d4_i], 0
      v_mov_b32 v[d4_i+64], 0
      .set d4_i, d4_i+1
    .endr
    v_mov_b32 v24, %[rb]
    v_mov_b32 v25, %[tb]
    v_mov_b32 v26, %[cb]
    v_add_u32 v27, s64, v24
    v_add_u32 v28, s64, v26
    s_waitcnt vmcnt(5)         ; K / V rows and tile 0 (tile 1: five pieces may still be in flight)
    s_barrier
    D4_KVRD
    )ASM" D4_STAMP_ASM(76) R"ASM(
    ; ---- block 0: row fragments + constants, S / dP -> generation 128
    .set d4_i, 0
    .rept 16
      D4_RD1 d4_i, v24, v26, 0
      .set d4_i, d4_i+1
    .endr
    s_waitcnt lgkmcnt(0)
    .set d4_i, 0
    .rept 16
      D4_M1 d4_i, 128
      .set d4_i, d4_i+1
    .endr
    s_nop 15
    s_nop 15
    .set d4_i, 0
    .if att_pre == 0
    .rept 16
      v_mul_f32 v[128+d4_i], %[c], v[128+d4_i]
      .set d4_i, d4_i+1
    .endr
    .endif
1:
    ; ==== tile boundary: tile T+1 has landed for every wave, tile T-1's buffer is free -> tile T+2 goes into it during this
    ; iteration (a fourth buffer and three tiles of distance measured the same; the space carries the K / V transit areas)
    s_waitcnt vmcnt(0)
    s_barrier
    ; even iteration (block 2T): row fragments of block 2T+1 (this tile, half 1), transposed fragments of block 2T (half 0)
    D4_ITER 128, 192, v24, v26, 1, v25, 0, 1
    ; odd iteration (block 2T+1): row fragments of block 2T+2 (next tile, half 0), transposed fragments of block 2T+1
    D4_ITER 192, 128, v27, v28, 0, v25, 1, 0
    ; rotate the buffers: cur <- nxt <- ld <- cur
    s_mov_b32 s67, s63
    s_mov_b32 s63, s64
    s_mov_b32 s64, s65
    s_mov_b32 s65, s67
    v_add_u32 v24, s63, %[rb]
    v_add_u32 v25, s63, %[tb]
    v_add_u32 v26, s63, %[cb]
    v_add_u32 v27, s64, %[rb]
    v_add_u32 v28, s64, %[cb]
    s_sub_u32 s66, s66, 1
    s_cmp_eq_u32 s66, 0
    s_cbranch_scc0 1b
    ; ---- dV / dK of the last block
    s_waitcnt lgkmcnt(0)
    )ASM" D4_STAMP_ASM(78) R"ASM(
    s_nop 1
    .set d4_i, 0
    .rept 16
      D4_M2 d4_i
      .set d4_i, d4_i+1
    .endr
    s_waitcnt vmcnt(0)         ; (the tiles requested past the last query block: zeros, but they must not land later)
    s_nop 15
  )ASM" D4_ASM_PURGE D4_ASM_PURGE2
               :
               : [rb] "v"(rb), [tb] "v"(tb), [cb] "v"(cb), [voQ0] "v"(voQ0), [voQ1] "v"(voQ1), [voD0] "v"(voD0), [voD1] "v"(voD1),
                 [voC] "v"(voC), [voKp] "v"(cur.voKp), [voVp] "v"(cur.voVp), [bK] "s"(cur.bK),
                 [bV] "s"(cur.bV), [bQ] "s"(cur.bQ), [bD] "s"(cur.bD), [bL] "s"(cur.bL), [bT] "s"(cur.bT), [tq] "s"(tq), [tk] "s"(tk),
                 [ldk2] "s"(ldk2), [ldv2] "s"(ldv2), [first] "s"(first), [stQ] "s"(stQ), [stD] "s"(stD), [npair] "s"(npair), [c] "s"(cbits),
                 [lds0] "s"(lds0), [wave] "s"(wv), [pre] "n"(PRE ? 1 : 0)
               : "memory", "vcc", "scc", D4_CLOBBER_A, W4_CLOBBER_V, W4_CLOBBER_S);

#ifdef D4_STAMPS
  const unsigned long long st3 = __builtin_amdgcn_s_memtime();
#endif
  if (t + wstep < nitems) {
    // ---- prefetch block: once every wave has left the LDS buffers, request the NEXT item's K / V rows (transit area) and
    // first two tiles; they fly while the accumulators of this item are scaled, summed and stored below
    const Item nx = item(t + wstep);
    asm volatile(".set att_pre, 0\n" D4_ASM_MACROS D4_ASM_MACROS2 R"ASM(
      s_barrier
      D4_SRD_INIT
      D4_KVDMA
      D4_STAGE2
    )ASM" D4_ASM_PURGE D4_ASM_PURGE2
                 :
                 : [voQ0] "v"(voQ0), [voQ1] "v"(voQ1), [voD0] "v"(voD0), [voD1] "v"(voD1), [voC] "v"(voC), [voKp] "v"(nx.voKp), [voVp] "v"(nx.voVp), [rb] "v"(rb), [bK] "s"(nx.bK), [bV] "s"(nx.bV), [bQ] "s"(nx.bQ),
                   [bD] "s"(nx.bD), [bL] "s"(nx.bL), [bT] "s"(nx.bT), [tq] "s"(tq), [tk] "s"(tk), [ldk2] "s"(ldk2), [ldv2] "s"(ldv2),
                   [stQ] "s"(stQ), [stD] "s"(stD), [lds0] "s"(lds0), [wave] "s"(wv), [c] "s"(cbits)
                 : "memory", "scc", "v29", "v30", W4_CLOBBER_S, W4_A8(13), W4_A8(14), W4_A8(15), W4_A8(16), W4_A8(17), W4_A8(18), "a128", "a129", "a190", "a191");
  }
#ifdef D4_STAMPS
  const unsigned long long st3b = __builtin_amdgcn_s_memtime();
#endif

  // ---- epilogue: lane (r, h) holds dK / dV [key kw0 + 32 kb + r][d = 32 db + 8 a + 4 h + e] in register 4 a + e of (kb, db).
  // Lanes r and r + 32 hold the two halves of each 8-column group a: one v_permlane32_swap per dword hands lane (r, 0) all of
  // group 2 m and lane (r, 1) all of group 2 m + 1 -> 16-byte stores (4 per tensor and key block instead of 16 8-byte ones)
  auto row16 = [&](const f32x16& acc, int m, float mul) {
    const unsigned x0 = pack2bf(acc[8 * m] * mul, acc[8 * m + 1] * mul), x1 = pack2bf(acc[8 * m + 2] * mul, acc[8 * m + 3] * mul);
    const unsigned y0 = pack2bf(acc[8 * m + 4] * mul, acc[8 * m + 5] * mul), y1 = pack2bf(acc[8 * m + 6] * mul, acc[8 * m + 7] * mul);
    const auto s0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false), s1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
    u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
    return o;
  };
  auto store = [&](auto kbc) {
    constexpr int kb = decltype(kbc)::value;
    const int kb0 = kw0 + 32 * kb, ki = kb0 + r;
    f32x16 dk[2], dv[2];
    dk[0] = w4_get16<64 * kb>(); dk[1] = w4_get16<64 * kb + 16>();
    dv[0] = w4_get16<64 * kb + 32>(); dv[1] = w4_get16<64 * kb + 48>();
    unsigned short* dkrow = p.dk + (long)b * p.dk_bs + (long)ki * p.lddk + hd * 64;
    unsigned short* dvrow = p.dv + (long)b * p.dv_bs + (long)ki * p.lddv + hd * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int d = 32 * db + 8 * (2 * m + h);
        const u32x4 pk = row16(dk[db], m, p.ls), pv = row16(dv[db], m, 1.0f);  // (every lane takes part in the swaps)
        if (ki < p.Tk) {
          *(u32x4*)(dkrow + d) = pk;
          *(u32x4*)(dvrow + d) = pv;
        }
      }
    if (p.cs_v && kb0 < p.Tk) {  // v-projection bias gradient: column sums over the block's 32 keys of the bf16 values written.
      // Halving butterfly over the 32 lanes of a half-wave: a lane keeps the half of its values its lane bit selects and adds
      // the partner's copy of that half — 31 exchanges for 32 sums (att_colsum_store: 160), same pairing, same bits.
      float cv[32];
      const bool ok = ki < p.Tk;
#pragma unroll
      for (int i = 0; i < 32; ++i) cv[i] = ok ? bf2f(f2bf(dv[i >> 4][i & 15])) : 0.f;
#pragma unroll
      for (int m = 16; m >= 1; m >>= 1) {
        const bool up = (r & m) != 0;
#pragma unroll
        for (int i = 0; i < m; ++i) {
          const float keep = up ? cv[i + m] : cv[i], send = up ? cv[i] : cv[i + m];
          cv[i] = keep + __shfl_xor(send, m, 64);
        }
      }
      // lane r now holds value index r = 16 db + 4 a + e, i.e. column 32 db + 8 a + 4 h + e
      float* dst = p.cs_v + ((long)b * ((p.Tk + 31) >> 5) + (kb0 >> 5)) * (p.H * 64) + hd * 64;
      dst[32 * (r >> 4) + 8 * ((r >> 2) & 3) + 4 * h + (r & 3)] = cv[0];
    }
  };
#ifdef D4_STAMPS
  unsigned long long st1, st2;
  asm volatile("s_mov_b64 %0, s[76:77]\n s_mov_b64 %1, s[78:79]" : "=s"(st1), "=s"(st2));
#endif
  store(IntC<0>{});
  store(IntC<1>{});
#ifdef D4_STAMPS
  const unsigned long long st4 = __builtin_amdgcn_s_memtime();
  if (tid == 0) {
    const int o = (t == w0) ? 0 : 8;  // first item of a workgroup | later items
    atomicAdd(&d4_dbg[o + 0], 1ull);
    atomicAdd(&d4_dbg[o + 1], st1 - st0);  // prologue: descriptors, (first item: requests), zeroing, wait, barrier
    atomicAdd(&d4_dbg[o + 2], st2 - st1);  // block 0 + the iteration loop
    atomicAdd(&d4_dbg[o + 3], st3 - st2);  // last dV / dK, drain
    atomicAdd(&d4_dbg[o + 4], st3b - st3);  // prefetch block
    atomicAdd(&d4_dbg[o + 5], st4 - st3b);  // accumulator read-back, column sums, stores (not drained)
  }
  st0 = st4;
#endif
  }  // work items of this workgroup
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Which dK/dV kernel: 0 (default) the one-wave-per-SIMD kernel where it applies, 1 always the 8-wave kernel: WFT_DKDV_VARIANT=8w|4w at
// load time (timing builds); per call: wft_attn_args.variant bit 4.
static int g_dkdv_variant = [] { const char* e = wft_dev_getenv("WFT_DKDV_VARIANT"); return (e && !strcmp(e, "8w")) ? 1 : 0; }();
// non-causal sweeps over at least two 64-query tiles
bool wft_dkdv4w_eligible(const wft_attn_args* a) {
  return g_dkdv_variant == 0 && !(a->variant & 4) && !a->causal && a->Tq >= 128 && attn_offsets_fit32(a);
}
int wft_dkdv4w_launch(const AttnP& p, dim3 grid, hipStream_t s) {
  return !p.qpre ? wft_launch_lds<attn_bwd_dkdv4w_kernel<false>>(grid, dim3(256), D4_LDS, s, p)
                 : wft_launch_lds<attn_bwd_dkdv4w_kernel<true>>(grid, dim3(256), D4_LDS, s, p);
}
