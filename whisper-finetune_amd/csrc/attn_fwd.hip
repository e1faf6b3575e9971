// attn_fwd.hip — attn_fwd_kernel, its software-pipelined form attn_fwd_pipe_kernel, the rule that chooses between them, their launch
#include "attn_common.h"
#ifdef FWD_STAMPS  // developer build (tools/dev/fwd_stamps.py, make ATTN_DEFS=-DFWD_STAMPS): clock-tick sums per phase of a key tile, all active waves
__device__ unsigned long long fwd_dbg[16];
extern "C" void wft_fwd_dbg_read(unsigned long long* host, int reset) {
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(fwd_dbg), z, sizeof z); return; }
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(fwd_dbg), 16 * sizeof(unsigned long long));
}
// stamp phase I behind the value DEP (a dependent v_mov makes the hardware wait for DEP's producer, e.g. an MFMA chain)
#define FWD_STAMP(I, DEP)                                                                                  \
  do {                                                                                                     \
    unsigned long long now_;                                                                               \
    asm volatile("v_mov_b32 %1, %1\n s_nop 0\n s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(now_), "+v"(DEP)); \
    fst[I] += now_ - flast;                                                                                \
    flast = now_;                                                                                          \
  } while (0)
#else
#define FWD_STAMP(I, DEP) do {} while (0)
#endif

// ------------------------------------------------------------------------------ forward
// K/V tiles travel through a THREE-slot LDS ring, staged two tiles ahead of their use, and the end-of-tile
// wait is a counted s_waitcnt vmcnt(4) (this wave's 4 LDS-DMA instructions of tile kt+2 may stay in flight).
// The transposed V reads are inline asm: with the builtin, hipcc drains every outstanding LDS-DMA
// (s_waitcnt vmcnt(0)) in front of the first ds_read_b64_tr of each tile, which cut the prefetch distance to
// half a tile and left the kernel latency-bound (no-load experiment: +27 %).
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[3 * 16384];  // [slot 3][K 8K | V 8K]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: conditions on it are scalar branches, not exec masks
  const int r = lane & 31, h = lane >> 5;
  int bx, hd, b;
  att_block_coords((p.Tq + 127) >> 7, p.H, p.B, p.xcd, bx, hd, b);
  const int q0 = bx * 128;
  const int qw0 = q0 + wave * 32;
  const int qi = qw0 + r;
  const int qc = qi < p.Tq ? qi : p.Tq - 1;
  const unsigned short* qrow = p.q + (long)b * p.q_bs + (long)qc * p.ldq + hd * 64;
  const unsigned short* kb = p.k + (long)b * p.k_bs + hd * 64;
  const unsigned short* vb = p.v + (long)b * p.v_bs + hd * 64;
  // (q_prescaled: c = 1.0 at run time.  A template instantiation without the multiplies measured 1 % SLOWER — 1 417 -> 1 432 us per
  // encoder call at 87 clips, three runs; the compiler's schedule, not the instruction count, decides here: profiles/r06_attn_prescale.md)
  const float c = p.c;
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = att_load_reg_frag(qrow, s, h);
  const AttOffs offs = att_offsets(lane);
  const AttStage stK = att_stage_init(p.ldk, wave, lane), stV = att_stage_init(p.ldv, wave, lane);
  const unsigned lds0 = lds_addr_of(smem);
  unsigned tra[2][2];  // absolute LDS byte addresses of the transposed reads in slot 0's K tile
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int t = 0; t < 2; ++t) tra[db][t] = lds0 + offs.tr[db][t];

  int nkt = (p.Tk + 63) >> 6;
  if (p.causal) {
    const int last = (q0 + 127) / 64 + 1;
    nkt = nkt < last ? nkt : last;
  }
  const f32x16 zero16 = f32x16{0};
  f32x16 oacc[2];
  oacc[0] = zero16;
  oacc[1] = zero16;
  // Lazy rescaling: `m` is a STALE running maximum (raw q.k units) that enters the S MFMA chains as their initial
  // accumulator (minit = -m in every register: S' = S - m costs no VALU), and is only raised when a tile's maximum exceeds
  // it by more than ATT_TAU in log2 units (P <= 2^ATT_TAU is exact in bf16's exponent range; l is fp32).  Most tiles then
  // skip the subtraction, the O rescale and the alpha exponential: the kernel is VALU-issue-bound (v_exp_f32 8 cycles,
  // everything else 4).  Same sums as the eager form up to fp32 rounding of l and O.
  float m = 0.f, l = 0.f;
  f32x16 minit = zero16;
#ifdef FWD_STAMPS
  unsigned long long fst[8] = {0, 0, 0, 0, 0, 0, 0, 0}, flast = __builtin_amdgcn_s_memtime(), fbegin = flast;
#endif

  att_stage2(stK, kb, p.ldk, smem, stV, vb, p.ldv, smem + 8192, 0, p.Tk, wave, lane);
  if (nkt > 1) {
    att_stage2(stK, kb, p.ldk, smem + 16384, stV, vb, p.ldv, smem + 16384 + 8192, 64, p.Tk, wave, lane);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  bf16x8 kf[2][4];  // K row fragments of the CURRENT tile; refilled for the next tile behind the mid-tile barrier
#pragma unroll
  for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[kb2][s] = att_row_frag(smem, offs, kb2, s);

  // One tile = [stage kt+2 | V^T reads | S MFMAs | softmax | wait + barrier | K reads of kt+1 | PV MFMAs]: every LDS
  // read is issued a phase ahead of its use, and the only barrier sits where tile kt+1 must have landed.
  auto tile = [&](auto cur_tag, int kt) {
    constexpr int CUR = decltype(cur_tag)::value;
    constexpr int NXT = (CUR + 1) % 3, NXT2 = (CUR + 2) % 3;
    const int key0 = kt * 64;
    const bool more = kt + 2 < nkt;
    if (more)
      att_stage2(stK, kb, p.ldk, smem + NXT2 * 16384, stV, vb, p.ldv, smem + NXT2 * 16384 + 8192, key0 + 128, p.Tk, wave, lane);
    // (a wave whose 32 queries all lie past the sequence end — T = 1500: the fourth wave of the last 128-query block — only
    // stages and keeps the barriers)
    const bool active = qw0 < p.Tq && !(p.causal && key0 > qw0 + 31);
    s16x4 vt[4][2][2];
    bf16x8 pf[4];
    FWD_STAMP(0, m);  // tile entry -> stage issue done
    if (active) {
      static_for<4>([&](auto ks_tag) {  // the k-step's 2048-byte stride rides in the immediate: no address add per read
        constexpr int ks = decltype(ks_tag)::value;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int t = 0; t < 2; ++t) vt[ks][db][t] = att_tr_asm<CUR * 16384 + 8192 + ks * 2048>(tra[db][t]);
      });
      f32x16 sacc[2];
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][0], qf[0], minit, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < 4; ++s) sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][s], qf[s], sacc[kb2], 0, 0, 0);
      }
      // mask (only tiles that touch the ragged end / the causal diagonal: wave-uniform branch, selects inside)
      if ((key0 + 64 > p.Tk) || (p.causal && key0 + 63 > qw0)) {
        const int lim = (p.causal ? (qi + 1 < p.Tk ? qi + 1 : p.Tk) : p.Tk) - key0 - 4 * h;  // valid iff key offset < lim
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            sacc[kb2][e] = (32 * kb2 + (e & 3) + 8 * (e >> 2)) < lim ? sacc[kb2][e] : ATT_NEG;
      }
      FWD_STAMP(1, sacc[1][15]);  // V^T read issue + S MFMA chains complete
      float tmax = att_xhalf_max(att_max32(sacc[0], sacc[1]));  // max over the tile of S - m
      FWD_STAMP(2, tmax);  // maximum (in-lane tree + half exchange)
      if (kt == 0 || __builtin_amdgcn_ballot_w64(tmax * c > ATT_TAU) != 0) {
        // rare path: move the reference maximum (first tile: to the tile's own maximum, whatever its sign)
        const float d = kt == 0 ? tmax : fmaxf(tmax, 0.f);
        const float alpha = __builtin_amdgcn_exp2f(-d * c);
        m += d;
        l *= alpha;
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 16; ++e) sacc[kb2][e] -= d;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) minit[e] = -m;
      }
      float ls0 = 0.f, ls1 = 0.f;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const float p0 = __builtin_amdgcn_exp2f(sacc[kb2][e] * c);
          const float p1 = __builtin_amdgcn_exp2f(sacc[kb2][e + 1] * c);
          ls0 += p0;
          ls1 += p1;
          sacc[kb2][e] = p0;
          sacc[kb2][e + 1] = p1;
        }
      l += att_xhalf_sum(ls0 + ls1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) pf[ks] = att_pack8(sacc[ks >> 1], ks & 1);
      FWD_STAMP(3, l);  // (rescale branch,) exponentials, row sums, packs
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    FWD_STAMP(4, m);  // own LDS-DMA pieces of tile kt+1 landed, V^T fragments landed
    __builtin_amdgcn_s_barrier();
    FWD_STAMP(5, m);  // barrier
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nkt) {
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[kb2][s] = att_row_frag(smem + NXT * 16384, offs, kb2, s);
    }
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int db = 0; db < 2; ++db)
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_join(vt[ks][db][0], vt[ks][db][1]), pf[ks], oacc[db], 0, 0, 0);
      FWD_STAMP(6, oacc[1][15]);  // K fragment reads of tile kt+1 issued + P.V MFMA chains complete
    }
  };
  int kt = 0;
  for (; kt + 2 < nkt; kt += 3) {
    tile(IntC<0>{}, kt);
    tile(IntC<1>{}, kt + 1);
    tile(IntC<2>{}, kt + 2);
  }
  if (kt < nkt) tile(IntC<0>{}, kt);
  if (kt + 1 < nkt) tile(IntC<1>{}, kt + 1);

  if (qi < p.Tq) {
    const float inv = 1.0f / l;
    unsigned short* orow = p.o + (long)b * p.o_bs + (long)qi * p.ldo + hd * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int d = 32 * db + 8 * a + 4 * h;
        u32x2 pk = {pack2bf(oacc[db][4 * a] * inv, oacc[db][4 * a + 1] * inv),
                    pack2bf(oacc[db][4 * a + 2] * inv, oacc[db][4 * a + 3] * inv)};
        *(u32x2*)(orow + d) = pk;
      }
    if (h == 0 && p.lse) p.lse[((long)b * p.H + hd) * p.Tq + qi] = m * p.ls + __logf(l);
  }
#ifdef FWD_STAMPS
  if (lane == 0 && qw0 < p.Tq) {
    for (int i = 0; i < 7; ++i) atomicAdd(&fwd_dbg[i], fst[i]);
    atomicAdd(&fwd_dbg[8], 1ull);
    atomicAdd(&fwd_dbg[9], __builtin_amdgcn_s_memtime() - fbegin);
    atomicAdd(&fwd_dbg[10], (unsigned long long)nkt);
  }
#endif
}


// Round 6: the softmax's vector section of the pipelined forward kernel runs at raised wave priority (s_setprio 1).  Two waves of
// DIFFERENT workgroups share a SIMD at an arbitrary phase; the arbiter is oldest-first, so without it the wave that is in its exponentials
// keeps losing issue slots to its partner's MFMA issue and both drift into phase.  Measured, alternating, three runs (encoder call at 87
// clips, prescaled q): 1 508 / 1 517 / 1 500 us -> 1 477 / 1 468 / 1 504 (-1.7 %); priority on the MFMA clusters instead: +-0.
// No arithmetic changes: bit-identical outputs (tests/test_attn_fwd_pipe_gpu.py).
#define FWD_PRIO_VALU_ON __builtin_amdgcn_s_setprio(1)
#define FWD_PRIO_VALU_OFF __builtin_amdgcn_s_setprio(0)
// ------------------------------------------------------------------------------ forward, software-pipelined (round 5)
// The ablation builds of attn_fwd_kernel (profiles/r05_attn_fwd.md; their switches are gone from the source) behaved like a SUM of their parts: taking out the S
// MFMAs saves 29 % of the kernel, the softmax's vector work 24 %, the P.V MFMAs 11 %, the LDS-DMA staging 13 %, the V^T reads
// 13 % — a wave issues its S chains and then sits on their results, and with the oldest-wave-first arbiter the second wave of the
// SIMD does not fill that hole reliably.  Here the S chains of tile kt+1 are issued BEHIND the softmax of tile kt and IN FRONT of
// its P.V chains: they run on the matrix pipe while the wave goes through the end-of-tile wait, the barrier, the next tile's
// staging and V^T reads, and tile kt+1's softmax finds its scores finished.  That needs tile kt+1's K fragments one barrier
// earlier, so the K/V ring has FOUR slots and is staged three tiles ahead (64 KiB per workgroup, two workgroups per CU):
//   iteration kt: stage kt+3 | V^T(kt) reads | softmax(kt) -> P | S(kt+1) MFMAs | wait own pieces of kt+2, barrier |
//                 K(kt+2) fragment reads | P.V(kt) MFMAs
// Same arithmetic in the same order as attn_fwd_kernel (the stale maximum that enters S(kt+1) as its initial accumulator is the
// one softmax(kt) has just settled, exactly what the un-pipelined kernel uses at the head of tile kt+1): bit-identical results.
__global__ __launch_bounds__(256, 2) void attn_fwd_pipe_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 16384];  // [slot 4][K 8K | V 8K]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  int bx, hd, b;
  att_block_coords((p.Tq + 127) >> 7, p.H, p.B, p.xcd, bx, hd, b);
  const int q0 = bx * 128;
  const int qw0 = q0 + wave * 32;
  const int qi = qw0 + r;
  const int qc = qi < p.Tq ? qi : p.Tq - 1;
  const unsigned short* qrow = p.q + (long)b * p.q_bs + (long)qc * p.ldq + hd * 64;
  const unsigned short* kb = p.k + (long)b * p.k_bs + hd * 64;
  const unsigned short* vb = p.v + (long)b * p.v_bs + hd * 64;
  const float c = p.c;  // (see attn_fwd_kernel)
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = att_load_reg_frag(qrow, s, h);
  const AttOffs offs = att_offsets(lane);
  const AttStage stK = att_stage_init(p.ldk, wave, lane), stV = att_stage_init(p.ldv, wave, lane);
  const unsigned lds0 = lds_addr_of(smem);
  unsigned tra[2][2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int t = 0; t < 2; ++t) tra[db][t] = lds0 + offs.tr[db][t];

  int nkt = (p.Tk + 63) >> 6;
  if (p.causal) {
    const int last = (q0 + 127) / 64 + 1;
    nkt = nkt < last ? nkt : last;
  }
  const f32x16 zero16 = f32x16{0};
  f32x16 oacc[2];
  oacc[0] = zero16;
  oacc[1] = zero16;
  float m = 0.f, l = 0.f;
  f32x16 minit = zero16;
  auto is_active = [&](int kt) { return qw0 < p.Tq && !(p.causal && kt * 64 > qw0 + 31); };

  // prologue: tiles 0, 1, 2 on their way; tiles 0 and 1 certified by the first barrier
  att_stage2(stK, kb, p.ldk, smem, stV, vb, p.ldv, smem + 8192, 0, p.Tk, wave, lane);
  if (nkt > 1) att_stage2(stK, kb, p.ldk, smem + 16384, stV, vb, p.ldv, smem + 16384 + 8192, 64, p.Tk, wave, lane);
  if (nkt > 2) {
    att_stage2(stK, kb, p.ldk, smem + 2 * 16384, stV, vb, p.ldv, smem + 2 * 16384 + 8192, 128, p.Tk, wave, lane);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  bf16x8 kf[2][4];  // K row fragments of the NEXT tile to be multiplied
  f32x16 sacc[2];   // scores of the CURRENT tile (S chains issued one tile ahead)
#pragma unroll
  for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[kb2][s] = att_row_frag(smem, offs, kb2, s);
  sacc[0] = sacc[1] = zero16;
  if (is_active(0)) {
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2) {
      sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][0], qf[0], minit, 0, 0, 0);
#pragma unroll
      for (int s = 1; s < 4; ++s) sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][s], qf[s], sacc[kb2], 0, 0, 0);
    }
  }
  if (nkt > 1) {
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[kb2][s] = att_row_frag(smem + 16384, offs, kb2, s);
  }

  auto tile = [&](auto cur_tag, int kt) {
    constexpr int CUR = decltype(cur_tag)::value;
    constexpr int NXT2 = (CUR + 2) % 4, NXT3 = (CUR + 3) % 4;
    const int key0 = kt * 64;
    const bool more = kt + 3 < nkt;
    if (more)
      att_stage2(stK, kb, p.ldk, smem + NXT3 * 16384, stV, vb, p.ldv, smem + NXT3 * 16384 + 8192, key0 + 192, p.Tk, wave, lane);
    const bool active = is_active(kt);
    s16x4 vt[4][2][2];
    bf16x8 pf[4];
    if (active) {
      static_for<4>([&](auto ks_tag) {
        constexpr int ks = decltype(ks_tag)::value;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int t = 0; t < 2; ++t) vt[ks][db][t] = att_tr_asm<CUR * 16384 + 8192 + ks * 2048>(tra[db][t]);
      });
      if ((key0 + 64 > p.Tk) || (p.causal && key0 + 63 > qw0)) {
        const int lim = (p.causal ? (qi + 1 < p.Tk ? qi + 1 : p.Tk) : p.Tk) - key0 - 4 * h;
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            sacc[kb2][e] = (32 * kb2 + (e & 3) + 8 * (e >> 2)) < lim ? sacc[kb2][e] : ATT_NEG;
      }
      const float tmax = att_xhalf_max(att_max32(sacc[0], sacc[1]));
      if (kt == 0 || __builtin_amdgcn_ballot_w64(tmax * c > ATT_TAU) != 0) {
        const float d = kt == 0 ? tmax : fmaxf(tmax, 0.f);
        const float alpha = __builtin_amdgcn_exp2f(-d * c);
        m += d;
        l *= alpha;
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int e = 0; e < 16; ++e) sacc[kb2][e] -= d;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) minit[e] = -m;
      }
      float ls0 = 0.f, ls1 = 0.f;
      FWD_PRIO_VALU_ON;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const f32x2 sc = f32x2{sacc[kb2][e], sacc[kb2][e + 1]} * c;  // (one v_pk_mul_f32 per pair: hipcc leaves the scalar form unpacked)
          const float p0 = __builtin_amdgcn_exp2f(sc[0]);
          const float p1 = __builtin_amdgcn_exp2f(sc[1]);
          ls0 += p0;
          ls1 += p1;
          sacc[kb2][e] = p0;
          sacc[kb2][e + 1] = p1;
        }
      l += att_xhalf_sum(ls0 + ls1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) pf[ks] = att_pack8(sacc[ks >> 1], ks & 1);
      FWD_PRIO_VALU_OFF;
    }
    // the NEXT tile's scores: on the matrix pipe from here, consumed by the next iteration's softmax
    if (kt + 1 < nkt && is_active(kt + 1)) {
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][0], qf[0], minit, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < 4; ++s) sacc[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb2][s], qf[s], sacc[kb2], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 2 < nkt) {
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[kb2][s] = att_row_frag(smem + NXT2 * 16384, offs, kb2, s);
    }
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int db = 0; db < 2; ++db)
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att_join(vt[ks][db][0], vt[ks][db][1]), pf[ks], oacc[db], 0, 0, 0);
    }
  };
  int kt = 0;
  for (; kt + 3 < nkt; kt += 4) {
    tile(IntC<0>{}, kt);
    tile(IntC<1>{}, kt + 1);
    tile(IntC<2>{}, kt + 2);
    tile(IntC<3>{}, kt + 3);
  }
  if (kt < nkt) tile(IntC<0>{}, kt);
  if (kt + 1 < nkt) tile(IntC<1>{}, kt + 1);
  if (kt + 2 < nkt) tile(IntC<2>{}, kt + 2);

  if (qi < p.Tq) {
    const float inv = 1.0f / l;
    unsigned short* orow = p.o + (long)b * p.o_bs + (long)qi * p.ldo + hd * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int d = 32 * db + 8 * a + 4 * h;
        u32x2 pk = {pack2bf(oacc[db][4 * a] * inv, oacc[db][4 * a + 1] * inv),
                    pack2bf(oacc[db][4 * a + 2] * inv, oacc[db][4 * a + 3] * inv)};
        *(u32x2*)(orow + d) = pk;
      }
    if (h == 0 && p.lse) p.lse[((long)b * p.H + hd) * p.Tq + qi] = m * p.ls + __logf(l);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// Forward kernel choice: 0 (default) = attn_fwd_pipe_kernel (software-pipelined: S of tile kt+1 behind the softmax of tile kt) for
// non-causal calls with Tk >= 512 — the encoder — and attn_fwd_kernel for the rest (the short key ranges of the decoder: the
// four-slot ring's longer prologue costs 2-5 % there); 1 = attn_fwd_kernel everywhere.  Bit-identical results either way.
// (Round 4's one-wave-per-SIMD forward kernel measured equal to attn_fwd_kernel and was removed in round 5.)
static int g_fwd_variant = [] { const char* e = wft_dev_getenv("WFT_FWD_VARIANT"); return (e && !strcmp(e, "8w")) ? 1 : 0; }();
bool wft_fwd_pipe_eligible(const wft_attn_args* a) {
  static const int min_tk = [] { const char* e = wft_dev_getenv("WFT_FWDPIPE_MIN_TK"); return e ? atoi(e) : 512; }();
  return g_fwd_variant == 0 && !(a->variant & 1) && !a->causal && a->Tk >= min_tk;
}
void wft_attn_fwd_launch(const AttnP& p, bool pipe, dim3 grid, hipStream_t s) {
  if (pipe) hipLaunchKernelGGL(attn_fwd_pipe_kernel, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(attn_fwd_kernel, grid, dim3(256), 0, s, p);
}
