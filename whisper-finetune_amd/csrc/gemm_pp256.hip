// gemm_pp256.hip — the 8-wave ping-pong 256x256 kernels: gemm_nt256_kernel (C = A · B^T; the fallback for the epilogues the
// one-wave-per-SIMD kernel of gemm_nt4w.hip does not carry) with the reduce kernel of its fused column sums, and
// gemm_tn256_kernel (weight gradients; wft_gemm_args.variant = 1 or a split-K call without a workspace).  Which calls take a
// 256x256 tile at all is decided by nt_uses_256 / tn_uses_256 (gemm.hip).
// (The two kernels stay in ONE file, NT first: compiled alone, gemm_tn256_kernel gets another scalar-register assignment.)
#include "gemm_common.h"
#ifndef WFT_EPI_PF_CNT
#define WFT_EPI_PF_CNT 4
#endif

// ---------------------------------------------------------------------------------- NT 256x256
// Large-shape variant: 256x256 output tile, 512 threads (8 waves as 2(M) x 4(N), 128x64 per wave), one
// workgroup per CU, LDS = ring of four 32-deep k-slabs (4 x {A [256][32], B [256][32]} = 128 KiB).
//
// Measured on the first version (all waves in lockstep, 64-deep tiles): the MFMA pipe was busy 44 % of
// the time; removing the global_load_lds (timing-only build) gave +38 %, i.e. the ~100-cycle issue cost
// of each LDS-DMA instruction was serialised in front of the MFMAs of BOTH waves of a SIMD.  This version
// is a ping-pong: waves 0-3 and 4-7 (SIMD partners) run half a period apart, separated by s_barrier —
//   L-unit: issue 4 global_load_lds (this wave's share of slab u+3) + 12 ds_read_b128 (slab u fragments)
//   C-unit: 32 MFMAs (16x16x32 bf16) on those fragments
// so one partner's loads always sit beside the other partner's MFMAs.  Loads run three slabs (six
// half-periods) ahead behind a COUNTED s_waitcnt vmcnt(8): never drained inside the loop.
__device__ __forceinline__ int nt_g(int row) { return (4 - ((row >> 2) & 3)) & 3; }  // 64-byte-row swizzle

// s_waitcnt for row h of the NT256 epilogue's register ring in its COUNTED body (the asm ties the wait to the registers it
// guards; there is exactly one such statement per half-pass, on no branch).  Vector-memory operations younger than row h's
// load when half-pass h starts — ST stores per half-pass, one ring load per row issued at the end of half-pass h - PF (rows
// 0 .. PF-1 in a prologue); the next tile's LDS-DMA pieces are older than all of them (main-loop tail or before the body):
//   h < PF : rows h+1 .. PF-1, then ST + 1 per half-pass before h
//   h >= PF: half-passes h-PF+1 .. h-1: ST, + 1 while rows remain (j + PF < 16)
template <int ST, int PF>
__device__ __forceinline__ void nt_wait_ring(int h, u32x4& q) {
  int n = 0;
  if (h < PF) n = (PF - 1 - h) + h * (ST + 1);
  else for (int j = h - PF + 1; j < h; ++j) n += ST + (j + PF < 16 ? 1 : 0);
#define WFT_VM_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(q) :: "memory"); break;
  switch (n) {  // h is a compile-time constant after unrolling: one case survives
    WFT_VM_CASE(1) WFT_VM_CASE(2) WFT_VM_CASE(3) WFT_VM_CASE(4) WFT_VM_CASE(5) WFT_VM_CASE(6) WFT_VM_CASE(7) WFT_VM_CASE(8) WFT_VM_CASE(9) WFT_VM_CASE(10) WFT_VM_CASE(11) WFT_VM_CASE(12) WFT_VM_CASE(13) WFT_VM_CASE(14) WFT_VM_CASE(15) WFT_VM_CASE(16) WFT_VM_CASE(17) WFT_VM_CASE(18) WFT_VM_CASE(19) WFT_VM_CASE(20) WFT_VM_CASE(21) WFT_VM_CASE(22) WFT_VM_CASE(23) WFT_VM_CASE(24) WFT_VM_CASE(25) WFT_VM_CASE(26) WFT_VM_CASE(27) WFT_VM_CASE(28) WFT_VM_CASE(29) WFT_VM_CASE(30) WFT_VM_CASE(31) WFT_VM_CASE(32) WFT_VM_CASE(33) WFT_VM_CASE(34) WFT_VM_CASE(35) WFT_VM_CASE(36) WFT_VM_CASE(37) WFT_VM_CASE(38) WFT_VM_CASE(39) WFT_VM_CASE(40)
    default: asm volatile("s_waitcnt vmcnt(0)" : "+v"(q) :: "memory"); break;
  }
#undef WFT_VM_CASE
}

// WFT_NT_RING slots of 32 KiB (A [256][32] | B [256][32]), LDS-DMA running WFT_NT_RING - 1 slabs ahead of the reads.
// 4 (default): lookahead 3 and a separate 32 KiB staging area for the epilogue.  5 (round 3, built and measured): all 160 KiB are
// ring, lookahead 4 (3.1 us instead of 2.3), slot numbers run on across tiles and the staged epilogue borrows the one slot that
// is free at the seam (the slot of the tile's last slab: the next tile's slabs 0-3 sit in the other four, slab 4 is staged into
// it by the next tile's first L-unit, behind the tile-start barrier).  With operands streamed from HBM (a GEMM run back to back
// on 261 MB activations) the deeper lookahead is worth +3-6 % — in-kernel stamps had shown tiles that open a fresh A panel
// 25 % slower than the others; inside the training step the operands were written just before and come from the Infinity
// Cache: 700.1 vs 701.7 ms per step, no gain (profiles/r03_nt256_ring5_ab.log, r03_step_ring_ab.log).
#ifndef WFT_NT_RING
#define WFT_NT_RING 4
#endif
template <int EPI, bool C_F32>
__global__ __launch_bounds__(512, 2) void gemm_nt256_kernel(GemmP p) {
  constexpr int NSLOT = WFT_NT_RING, LA = NSLOT - 1;  // ring slots, lookahead in slabs
  extern __shared__ __attribute__((aligned(16))) char dsmem[];  // the ring (+ 32 KiB epilogue staging when NSLOT == 4)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const bool grp_b = wave >= 4;
  const int tiles_n = p.N >> 8;
  const int tiles_m = (p.M + 255) >> 8;
  const int tiles = tiles_m * tiles_n;
  const int total = tiles * p.batch;

  // staging share of this wave: group A (waves 0-3) loads the A part of every slab, group B the B part;
  // wave-instruction = 16 rows x 64 B; this wave owns rows 64*(wave&3) .. +63 of its part (4 instructions)
  const int rr = lane >> 2, cc = lane & 3;
  // Source address of an LDS-DMA piece = wave-uniform tile base (SGPR pair, advanced per slab on the scalar unit) + a
  // per-lane 32-bit byte offset that is constant for the tile: the `saddr + voffset` form, NO vector instruction per
  // piece.  (In-kernel stamps: the 12 reads + 4 pieces of an L-unit took 560-820 cycles to ISSUE — the partner wave's
  // MFMAs run at s_setprio 1 and starve this wave's address arithmetic on the shared VALU port.)
  const char* sbase;
  unsigned soff[4];
  auto set_src = [&](int t) {  // PERSISTENT: tile t of this workgroup's sequence
    const int bz = t / tiles, sid = xcd_remap(t - bz * tiles, tiles);
    int tm, tn;
    band_coords(sid, tiles_m, tiles_n, tm, tn, p.band);
    const unsigned long long b64 = !grp_b ? (unsigned long long)(p.A + (long)bz * p.sA + (long)(tm << 8) * p.lda)
                                          : (unsigned long long)(p.B + (long)bz * p.sB + (long)(tn << 8) * p.ldb);
    // pin the base to SGPRs (it is wave-uniform by construction; the compiler does not prove it through the tile loop)
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b64), hi = __builtin_amdgcn_readfirstlane((unsigned)(b64 >> 32));
    sbase = (const char*)(((unsigned long long)hi << 32) | lo);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int row = (wave & 3) * 64 + j * 16 + rr;
      const int chunk = cc ^ nt_g(rr);
      if (!grp_b) {
        const int last = p.M - 1 - (tm << 8);  // clamp to the last valid row of A
        row = row < last ? row : last;
        soff[j] = (unsigned)(row * (int)p.lda + chunk * 8) * 2u;
      } else {
        soff[j] = (unsigned)(row * (int)p.ldb + chunk * 8) * 2u;
      }
    }
  };
  const unsigned stage_dst = __builtin_amdgcn_readfirstlane(lds_addr_of(dsmem) + (grp_b ? 16384 : 0) + (wave & 3) * 4096);
  auto stage = [&](int u, int slot_dst) {  // this wave's 4 KiB of slab u of the tile `sbase` points at -> ring slot slot_dst
    const unsigned dst = stage_dst + slot_dst * 32768;
    const unsigned long long sb = (unsigned long long)sbase + (unsigned long long)u * 64;  // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16_saddr(soff[j], sb, dst + j * 1024);
  };

  const int nslab = p.K >> 5;
  const int frow = lane & 15, fg = lane >> 4;
  const int coff = (fg ^ nt_g(frow)) << 4;
  const int a_off = (wm * 128 + frow) * 64 + coff;
  const int b_off = 16384 + (wn * 64 + frow) * 64 + coff;
  int slot = 0;  // ring slot of the slab the next L-unit reads; runs on across tiles (wave-uniform scalar)
  auto slot_add = [&](int s_, int d) { const int x = s_ + d; return x >= NSLOT ? x - NSLOT : x; };
  auto prefetch = [&]() {  // shares of slabs 0 .. LA-1 of the tile `src` points at, into the slots the next tile will read
#pragma unroll
    for (int j = 0; j < LA; ++j)
      if (j < nslab) stage(j, slot_add(slot, j));
  };

  int t = blockIdx.x;
  if (t >= total) return;
  set_src(t);
  prefetch();

  for (; t < total; t += gridDim.x) {
    const int bz = t / tiles, sid = xcd_remap(t - bz * tiles, tiles);
    int tm, tn;
    band_coords(sid, tiles_m, tiles_n, tm, tn, p.band);
    const int m0 = tm << 8, n0 = tn << 8;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 af[8], bq[4];

    // slab 0 complete (its 4 glds are older than everything issued since: epilogue stores, slabs 1 .. LA-1)
    if (nslab >= LA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (LA - 1)) : "memory");
    else if (nslab == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nslab == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp_b) __builtin_amdgcn_s_barrier();  // group B runs half a period behind group A

    // CONTINUOUS staging: with another tile to come and nslab % 4 == 0 (slab j of the next tile then belongs in the slot
    // slab nslab - 4 + j just left), the last three L-units stage the NEXT tile's slabs 0-2 instead of nothing: the 12
    // LDS-DMA pieces are issued beside the partner group's MFMAs like every other slab, not in the epilogue where both
    // groups pay their issue cost with nothing to hide it (stamps: 1-2 us per tile), and the waits never drain.
    const bool more = t + (int)gridDim.x < total;
    const bool cont = more && (NSLOT == 5 || (nslab & 3) == 0) && nslab >= 8 && p.diag != 8;  // (4 slots: slot = u & 3 needs nslab % 4 == 0)
    for (int u = 0; u < nslab; ++u) {
      // ---------------- L-unit (fragment reads first: their latency hides behind the LDS-DMA issue)
      {
        const char* sl = dsmem + slot * 32768;
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = *(const bf16x8*)(sl + b_off + j * 1024);
#pragma unroll
        for (int i = 0; i < 8; ++i) af[i] = *(const bf16x8*)(sl + a_off + i * 1024);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int sdst = slot == 0 ? NSLOT - 1 : slot - 1;  // slot (u + LA) mod NSLOT: slab u - 1 has just left it
        if (u + LA < nslab) {
          stage(u + LA, sdst);
        } else if (cont) {
          if (u + LA == nslab) set_src(t + gridDim.x);  // this tile's source addresses are not needed any more
          stage(u + LA - nslab, sdst);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // slab u+1's share (issued LA L-units ago) must have landed before the partner group reads it
      const int ahead = nslab - 1 - u;
      if (ahead >= LA || cont) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (LA - 1)) : "memory");
      else if (ahead == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (ahead == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---------------- C-unit
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      slot = slot + 1 == NSLOT ? 0 : slot + 1;
    }
    if (!grp_b) __builtin_amdgcn_s_barrier();  // group A idles through group B's last C-unit
    const int free_slot = slot == 0 ? NSLOT - 1 : slot - 1;  // the tile's last slab has left it; nothing is staged into it before the next tile's first L-unit

    // the ring is free: put the next tile's first three slabs in flight, then write this tile out
    const bool staged = !C_F32 && p.diag != 6;
    constexpr bool RD_AUX = (EPI == WFT_EPI_DGELU || EPI == WFT_EPI_MUL_AUX);
    constexpr bool PF_RES = (EPI == WFT_EPI_NONE || EPI == WFT_EPI_GELU);  // the others (no residual in practice) read it in place: registers
    // COUNTED epilogue body: every vector-memory instruction it issues is known (all 128 rows of the wave valid -> every
    // lane active in every half-pass; one ring load per row; EPI_ST stores per half-pass)
    const bool counted = staged && EPI != WFT_EPI_GELU && m0 + wm * 128 + 128 <= p.M && (PF_RES || !p.res) && p.diag != 7;
    if (more && !cont) {  // (older than everything the epilogue issues: outside its counts)
      set_src(t + gridDim.x);
      prefetch();
    }

    const long cb = (long)bz * p.sC;
    if (staged) {
      // ---- epilogue through the 32 KiB of LDS above the ring (4 KiB per wave, one 16-row m-tile per pass,
      // XOR-swizzled 16-byte chunks): every global access below is 16 bytes per lane, 8 lanes = one full
      // 128-byte line (bias / residual / aux / C) instead of 8-byte pieces of 16 different lines.
      //
      // Residual / aux rows are fetched EPI_PF half-passes ahead of their use into a ring of registers.  In the general
      // body (CNT = false) hipcc places the waits, and with row masks and `if (p.res)` around the loads it falls back to
      // vmcnt(0) in front of every use: each of the 16 half-passes drains its own store and the load issued just before
      // it (in-kernel stamps: 18 us per tile with a residual / aux operand from HBM, 6.5 us store-only, 8.5 us with the
      // operand served from L2; main loop 30 - 120 us).  The COUNTED body issues the ring loads as inline asm and waits
      // with hand-counted s_waitcnt vmcnt(N): the counter retires in issue order (loads, stores, LDS-DMA alike), so "at
      // most N younger operations outstanding" is exact when every operation of the body is known.  The two bodies are
      // separate copies of the code: a register that an asm load is still filling must never be copied, and a wait that
      // exists on one side of a branch only makes hipcc copy the ring at the join.
      char* lds = dsmem + (NSLOT == 4 ? 131072 : free_slot * 32768) + wave * 4096;
      const int er = lane >> 3, ec = (lane & 7) * 8;  // row within an 8-row group, first of this lane's 8 columns
      const int ncol = n0 + wn * 64 + ec;
      auto body = [&](auto cnt_c) {
      constexpr bool CNT = decltype(cnt_c)::value;
      constexpr int EPI_PF = CNT ? WFT_EPI_PF_CNT : 4;  // general body: 6 and 8 spill beside the 128 accumulator registers
      constexpr int EPI_ST = (EPI == WFT_EPI_GELU || EPI == WFT_EPI_GELU_GRAD) ? 2 : 1;  // stores per half-pass (GELU: with aux)
      float bias8[8], cs8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bias8[e] = 0.f; cs8[e] = 0.f; }
      if (p.bias) {
        const f32x4 b0 = *(const f32x4*)(p.bias + ncol), b1 = *(const f32x4*)(p.bias + ncol + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bias8[e] = b0[e]; bias8[4 + e] = b1[e]; }
      }
      // (the counted body of an epilogue that reads the residual in place is only entered without a residual)
      const bool has_res = (CNT && !PF_RES) ? false : (p.res != nullptr);
      const bool ring = RD_AUX || (PF_RES && has_res);
      // row er of this wave's block; later rows = + h * 8 * ld, a wave-uniform step (no 64-bit multiply per access)
      const long row0 = (long)(m0 + wm * 128 + er);
      unsigned short* const c_row0 = (unsigned short*)p.C + cb + row0 * p.ldc + ncol;
      unsigned short* const aux_row0 = p.aux ? p.aux + (long)bz * p.sAux + row0 * p.ldaux + ncol : nullptr;
      const unsigned short* const res_row0 = p.res ? p.res + (long)bz * p.sR + row0 * p.ldr + ncol : nullptr;
      u32x4 auxq[EPI_PF], resq[EPI_PF];
      auto fetch_row = [&](int h, int slot) {
        const int m = m0 + wm * 128 + (h >> 1) * 16 + (h & 1) * 8 + er;
        if (CNT) {  // every row valid
          if (RD_AUX) {
            const unsigned short* src = aux_row0 + (long)(h * 8) * p.ldaux;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(auxq[slot]) : "v"(src) : "memory");
          } else if (PF_RES && has_res) {
            const unsigned short* src = res_row0 + (long)(h * 8) * p.ldr;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(resq[slot]) : "v"(src) : "memory");
          }
        } else if (m < p.M) {
          if (RD_AUX) auxq[slot] = *(const u32x4*)(p.aux + (long)bz * p.sAux + (long)m * p.ldaux + ncol);
          if (PF_RES && has_res) resq[slot] = *(const u32x4*)(p.res + (long)bz * p.sR + (long)m * p.ldr + ncol);
        }
      };
#pragma unroll
      for (int h = 0; h < EPI_PF; ++h) fetch_row(h, h);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          *(f32x4*)(lds + frow * 256 + (((jj * 4 + fg) ^ frow) << 4)) = acc[i][jj];
        // A wave's LDS instructions execute in order: the reads below see these writes, and the next pass's writes cannot
        // overtake the reads, so the COUNTED body needs no wait between them — it issues the four reads of both half-passes
        // at once and lets hipcc place one counted lgkmcnt wait in front of their first use (one LDS round trip per pass
        // instead of three; two waves per SIMD cannot hide them).  The general body keeps the explicit fences.
        if (!CNT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        f32x4 xa[2], xb[2];
        if (CNT) {
#pragma unroll
          for (int g8 = 0; g8 < 2; ++g8) {
            const int lr = g8 * 8 + er, ch = (lane & 7) * 2;
            xa[g8] = *(const f32x4*)(lds + lr * 256 + ((ch ^ lr) << 4));
            xb[g8] = *(const f32x4*)(lds + lr * 256 + (((ch + 1) ^ lr) << 4));
          }
        }
#pragma unroll
        for (int g8 = 0; g8 < 2; ++g8) {
          const int h = i * 2 + g8;
          const int lr = g8 * 8 + er;
          const int m = m0 + wm * 128 + i * 16 + lr;
          const int ch = (lane & 7) * 2;
          const int slot = h % EPI_PF;
          const f32x4 x0 = CNT ? xa[g8] : *(const f32x4*)(lds + lr * 256 + ((ch ^ lr) << 4));
          const f32x4 x1 = CNT ? xb[g8] : *(const f32x4*)(lds + lr * 256 + (((ch + 1) ^ lr) << 4));
          if (CNT && ring) nt_wait_ring<EPI_ST, EPI_PF>(h, RD_AUX ? auxq[slot] : resq[slot]);
          if (CNT || m < p.M) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = x0[e] * p.alpha + bias8[e]; v[4 + e] = x1[e] * p.alpha + bias8[4 + e]; }
            const long roff = (long)m;
            u32x4 r4 = resq[slot];
            if (!PF_RES && has_res) r4 = *(const u32x4*)(p.res + (long)bz * p.sR + roff * p.ldr + ncol);
            if (has_res && p.res_first) {
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[2 * e] += p.beta * bf2f((unsigned short)(r4[e] & 0xffff)); v[2 * e + 1] += p.beta * bf2f((unsigned short)(r4[e] >> 16)); }
            }
            if (EPI == WFT_EPI_GELU) {
              if (p.aux) {
                u32x4 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
                *(u32x4*)(p.aux + (long)bz * p.sAux + roff * p.ldaux + ncol) = pk;
              }
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = gelu_f(v[e]);
            } else if (EPI == WFT_EPI_DGELU) {
              const u32x4 a4 = auxq[slot];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                v[2 * e] *= dgelu_f(bf2f((unsigned short)(a4[e] & 0xffff)));
                v[2 * e + 1] *= dgelu_f(bf2f((unsigned short)(a4[e] >> 16)));
              }
            } else if (EPI == WFT_EPI_GELU_GRAD) {
              float dv[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) gelu_both_f(v[e], v[e], dv[e]);
              u32x4 pk = {pack2bf(dv[0], dv[1]), pack2bf(dv[2], dv[3]), pack2bf(dv[4], dv[5]), pack2bf(dv[6], dv[7])};
              if (CNT) *(u32x4*)(aux_row0 + (long)(h * 8) * p.ldaux) = pk;
              else *(u32x4*)(p.aux + (long)bz * p.sAux + roff * p.ldaux + ncol) = pk;
            } else if (EPI == WFT_EPI_MUL_AUX) {
              const u32x4 a4 = auxq[slot];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                v[2 * e] *= bf2f((unsigned short)(a4[e] & 0xffff));
                v[2 * e + 1] *= bf2f((unsigned short)(a4[e] >> 16));
              }
            }
            if (has_res && !p.res_first) {
#pragma unroll
              for (int e = 0; e < 4; ++e) { v[2 * e] += p.beta * bf2f((unsigned short)(r4[e] & 0xffff)); v[2 * e + 1] += p.beta * bf2f((unsigned short)(r4[e] >> 16)); }
            }
            if (p.period > 0 && (m % p.period) >= p.valid) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
            u32x4 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
            if (CNT) *(u32x4*)(c_row0 + (long)(h * 8) * p.ldc) = pk;
            else *(u32x4*)((unsigned short*)p.C + cb + roff * p.ldc + ncol) = pk;
            if (p.cs_part) {
#pragma unroll
              for (int e = 0; e < 8; ++e) cs8[e] += v[e];
            }
          }
          if (h + EPI_PF < 16) fetch_row(h + EPI_PF, slot);
        }
        if (!CNT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      if (p.cs_part) {  // column sums of this wave's 128 x 64 block: reduce over the 8 row-lanes, lanes 0-7 store 8 columns each
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float t2 = cs8[e];
          t2 += __shfl_xor(t2, 8, 64);
          t2 += __shfl_xor(t2, 16, 64);
          t2 += __shfl_xor(t2, 32, 64);
          cs8[e] = t2;
        }
        if (lane < 8) {
          float* dstp = p.cs_part + (long)(tm * 2 + wm) * p.N + ncol;
          *(f32x4*)dstp = f32x4{cs8[0], cs8[1], cs8[2], cs8[3]};
          *(f32x4*)(dstp + 4) = f32x4{cs8[4], cs8[5], cs8[6], cs8[7]};
        }
      }
      };  // body
      if constexpr (EPI == WFT_EPI_GELU) {  // (conv stem / inference only: its counted copy spills)
        body(std::false_type{});
      } else {
        if (counted) body(std::true_type{}); else body(std::false_type{});
      }
      continue;
    }
    // direct epilogue (fp32 C, accumulate): lane holds C[m][n..n+3] per (i, j)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + wm * 128 + i * 16 + frow;
      if (m >= p.M) continue;
      const bool zero_row = p.period > 0 && (m % p.period) >= p.valid;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + fg * 4;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] * p.alpha;
        if (p.bias) {
          const f32x4 b4 = *(const f32x4*)(p.bias + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += b4[e];
        }
        if (p.res && p.res_first) {
          const u32x2 r2 = *(const u32x2*)(p.res + (long)bz * p.sR + (long)m * p.ldr + n);
          v[0] += p.beta * bf2f((unsigned short)(r2[0] & 0xffff)); v[1] += p.beta * bf2f((unsigned short)(r2[0] >> 16));
          v[2] += p.beta * bf2f((unsigned short)(r2[1] & 0xffff)); v[3] += p.beta * bf2f((unsigned short)(r2[1] >> 16));
        }
        if (EPI == WFT_EPI_GELU) {
          if (p.aux) {
            u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
            *(u32x2*)(p.aux + (long)bz * p.sAux + (long)m * p.ldaux + n) = pk;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = gelu_f(v[e]);
        } else if (EPI == WFT_EPI_DGELU) {
          const u32x2 a2 = *(const u32x2*)(p.aux + (long)bz * p.sAux + (long)m * p.ldaux + n);
          v[0] *= dgelu_f(bf2f((unsigned short)(a2[0] & 0xffff))); v[1] *= dgelu_f(bf2f((unsigned short)(a2[0] >> 16)));
          v[2] *= dgelu_f(bf2f((unsigned short)(a2[1] & 0xffff))); v[3] *= dgelu_f(bf2f((unsigned short)(a2[1] >> 16)));
        } else if (EPI == WFT_EPI_GELU_GRAD) {
          float dv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) gelu_both_f(v[e], v[e], dv[e]);
          u32x2 pk = {pack2bf(dv[0], dv[1]), pack2bf(dv[2], dv[3])};
          *(u32x2*)(p.aux + (long)bz * p.sAux + (long)m * p.ldaux + n) = pk;
        } else if (EPI == WFT_EPI_MUL_AUX) {
          const u32x2 a2 = *(const u32x2*)(p.aux + (long)bz * p.sAux + (long)m * p.ldaux + n);
          v[0] *= bf2f((unsigned short)(a2[0] & 0xffff)); v[1] *= bf2f((unsigned short)(a2[0] >> 16));
          v[2] *= bf2f((unsigned short)(a2[1] & 0xffff)); v[3] *= bf2f((unsigned short)(a2[1] >> 16));
        }
        if (p.res && !p.res_first) {
          const u32x2 r2 = *(const u32x2*)(p.res + (long)bz * p.sR + (long)m * p.ldr + n);
          v[0] += p.beta * bf2f((unsigned short)(r2[0] & 0xffff)); v[1] += p.beta * bf2f((unsigned short)(r2[0] >> 16));
          v[2] += p.beta * bf2f((unsigned short)(r2[1] & 0xffff)); v[3] += p.beta * bf2f((unsigned short)(r2[1] >> 16));
        }
        if (zero_row) { v[0] = v[1] = v[2] = v[3] = 0.f; }
        if (C_F32) {
          float* cp = (float*)p.C + cb + (long)m * p.ldc + n;
          f32x4 o = {v[0], v[1], v[2], v[3]};
          if (p.accumulate) o += *(const f32x4*)cp;
          *(f32x4*)cp = o;
        } else {
          unsigned short* cp = (unsigned short*)p.C + cb + (long)m * p.ldc + n;
          u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *(u32x2*)cp = pk;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------- TN 256x256
// Weight-gradient GEMM, large-shape variant: 256(p) x 256(q) output tile, 8 waves as 2(q) x 4(p)
// (128 q x 64 p per wave), same ping-pong as gemm_nt256_kernel: ring of four 32-row reduction slabs
// ({A [32 r][256 p], B [32 r][256 q]} = 32 KiB each), waves 0-3 / 4-7 half a period apart, group A stages
// the A part, group B the B part, counted vmcnt(8).  Fragments are transposed LDS reads
// (ds_read_b64_tr_b16) with the pair swizzle of the 128 kernel.  Split-K partials are added to C with
// fp32 atomics issued as contiguous 256-byte half rows staged through LDS.
#ifndef WFT_TN_RING
#define WFT_TN_RING 4  // ring slots of 32 KiB (lookahead = slots - 1); 5 measured +-0.5 % here (profiles/r03_tn_ring5_ab.log): the long reduction loop of one tile per workgroup is not stall-bound the way the NT kernel's fresh operand panels are
#endif
template <bool C_F32>
__global__ __launch_bounds__(512, 2) void gemm_tn256_kernel(GemmP p) {
  constexpr int NSLOT = WFT_TN_RING, LA = NSLOT - 1;
  extern __shared__ __attribute__((aligned(16))) char dsmem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave >> 2, wp = wave & 3;
  const bool grp_b = wave >= 4;
  const int P = p.M, Q = p.N, R = p.K;
  const int tiles_q = Q >> 8;
  const int tiles_p = P >> 8;
  // 1-D grid over (split, tile) pairs, SPLIT-MAJOR through the XCD map: the hardware deals consecutive workgroup ids round-robin
  // over the 8 XCDs; xcd_remap hands every XCD one contiguous range of pairs, so the ~32 workgroups an XCD runs at a time are
  // tiles of ONE split (or of two neighbours): they walk the same reduction range in step and every A / B slab crosses the
  // fabric once per XCD that needs it, instead of once per XCD for EVERY split (round-2 layout: each split's tiles spread over
  // all 8 XCDs — PMC: 2.27 GB fetched per launch, 2.5x the operands, at 4.1 TB/s)
  const int ntile = tiles_p * tiles_q;
  const int nsplit = p.nsplit < 0 ? -p.nsplit : p.nsplit;
  const bool old_map = p.nsplit < 0;  // round 2's placement (A/B switch)
  const int wsid = old_map ? (int)blockIdx.x : xcd_remap(blockIdx.x, ntile * nsplit);
  const int split = wsid / ntile;
  const int sid = old_map ? xcd_remap(wsid - split * ntile, ntile) : wsid - split * ntile;
  int tp, tq;
  band_coords(sid, tiles_p, tiles_q, tp, tq);
  const int p0 = tp << 8, q0 = tq << 8;

  const int spb = (R + 31) >> 5;  // 32-row slabs per batch item
  const int nslab_all = spb * p.batch;
  const int per = (nslab_all + nsplit - 1) / nsplit;
  const int s_begin = split * per;
  const int s_end = (s_begin + per) < nslab_all ? (s_begin + per) : nslab_all;
  const int nslab = s_end - s_begin;
  if (nslab <= 0) return;

  // staging share: one wave-instruction = 2 rows of 512 B; a part = 16 instructions; wave (w & 3) of the
  // group owns instructions 4(w&3) .. +3 = rows 8(w&3) .. +7 of its part
  const int rr = lane >> 5, cp = lane & 31;
  const unsigned short* const gbase = grp_b ? p.B : p.A;
  const long gld = grp_b ? p.ldb : p.lda;
  const long gbs = grp_b ? p.sB : p.sA;
  const int col0 = grp_b ? q0 : p0;
  char* const stage_dst = dsmem + (grp_b ? 16384 : 0) + (wave & 3) * 4096;
  const unsigned stage_dst_s = __builtin_amdgcn_readfirstlane(lds_addr_of(stage_dst));
  // full slabs: scalar base + constant per-lane byte offset (saddr form, no vector instruction per piece; see the NT kernel)
  unsigned soff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wave & 3) * 8 + j * 2 + rr;
    soff[j] = (unsigned)(r * (int)gld + ((cp ^ (tn_f(r) << 1)) << 3)) * 2u;
  }
  // (batch item, slab-in-item) of the next slab to stage / to read, advanced incrementally (no division in the loop)
  int ld_b = s_begin / spb, ld_t = s_begin - ld_b * spb;
  int rd_t = ld_t;
  int ld_slot = 0, rd_slot = 0;  // ring slots of the next slab to stage / to read (stage() is called in slab order)
  auto stage = [&](int u) {  // local slab index u -> ring slot u mod NSLOT; rows past R are clamped (masked at read time)
    const unsigned short* base = gbase + (long)ld_b * gbs + col0;
    if (ld_t * 32 + 32 <= R) {
      const unsigned long long b64 = (unsigned long long)(base + (long)ld_t * 32 * gld);
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b64), hi = __builtin_amdgcn_readfirstlane((unsigned)(b64 >> 32));
      const unsigned long long sb = ((unsigned long long)hi << 32) | lo;
      const unsigned dsts = stage_dst_s + ld_slot * 32768;
#pragma unroll
      for (int j = 0; j < 4; ++j) glds16_saddr(soff[j], sb, dsts + j * 1024);
    } else {
      char* dst = stage_dst + ld_slot * 32768;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (wave & 3) * 8 + j * 2 + rr;
        int gr = ld_t * 32 + r;
        gr = gr < R ? gr : R - 1;
        const int c = cp ^ (tn_f(r) << 1);
        glds16(base + (long)gr * gld + (c << 3), dst + j * 1024);
      }
    }
    if (++ld_t == spb) { ld_t = 0; ++ld_b; }
    ld_slot = ld_slot + 1 == NSLOT ? 0 : ld_slot + 1;
  };
  const int rem_last = R - (spb - 1) * 32;  // valid rows of the last slab of a batch item (32 = full)

  f32x4 acc[8][4];  // [q tile][p tile]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, li = lane & 15;
  const int r_in = li >> 2;
  const int fsw = (r_in | ((g & 1) << 2)) << 1;
  const int colq = wq * 128 + 4 * (li & 3);  // + i*16
  const int colp = wp * 64 + 4 * (li & 3);   // + j*16
  const unsigned lds0 = lds_addr_of(dsmem);
  // per-lane byte offsets (within a slab part) of the two transposed reads of a fragment at column `col`
  auto frag_off = [&](int col, int t) -> unsigned {
    const int r = 8 * g + 4 * t + r_in;
    return (unsigned)(r * 512 + (((col >> 3) ^ fsw) << 4) + ((col & 7) << 1));
  };
  s16x4 qh[8][2], ph[4][2];  // raw halves of the fragments (inline-asm reads: waited for by hand below)

#pragma unroll
  for (int j = 0; j < LA; ++j)
    if (j < nslab) stage(j);
  if (nslab >= LA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (LA - 1)) : "memory");
  else if (nslab == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (nslab == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (grp_b) __builtin_amdgcn_s_barrier();

  bf16x8 qf[8], pf[4];
  for (int u = 0; u < nslab; ++u) {
    // ---------------- L-unit
    if (u + LA < nslab) stage(u + LA);
    {
      const unsigned sa = lds0 + rd_slot * 32768;
      const unsigned sb = sa + 16384;
      // the second 4-row group of a fragment is +4 rows = +2048 B: in the instruction's immediate, not a second address
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned ad = sa + frag_off(colp + j * 16, 0);
        ph[j][0] = tn_tr_asm<0>(ad);
        ph[j][1] = tn_tr_asm<2048>(ad);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned ad = sb + frag_off(colq + i * 16, 0);
        qh[i][0] = tn_tr_asm<0>(ad);
        qh[i][1] = tn_tr_asm<2048>(ad);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = ph[j][0][e]; o[4 + e] = ph[j][1][e]; }
      pf[j] = __builtin_bit_cast(bf16x8, o);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = qh[i][0][e]; o[4 + e] = qh[i][1][e]; }
      qf[i] = __builtin_bit_cast(bf16x8, o);
    }
    if (rd_t == spb - 1 && rem_last < 32) {
      // ragged end of the reduction: rows >= rem_last of this slab hold clamped duplicates; zero them in
      // ONE operand (element 4t+e of the fragment is row 8g + 4t + e)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (8 * g + e >= rem_last) pf[j][e] = (__bf16)0.0f;
    }
    if (++rd_t == spb) rd_t = 0;
    const int ahead = nslab - 1 - u;
    if (ahead >= LA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (LA - 1)) : "memory");
    else if (ahead == 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // ---------------- C-unit
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[i], pf[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    rd_slot = rd_slot + 1 == NSLOT ? 0 : rd_slot + 1;
  }
  if (!grp_b) __builtin_amdgcn_s_barrier();

  // D[q][p]: lane (li, g) holds acc[i][j][e] = C[p = j*16 + li][q = i*16 + 4g + e] of the wave tile
  if (nsplit > 1 || p.ws) {  // (a workspace with ONE split: segmented output, written by the reduce kernel)
    float* lds = (float*)(dsmem + wave * 8448);  // [16 p][132] fp32 per pass
    if (p.ws) {
      // deterministic split-K: this split's partial tile goes to the workspace with plain 16-byte stores
      // (rows of 128 fp32 = 512 B per wave: 32 lanes x 16 B), summed later in split order
      float* wbase = p.ws + ((long)split * P + p0 + wp * 64) * Q + q0 + wq * 128;
      const int hr = lane >> 5, c4 = (lane & 31) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *(f32x4*)(lds + li * 132 + i * 16 + 4 * g) = acc[i][j] * p.alpha;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; r += 2)
          *(f32x4*)(wbase + (long)(j * 16 + r + hr) * Q + c4) = *(const f32x4*)(lds + (r + hr) * 132 + c4);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      return;
    }
    float* cbase = (float*)p.C + (long)(p0 + wp * 64) * p.ldc + q0 + wq * 128 + lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 8; ++i) *(f32x4*)(lds + li * 132 + i * 16 + 4 * g) = acc[i][j] * p.alpha;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
      for (int r = 0; r < 16; ++r) {
        float* crow = cbase + (long)(j * 16 + r) * p.ldc;
        atomicAdd(crow, lds[r * 132 + lane]);
        atomicAdd(crow + 64, lds[r * 132 + 64 + lane]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pp = p0 + wp * 64 + j * 16 + li;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int qq = q0 + wq * 128 + i * 16 + g * 4;
      f32x4 o = acc[i][j] * p.alpha;
      if (C_F32) {
        float* cptr = (float*)p.C + (long)pp * p.ldc + qq;
        if (p.accumulate) o += *(const f32x4*)cptr;
        *(f32x4*)cptr = o;
      } else {
        unsigned short* cptr = (unsigned short*)p.C + (long)pp * p.ldc + qq;
        u32x2 pk = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
        *(u32x2*)cptr = pk;
      }
    }
  }
}

// out[col] = sum over `nrows` partial rows (fixed order): finishes the fused bias-gradient column sums of gemm_nt256_kernel
__global__ __launch_bounds__(256) void nt_colsum_reduce_kernel(const float* partial, int nrows, int n, float* out) {
  // 64 columns per workgroup as 16 groups of four (16-byte loads: a wave instruction covers four whole 256-byte row segments),
  // 16 row lanes; round 5: the 32-column / 4-byte form streamed its 20 MB at 0.7 TB/s (29.8 us per fc2 backward-data GEMM)
  __shared__ f32x4 red[16][17];
  const int cg = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + cg * 4;
  f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (col < n)
    for (int r = ry; r < nrows; r += 16) sacc += *(const f32x4*)(partial + (long)r * n + col);
  red[ry][cg] = sacc;
  __syncthreads();
  if (ry == 0 && col < n) {
    f32x4 t = red[0][cg];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][cg];
    *(f32x4*)(out + col) = t;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int wft_nt256_launch(const wft_gemm_args* a, const GemmP& p, unsigned grid, hipStream_t s) {
  return nt_with_epilogue(a, [&](auto e, auto f32) {
    return wft_launch_lds<gemm_nt256_kernel<decltype(e)::value, decltype(f32)::value>>(dim3(grid), dim3(512), 163840, s, p);
  });
}
// the column sums of C from the partial rows the epilogue left in a->workspace (both 256x256 NT kernels write them)
void wft_nt_colsum_reduce_launch(const wft_gemm_args* a, hipStream_t s) {
  hipLaunchKernelGGL(nt_colsum_reduce_kernel, dim3((unsigned)((a->N + 63) / 64)), dim3(256), 0, s, (const float*)a->workspace,
                     (int)(2 * ((a->M + 255) / 256)), (int)a->N, a->colsum);
}

// 256x256 tiles, one workgroup per CU: the split-K factor that fills 256 slots in whole waves
int wft_tn256_nsplit(const wft_gemm_args* a) {
  const long t256 = (a->M / 256) * (a->N / 256);
  const long nslabs = ((a->K + 31) / 32) * a->batch;
  const int ncu = wft_num_cus();
  int nsplit = 1;
  double best = 0.0;
  for (int sp = 1; sp <= 16; ++sp) {
    if (sp > 1 && nslabs / sp < 48) break;
    const double waves = (double)(t256 * sp) / (double)ncu;
    const double eff = waves / (double)((long)(waves + 0.999999));
    if (eff > best + 0.02) { best = eff; nsplit = sp; }
  }
  // the kernel gives split y the slab range [y * per, (y + 1) * per), per = ceil(nslabs / nsplit): drop the splits that range
  // leaves EMPTY (they would return before storing their workspace tile, and the reduce kernel would add garbage)
  const long per = (nslabs + nsplit - 1) / nsplit;
  return (int)((nslabs + per - 1) / per);
}
// p.nsplit carries the plan; grid = output tiles x splits
int wft_tn256_launch(const GemmP& p, unsigned grid, hipStream_t s) {
  GemmP q = p;
  if (p.diag == 20) q.nsplit = -p.nsplit;  // (WFT_GEMM_DIAG=20: round 2's tile-major placement, A/B runs)
  return wft_launch_lds<gemm_tn256_kernel<true>>(dim3(grid), dim3(512), WFT_TN_RING * 32768, s, q);
}
