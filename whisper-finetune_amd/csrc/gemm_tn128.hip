// gemm_tn128.hip — C[P,Q] = A[R,P]^T · B[R,Q] (weight gradients) on 128x128 tiles: the TN kernel for every shape the 256x256
// kernels (gemm_tn4w.hip, gemm_pp256.hip) and the rank-r kernel (gemm_rank.hip) do not take, and the rules between its forms.
//
// Tile, waves and staging as in gemm_nt128.hip.  C[p][q] = sum_r A[r][p] * B[r][q]: LDS tiles are [64 r][128 cols] (256-byte
// rows); MFMA operands are column reads of those tiles -> ds_read_b64_tr_b16.
#include "gemm_common.h"

// PB > 0: only the first 16*PB (<= 64) columns of A are non-zero (a rank-r LoRA operand in its 128-wide padded buffer): the
// wave column wp = 1 and the p-blocks >= PB of wp = 0 skip their fragment reads and MFMAs (their part of C is written as zero).
// NST = 2: two reduction-step buffers in 64 KiB of static LDS, two workgroups per CU (grids of more than one workgroup per CU).
// NST = 4 (round 6, PB = 0): a ring of four buffers in 128 KiB of dynamic LDS for grids of at most one workgroup per CU — a decoder
//   block's weight gradients at R = B*S = 1 024 rows are 16-64 tiles of 16 reduction steps, and the two-buffer form pays an exposed
//   load latency per step there (26 us for 512 x 512 x 1 024, whatever the tile count).  Loads run three steps ahead behind counted
//   s_waitcnt vmcnt, plain s_barrier, inline-asm transposed reads.  Same products in the same order: bit-identical per split.
template <bool C_F32, int PB = 0, int NST = 2>
__global__ __launch_bounds__(256, NST == 2 ? 2 : 1) void gemm_tn_kernel(GemmP p) {
  static_assert(NST == 2 || PB == 0, "the ring form is the general kernel only");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wq = wave >> 1, wp = wave & 1;
  const int P = p.M, Q = p.N, R = p.K;
  const int tiles_q = Q >> 7;
  const int tiles_p = P >> 7;
  const int sid = xcd_remap(blockIdx.x, tiles_p * tiles_q);
  const int tp = sid / tiles_q, tq = sid - tp * tiles_q;
  const int p0 = tp << 7, q0 = tq << 7;

  const int tpb = (R + 63) >> 6;  // reduction tiles per batch item
  const int nsteps_all = tpb * p.batch;
  // split-K: blockIdx.y owns a contiguous range of reduction steps; partial tiles are summed into C
  // with fp32 atomics issued as whole 256-byte rows (MI355X_MICROARCH.md "Global float atomics")
  const int nsplit = gridDim.y;
  const int per = (nsteps_all + nsplit - 1) / nsplit;
  const int s_begin = blockIdx.y * per;
  const int s_end = (s_begin + per) < nsteps_all ? (s_begin + per) : nsteps_all;
  const int nsteps = s_end - s_begin;
  if (nsteps <= 0) return;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  char* ep_lds;
  if constexpr (NST == 2) {
    __shared__ __attribute__((aligned(16))) char smem[65536];  // [buf 2][A 16K | B 16K]
    ep_lds = smem;
    // staging: instruction i (0..15) covers r rows 4i..4i+3; lane -> (rr = lane>>4, c' = lane&15)
    const int rr = lane >> 4, cp = lane & 15;
    auto stage = [&](int buf, int step) {
      const int b = step / tpb, t = step - b * tpb;
      const unsigned short* Ab = p.A + (long)b * p.sA;
      const unsigned short* Bb = p.B + (long)b * p.sB;
      char* sa = smem + buf * 32768 + wave * 4096;
      char* sb = sa + 16384;
  #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = wave * 4 + j;
        const int r = i * 4 + rr;
        int gr = t * 64 + r;
        gr = gr < R ? gr : R - 1;
        const int c = cp ^ (tn_f(r) << 1);
        // rank-r operand: only its first 2*PB 16-byte chunks per row are ever read back (the other LDS slots keep stale bytes)
        if (PB == 0 || c < 2 * PB) glds16(Ab + (long)gr * p.lda + p0 + (c << 3), sa + j * 1024);
        glds16(Bb + (long)gr * p.ldb + q0 + (c << 3), sb + j * 1024);
      }
    };
    auto zero_tail = [&](int buf, int step) {
      const int t = step % tpb;
      const int rem = R - t * 64;  // valid rows in this tile
      if (rem >= 64) return false;
      // rows [rem, 64) of both tiles -> 0 ; 16 chunks of 16 B per row per operand
      char* base = smem + buf * 32768;
      const int nchunk = (64 - rem) * 16;
      for (int c = tid; c < nchunk; c += 256) {
        const int off = (rem * 16 + c) * 16;
        *(u32x4*)(base + off) = u32x4{0, 0, 0, 0};
        *(u32x4*)(base + 16384 + off) = u32x4{0, 0, 0, 0};
      }
      return true;
    };

    stage(0, s_begin);
    __syncthreads();
    if (zero_tail(0, s_begin)) __syncthreads();

    const int g = lane >> 4, li = lane & 15;
    const int r_in = (li >> 2);               // row within the 4-row block
    const int fsw = (r_in | ((g & 1) << 2)) << 1;  // tn_f(r) << 1 for r = 32s + 8g + 4t + r_in
    const int colq = wq * 64 + 4 * (li & 3);  // + iq*16
    const int colp = wp * 64 + 4 * (li & 3);  // + jp*16
    constexpr int NPB = PB > 0 ? PB : 4;      // p-blocks this wave multiplies
    const bool idle = PB > 0 && wp == 1;      // wave-uniform
    for (int step = 0; step < nsteps; ++step) {
      const int cur = step & 1;
      if (step + 1 < nsteps) stage(cur ^ 1, s_begin + step + 1);
      const char* sa = smem + cur * 32768;
      const char* sb = sa + 16384;
      if (!idle) {
  #pragma unroll
      for (int s = 0; s < 2; ++s) {
        s16x8 qf[4], pf[NPB];
  #pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int r = 32 * s + 8 * g + 4 * t + r_in;
  #pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int cq = colq + i * 16;
            const int aq = r * 256 + (((cq >> 3) ^ fsw) << 4) + ((cq & 7) << 1);
            const s16x4 x = lds_read_tr16(sb + aq);
  #pragma unroll
            for (int e = 0; e < 4; ++e) qf[i][4 * t + e] = x[e];
            if (i < NPB) {
              const int cpp = colp + i * 16;
              const int ap = r * 256 + (((cpp >> 3) ^ fsw) << 4) + ((cpp & 7) << 1);
              const s16x4 y = lds_read_tr16(sa + ap);
  #pragma unroll
              for (int e = 0; e < 4; ++e) pf[i][4 * t + e] = y[e];
            }
          }
        }
  #pragma unroll
        for (int i = 0; i < 4; ++i)
  #pragma unroll
          for (int j = 0; j < NPB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8, qf[i]), __builtin_bit_cast(bf16x8, pf[j]), acc[i][j], 0, 0, 0);
      }
      }
      __syncthreads();
      if (step + 1 < nsteps) {
        if (zero_tail(cur ^ 1, s_begin + step + 1)) __syncthreads();
      }
    }

  } else {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];  // [slot NST][A 16K | B 16K]
    ep_lds = dsmem;
    const int rr = lane >> 4, cp = lane & 15;
    int ld_slot = 0, ld_step = s_begin;
    auto stage = [&]() {
      const int b = ld_step / tpb, t = ld_step - b * tpb;
      const unsigned short* Ab = p.A + (long)b * p.sA;
      const unsigned short* Bb = p.B + (long)b * p.sB;
      char* sa = dsmem + ld_slot * 32768 + wave * 4096;
      char* sb = sa + 16384;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (wave * 4 + j) * 4 + rr;
        int gr = t * 64 + r;
        gr = gr < R ? gr : R - 1;
        const int c = cp ^ (tn_f(r) << 1);
        glds16(Ab + (long)gr * p.lda + p0 + (c << 3), sa + j * 1024);
        glds16(Bb + (long)gr * p.ldb + q0 + (c << 3), sb + j * 1024);
      }
      ++ld_step;
      if (++ld_slot == NST) ld_slot = 0;
    };
    // fragment read offsets inside a slot for (s, t) = (0, 0); (s, t) adds the immediate 8192 s + 1024 t.  The 16-byte chunk of
    // fragment i is (i ^ r_in) in bits 1-2: lane-dependent, one address register per fragment and operand
    const int g = lane >> 4, li = lane & 15;
    const int r_in = li >> 2;
    const int fsw = (r_in | ((g & 1) << 2)) << 1;
    unsigned qoff[4], poff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cq = wq * 64 + 4 * (li & 3) + i * 16, cpp = wp * 64 + 4 * (li & 3) + i * 16;
      const unsigned rowb = (unsigned)(8 * g + r_in) * 256u;
      qoff[i] = 16384u + rowb + (unsigned)((((cq >> 3) ^ fsw) << 4) + ((cq & 7) << 1));
      poff[i] = rowb + (unsigned)((((cpp >> 3) ^ fsw) << 4) + ((cpp & 7) << 1));
    }
    const unsigned lds0 = lds_addr_of(dsmem);
#pragma unroll
    for (int u = 0; u < NST - 1; ++u)
      if (u < nsteps) stage();
    int rd_slot = 0;
    for (int step = 0; step < nsteps; ++step) {
      const int ahead = nsteps - 1 - step;
      if (ahead >= NST - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * 8) : "memory");
      else if (NST == 4 && ahead == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      {  // rows past R of a batch item's last step: zeros (the loads clamped them to row R - 1)
        const int t = (s_begin + step) % tpb;
        const int rem = R - t * 64;
        if (rem < 64) {  // workgroup-uniform
          char* base = dsmem + rd_slot * 32768;
          const int nchunk = (64 - rem) * 16;
          for (int c = tid; c < nchunk; c += 256) {
            const int off = (rem * 16 + c) * 16;
            *(u32x4*)(base + off) = u32x4{0, 0, 0, 0};
            *(u32x4*)(base + 16384 + off) = u32x4{0, 0, 0, 0};
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
      }
      if (step + NST - 1 < nsteps) stage();
      const unsigned sb = lds0 + rd_slot * 32768;
      unsigned qa[4], pa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { qa[i] = sb + qoff[i]; pa[i] = sb + poff[i]; }
      s16x4 qf[2][2][4], pf[2][2][4];  // [s][t][fragment]
#pragma unroll
      for (int i = 0; i < 4; ++i) { qf[0][0][i] = tn_tr_asm<0>(qa[i]); qf[0][1][i] = tn_tr_asm<1024>(qa[i]); }
#pragma unroll
      for (int i = 0; i < 4; ++i) { pf[0][0][i] = tn_tr_asm<0>(pa[i]); pf[0][1][i] = tn_tr_asm<1024>(pa[i]); }
#pragma unroll
      for (int i = 0; i < 4; ++i) { qf[1][0][i] = tn_tr_asm<8192>(qa[i]); qf[1][1][i] = tn_tr_asm<8192 + 1024>(qa[i]); }
      // LDS reads return in order (the counter holds 15 at most): the first half's 16 fragments are there when 8 are outstanding
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) { pf[1][0][i] = tn_tr_asm<8192>(pa[i]); pf[1][1][i] = tn_tr_asm<8192 + 1024>(pa[i]); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (s2 == 1) {
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
        }
        s16x8 q8[4], p8[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            q8[i][e] = qf[s2][0][i][e]; q8[i][4 + e] = qf[s2][1][i][e];
            p8[i][e] = pf[s2][0][i][e]; p8[i][4 + e] = pf[s2][1][i][e];
          }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, q8[i]), __builtin_bit_cast(bf16x8, p8[j]), acc[i][j], 0, 0, 0);
      }
      if (++rd_slot == NST) rd_slot = 0;
    }
    __syncthreads();  // (the epilogue stages through LDS other waves may still be reading)
  }
  const int g = lane >> 4, li = lane & 15;
  constexpr int NPB = PB > 0 ? PB : 4;  // p-blocks this wave multiplied
  if (nsplit > 1) {
    // stage the wave's 64(p) x 64(q) fp32 tile through LDS (two halves of 32 p-rows, row pitch 68
    // floats) so that every atomic wave-instruction adds one contiguous 256-byte row of C
    float* lds = (float*)(ep_lds + wave * 16384);
    if (PB > 0 && p.ws) {
      // rank-r operand: the workspace holds only the 16*PB valid rows of every split, ws[split][16 PB][Q] (P == 128, p0 == 0)
      if (wp == 0) {
        float* wb = p.ws + (long)blockIdx.y * (16 * NPB) * Q + q0 + wq * 64 + lane;
#pragma unroll
        for (int jj = 0; jj < NPB; ++jj) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *(f32x4*)(lds + li * 68 + i * 16 + 4 * g) = acc[i][jj] * p.alpha;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 8
          for (int r = 0; r < 16; ++r) wb[(long)(jj * 16 + r) * Q] = lds[r * 68 + lane];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
      }
      return;
    }
    // with a workspace (the default: wft_gemm_tn_workspace_bytes) the partial tile of split blockIdx.y is STORED to
    // ws[split][P][Q] and tn_splitk_reduce_kernel adds the splits in index order: bitwise reproducible.  Without one the
    // partial tiles are added into C with fp32 atomics (order, hence rounding, varies run to run).
    float* cbase = p.ws ? p.ws + ((long)blockIdx.y * P + p0 + wp * 64) * Q + q0 + wq * 64 + lane
                        : (float*)p.C + (long)(p0 + wp * 64) * p.ldc + q0 + wq * 64 + lane;
    const long cld = p.ws ? (long)Q : p.ldc;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *(f32x4*)(lds + (jj * 16 + li) * 68 + i * 16 + 4 * g) = acc[i][half * 2 + jj] * p.alpha;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (p.ws) {
#pragma unroll 8
        for (int r = 0; r < 32; ++r) cbase[(long)(half * 32 + r) * cld] = lds[r * 68 + lane];
      } else {
#pragma unroll 8
        for (int r = 0; r < 32; ++r) atomicAdd(cbase + (long)(half * 32 + r) * cld, lds[r * 68 + lane]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    return;
  }

  // epilogue: D[q][p]: col (lane&15) = p index, rows 4*(lane>>4)+e = q index
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pp = p0 + wp * 64 + j * 16 + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qq = q0 + wq * 64 + i * 16 + g * 4;
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

// ---- host ----------------------------------------------------------------------------------------------------------------
// the ring form of gemm_tn_kernel (one workgroup per CU): the general fp32 product on a grid that fits the chip once
// (WFT_GEMM_DIAG=13 keeps the two-buffer form for A/B runs)
bool wft_tn128_ring(const wft_gemm_args* a, int diag) {
  // (P = 128 is the rank-r operand's buffer width: that product stays bit-identical to its p_valid form, gemm_tn_rank_kernel)
  // measured (tools/dev/small_gemm_time.py, two-buffer -> ring): R = 1 024: 16 tiles 19.2 -> 12.8 us, 48-64 tiles 19.1 -> 16.9-19.0;
  // R = 12 000: 16 tiles 28.4 -> 23.8, 32 tiles 34.3 -> 32.1, but 48 / 64 tiles 41.6 -> 43.2 / 50.4 -> 52.0 (two workgroups per CU win)
  const long tiles = (a->M / 128) * (a->N / 128), nsteps = ((a->K + 63) / 64) * a->batch;
  return a->c_is_f32 && a->M != 128 && a->tn_col_scale == nullptr && a->tn_block_n == 0 && tiles <= wft_num_cus() &&
         (tiles <= 32 || nsteps <= 32) && diag != 13;
}
int wft_tn128_nsplit(const wft_gemm_args* a, bool ring) {
  const long tiles = (a->M / 128) * (a->N / 128);
  const long nsteps = ((a->K + 63) / 64) * a->batch;
  if (!a->c_is_f32 || tiles < 1 || nsteps < 1) return 1;  // (the plan is made before the arguments are checked)
  if (ring) {
    // as many splits as fill the chip once, four reduction steps each at least (the ring's depth)
    long sp = wft_num_cus() / tiles;
    if (sp > nsteps / 4) sp = nsteps / 4;
    if (sp < 1) sp = 1;
    const long per = (nsteps + sp - 1) / sp;
    return (int)((nsteps + per - 1) / per);
  }
  int nsplit = 1;
  double best = 0.0;
  // the two-buffer form: the split-K factor that fills the 512 resident-block slots (256 CUs x 2) in whole waves;
  // up to 64 splits: rank-r LoRA gradients are ONE 128-wide tile row (10-40 tiles) over a 48 000+ row reduction
  for (int sp = 1; sp <= 64; ++sp) {
    if (sp > 1 && nsteps / sp < (sp <= 8 ? 16 : 12)) break;
    const double waves = (double)(tiles * sp) / 512.0;
    const double eff = waves / (double)((long)(waves + 0.999999));
    if (eff > best + 0.03) { best = eff; nsplit = sp; }
  }
  const long per = (nsteps + nsplit - 1) / nsplit;  // no empty split (see wft_tn256_nsplit)
  return (int)((nsteps + per - 1) / per);
}
// p_valid: A is a rank-r operand in a 128-wide zero-padded buffer -> number of 16-column blocks that hold data (0: general path)
int wft_tn128_pb(const wft_gemm_args* a) {
  return (a->c_is_f32 && a->M == 128 && a->p_valid > 0 && a->p_valid <= 64) ? (a->p_valid + 15) / 16 : 0;
}

// kind: TN_128_BF16C / TN_128_PB (pb p-blocks) / TN_128_RING / TN_128_2BUF; grid = (output tiles, K splits)
int wft_tn128_launch(const GemmP& p, TnKind kind, int pb, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  if (kind == TN_128_RING) return wft_launch_lds<gemm_tn_kernel<true, 0, 4>>(grid, block, 131072, s, p);
  if (kind == TN_128_BF16C) hipLaunchKernelGGL((gemm_tn_kernel<false>), grid, block, 0, s, p);
  else if (kind == TN_128_2BUF) hipLaunchKernelGGL((gemm_tn_kernel<true>), grid, block, 0, s, p);
  else if (pb == 1) hipLaunchKernelGGL((gemm_tn_kernel<true, 1>), grid, block, 0, s, p);
  else if (pb == 2) hipLaunchKernelGGL((gemm_tn_kernel<true, 2>), grid, block, 0, s, p);
  else if (pb == 3) hipLaunchKernelGGL((gemm_tn_kernel<true, 3>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((gemm_tn_kernel<true, 4>), grid, block, 0, s, p);
  return WFT_OK;
}
