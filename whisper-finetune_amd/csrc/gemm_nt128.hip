// gemm_nt128.hip — C[M,N] = A[M,K] · B[N,K]^T on 128x128 tiles: the NT kernel for every shape the 256x256 kernels (gemm_nt4w.hip,
// gemm_pp256.hip) and the rank-r kernel (gemm_rank.hip) do not take, its split-K reduce, and the rules between its three forms.
//
// 128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave, 4x4 tiles of v_mfma_f32_16x16x32_bf16), K-step 64,
// LDS filled by global_load_lds_dwordx4 (the LDS image is lane-linear, so the bank swizzle is applied to the per-lane SOURCE
// address and again on the read — cdna_hip_programming.md rule 21), XCD-aware bijective tile remap so that tiles sharing an A
// row-panel sit on one L2.  MFMA operands are swapped (D^T = B·A^T) so that each lane ends up with 4 consecutive output columns
// of one row: 8-byte bf16 / 16-byte f32 stores.
#include "gemm_common.h"

// NST = 2: two k-step buffers in 64 KiB of static LDS, two workgroups per CU hide each other's load latency — the form for grids
//   of more than one workgroup per CU.
// NST = 4 (round 6): a ring of four k-step buffers (128 KiB of dynamic LDS, one workgroup per CU) for grids that do NOT fill the
//   chip (a decoder block's Linears at 1 024 rows: 32 workgroups): with a single workgroup per CU the two-buffer form pays one
//   exposed HBM/L2 latency per k-step (measured 0.8-1.5 us per k-step: 47 us for 1 024 x 512 x 2 048, 675 us for the tied-embedding
//   backward-data product 1 024 x 512 x 51 968).  Loads run three k-steps ahead behind counted s_waitcnt vmcnt, plain s_barrier,
//   inline-asm fragment reads (hipcc would drain the LDS-DMA queue in front of its own ds_reads).  Same products in the same order:
//   bit-identical to NST = 2.  With p.nsplit > 1 blockIdx.z is a split of the K range (p.band k-steps each, every split non-empty)
//   and C is the fp32 partial buffer [split][M][ldc] (host: wft_nt128_splitk_plan; summed in split order by nt_splitk_reduce_kernel).
template <int EPI, bool C_F32, int NST = 2>
__global__ __launch_bounds__(256, NST == 2 ? 2 : 1) void gemm_nt_kernel(GemmP p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = p.N >> 7;
  const int tiles_m = (p.M + 127) >> 7;
  const int sid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tm = sid / tiles_n, tn = sid - tm * tiles_n;
  const int m0 = tm << 7, n0 = tn << 7;
  const int bz = blockIdx.z;
  const bool ksplit = NST > 2 && p.nsplit > 1;
  const int kb = ksplit ? bz * p.band : 0;  // first k-step of this workgroup
  const unsigned short* Ab = ksplit ? p.A + (long)kb * 64 : p.A + (long)bz * p.sA;
  const unsigned short* Bb = ksplit ? p.B + (long)kb * 64 : p.B + (long)bz * p.sB;

  // per-lane source pointers for the 4+4 staging instructions this wave issues per K-tile
  const int lr = lane >> 3, lc = lane & 7;
  const unsigned short* asrc[4];
  const unsigned short* bsrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (wave * 4 + j) * 8 + lr;
    int gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    asrc[j] = Ab + (long)gm * p.lda + ((lc ^ lr) << 3);
    bsrc[j] = Bb + (long)(n0 + row) * p.ldb + ((lc ^ lr) << 3);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk_all = p.K >> 6;
  const int nk = ksplit ? ((kb + p.band <= nk_all) ? p.band : nk_all - kb) : nk_all;
  const int frow = lane & 15, fg = lane >> 4, sw = lane & 7;
  if constexpr (NST == 2) {
    __shared__ __attribute__((aligned(16))) char smem[65536];  // [buf 2][A 16K | B 16K]
    auto stage = [&](int buf, int kt) {
      char* sa = smem + buf * 32768 + wave * 4096;
      char* sb = sa + 16384;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        glds16(asrc[j] + kt * 64, sa + j * 1024);
        glds16(bsrc[j] + kt * 64, sb + j * 1024);
      }
    };
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      const char* sa = smem + cur * 32768 + (wm * 64 + frow) * 128;
      const char* sb = smem + cur * 32768 + 16384 + (wn * 64 + frow) * 128;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int coff = ((s * 4 + fg) ^ sw) << 4;
        bf16x8 af[4], bfr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = *(const bf16x8*)(sa + i * 2048 + coff);
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = *(const bf16x8*)(sb + j * 2048 + coff);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  } else {
    extern __shared__ __attribute__((aligned(16))) char dsmem[];  // [slot NST][A 16K | B 16K]
    int ld_slot = 0, ld_k = 0;
    auto stage = [&]() {
      char* sa = dsmem + ld_slot * 32768 + wave * 4096;
      char* sb = sa + 16384;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        glds16(asrc[j] + ld_k * 64, sa + j * 1024);
        glds16(bsrc[j] + ld_k * 64, sb + j * 1024);
      }
      ++ld_k;
      if (++ld_slot == NST) ld_slot = 0;
    };
    // fragment addresses inside a slot: the k half s flips chunk bit 2 (an XOR with the lane's swizzle: one base per half)
    const unsigned lds0 = lds_addr_of(dsmem);
    unsigned aoff[2], boff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned coff = (unsigned)(((s * 4 + fg) ^ sw) << 4);
      aoff[s] = (unsigned)((wm * 64 + frow) * 128) + coff;
      boff[s] = 16384u + (unsigned)((wn * 64 + frow) * 128) + coff;
    }
#pragma unroll
    for (int u = 0; u < NST - 1; ++u)
      if (u < nk) stage();
    int rd_slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      // k-step kt has landed when at most the younger k-steps' loads (8 per wave and k-step) are outstanding
      const int ahead = nk - 1 - kt;
      if (ahead >= NST - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * 8) : "memory");
      else if (NST == 4 && ahead == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // ... for every wave; and every wave is done reading the slot stage() refills now
      if (kt + NST - 1 < nk) stage();
      const unsigned sb = lds0 + rd_slot * 32768;
      bf16x8 af[2][4], bfr[2][4];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        af[s][0] = lds_b128_asm<0>(sb + aoff[s]); af[s][1] = lds_b128_asm<2048>(sb + aoff[s]);
        af[s][2] = lds_b128_asm<4096>(sb + aoff[s]); af[s][3] = lds_b128_asm<6144>(sb + aoff[s]);
        bfr[s][0] = lds_b128_asm<0>(sb + boff[s]); bfr[s][1] = lds_b128_asm<2048>(sb + boff[s]);
        bfr[s][2] = lds_b128_asm<4096>(sb + boff[s]); bfr[s][3] = lds_b128_asm<6144>(sb + boff[s]);
      }
      // LDS reads return in order: the first half's 8 fragments are there when 8 reads are still outstanding
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[0][j], af[0][i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[1][j], af[1][i], acc[i][j], 0, 0, 0);
      if (++rd_slot == NST) rd_slot = 0;
    }
  }

  // ---- epilogue: lane holds C[m][n..n+3] per (i,j)
  const long cb = ksplit ? (long)bz * p.M * p.ldc : (long)bz * p.sC;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + frow;
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
        v[0] += p.beta * bf2f((unsigned short)(r2[0] & 0xffff));
        v[1] += p.beta * bf2f((unsigned short)(r2[0] >> 16));
        v[2] += p.beta * bf2f((unsigned short)(r2[1] & 0xffff));
        v[3] += p.beta * bf2f((unsigned short)(r2[1] >> 16));
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
        v[0] *= dgelu_f(bf2f((unsigned short)(a2[0] & 0xffff)));
        v[1] *= dgelu_f(bf2f((unsigned short)(a2[0] >> 16)));
        v[2] *= dgelu_f(bf2f((unsigned short)(a2[1] & 0xffff)));
        v[3] *= dgelu_f(bf2f((unsigned short)(a2[1] >> 16)));
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
        v[0] += p.beta * bf2f((unsigned short)(r2[0] & 0xffff));
        v[1] += p.beta * bf2f((unsigned short)(r2[0] >> 16));
        v[2] += p.beta * bf2f((unsigned short)(r2[1] & 0xffff));
        v[3] += p.beta * bf2f((unsigned short)(r2[1] >> 16));
      }
      if (zero_row) { v[0] = v[1] = v[2] = v[3] = 0.f; }
      if (C_F32) {
        float* cp = (float*)p.C + cb + (long)m * p.ldc + n;
        f32x4 o = {v[0], v[1], v[2], v[3]};
        if (p.accumulate) {
          const f32x4 old = *(const f32x4*)cp;
          o += old;
        }
        *(f32x4*)cp = o;
      } else {
        unsigned short* cp = (unsigned short*)p.C + cb + (long)m * p.ldc + n;
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)cp = pk;
      }
    }
  }
}

// C[m][n] = bf16(sum over splits, in split order, of ws[split][m][n]): finishes the split-K form of the 128-tile NT kernel
__global__ __launch_bounds__(256) void nt_splitk_reduce_kernel(const float* ws, int nsplit, int M, int N, unsigned short* C, long ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // one thread per 4 consecutive columns
  const int n4 = N >> 2;
  if (i >= (long)M * n4) return;
  const int m = (int)(i / n4), n = (int)(i - (long)m * n4) << 2;
  const float* src = ws + (long)m * N + n;
  f32x4 t = *(const f32x4*)src;
  for (int k = 1; k < nsplit; ++k) t += *(const f32x4*)(src + (long)k * M * N);
  const u32x2 pk = {pack2bf(t[0], t[1]), pack2bf(t[2], t[3])};
  *(u32x2*)(C + (long)m * ldc + n) = pk;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// a grid of at most one workgroup per CU: the four-buffer ring form (one exposed load latency per CALL instead of one per
// k-step; WFT_GEMM_DIAG=11 keeps the two-buffer form for A/B runs)
bool wft_nt128_ring(const wft_gemm_args* a, int diag) {
  return ((a->M + 127) / 128) * (a->N / 128) * a->batch <= wft_num_cus() && diag != 11;
}
// 128-tile NT problems whose grid leaves most CUs idle over a deep K (the tied-embedding backward-data product of a short decoder
// batch: 1 024 x 512 x 51 968 = 32 tiles of 812 k-steps): K is split over the idle CUs, fp32 partial tiles go to the caller's
// workspace and are summed in split order (bitwise reproducible).  Plain products only, and not N = 128: those are the rank-r adapter
// products, which stay bit-identical to their p_valid form (gemm_nt_rank_kernel).  Returns the split count (1 = unsplit; which
// WFT_GEMM_DIAG=11 forces for A/B runs, and 12 because tools/dev/nt_stamps.py passes a stamp buffer as the workspace).
int wft_nt128_splitk_plan(const wft_gemm_args* a, int diag, int* per_out) {
  if (a->c_is_f32 || a->batch != 1 || a->epilogue != WFT_EPI_NONE || a->bias || a->residual || a->aux || a->colsum ||
      a->valid_rows_period != 0 || a->p_valid != 0 || a->N % 128 != 0 || a->N == 128 || diag == 11 || diag == 12)
    return 1;
  const long tiles = ((a->M + 127) / 128) * (a->N / 128), nk = a->K / 64;
  const int ncu = wft_num_cus();
  if (tiles < 1 || tiles * 2 > ncu || nk < 64) return 1;  // (at least two splits' worth of idle CUs)
  long nsplit = ncu / tiles;
  if (nsplit > nk / 16) nsplit = nk / 16;
  const long per = (nk + nsplit - 1) / nsplit;
  *per_out = (int)per;
  return (int)((nk + per - 1) / per);  // (no empty split)
}

// kind: NT_128_2BUF / NT_128_RING / NT_128_SPLITK (then nsplit splits of `per` k-steps each, partial tiles in a->workspace)
int wft_nt128_launch(const wft_gemm_args* a, const GemmP& p, NtKind kind, int nsplit, int per, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  if (kind == NT_128_SPLITK) {
    GemmP ps = p;  // fp32 partial tiles [split][M][N]; alpha is applied to every partial (linear)
    ps.C = a->workspace; ps.ldc = a->N; ps.accumulate = 0; ps.nsplit = nsplit; ps.band = per;
    const int rc = wft_launch_lds<gemm_nt_kernel<WFT_EPI_NONE, true, 4>>(grid, block, 131072, s, ps);
    if (rc == WFT_OK)
      hipLaunchKernelGGL(nt_splitk_reduce_kernel, dim3((unsigned)((a->M * (a->N / 4) + 255) / 256)), dim3(256), 0, s,
                         (const float*)a->workspace, nsplit, (int)a->M, (int)a->N, (unsigned short*)a->C, (long)a->ldc);
    return rc;
  }
  if (kind == NT_128_RING)
    return nt_with_epilogue(a, [&](auto e, auto f32) {
      return wft_launch_lds<gemm_nt_kernel<decltype(e)::value, decltype(f32)::value, 4>>(grid, block, 131072, s, p);
    });
  return nt_with_epilogue(a, [&](auto e, auto f32) {
    hipLaunchKernelGGL((gemm_nt_kernel<decltype(e)::value, decltype(f32)::value>), grid, block, 0, s, p);
    return (int)WFT_OK;
  });
}
