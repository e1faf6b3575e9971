// gemm_rank.hip — the load-stream kernels for the four rank-r (LoRA adapter) products of an adapted Linear: gemm_nt_rank_kernel
// (u = x (s A*mask)^T, du = dy (s B)) and gemm_tn_rank_kernel (dA = du^T x, dB^T = u^T dy).  HBM-bound on the activation operand,
// so both are built around the load stream instead of the 128x128 tile of gemm_nt128.hip / gemm_tn128.hip, whose results they
// reproduce bit for bit.
#include "gemm_common.h"

template <int V>
struct RankIntC { static constexpr int value = V; };
template <int N, class F>
__device__ __forceinline__ void static_for_rank(F&& f) {
  if constexpr (N > 0) {
    static_for_rank<N - 1>(f);
    f(RankIntC<N - 1>{});
  }
}
// ---------------------------------------------------------------------------------- NT, rank-r B operand
// The other two LoRA adapter products, u = x (s A*mask)^T and du = dy (s B): C[M, 16 PB] = A[M, K] B[16 PB, K]^T with B a rank-r
// operand in the first rows of a 128-row zero-padded buffer.  HBM-bound on A (the activation, read once): the 128-tile
// kernel spends half of its loads in flight on B's zero rows and drains its one-deep prefetch at every __syncthreads; here a
// workgroup streams 128 rows of A through a ring of NST stages {A [128][64 k] 16 KB, B [16 PB][64 k] 2 PB KB} (counted vmcnt,
// plain s_barrier, inline-asm fragment reads) and writes only the 16 PB data columns of the 128-wide C buffer — its consumer,
// gemm_tn_rank_kernel, reads no others.  Same products in the same order as gemm_nt_kernel: bit-identical in those columns.
template <int PB>
__global__ __launch_bounds__(256, 2) void gemm_nt_rank_kernel(GemmP pa, GemmP pb, int na) {
  // TWO independent products in one launch (round 3: u = x (sA*m)^T and du = dy (sB) of one adapted Linear group — each alone is
  // 375 workgroups at 32 clips, 1.46 rounds of the chip): workgroups >= na work on the second parameter set.  A single product
  // passes na = gridDim.x.
  const bool second = (int)blockIdx.x >= na;  // workgroup-uniform
  const GemmP& p = second ? pb : pa;
  const int bid = (int)blockIdx.x - (second ? na : 0);
  constexpr int NST = PB <= 2 ? 4 : 3;
  constexpr int BBYTES = 2048 * PB;
  constexpr int SBYTES = 16384 + BBYTES;  // stage = A part, then B part
  constexpr int NBI = (2 * PB + 3) / 4;   // B staging instructions per wave and stage (surplus ones repeat a piece)
  constexpr int LPS = 4 + NBI;
  extern __shared__ __attribute__((aligned(16))) char dsmem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = bid << 7;
  const int lr = lane >> 3, lc = lane & 7;
  // per-lane source pointers of the staging instructions (row of the piece, swizzled 16-byte chunk), advanced by 64 k per step
  const unsigned short* asrc[4];
  const unsigned short* bsrc[NBI];
  int bpiece[NBI];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int gm = m0 + (wave * 4 + j) * 8 + lr;
    gm = gm < p.M ? gm : p.M - 1;
    asrc[j] = p.A + (long)gm * p.lda + ((lc ^ lr) << 3);
  }
#pragma unroll
  for (int k = 0; k < NBI; ++k) {
    bpiece[k] = (wave + 4 * k) % (2 * PB);
    bsrc[k] = p.B + (long)(bpiece[k] * 8 + lr) * p.ldb + ((lc ^ lr) << 3);
  }
  int ld_slot = 0, ld_k = 0;
  auto stage = [&]() {
    char* sbase = dsmem + ld_slot * SBYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(asrc[j] + ld_k * 64, sbase + (wave * 4 + j) * 1024);
#pragma unroll
    for (int k = 0; k < NBI; ++k) glds16(bsrc[k] + ld_k * 64, sbase + 16384 + bpiece[k] * 1024);
    ++ld_k;
    if (++ld_slot == NST) ld_slot = 0;
  };

  f32x4 acc[2][PB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < PB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fg = lane >> 4, sw = lane & 7;
  const unsigned lds0 = lds_addr_of(dsmem);
  // fragment addresses inside a stage for the k half s = 0; s = 1 flips chunk bit 2 (an XOR, so not an immediate: two bases)
  unsigned aoff[2][2], boff[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const unsigned coff = (unsigned)(((s2 * 4 + fg) ^ sw) << 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) aoff[s2][i] = (unsigned)((wave * 32 + i * 16 + frow) * 128) + coff;
    boff[s2] = 16384u + (unsigned)(frow * 128) + coff;
  }

  const int nk = p.K >> 6;
#pragma unroll
  for (int u = 0; u < NST - 1; ++u)
    if (u < nk) stage();
  int rd_slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = nk - 1 - kt;
    if (ahead >= NST - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPS) : "memory");
    else if (NST == 4 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + NST - 1 < nk) stage();
    const unsigned sb = lds0 + rd_slot * SBYTES;
    bf16x8 af[2][2], bfr[2][PB];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
      for (int i = 0; i < 2; ++i) af[s2][i] = lds_b128_asm<0>(sb + aoff[s2][i]);
      static_for_rank<PB>([&](auto jt) {
        constexpr int j = decltype(jt)::value;
        bfr[s2][j] = lds_b128_asm<j * 2048>(sb + boff[s2]);
      });
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < PB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[s2][j], af[s2][i], acc[i][j], 0, 0, 0);
    if (++rd_slot == NST) rd_slot = 0;
  }

  // lane holds C[m = 16 i + frow][n = 16 j + 4 fg + e] of the wave's 32 rows
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wave * 32 + i * 16 + frow;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const f32x4 v = acc[i][j] * p.alpha;
      const u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *(u32x2*)((unsigned short*)p.C + (long)m * p.ldc + j * 16 + fg * 4) = pk;
    }
  }
}

// ---------------------------------------------------------------------------------- TN, rank-r A operand
// The two LoRA adapter gradients dA = du^T x and dB^T = u^T dy: A is a rank-r operand (du / u, [R, lda]) whose data sits in the
// first 16*PB columns of a 128-wide zero-padded buffer, B the [R, Q] activation stream.  HBM-bound on B (2 bytes per element
// read once; the MFMA work is r/128 of a square tile's), so the kernel is built around the load stream instead of the tile:
//   * ring of NST (4; 3 for PB > 2) stages {B [64 r][128 q] 16 KB, A [64 r][16 PB] 2 PB KB compact}: two workgroups per CU
//     keep 2 x (NST - 1) x 18 KB in flight; LDS-DMA waited for with counted vmcnt and a plain s_barrier per step (the
//     128-tile kernel's __syncthreads is a fence: it drains the prefetch it has just issued)
//   * only the valid rows of a split's partial tile go to the workspace: ws[split][16 PB][Q] (tn_splitk_reduce_kernel adds
//     the splits in index order and writes the padding rows of C as zero)
//   * 1-D grid, split-major through xcd_remap: the q-tiles of one split run on one XCD and share its A rows in that L2.
// All four waves multiply: wave w owns q columns [32 w, 32 w + 32) of the tile and all PB p-blocks.
template <int PB>
__global__ __launch_bounds__(256, 2) void gemm_tn_rank_kernel(GemmP pa, GemmP pb, int na) {
  // two products in one launch (dA = du^T x and dB^T = u^T dy of one adapted group): workgroups >= na take the second set
  const bool second = (int)blockIdx.x >= na;
  const GemmP& p = second ? pb : pa;
  const int bid = (int)blockIdx.x - (second ? na : 0);
  constexpr int NST = PB <= 2 ? 4 : 3;
  constexpr int APITCH = 32 * PB;        // bytes per A row in LDS
  constexpr int ABYTES = 64 * APITCH;    // a stage's A part
  constexpr int SBYTES = 16384 + ABYTES; // stage = B part, then A part
  constexpr int NAI = (2 * PB + 3) / 4;  // A staging instructions per wave and stage (2 PB needed; surplus ones repeat a piece)
  constexpr int LPS = 4 + NAI;           // LDS-DMA instructions per wave and stage
  extern __shared__ __attribute__((aligned(16))) char dsmem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Q = p.N, R = p.K;
  const int tiles_q = Q >> 7;
  const int nsplit = p.nsplit;
  const int sid = xcd_remap(bid, tiles_q * nsplit);
  const int split = sid / tiles_q, tq = sid - split * tiles_q;
  const int q0 = tq << 7;

  const int tpb = (R + 63) >> 6;  // reduction tiles per batch item
  const int nsteps_all = tpb * p.batch;
  const int per = (nsteps_all + nsplit - 1) / nsplit;
  const int s_begin = split * per;
  const int s_end = (s_begin + per) < nsteps_all ? (s_begin + per) : nsteps_all;
  const int nsteps = s_end - s_begin;
  if (nsteps <= 0) return;  // (the host drops empty splits)

  // staging.  B as in gemm_tn_kernel: instruction i (0..15) covers rows 4i..4i+3, lane -> (rr = lane>>4, position cp = lane&15)
  // holding global chunk cp ^ swizzle(row); A compact row-major: piece ai (1 KB) = chunks 64 ai .. 64 ai + 63 of the
  // [64][2 PB] chunk array.
  const int rr = lane >> 4, cp = lane & 15;
  int ld_b = s_begin / tpb, ld_t = s_begin - ld_b * tpb;
  int ld_slot = 0;
  auto stage = [&]() {
    char* sbase = dsmem + ld_slot * SBYTES;
    const unsigned short* Bb = p.B + (long)ld_b * p.sB + q0;
    const unsigned short* Ab = p.A + (long)ld_b * p.sA;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (wave * 4 + j) * 4 + rr;
      int gr = ld_t * 64 + r;
      gr = gr < R ? gr : R - 1;
      const int c = cp ^ (tn_f(r) << 1);
      glds16(Bb + (long)gr * p.ldb + (c << 3), sbase + wave * 4096 + j * 1024);
    }
#pragma unroll
    for (int k = 0; k < NAI; ++k) {
      const int ai = (wave + 4 * k) % (2 * PB);
      const int id = ai * 64 + lane;
      const int r = id / (2 * PB), c = id - r * (2 * PB);
      int gr = ld_t * 64 + r;
      gr = gr < R ? gr : R - 1;
      glds16(Ab + (long)gr * p.lda + (c << 3), sbase + 16384 + ai * 1024);
    }
    if (++ld_t == tpb) { ld_t = 0; ++ld_b; }
    if (++ld_slot == NST) ld_slot = 0;
  };
  const int rem_last = R - (tpb - 1) * 64;  // valid rows of the last tile of a batch item (64 = full)
  int rd_t = ld_t, rd_slot = 0;

  f32x4 acc[2][PB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < PB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4, li = lane & 15;
  const int r_in = li >> 2;
  const int fsw = (r_in | ((g & 1) << 2)) << 1;  // tn_f(r) << 1 for r = 32 s + 8 g + 4 t + r_in
  const unsigned lds0 = lds_addr_of(dsmem);
  // per-lane byte offsets inside a stage of the (s = 0, t = 0) reads; t adds 4 rows, s adds 32 rows (immediates)
  unsigned boff[2], aoff[PB];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cq = wave * 32 + i * 16 + 4 * (li & 3);
    boff[i] = (unsigned)((8 * g + r_in) * 256 + (((cq >> 3) ^ fsw) << 4) + ((cq & 7) << 1));
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) aoff[j] = (unsigned)(16384 + (8 * g + r_in) * APITCH + (j * 16 + 4 * (li & 3)) * 2);

#pragma unroll
  for (int u = 0; u < NST - 1; ++u)
    if (u < nsteps) stage();

  for (int step = 0; step < nsteps; ++step) {
    const int ahead = nsteps - 1 - step;  // stages issued after this one so far: min(ahead, NST - 2)
    if (ahead >= NST - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * LPS) : "memory");
    else if (NST == 4 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's pieces of this stage have landed; every wave is done reading the previous one
    if (step + NST - 1 < nsteps) stage();
    const unsigned sb = lds0 + rd_slot * SBYTES;
    s16x4 qh[2][2][2], ph[2][PB][2];  // [s][block][t]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const unsigned ad = sb + aoff[j] + s * (32 * APITCH);
        ph[s][j][0] = tn_tr_asm<0>(ad);
        ph[s][j][1] = tn_tr_asm<4 * APITCH>(ad);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned ad = sb + boff[i] + s * 8192;
        qh[s][i][0] = tn_tr_asm<0>(ad);
        qh[s][i][1] = tn_tr_asm<1024>(ad);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const bool ragged = rd_t == tpb - 1 && rem_last < 64;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 qf[2], pf[PB];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        s16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = qh[s][i][0][e]; o[4 + e] = qh[s][i][1][e]; }
        qf[i] = __builtin_bit_cast(bf16x8, o);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        s16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = ph[s][j][0][e]; o[4 + e] = ph[s][j][1][e]; }
        pf[j] = __builtin_bit_cast(bf16x8, o);
      }
      if (ragged) {
        // rows >= rem_last of this tile hold clamped duplicates: zero them in ONE operand (element e of the fragment is row
        // 32 s + 8 g + e of the tile)
#pragma unroll
        for (int j = 0; j < PB; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (32 * s + 8 * g + e >= rem_last) pf[j][e] = (__bf16)0.0f;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < PB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[i], pf[j], acc[i][j], 0, 0, 0);
    }
    if (++rd_t == tpb) rd_t = 0;
    if (++rd_slot == NST) rd_slot = 0;
  }

  // D[q][p]: lane (li, g) holds acc[i][j][e] = C[p = 16 j + li][q = 16 i + 4 g + e] of the wave's 32 columns
  if (p.ws) {  // also with ONE split when the reduce kernel has work of its own (column scale, block-transposed output)
    float* wb = p.ws + (long)split * (16 * PB) * Q + q0 + wave * 32 + 4 * g;
#pragma unroll
    for (int j = 0; j < PB; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) *(f32x4*)(wb + (long)(j * 16 + li) * Q + i * 16) = acc[i][j] * p.alpha;
    return;
  }
  float* cb = (float*)p.C + q0 + wave * 32 + 4 * g;
#pragma unroll
  for (int j = 0; j < PB; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* cptr = cb + (long)(j * 16 + li) * p.ldc + i * 16;
      f32x4 o = acc[i][j] * p.alpha;
      if (p.accumulate) o += *(const f32x4*)cptr;
      *(f32x4*)cptr = o;
    }
  if (!p.accumulate)  // the padding rows of C
    for (int idx = tid; idx < (128 - 16 * PB) * 32; idx += 256) {
      const int row = 16 * PB + (idx >> 5), c4 = (idx & 31) * 4;
      *(f32x4*)((float*)p.C + (long)row * p.ldc + q0 + c4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// p_valid: B is a rank-r operand in the first rows of a 128-row zero-padded buffer (u = x (sA*mask)^T, du = dy (sB)): the
// load-stream kernel, which writes only the data columns of C.
// -> number of 16-row blocks of B that hold data (0: not that form)
int wft_nt_rank_pb(const wft_gemm_args* a) {
  return (!a->c_is_f32 && a->N == 128 && a->batch == 1 && a->p_valid > 0 && a->p_valid <= 64 && a->epilogue == WFT_EPI_NONE &&
          !a->bias && !a->residual && !a->aux && !a->colsum && a->valid_rows_period == 0)
             ? (a->p_valid + 15) / 16 : 0;
}

// the kernels take TWO products per launch (workgroups >= n0 work on p1): the paired entry points pass both, a single product
// is (p, p, its grid, 0)
template <bool TN, int PB>
static int launch_rank_pb(const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s) {
  constexpr int nst = PB <= 2 ? 4 : 3;
  constexpr int bytes = nst * (16384 + 2048 * PB);
  const dim3 grid((unsigned)(n0 + n1)), block(256);
  if constexpr (TN) return wft_launch_lds<gemm_tn_rank_kernel<PB>>(grid, block, bytes, s, p0, p1, n0);
  else return wft_launch_lds<gemm_nt_rank_kernel<PB>>(grid, block, bytes, s, p0, p1, n0);
}
template <bool TN>
static int launch_rank(int pb, const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s) {
  switch (pb) {
    case 1: return launch_rank_pb<TN, 1>(p0, p1, n0, n1, s);
    case 2: return launch_rank_pb<TN, 2>(p0, p1, n0, n1, s);
    case 3: return launch_rank_pb<TN, 3>(p0, p1, n0, n1, s);
    default: return launch_rank_pb<TN, 4>(p0, p1, n0, n1, s);
  }
}
int wft_nt_rank_launch(int pb, const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s) { return launch_rank<false>(pb, p0, p1, n0, n1, s); }
int wft_tn_rank_launch(int pb, const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s) { return launch_rank<true>(pb, p0, p1, n0, n1, s); }
