// gemm.hip — host side of the bf16 MFMA GEMMs for the Linear / Conv1d-as-GEMM / logits paths: argument check, plan, entry points.
//
//   wft_gemm_nt_bf16 : C[M,N] = A[M,K] · B[N,K]^T   (forward, backward-data with a transposed weight shadow)
//   wft_gemm_tn_bf16 : C[P,Q] = A[R,P]^T · B[R,Q]   (weight gradients)
//
// The kernels live in one file per family, each with its eligibility rule, thresholds, timing-build switches and launch
// (gemm_common.h lists what they offer): gemm_nt4w.hip / gemm_tn4w.hip (256x256, one wave per SIMD), gemm_pp256.hip (256x256,
// 8-wave ping-pong), gemm_nt128.hip / gemm_tn128.hip (128x128), gemm_rank.hip (rank-r operands).  Which kernel serves a call, on
// which grid, with how many K splits and how much workspace is decided ONCE per family, by nt_plan / tn_plan below: the dispatch
// and workspace queries, the launchers and the paired entry points all read that plan, and nt_check / tn_check are each family's
// one argument check.  Only the split-K reduce kernels of the TN family are device code here: every TN kernel feeds them.
#include "gemm_common.h"
#include <stdlib.h>

// split-K reduction: C[p][q] (+)= sum_s ws[s][p][q], splits added in index order (reproducible)
// Rows P .. Pz-1 of C (the padding rows of a rank-r operand, absent from the workspace) are written as zero.
// col_scale / blk_n: the LoRA adapter-gradient forms of wft_gemm_args (tn_col_scale, tn_block_n): a per-(row group, column)
// factor, and the transposed block-diagonal output.
struct TnReduceP {
  const float* ws; float* C; long ldc; int P, Q, nsplit, accumulate, Pz; const float* col_scale; int scale_rows, blk_n, blk_r, Pv;
};
__device__ __forceinline__ void tn_splitk_reduce_body(const float* ws, float* C, long ldc, int P, int Q, int nsplit,
                                                      int accumulate, int Pz, const float* col_scale, int scale_rows,
                                                      int blk_n, int blk_r, int Pv, long bid, long nblk) {
  const long nq4 = Q >> 2;
  const long total = (long)(Pz > P ? Pz : P) * nq4;
  for (long i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
    const long pp = i / nq4, q4 = (i - pp * nq4) * 4;
    float* cp = C + pp * ldc + q4;
    if (col_scale && blk_n == 0 && pp >= Pv) continue;  // col-scale form: C has p_valid rows, nothing is written below them
    if (pp >= P) {
      if (!accumulate && blk_n == 0) *(f32x4*)cp = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    int pr = 0;
    float* ob = nullptr;
    if (blk_n > 0) {
      const int blk = (int)(q4 / blk_n);  // q4 .. q4+3 lie in one block (blk_n % 4 == 0)
      pr = (int)pp - blk * blk_r;
      if (pr < 0 || pr >= blk_r) continue;  // off-diagonal: not stored
      ob = C + (long)blk * blk_n * blk_r + (q4 - (long)blk * blk_n) * blk_r + pr;
    }
    const bool plain = !col_scale && !ob;
    // plain form: C (+)= sum of the splits, starting from C when accumulating (the order the 256x256 path always had)
    f32x4 s = (plain && accumulate) ? *(const f32x4*)cp : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < nsplit; ++k) s += *(const f32x4*)(ws + ((long)k * P + pp) * Q + q4);
    if (plain) {
      *(f32x4*)cp = s;
      continue;
    }
    // rows >= Pv (p_valid rounded up to 16 leaves up to 15 of them) are sums of zeros and have no scale row
    if (col_scale && pp < Pv) s *= *(const f32x4*)(col_scale + (scale_rows > 0 ? pp / scale_rows : 0) * Q + q4);
    if (ob) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[(long)e * blk_r] = accumulate ? ob[(long)e * blk_r] + s[e] : s[e];
    } else {
      if (accumulate) s += *(const f32x4*)cp;
      *(f32x4*)cp = s;
    }
  }
}

__global__ __launch_bounds__(256) void tn_splitk_reduce_kernel(const float* ws, float* C, long ldc, int P, int Q, int nsplit,
                                                                int accumulate, int Pz, const float* col_scale, int scale_rows,
                                                                int blk_n, int blk_r, int Pv) {
  tn_splitk_reduce_body(ws, C, ldc, P, Q, nsplit, accumulate, Pz, col_scale, scale_rows, blk_n, blk_r, Pv, (long)blockIdx.x, (long)gridDim.x);
}
// the plain form with SEGMENTED output (wft_gemm_args tn_seg_*): row range i of the product goes to its own contiguous [rows][Q]
// tensor — each parameter of a fused Linear group gets its gradient where it lives (a DDP bucket view).  Same order of additions
// as tn_splitk_reduce_body: C first when accumulating, then the splits in index order.
struct TnSegs { float* ptr[4]; int end[4]; };
__global__ __launch_bounds__(256) void tn_splitk_reduce_seg_kernel(const float* ws, TnSegs sg, int P, int Q, int nsplit, int accumulate) {
  const long nq4 = Q >> 2;
  const long total = (long)P * nq4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long pp = i / nq4, q4 = (i - pp * nq4) * 4;
    int sgi = 0, start = 0;
    while (sgi < 3 && pp >= sg.end[sgi]) start = sg.end[sgi++];
    float* cp = sg.ptr[sgi] + (pp - start) * Q + q4;
    f32x4 s = accumulate ? *(const f32x4*)cp : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < nsplit; ++k) s += *(const f32x4*)(ws + ((long)k * P + pp) * Q + q4);
    *(f32x4*)cp = s;
  }
}
// both adapter gradients of a group (dA with its column scale, dB in block layout) in ONE launch: workgroups >= g0 take r1
__global__ __launch_bounds__(256) void tn_splitk_reduce_pair_kernel(TnReduceP r0, TnReduceP r1, int g0) {
  const bool second = (int)blockIdx.x >= g0;
  const TnReduceP& r = second ? r1 : r0;
  tn_splitk_reduce_body(r.ws, r.C, r.ldc, r.P, r.Q, r.nsplit, r.accumulate, r.Pz, r.col_scale, r.scale_rows, r.blk_n, r.blk_r, r.Pv,
                        (long)blockIdx.x - (second ? g0 : 0), (long)(second ? (int)gridDim.x - g0 : g0));
}

// ---------------------------------------------------------------------------------- check
// WFT_GEMM_DIAG (timing builds): read once; the kernel files see it as GemmP.diag or as an argument of their rules
static const int g_diag = [] { const char* e = wft_dev_getenv("WFT_GEMM_DIAG"); return e ? atoi(e) : 0; }();
// NT256 / NT4W tile-order band width in column tiles
static const int g_nt256_band = [] { const char* e = wft_dev_getenv("WFT_NT256_BAND"); return (e && atoi(e) > 0) ? atoi(e) : 5; }();

static void fill_params(const wft_gemm_args* a, GemmP& p) {
  p.A = a->A; p.lda = a->lda; p.sA = a->strideA;
  p.B = a->B; p.ldb = a->ldb; p.sB = a->strideB;
  p.C = a->C; p.ldc = a->ldc; p.sC = a->strideC;
  p.bias = a->bias;
  p.res = a->residual; p.ldr = a->ldr; p.sR = a->strideR;
  p.aux = a->aux; p.ldaux = a->ldaux; p.sAux = a->strideAux;
  p.alpha = a->alpha;
  p.beta = a->beta == 0.f ? 1.f : a->beta;
  p.M = (int)a->M; p.N = (int)a->N; p.K = (int)a->K; p.batch = a->batch;
  p.accumulate = a->accumulate;
  p.period = a->valid_rows_period; p.valid = a->valid_rows;
  p.res_first = a->residual_first;
  p.diag = g_diag;
  p.band = g_nt256_band;
  p.ws = nullptr;
  p.cs_part = nullptr;
  p.nsplit = 1;
}

// the caller granted at least `bytes` of 16-byte aligned workspace
static bool ws_granted(const wft_gemm_args* a, int64_t bytes) {
  return a->workspace && a->workspace_bytes >= bytes && (((uintptr_t)a->workspace) & 15) == 0;
}

// what both families check alike
static int gemm_check_common(const wft_gemm_args* a, const char* who) {
  WFT_CHECK_ARG_AS(who, a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 4 == 0, "ld alignment");
  WFT_CHECK_ARG_AS(who, ((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->B & 15) == 0 && ((uintptr_t)a->C & 15) == 0,
                   "base pointers must be 16-byte aligned");
  WFT_CHECK_ARG_AS(who, !(a->accumulate && !a->c_is_f32), "accumulate needs an f32 C");
  return WFT_OK;
}

// dispatch thresholds between the 128x128 and the 256x256 kernels (one-wave-per-SIMD and ping-pong alike), measured at
// M = R = 4096 and 8704 (decoder-sized problems; tools/dev/small_gemm_time.py): the 256x256 kernels win once they can occupy half
// of the CUs (NT: >= 128 tiles) / have >= 50 output tiles to split (TN)
static const int g_force_128 = [] { const char* e = wft_dev_getenv("WFT_GEMM_FORCE_128"); return (e && e[0] == '1') ? 1 : 0; }();
static const int g_nt256_min_tiles = [] { const char* e = wft_dev_getenv("WFT_NT256_MIN_TILES"); return e ? atoi(e) : 128; }();
static const int g_tn256_min_steps = [] { const char* e = wft_dev_getenv("WFT_TN256_MIN_STEPS"); return e ? atoi(e) : 64; }();
static const int g_tn256_min_out_tiles = [] { const char* e = wft_dev_getenv("WFT_TN256_MIN_OUT_TILES"); return e ? atoi(e) : 50; }();

// ---------------------------------------------------------------------------------- NT
// big, 256-aligned-N problems go to the 256x256 kernels (one workgroup per CU, 128 KiB LDS and more)
static bool nt_uses_256(const wft_gemm_args* a) {
  const bool wide_ok = a->c_is_f32 || (a->ldc % 8 == 0 && (!a->residual || (a->ldr % 8 == 0 && ((uintptr_t)a->residual & 15) == 0)) &&
                                       (!a->aux || (a->ldaux % 8 == 0 && ((uintptr_t)a->aux & 15) == 0)) &&
                                       (!a->bias || ((uintptr_t)a->bias & 15) == 0));
  return !g_force_128 && wide_ok && a->N % 256 == 0 && a->M >= 1024 &&
         ((a->M + 255) / 256) * (a->N / 256) * a->batch >= g_nt256_min_tiles;
}
static bool epi_is_aux8(int e) { return e == WFT_EPI_GELU_GRAD8 || e == WFT_EPI_MUL_AUX8; }

// launch state is per call (wft_gemm_args.launch_mode / variant); the process-wide start values come from the environment at load
// time only (WFT_NT256_PERSISTENT; the variant variables in timing builds) and never change afterwards.
// persistent (one workgroup per CU walks the tiles, prefetching across tile seams) unless WFT_NT256_PERSISTENT=0: with
// collectives running beside the GEMMs (DDP over RCCL) some CUs are busy when the kernel starts, and a static tile
// walk would leave their share for the end; one workgroup per tile lets the hardware dispatcher balance instead
static const int g_nt256_persistent = [] { const char* e = getenv("WFT_NT256_PERSISTENT"); return (e && e[0] == '0') ? 0 : 1; }();
// which 256x256 NT kernel: 0 = the one-wave-per-SIMD kernel where it applies (gemm_nt4w.hip), 1 = always the ping-pong kernel
// (gemm_pp256.hip).  WFT_NT_VARIANT=pp|4w at load time (timing builds); per call: wft_gemm_args.variant.
static const int g_nt_variant = [] { const char* e = wft_dev_getenv("WFT_NT_VARIANT"); return (e && e[0] == 'p') ? 1 : 0; }();

struct NtPlan {
  NtKind kind = NT_128_2BUF;
  unsigned grid_x = 0, grid_z = 1;
  int pb = 0;                // NT_RANK: wft_nt_rank_pb
  int nsplit = 1, per = 0;   // NT_128_SPLITK: K splits, k-steps per split
  // what the three size queries answer (0: not served in that form); colsum_bytes and splitk_bytes are workspace to grant
  int64_t aux8_bytes = 0, colsum_bytes = 0, splitk_bytes = 0;
  bool cs_fused = false;     // the column sums come out of the GEMM's epilogue (their workspace was granted)
};
static NtPlan nt_plan(const wft_gemm_args* a) {
  NtPlan pl;
  if (!a) return pl;
  const int ncu = wft_num_cus();
  if (nt_uses_256(a)) {
    const long tm = (a->M + 255) / 256, tn = a->N / 256, t256 = tm * tn * a->batch;
    pl.kind = (g_nt_variant != 1 && a->variant == 0 && wft_nt4w_eligible(a)) ? NT_4W : NT_256;
    const bool persistent = g_nt256_persistent && a->launch_mode != 1;
    pl.grid_x = (unsigned)((t256 < ncu || !persistent) ? t256 : ncu);
    // 16 KiB of one-byte gelu' per (256x256 tile, wave) = one byte per tile element: only gemm_nt4w_kernel carries the two epilogues
    if (pl.kind == NT_4W && epi_is_aux8(a->epilogue)) pl.aux8_bytes = tm * tn * 65536;
    if (a->colsum && !a->c_is_f32 && a->batch == 1) {
      pl.colsum_bytes = 2 * tm * a->N * (int64_t)sizeof(float);
      pl.cs_fused = ws_granted(a, pl.colsum_bytes) && ((uintptr_t)a->colsum & 15) == 0;  // (16-byte accesses in the reduce kernel)
    }
    return pl;
  }
  pl.pb = wft_nt_rank_pb(a);
  if (pl.pb) {
    pl.kind = NT_RANK;
    pl.grid_x = (unsigned)((a->M + 127) / 128);
    return pl;
  }
  pl.grid_x = (unsigned)(((a->M + 127) / 128) * (a->N / 128));
  pl.grid_z = (unsigned)a->batch;
  pl.kind = wft_nt128_ring(a, g_diag) ? NT_128_RING : NT_128_2BUF;
  pl.nsplit = wft_nt128_splitk_plan(a, g_diag, &pl.per);
  if (pl.nsplit > 1) {  // (which implies the ring form: at most half a workgroup per CU)
    pl.splitk_bytes = (int64_t)pl.nsplit * a->M * a->N * 4;
    if (ws_granted(a, pl.splitk_bytes)) {
      pl.kind = NT_128_SPLITK;
      pl.grid_z = (unsigned)pl.nsplit;
    }
  }
  return pl;
}

static int nt_check(const wft_gemm_args* a, const NtPlan& pl, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->A && a->B && a->C, "null pointer");
  WFT_CHECK_ARG_AS(who, a->M >= 1 && a->N >= 128 && a->K >= 64 && a->batch >= 1, "bad shape");
  WFT_CHECK_ARG_AS(who, a->N % 128 == 0, "N must be a multiple of 128");
  WFT_CHECK_ARG_AS(who, a->K % 64 == 0, "K must be a multiple of 64");
  const int rc = gemm_check_common(a, who);
  if (rc != WFT_OK) return rc;
  const bool aux8 = epi_is_aux8(a->epilogue);
  WFT_CHECK_ARG_AS(who, (a->epilogue != WFT_EPI_DGELU && a->epilogue != WFT_EPI_GELU_GRAD && a->epilogue != WFT_EPI_MUL_AUX && !aux8) || a->aux,
                   "DGELU / GELU_GRAD / MUL_AUX epilogues need aux");
  WFT_CHECK_ARG_AS(who, (a->epilogue != WFT_EPI_GELU_GRAD && a->epilogue != WFT_EPI_MUL_AUX && !aux8) || !a->c_is_f32,
                   "GELU_GRAD / MUL_AUX epilogues write a bf16 C");
  if (aux8 && pl.aux8_bytes == 0) {
    wft_set_error("%s: the one-byte gelu' epilogues exist on gemm_nt4w_kernel only (ask wft_gemm_nt_aux8_bytes first)", who);
    return WFT_ERR_UNSUPPORTED;
  }
  WFT_CHECK_ARG_AS(who, a->M < (1ll << 31) && a->N < (1ll << 31) && a->K < (1ll << 31), "dims exceed int32");
  if (a->colsum) WFT_CHECK_ARG_AS(who, !a->c_is_f32 && a->batch == 1, "colsum needs a bf16 C and batch == 1");
  return WFT_OK;
}

extern "C" int wft_gemm_nt_variant(const wft_gemm_args* a) {
  const NtKind k = nt_plan(a).kind;
  return k == NT_4W ? 4 : k == NT_256 ? 256 : 128;
}
extern "C" int64_t wft_gemm_nt_aux8_bytes(const wft_gemm_args* a) { return nt_plan(a).aux8_bytes; }
extern "C" int64_t wft_gemm_nt_colsum_workspace_bytes(const wft_gemm_args* a) { return nt_plan(a).colsum_bytes; }
extern "C" int64_t wft_gemm_nt_splitk_workspace_bytes(const wft_gemm_args* a) { return nt_plan(a).splitk_bytes; }

extern "C" int wft_gemm_nt_bf16(const wft_gemm_args* a, void* stream) {
  const NtPlan pl = nt_plan(a);
  int rc = nt_check(a, pl, __func__);
  if (rc != WFT_OK) return rc;
  GemmP p;
  fill_params(a, p);
  if (pl.cs_fused) p.cs_part = (float*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  switch (pl.kind) {
    case NT_4W: rc = wft_nt4w_launch(a, p, pl.grid_x, stream); break;
    case NT_256: rc = wft_nt256_launch(a, p, pl.grid_x, s); break;
    case NT_RANK: rc = wft_nt_rank_launch(pl.pb, p, p, (int)pl.grid_x, 0, s); break;
    default: rc = wft_nt128_launch(a, p, pl.kind, pl.nsplit, pl.per, dim3(pl.grid_x, 1, pl.grid_z), s); break;
  }
  if (rc != WFT_OK) return rc;
  // column sums of C: finished from the epilogue's partial rows, or (not fused) a second pass over C
  if (pl.cs_fused) wft_nt_colsum_reduce_launch(a, s);
  WFT_CHECK_LAUNCH();
  if (a->colsum && !pl.cs_fused) return wft_colsum_bf16((const wft_bf16*)a->C, a->M, a->N, a->ldc, a->colsum, 0, stream);
  return WFT_OK;
}

// ---------------------------------------------------------------------------------- TN
static bool tn_uses_256(const wft_gemm_args* a) {
  const long nsteps = ((a->K + 63) / 64) * a->batch;
  // (round 5: 25 output tiles — a decoder block's 1280 x 1280 gradients — take the 256 x 256 kernel from 8 192 reduction rows on:
  // 59 -> 57 us at R = 8 704, 66 -> 56 us at R = 11 136, but 35 -> 53 us at R = 4 096; tools/dev/tn_small.py)
  const long t256 = (a->M / 256) * (a->N / 256);
  return !g_force_128 && a->c_is_f32 && a->M % 256 == 0 && a->N % 256 == 0 && nsteps >= g_tn256_min_steps &&
         (nsteps >= 256 || t256 >= g_tn256_min_out_tiles || (t256 >= g_tn256_min_out_tiles / 2 && nsteps >= 128));
}
// the adapter-gradient forms (column scale / block-transposed output) are applied by the reduce kernel: always through the workspace
static bool tn_needs_reduce(const wft_gemm_args* a) { return a->tn_col_scale != nullptr || a->tn_block_n > 0; }
// the one-wave-per-SIMD weight-gradient kernel (gemm_tn4w.hip): WFT_TN_VARIANT=pp keeps gemm_tn256_kernel
static const int g_tn_variant = [] { const char* e = wft_dev_getenv("WFT_TN_VARIANT"); return (e && e[0] == 'p') ? 1 : 0; }();

struct TnPlan {
  TnKind kind = TN_128_2BUF;
  long tiles = 0;            // output tiles of the kernel's tile size (256 x 256: TN_4W, TN_256; else 128 x 128)
  int nsplit = 1, per = 0;   // K splits; TN_4W: reduction steps per split
  int pb = 0;                // wft_tn128_pb (TN_RANK, TN_128_PB)
  int64_t ws_rows = 0;       // rows of a split's partial tile kept in the workspace
  int64_t part_bytes = 0;    // the partial tiles [nsplit][ws_rows][Q] of the kernel chosen
  int64_t ws_bytes = 0;      // what wft_gemm_tn_workspace_bytes answers: the workspace to grant (0: none wanted)
  bool use_ws = false;       // the partial tiles go to the granted workspace and the reduce kernel finishes C
};
static TnPlan tn_plan(const wft_gemm_args* a) {
  TnPlan pl;
  if (!a) return pl;
  const bool seg = a->tn_seg_count > 0;  // segmented output: always through the workspace, even unsplit
  const auto part = [&](int nsplit) { return (int64_t)nsplit * pl.ws_rows * a->N * 4; };
  if (tn_uses_256(a)) {
    pl.tiles = (a->M / 256) * (a->N / 256);
    pl.ws_rows = a->M;
    const int ns256 = wft_tn256_nsplit(a);
    int ns4 = 0, per4 = 0;
    const bool elig4 = wft_tn4w_eligible(a);
    if (elig4) wft_tn4w_plan(a, &ns4, &per4);
    // (the larger of the two kernels' plans: with it granted, the call is served whichever of them the variant switch selects)
    const int nsq = ns4 > ns256 ? ns4 : ns256;
    pl.ws_bytes = (nsq > 1 || seg || tn_needs_reduce(a)) ? part(nsq) : 0;
    if (elig4 && g_tn_variant != 1 && a->variant == 0) {
      const bool use4 = (ns4 > 1 || seg) && ws_granted(a, part(ns4));
      if (ns4 == 1 || use4) {  // (split without a workspace: the ping-pong kernel's atomic path)
        pl.kind = TN_4W; pl.nsplit = ns4; pl.per = per4; pl.use_ws = use4; pl.part_bytes = part(ns4);
        return pl;
      }
    }
    pl.kind = TN_256; pl.nsplit = ns256; pl.part_bytes = part(ns256);
    pl.use_ws = (ns256 > 1 || seg) && ws_granted(a, pl.part_bytes);
    return pl;
  }
  pl.tiles = (a->M / 128) * (a->N / 128);
  const bool ring = wft_tn128_ring(a, g_diag);
  pl.nsplit = wft_tn128_nsplit(a, ring);
  pl.pb = wft_tn128_pb(a);
  pl.ws_rows = pl.pb ? 16 * pl.pb : a->M;
  pl.part_bytes = part(pl.nsplit);
  const bool want_ws = pl.nsplit > 1 || tn_needs_reduce(a);
  pl.ws_bytes = (want_ws || seg) ? pl.part_bytes : 0;
  pl.use_ws = want_ws && ws_granted(a, pl.part_bytes);
  // p_valid: A is a rank-r operand in a 128-wide zero-padded buffer — its own load-stream kernel (gemm_tn_rank_kernel); the
  // 128-tile kernel only when a split-K run was given no workspace
  if (pl.pb > 0 && (pl.nsplit == 1 || pl.use_ws)) pl.kind = TN_RANK;
  else if (!a->c_is_f32) pl.kind = TN_128_BF16C;
  else if (pl.pb > 0) pl.kind = TN_128_PB;
  else pl.kind = ring ? TN_128_RING : TN_128_2BUF;
  return pl;
}

extern "C" int wft_gemm_tn_segments_ok(const wft_gemm_args* a) {
  const TnKind k = tn_plan(a).kind;
  if ((k != TN_4W && k != TN_256) || a->tn_seg_count < 1 || a->tn_seg_count > 4 || tn_needs_reduce(a) || a->p_valid != 0 || a->batch != 1) return 0;
  int prev = 0;
  for (int i = 0; i < a->tn_seg_count; ++i) {
    if (a->tn_seg_end[i] <= prev || !a->tn_seg_ptr[i] || (((uintptr_t)a->tn_seg_ptr[i]) & 15) != 0) return 0;
    prev = a->tn_seg_end[i];
  }
  return prev == a->M ? 1 : 0;
}
extern "C" int64_t wft_gemm_tn_workspace_bytes(const wft_gemm_args* a) { return tn_plan(a).ws_bytes; }
// 4 gemm_tn4w_kernel, 256 gemm_tn256_kernel, 128 the 128-tile kernel and its rank-r load-stream form
extern "C" int wft_gemm_tn_variant(const wft_gemm_args* a) {
  const TnKind k = tn_plan(a).kind;
  return k == TN_4W ? 4 : k == TN_256 ? 256 : 128;
}

static int tn_check(const wft_gemm_args* a, const TnPlan& pl, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->A && a->B && a->C, "null pointer");
  WFT_CHECK_ARG_AS(who, a->M >= 128 && a->N >= 128 && a->K >= 1 && a->batch >= 1, "bad shape");
  WFT_CHECK_ARG_AS(who, a->M % 128 == 0 && a->N % 128 == 0, "P and Q must be multiples of 128");
  const int rc = gemm_check_common(a, who);
  if (rc != WFT_OK) return rc;
  WFT_CHECK_ARG_AS(who, a->M < (1ll << 31) && a->N < (1ll << 31) && a->K < (1ll << 31), "dims exceed int32");
  if (tn_needs_reduce(a)) {
    WFT_CHECK_ARG_AS(who, pl.pb > 0, "tn_col_scale / tn_block_n need a rank-r operand (P = 128, 0 < p_valid <= 64)");
    WFT_CHECK_ARG_AS(who, ws_granted(a, pl.ws_bytes), "tn_col_scale / tn_block_n need the workspace of wft_gemm_tn_workspace_bytes");
    WFT_CHECK_ARG_AS(who, a->tn_scale_rows >= 0 && (((uintptr_t)a->tn_col_scale) & 15) == 0, "tn_col_scale: 16-byte aligned f32 [S][Q]");
    if (a->tn_block_n > 0)
      WFT_CHECK_ARG_AS(who, a->tn_block_n % 4 == 0 && a->N % a->tn_block_n == 0 && a->tn_block_r >= 1 &&
                       (a->N / a->tn_block_n) * (int64_t)a->tn_block_r <= 16 * pl.pb, "tn_block_n / tn_block_r do not tile the product");
  }
  if (a->tn_seg_count > 0)
    WFT_CHECK_ARG_AS(who, wft_gemm_tn_segments_ok(a) && ws_granted(a, pl.ws_bytes),
                     "tn_seg_*: not a segmentable call (wft_gemm_tn_segments_ok) or no workspace");
  return WFT_OK;
}

static TnSegs tn_segs_of(const wft_gemm_args* a) {
  TnSegs sg;
  for (int i = 0; i < 4; ++i) {
    const int j = i < a->tn_seg_count ? i : a->tn_seg_count - 1;
    sg.ptr[i] = a->tn_seg_ptr[j];
    sg.end[i] = i < a->tn_seg_count ? a->tn_seg_end[i] : 0x7fffffff;
  }
  return sg;
}
// the kernel that sums the split-K partial tiles of the workspace into C (and applies the adapter-gradient forms)
static unsigned tn_reduce_grid(const wft_gemm_args* a) {
  const long g = (a->M * (a->N / 4) + 255) / 256;
  return (unsigned)(g > 2048 ? 2048 : g);
}
static TnReduceP tn_reduce_params(const wft_gemm_args* a, const TnPlan& pl) {
  return TnReduceP{(const float*)a->workspace, (float*)a->C, (long)a->ldc, (int)pl.ws_rows, (int)a->N, pl.nsplit, a->accumulate, (int)a->M,
                   a->tn_col_scale, a->tn_scale_rows, a->tn_block_n, a->tn_block_r, pl.pb > 0 ? a->p_valid : (int)a->M};
}
static void launch_tn_reduce(const wft_gemm_args* a, const TnPlan& pl, hipStream_t s) {
  const dim3 grid(tn_reduce_grid(a)), block(256);
  if (a->tn_seg_count > 0) {
    hipLaunchKernelGGL(tn_splitk_reduce_seg_kernel, grid, block, 0, s, (const float*)a->workspace, tn_segs_of(a), (int)a->M, (int)a->N,
                       pl.nsplit, a->accumulate);
    return;
  }
  const TnReduceP r = tn_reduce_params(a, pl);
  hipLaunchKernelGGL(tn_splitk_reduce_kernel, grid, block, 0, s, r.ws, r.C, r.ldc, r.P, r.Q, r.nsplit, r.accumulate, r.Pz, r.col_scale,
                     r.scale_rows, r.blk_n, r.blk_r, r.Pv);
}

extern "C" int wft_gemm_tn_bf16(const wft_gemm_args* a, void* stream) {
  const TnPlan pl = tn_plan(a);
  int rc = tn_check(a, pl, __func__);
  if (rc != WFT_OK) return rc;
  GemmP p;
  fill_params(a, p);
  hipStream_t s = (hipStream_t)stream;
  if (pl.use_ws) p.ws = (float*)a->workspace;
  else if (pl.nsplit > 1 && !a->accumulate)  // (the splits add to C atomically)
    (void)hipMemset2DAsync(a->C, (size_t)a->ldc * 4, 0, (size_t)a->N * 4, (size_t)a->M, s);
  const unsigned grid1d = (unsigned)(pl.tiles * pl.nsplit);  // the 256x256 and rank kernels: (tile, split) pairs on a 1-D grid
  switch (pl.kind) {
    case TN_4W:
      p.nsplit = pl.nsplit;
      p.band = pl.per;  // (reused field: reduction steps per split)
      rc = wft_tn4w_launch(p, grid1d, stream);
      break;
    case TN_256:
      p.nsplit = pl.nsplit;
      rc = wft_tn256_launch(p, grid1d, s);
      break;
    case TN_RANK:
      p.nsplit = pl.nsplit;
      rc = wft_tn_rank_launch(pl.pb, p, p, (int)grid1d, 0, s);
      break;
    default: rc = wft_tn128_launch(p, pl.kind, pl.pb, dim3((unsigned)pl.tiles, (unsigned)pl.nsplit), s); break;
  }
  if (rc != WFT_OK) return rc;
  if (pl.use_ws) launch_tn_reduce(a, pl, s);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ---------------------------------------------------------------------------------- paired rank-r launches (round 3)
// The four rank-r products of one adapted Linear group's backward are two independent pairs: {u = x (sA*m)^T, du = dy (sB)} and
// {dA = du^T x, dB^T = u^T dy}.  Each pair goes out as ONE launch of the load-stream kernel (and the two split-K reduces of the
// second pair as one): half the launches, and a grid that fills the chip (an NT rank product alone is 1.46 rounds of 256 CUs at
// 32 clips).  Same arithmetic per product as the single entry points: bit-identical results.  Anything the load-stream kernels do
// not take falls back to two calls of the single entry point, which reports what is wrong with it.
extern "C" int wft_gemm_nt_rank_pair_bf16(const wft_gemm_args* a0, const wft_gemm_args* a1, void* stream) {
  WFT_CHECK_ARG(a0 && a1, "null pointer");
  const NtPlan pl0 = nt_plan(a0), pl1 = nt_plan(a1);
  if (pl0.kind != NT_RANK || pl1.kind != NT_RANK || pl0.pb != pl1.pb ||
      nt_check(a0, pl0, __func__) != WFT_OK || nt_check(a1, pl1, __func__) != WFT_OK) {
    const int rc = wft_gemm_nt_bf16(a0, stream);
    return rc != WFT_OK ? rc : wft_gemm_nt_bf16(a1, stream);
  }
  GemmP p0, p1;
  fill_params(a0, p0);
  fill_params(a1, p1);
  const int rc = wft_nt_rank_launch(pl0.pb, p0, p1, (int)pl0.grid_x, (int)pl1.grid_x, (hipStream_t)stream);
  if (rc != WFT_OK) return rc;
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// both through the workspace + reduce (what the adapter-gradient forms tn_col_scale / tn_block_n always do)
extern "C" int wft_gemm_tn_rank_pair_bf16(const wft_gemm_args* a0, const wft_gemm_args* a1, void* stream) {
  WFT_CHECK_ARG(a0 && a1, "null pointer");
  const wft_gemm_args* as[2] = {a0, a1};
  const TnPlan pl[2] = {tn_plan(a0), tn_plan(a1)};
  bool paired = pl[0].pb == pl[1].pb;
  for (int i = 0; i < 2 && paired; ++i)
    paired = pl[i].kind == TN_RANK && ws_granted(as[i], pl[i].part_bytes) && tn_check(as[i], pl[i], __func__) == WFT_OK;
  if (!paired) {
    const int rc = wft_gemm_tn_bf16(a0, stream);
    return rc != WFT_OK ? rc : wft_gemm_tn_bf16(a1, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  GemmP p[2];
  TnReduceP r[2];
  int nb[2], gr[2];
  for (int i = 0; i < 2; ++i) {
    fill_params(as[i], p[i]);
    p[i].ws = (float*)as[i]->workspace;
    p[i].nsplit = pl[i].nsplit;
    nb[i] = (int)(pl[i].tiles * pl[i].nsplit);
    gr[i] = (int)tn_reduce_grid(as[i]);
    r[i] = tn_reduce_params(as[i], pl[i]);
  }
  const int rc = wft_tn_rank_launch(pl[0].pb, p[0], p[1], nb[0], nb[1], s);
  if (rc != WFT_OK) return rc;
  hipLaunchKernelGGL(tn_splitk_reduce_pair_kernel, dim3((unsigned)(gr[0] + gr[1])), dim3(256), 0, s, r[0], r[1], gr[0]);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
