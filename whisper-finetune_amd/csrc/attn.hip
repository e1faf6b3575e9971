// attn.hip — host side of attention: argument check, dispatch plan, entry points (+ the kernel that folds the column-sum partials).
// The kernels live in attn_fwd.hip, attn_bwd.hip, attn_dq4w.hip, attn_dkdv4w.hip, each with its eligibility rule and launch.
#include "attn_common.h"

static void attn_fill(const wft_attn_args* a, AttnP& p) {
  p.q = a->q; p.ldq = a->ldq; p.q_bs = a->q_bs;
  p.k = a->k; p.ldk = a->ldk; p.k_bs = a->k_bs;
  p.v = a->v; p.ldv = a->ldv; p.v_bs = a->v_bs;
  p.o = a->o; p.ldo = a->ldo; p.o_bs = a->o_bs;
  p.lse = a->lse;
  p.B = a->B; p.H = a->H; p.Tq = a->Tq; p.Tk = a->Tk; p.causal = a->causal;
  p.scale = a->scale;
  p.qpre = a->q_prescaled ? 1 : 0;
  p.c = p.qpre ? 1.0f : a->scale * LOG2E;
  p.ls = p.qpre ? LN2 : a->scale;
  p.d_o = a->d_o; p.lddo = a->lddo; p.do_bs = a->do_bs;
  p.delta = a->delta;
  p.dq = a->dq; p.lddq = a->lddq; p.dq_bs = a->dq_bs;
  p.dk = a->dk; p.lddk = a->lddk; p.dk_bs = a->dk_bs;
  p.dv = a->dv; p.lddv = a->lddv; p.dv_bs = a->dv_bs;
  p.cs_q = nullptr; p.cs_v = nullptr;
  static const int xcd_on = [] { const char* e = wft_dev_getenv("WFT_ATTN_XCD"); return e ? atoi(e) : 1; }();
  p.xcd = xcd_on;
}

// out[chunk][col] = sum over this chunk's partial rows (fixed order).  64 columns per workgroup (256-byte row segments),
// 4 waves stride the rows; gridDim.y row chunks.  Run twice: [nrows] -> [ATT_CS_CHUNKS] -> [1].
#define ATT_CS_CHUNKS 32
__global__ __launch_bounds__(256) void attn_colsum_reduce_kernel(const float* partial0, long nrows0, float* out0,
                                                                 const float* partial1, long nrows1, float* out1, int n) {
  // blockIdx.z = 0: the q-projection's sums, 1: the v-projection's (one launch per level for both)
  const float* partial = blockIdx.z ? partial1 : partial0;
  const long nrows = blockIdx.z ? nrows1 : nrows0;
  float* out = blockIdx.z ? out1 : out0;
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cx;
  const long per = (nrows + gridDim.y - 1) / gridDim.y;
  const long r0 = (long)blockIdx.y * per;
  const long r1 = r0 + per < nrows ? r0 + per : nrows;
  float sacc = 0.f;
  if (col < n)
    for (long rr = r0 + wv; rr < r1; rr += 4) sacc += partial[rr * n + col];
  red[wv][cx] = sacc;
  __syncthreads();
  if (wv == 0 && col < n) out[(long)blockIdx.y * n + col] = red[0][cx] + red[1][cx] + red[2][cx] + red[3][cx];
}

// one check for forward and backward; who / align_msg: the entry point's name and its wording of the alignment rule
#define ATT_ALIGNED(ptr, ld, bs) ((((uintptr_t)(ptr)) & 15) == 0 && ((ld) % 8) == 0 && ((bs) % 8) == 0)
static int attn_check(const wft_attn_args* a, bool bwd, const char* who, const char* align_msg) {
  WFT_CHECK_ARG_AS(who, a && a->q && a->k && a->v && a->o && a->lse &&
                            (!bwd || (a->d_o && a->delta && a->dq && a->dk && a->dv)),
                   "null pointer");
  WFT_CHECK_ARG_AS(who, a->B >= 1 && a->H >= 1 && a->Tq >= 1 && a->Tk >= 1, "bad shape");
  WFT_CHECK_ARG_AS(who, ATT_ALIGNED(a->q, a->ldq, a->q_bs) && ATT_ALIGNED(a->k, a->ldk, a->k_bs) &&
                            ATT_ALIGNED(a->v, a->ldv, a->v_bs) && ATT_ALIGNED(a->o, a->ldo, a->o_bs) &&
                            (!bwd || (ATT_ALIGNED(a->d_o, a->lddo, a->do_bs) && ATT_ALIGNED(a->dq, a->lddq, a->dq_bs) &&
                                      ATT_ALIGNED(a->dk, a->lddk, a->dk_bs) && ATT_ALIGNED(a->dv, a->lddv, a->dv_bs))),
                   align_msg);
  WFT_CHECK_ARG_AS(who, !a->causal || a->Tq == a->Tk, "causal attention needs Tq == Tk");
  if (!bwd) return WFT_OK;
  WFT_CHECK_ARG_AS(who, a->scale > 0.f, "scale must be positive (the row constants are -lse / scale)");
  WFT_CHECK_ARG_AS(who, (!a->dq_colsum && !a->dv_colsum && !a->colsum_ws) || (a->dq_colsum && a->dv_colsum && a->colsum_ws),
                   "dq_colsum, dv_colsum and colsum_ws go together");
  return WFT_OK;
}

// ---- the plan (pure host function): which kernels serve a call, their grids, the column-sum workspace layout; the two queries
// answer from it, the two launchers follow it
// persistent launches (one workgroup per CU) or one item per workgroup: WFT_ATTN_PERSISTENT=0 at load time (engine/lib.py sets it
// in a multi-GPU job); per call: wft_attn_args.launch_mode = 1 (bench.py's ddp_mode_1gpu block)
static int g_attn_persistent = [] { const char* e = getenv("WFT_ATTN_PERSISTENT"); return (e && e[0] == '0') ? 0 : 1; }();
struct AttnPlan {
  bool fwd_pipe = false;             // attn_fwd_pipe_kernel | attn_fwd_kernel
  bool dq4w = false, dkdv4w = false;  // the one-wave-per-SIMD kernel | the 8-wave kernel
  unsigned fwd_grid = 0, dq_grid = 0, dkdv_grid = 0;  // 1-D grids of 256 threads (8-wave kernels: see att_block_coords)
  // column-sum workspace, in floats from colsum_ws: per-wave partial rows [rows_q][H*64] of dq at cs_q and [rows_v][H*64] of dv at
  // cs_v (one row per 32 queries / keys of a batch entry), then the [ATT_CS_CHUNKS][H*64] middle stages of the two-level reduce
  long rows_q = 0, rows_v = 0, cs_q = 0, cs_v = 0, mid_q = 0, mid_v = 0;
  int64_t colsum_bytes = 0;
};
// grid of a persistent backward kernel: one workgroup per CU walks the (batch, head, 256-row block) items (wgs_env > 0 overrides:
// A/B runs; >= the number of items = one item per workgroup).
// WFT_ATTN_PERSISTENT=0 (set by engine/lib.py in a multi-GPU job, like WFT_NT256_PERSISTENT) or launch_mode = 1: one item per
// workgroup — RCCL's collective kernels hold CUs during the backward pass, and a static walk would leave those CUs' share of the
// items for a second round; the hardware dispatcher balances single-item workgroups (measured equal on one GPU: 732 vs 735 us)
static unsigned attn_persistent_grid(const wft_attn_args* a, int rows, int wgs_env) {
  const bool persistent = g_attn_persistent != 0 && a->launch_mode != 1;
  const long items = (long)((rows + 255) / 256) * a->H * a->B;
  long wgs = wgs_env > 0 ? wgs_env : (persistent ? wft_num_cus() : items);
  if (wgs > items) wgs = items;
  if (((long)a->H * a->B) % 8 == 0 && wgs >= 8) wgs -= wgs % 8;  // XCD mode needs the same number of workgroups on every XCD
  return (unsigned)wgs;
}
static AttnPlan attn_plan(const wft_attn_args* a) {
  AttnPlan pl;
  if (!a) return pl;
  static const int dkdv_wgs_env = [] { const char* e = wft_dev_getenv("WFT_DKDV_WGS"); return e ? atoi(e) : 0; }();
  pl.fwd_pipe = wft_fwd_pipe_eligible(a);
  pl.dq4w = wft_dq4w_eligible(a);
  pl.dkdv4w = wft_dkdv4w_eligible(a);
  // the forward and the 8-wave backward kernels: one workgroup per 128 queries (dK/dV: keys) of a (batch, head)
  const unsigned grid_q = (unsigned)(((a->Tq + 127) / 128) * a->H * a->B), grid_k = (unsigned)(((a->Tk + 127) / 128) * a->H * a->B);
  pl.fwd_grid = grid_q;
  pl.dq_grid = pl.dq4w ? attn_persistent_grid(a, a->Tq, 0) : grid_q;
  pl.dkdv_grid = pl.dkdv4w ? attn_persistent_grid(a, a->Tk, dkdv_wgs_env) : grid_k;
  const long n = (long)a->H * 64;
  pl.rows_q = (long)a->B * ((a->Tq + 31) / 32);
  pl.rows_v = (long)a->B * ((a->Tk + 31) / 32);
  pl.cs_v = pl.rows_q * n;
  pl.mid_q = pl.cs_v + pl.rows_v * n;
  pl.mid_v = pl.mid_q + (long)ATT_CS_CHUNKS * n;
  pl.colsum_bytes = (pl.mid_v + (int64_t)ATT_CS_CHUNKS * n) * (int64_t)sizeof(float);
  return pl;
}

extern "C" int64_t wft_attn_bwd_colsum_workspace_bytes(const wft_attn_args* a) { return attn_plan(a).colsum_bytes; }

// Which kernel serves these arguments (pure host function; bench.py / tests attribute timings and assert the dispatch):
// which = 0 forward: 2 attn_fwd_pipe_kernel, 1 attn_fwd_kernel; 1 dQ: 4 attn_bwd_dq4w_kernel, 8 attn_bwd_dq_kernel;
// 2 dK/dV: 4 attn_bwd_dkdv4w_kernel, 8 attn_bwd_dkdv_kernel
extern "C" int wft_attn_variant(const wft_attn_args* a, int which) {
  if (!a) return WFT_ERR_ARG;
  const AttnPlan pl = attn_plan(a);
  if (which == 0) return pl.fwd_pipe ? 2 : 1;
  if (which == 1) return pl.dq4w ? 4 : 8;
  if (which == 2) return pl.dkdv4w ? 4 : 8;
  return WFT_ERR_ARG;
}

extern "C" int wft_attn_fwd_bf16(const wft_attn_args* a, void* stream) {
  if (const int rc = attn_check(a, false, __func__, "q/k/v/o need 16-byte aligned bases and strides that are multiples of 8")) return rc;
  AttnP p;
  attn_fill(a, p);
  const AttnPlan pl = attn_plan(a);
  wft_attn_fwd_launch(p, pl.fwd_pipe, dim3(pl.fwd_grid), (hipStream_t)stream);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_attn_bwd_bf16(const wft_attn_args* a, void* stream) {
  if (const int rc = attn_check(a, true, __func__, "tensors need 16-byte aligned bases and strides that are multiples of 8")) return rc;
  AttnP p;
  attn_fill(a, p);
  const AttnPlan pl = attn_plan(a);
  if (a->colsum_ws) {
    p.cs_q = a->colsum_ws + pl.cs_q;
    p.cs_v = a->colsum_ws + pl.cs_v;
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = WFT_OK;
  if (pl.dq4w) rc = wft_dq4w_launch(p, dim3(pl.dq_grid), s);
  else wft_attn_dq8w_launch(p, dim3(pl.dq_grid), s);
  if (rc != WFT_OK) return rc;
  rc = pl.dkdv4w ? wft_dkdv4w_launch(p, dim3(pl.dkdv_grid), s) : wft_attn_dkdv8w_launch(p, dim3(pl.dkdv_grid), s);
  if (rc != WFT_OK) return rc;
  if (p.cs_q) {
    const int n = a->H * 64;
    float* mid_q = a->colsum_ws + pl.mid_q;
    float* mid_v = a->colsum_ws + pl.mid_v;
    const dim3 g1((n + 63) / 64, ATT_CS_CHUNKS, 2), g2((n + 63) / 64, 1, 2);
    hipLaunchKernelGGL(attn_colsum_reduce_kernel, g1, dim3(256), 0, s, (const float*)p.cs_q, pl.rows_q, mid_q, (const float*)p.cs_v, pl.rows_v, mid_v, n);
    hipLaunchKernelGGL(attn_colsum_reduce_kernel, g2, dim3(256), 0, s, (const float*)mid_q, (long)ATT_CS_CHUNKS, a->dq_colsum,
                       (const float*)mid_v, (long)ATT_CS_CHUNKS, a->dv_colsum, n);
  }
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
