// gemm_stream.hip — weight-streaming NT GEMM for the projections of a KV-cached decoding step (M = batch <= 32).
//
//   C[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) (gelu) (+ residual[m][n]),   bf16 in, fp32 accumulation, bf16 out
//
// At M = B the 128-tile kernel of gemm_nt128.hip runs N / 128 workgroups that each walk all of K through LDS: 10 workgroups x 80
// k-steps for mlp.2 of large-v3 on a 256-CU chip, 14-47 us per call against 0.5-2 us of weight bytes.  Here
// the weight matrix is the only operand that matters, nobody shares a weight element, and the work is cut so that the grid
// covers the chip whatever N is:
//
//  * nt_stream_kernel: a workgroup of 4 waves owns 128 weight rows (32 per wave, two 16-row MFMA tiles) and ONE slice of K.
//    Both operands are K-contiguous, so a 16-byte global load per lane IS an operand of v_mfma_f32_16x16x32_bf16 (8
//    K-consecutive bf16 of one row): W rows as source A, the x rows as source B, C^T in the accumulators (a lane's 4 result
//    registers are 4 consecutive n of one m).  Weights go straight to VGPRs — no LDS round trip for an operand no other wave
//    reads.  The k index inside an MFMA is a dummy, so lane group g = lane >> 4 takes bytes [32g, 32g + 32) of each 128-byte
//    line of its row (two 16-byte loads feeding two MFMAs): a wave reads whole lines of 16 rows per 64-wide k-step.  x
//    (<= 32 x 5120 bf16) is L2-resident and read with the same lane-to-k assignment; rows >= M of a tile read row M - 1 (a
//    column of the product depends on its own x row only, and those columns are never stored).
//  * the split of K is a function of (N, K) and the CU count, NOT of M (stream_plan): row m of C is then bit-identical whatever
//    batch it sat in.  fp32 partials go to the caller's workspace [split][M][N];
//  * nt_stream_reduce_kernel sums them IN SPLIT ORDER and applies bias / GELU / residual: a second launch, no floating-point
//    atomics, no arrival counter (DESIGN.md §3 "Weight-streaming GEMM" says why), bitwise reproducible.
//
// Which calls are served (wft_gemm_nt_stream_ok) — the rule: 1 <= M <= 32, batch 1, bf16 C, alpha 1, no epilogue or the plain
// GELU one (aux NULL or the pre-activation), optional f32 bias, optional bf16 residual added after the epilogue with beta 1,
// N % 128 == 0, K % 64 == 0, the alignment rules of wft_gemm_nt_bf16.  A (N, K, M) region where this kernel does not beat the
// 128-tile kernel by more than both spreads of `tools/dev/decode_bench.py --parts gemm_stream` is to be excluded HERE, not by
// the caller (the tied logits product, 406 workgroups and 1.7x over its bytes on the old kernel, is the open case).
// No region is excluded so far.  The table was first measured together with the int8 twin (DESIGN.md §5 "Weight-only int8"): the
// tied logits product (0.59-0.78x) and N >= 3840 at M = 32 (0.87-0.93x) lose to the 128-tile kernel; acting on it changes what
// step="graph" computes and is left to a change of its own.
//
// Weight-only int8 twin (wft_gemm_nt_stream_q8): B is int8 [N, K] with one f32 scale per row (wft_quantize_rows_i8, shadow.hip).
//   C[m][n] = bf16(epi(b_scale[n] * sum_k A[m][k] * Q[n][k] + bias[n]) + residual[m][n])
// nt_stream_q8_kernel keeps the plan, the grid, the wave's 32 rows, the lane-to-k assignment and the accumulation order of
// nt_stream_kernel; a lane's 16 k of a 64-wide k-step are ONE 16-byte load (16 int8) instead of two, sign-extended and converted
// in registers (int8 -> f32 -> bf16, both exact: |q| <= 128 < 2^8) into the same two bf16x8 MFMA operands.  The partials are
// therefore the bits nt_stream_kernel gives on Q.to(bf16), and the scale is applied once, in the reduce, to the slice-ordered
// sum — before the bias.  A power-of-two scale commutes with every rounding: the bit-for-bit tests of tests/test_q8_kernels_gpu.py.
#include "gemm_common.h"

namespace {

struct StreamPlan {
  int split;  // slices of K
  int per;    // 64-wide k-steps per slice (the last slice may be shorter, never empty)
};

// Grid = (N / 128) x split workgroups of 4 waves.  All of them are co-resident (<= 8 per CU), so more workgroups means more
// weight bytes in flight, not more rounds: aim at 4 per CU, keep at least one k-step per slice.
static StreamPlan stream_plan(int64_t N, int64_t K) {
  const int64_t nblk = N / 128, nk = K / 64;
  int64_t split = (4 * (int64_t)wft_num_cus()) / nblk;
  if (split < 1) split = 1;
  if (split > nk) split = nk;
  const int64_t per = (nk + split - 1) / split;
  StreamPlan p;
  p.per = (int)per;
  p.split = (int)((nk + per - 1) / per);
  return p;
}

static const char* stream_why_not(const wft_gemm_args* a) {
  if (!a || !a->A || !a->B || !a->C) return "null pointer";
  if (a->M < 1 || a->M > 32) return "M must lie in [1, 32]";
  if (a->batch != 1) return "batch must be 1";
  if (a->c_is_f32 || a->accumulate) return "C must be bf16, not accumulated into";
  if (a->alpha != 1.0f) return "alpha must be 1";
  if (a->epilogue != WFT_EPI_NONE && a->epilogue != WFT_EPI_GELU) return "only the plain and the gelu epilogue are served";
  if (a->aux && a->epilogue != WFT_EPI_GELU) return "aux needs the gelu epilogue";
  if (a->colsum || a->p_valid != 0 || a->valid_rows_period != 0) return "colsum / p_valid / valid_rows_period are not served";
  if (a->residual && (a->residual_first != 0 || (a->beta != 0.0f && a->beta != 1.0f))) return "the residual is added after the epilogue with beta 1";
  if (a->N < 128 || a->N % 128 != 0) return "N must be a multiple of 128";
  if (a->K < 64 || a->K % 64 != 0) return "K must be a multiple of 64";
  if (a->N >= (1ll << 31) || a->K >= (1ll << 31)) return "dims exceed int32";
  if (a->lda % 8 != 0 || a->ldb % 8 != 0 || a->ldc % 4 != 0) return "ld alignment";
  if ((((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C) & 15) != 0) return "base pointers must be 16-byte aligned";
  if (a->bias && ((uintptr_t)a->bias & 15) != 0) return "bias must be 16-byte aligned";
  if (a->residual && (a->ldr % 4 != 0 || ((uintptr_t)a->residual & 7) != 0)) return "residual alignment";
  if (a->aux && (a->ldaux % 4 != 0 || ((uintptr_t)a->aux & 7) != 0)) return "aux alignment";
  return nullptr;
}

// the int8 twin: the same rule; B's rows are 16-byte loads of int8, the scales are read four at a time
static const char* stream_q8_why_not(const wft_gemm_args* a) {
  const char* why = stream_why_not(a);
  if (why) return why;
  if (a->ldb % 16 != 0) return "ldb must be a multiple of 16 (int8 rows are read 16 bytes at a time)";
  // measured against the bf16 streaming kernel at the same shape (profiles/decode_bench_q8.jsonl): 0.98-1.01x at M = 1, 8,
  // 32 — two launches of ~9 us whatever the 1.6 MB of weights cost.  The d x d projections of large-v3 keep their bf16 shadow.
  if (a->N == 1280 && a->K == 1280) return "excluded shape: N = K = 1280 is no faster than wft_gemm_nt_stream_bf16 (DESIGN.md §5)";
  return nullptr;
}

typedef __attribute__((ext_vector_type(4))) int i32x4;

// sixteen int8 of one 16-byte load -> the two bf16x8 operands of a k-step: bytes 0..7 feed MFMA h = 0, bytes 8..15 h = 1
__device__ __forceinline__ void q8_operands(i32x4 q, bf16x8 (&w)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    u32x4 pk;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int d = q[2 * h + (p >> 1)], sh = 16 * (p & 1);
      pk[p] = pack2bf((float)(int)(signed char)(d >> sh), (float)(int)(signed char)(d >> (sh + 8)));
    }
    w[h] = __builtin_bit_cast(bf16x8, pk);
  }
}

// MT: 16-row tiles of x (1: M <= 16, 2: M <= 32).  ws[split][M][N] fp32.
template <int MT>
__global__ __launch_bounds__(256) void nt_stream_kernel(const unsigned short* __restrict__ A, long lda, const unsigned short* __restrict__ W,
                                                        long ldb, float* __restrict__ ws, int M, int N, int nk, int per) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + wave * 32;
  const int ks0 = blockIdx.y * per;
  const int ks1 = ks0 + per < nk ? ks0 + per : nk;
  const unsigned short* w0 = W + (long)(n0 + r) * ldb + g * 16;
  const unsigned short* w1 = w0 + 16 * ldb;
  const unsigned short* x[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + r;
    x[t] = A + (long)(m < M ? m : M - 1) * lda + g * 16;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // two k-steps' loads are issued before the first MFMA waits for any of them (written out: `#pragma unroll 2` is refused here)
  auto load = [&](int ks, bf16x8 (&wf)[2][2], bf16x8 (&xf)[MT][2]) {
    const long ko = (long)ks * 64;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      wf[0][h] = *(const bf16x8*)(w0 + ko + 8 * h);
      wf[1][h] = *(const bf16x8*)(w1 + ko + 8 * h);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) xf[t][h] = *(const bf16x8*)(x[t] + ko + 8 * h);
  };
  auto mma = [&](const bf16x8 (&wf)[2][2], const bf16x8 (&xf)[MT][2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][h], xf[t][h], acc[i][t], 0, 0, 0);
  };
  int ks = ks0;
  for (; ks + 2 <= ks1; ks += 2) {
    bf16x8 wa[2][2], xa[MT][2], wb[2][2], xb[MT][2];
    load(ks, wa, xa);
    load(ks + 1, wb, xb);
    mma(wa, xa);
    mma(wb, xb);
  }
  if (ks < ks1) {
    bf16x8 wa[2][2], xa[MT][2];
    load(ks, wa, xa);
    mma(wa, xa);
  }
  // D[row = n within the tile = 4g + reg][col = m within the tile = r]
  float* out = ws + (long)blockIdx.y * M * N;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + r;
    if (m < M) {
#pragma unroll
      for (int i = 0; i < 2; ++i) *(f32x4*)(out + (long)m * N + n0 + i * 16 + g * 4) = acc[i][t];
    }
  }
}

// nt_stream_kernel on int8 weight rows (see the head of the file): same indices, same order of MFMAs, half the loads per weight row
template <int MT>
__global__ __launch_bounds__(256) void nt_stream_q8_kernel(const unsigned short* __restrict__ A, long lda, const signed char* __restrict__ Q,
                                                           long ldb, float* __restrict__ ws, int M, int N, int nk, int per) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 128 + wave * 32;
  const int ks0 = blockIdx.y * per;
  const int ks1 = ks0 + per < nk ? ks0 + per : nk;
  const signed char* w0 = Q + (long)(n0 + r) * ldb + g * 16;
  const signed char* w1 = w0 + 16 * ldb;
  const unsigned short* x[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + r;
    x[t] = A + (long)(m < M ? m : M - 1) * lda + g * 16;
  }
  f32x4 acc[2][MT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // as in nt_stream_kernel, two k-steps' loads are issued before the first conversion waits for any of them
  auto load = [&](int ks, i32x4 (&qf)[2], bf16x8 (&xf)[MT][2]) {
    const long ko = (long)ks * 64;
    qf[0] = *(const i32x4*)(w0 + ko);
    qf[1] = *(const i32x4*)(w1 + ko);
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) xf[t][h] = *(const bf16x8*)(x[t] + ko + 8 * h);
  };
  auto mma = [&](const i32x4 (&qf)[2], const bf16x8 (&xf)[MT][2]) {
    bf16x8 wf[2][2];
    q8_operands(qf[0], wf[0]);
    q8_operands(qf[1], wf[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][h], xf[t][h], acc[i][t], 0, 0, 0);
  };
  int ks = ks0;
  for (; ks + 2 <= ks1; ks += 2) {
    i32x4 qa[2], qb[2];
    bf16x8 xa[MT][2], xb[MT][2];
    load(ks, qa, xa);
    load(ks + 1, qb, xb);
    __builtin_amdgcn_sched_barrier(0);  // (MT = 2: the scheduler otherwise sinks the second step's weight loads below the first MFMAs)
    mma(qa, xa);
    mma(qb, xb);
  }
  if (ks < ks1) {
    i32x4 qa[2];
    bf16x8 xa[MT][2];
    load(ks, qa, xa);
    mma(qa, xa);
  }
  float* out = ws + (long)blockIdx.y * M * N;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + r;
    if (m < M) {
#pragma unroll
      for (int i = 0; i < 2; ++i) *(f32x4*)(out + (long)m * N + n0 + i * 16 + g * 4) = acc[i][t];
    }
  }
}

// C[m][n..n+3] = bf16(epilogue(scale[n..n+3] * sum over slices, in slice order, of ws[s][m][n..n+3])): one thread per 4 consecutive
// columns.  scale NULL (the bf16 entry point): no multiply at all.  The multiply is a correctly rounded one of its own, never fused
// with the bias add — the definition tests/_q8_cases.py restates.
template <int GELU>
__global__ __launch_bounds__(256) void nt_stream_reduce_kernel(const float* __restrict__ ws, int split, int M, int N, const float* __restrict__ scale,
                                                               const float* __restrict__ bias,
                                                               const unsigned short* res, long ldr, unsigned short* aux,
                                                               long ldaux, unsigned short* C, long ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = N >> 2;
  if (i >= (long)M * n4) return;
  const int m = (int)(i / n4), n = (int)(i - (long)m * n4) << 2;
  const float* src = ws + (long)m * N + n;
  f32x4 t = *(const f32x4*)src;
  for (int s = 1; s < split; ++s) t += *(const f32x4*)(src + (long)s * M * N);
  if (scale) {
    const f32x4 sc = *(const f32x4*)(scale + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = __fmul_rn(t[j], sc[j]);
  }
  if (bias) t += *(const f32x4*)(bias + n);
  if (GELU) {
    if (aux) {
      const u32x2 pre = {pack2bf(t[0], t[1]), pack2bf(t[2], t[3])};
      *(u32x2*)(aux + (long)m * ldaux + n) = pre;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = gelu_f(t[j]);
  }
  if (res) {
    const u32x2 rv = *(const u32x2*)(res + (long)m * ldr + n);
    t[0] += bf2f((unsigned short)(rv[0] & 0xffffu));
    t[1] += bf2f((unsigned short)(rv[0] >> 16));
    t[2] += bf2f((unsigned short)(rv[1] & 0xffffu));
    t[3] += bf2f((unsigned short)(rv[1] >> 16));
  }
  const u32x2 pk = {pack2bf(t[0], t[1]), pack2bf(t[2], t[3])};
  *(u32x2*)(C + (long)m * ldc + n) = pk;
}

}  // namespace

extern "C" int wft_gemm_nt_stream_ok(const wft_gemm_args* a) { return stream_why_not(a) == nullptr ? 1 : 0; }

extern "C" int64_t wft_gemm_nt_stream_workspace_bytes(const wft_gemm_args* a) {
  if (stream_why_not(a) != nullptr) return 0;
  return (int64_t)stream_plan(a->N, a->K).split * a->M * a->N * (int64_t)sizeof(float);
}

// both entry points behind their checks: b_scale NULL = bf16 weights, else int8 weights with one scale per row
static int stream_launch(const wft_gemm_args* a, const float* b_scale, const char* who, const char* ws_query, void* stream) {
  const StreamPlan p = stream_plan(a->N, a->K);
  const int64_t need = (int64_t)p.split * a->M * a->N * (int64_t)sizeof(float);
  if (!a->workspace || a->workspace_bytes < need || ((uintptr_t)a->workspace & 15) != 0) {
    wft_set_error("%s: needs a 16-byte aligned workspace of %lld bytes (%s)", who, (long long)need, ws_query);
    return WFT_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int M = (int)a->M, N = (int)a->N, nk = (int)(a->K / 64);
  const dim3 grid((unsigned)(N / 128), (unsigned)p.split);
  float* ws = (float*)a->workspace;
  if (b_scale) {
    if (M <= 16)
      hipLaunchKernelGGL(nt_stream_q8_kernel<1>, grid, dim3(256), 0, s, (const unsigned short*)a->A, (long)a->lda, (const signed char*)a->B,
                         (long)a->ldb, ws, M, N, nk, p.per);
    else
      hipLaunchKernelGGL(nt_stream_q8_kernel<2>, grid, dim3(256), 0, s, (const unsigned short*)a->A, (long)a->lda, (const signed char*)a->B,
                         (long)a->ldb, ws, M, N, nk, p.per);
  } else if (M <= 16)
    hipLaunchKernelGGL(nt_stream_kernel<1>, grid, dim3(256), 0, s, (const unsigned short*)a->A, (long)a->lda, (const unsigned short*)a->B,
                       (long)a->ldb, ws, M, N, nk, p.per);
  else
    hipLaunchKernelGGL(nt_stream_kernel<2>, grid, dim3(256), 0, s, (const unsigned short*)a->A, (long)a->lda, (const unsigned short*)a->B,
                       (long)a->ldb, ws, M, N, nk, p.per);
  WFT_CHECK_LAUNCH_AS(who);
  const dim3 rgrid((unsigned)(((int64_t)M * (N / 4) + 255) / 256));
  if (a->epilogue == WFT_EPI_GELU)
    hipLaunchKernelGGL(nt_stream_reduce_kernel<1>, rgrid, dim3(256), 0, s, (const float*)ws, p.split, M, N, b_scale, a->bias,
                       (const unsigned short*)a->residual, (long)a->ldr, (unsigned short*)a->aux, (long)a->ldaux, (unsigned short*)a->C, (long)a->ldc);
  else
    hipLaunchKernelGGL(nt_stream_reduce_kernel<0>, rgrid, dim3(256), 0, s, (const float*)ws, p.split, M, N, b_scale, a->bias,
                       (const unsigned short*)a->residual, (long)a->ldr, (unsigned short*)nullptr, 0L, (unsigned short*)a->C, (long)a->ldc);
  WFT_CHECK_LAUNCH_AS(who);
  return WFT_OK;
}

extern "C" int wft_gemm_nt_stream_bf16(const wft_gemm_args* a, void* stream) {
  const char* why = stream_why_not(a);
  if (why) {  // (before any device call: the refusal is a pure host decision)
    wft_set_error("wft_gemm_nt_stream_bf16: not served: %s (ask wft_gemm_nt_stream_ok; wft_gemm_nt_bf16 takes the call)", why);
    return WFT_ERR_UNSUPPORTED;
  }
  return stream_launch(a, nullptr, "wft_gemm_nt_stream_bf16", "wft_gemm_nt_stream_workspace_bytes", stream);
}

// ----------------------------------------------------------------------------- int8 weights
// A shape where q8 does not beat the bf16 streaming kernel by more than both spreads of `tools/dev/decode_bench.py --parts gemm_stream`
// (arm q8_vs_stream) is refused in stream_q8_why_not, and the caller then takes the bf16 streaming kernel for that group: so far
// (N, K) = (1280, 1280), the one measured shape that does not win.
extern "C" int wft_gemm_nt_stream_q8_ok(const wft_gemm_args* a) { return stream_q8_why_not(a) == nullptr ? 1 : 0; }

extern "C" int64_t wft_gemm_nt_stream_q8_workspace_bytes(const wft_gemm_args* a) {
  if (stream_q8_why_not(a) != nullptr) return 0;
  return (int64_t)stream_plan(a->N, a->K).split * a->M * a->N * (int64_t)sizeof(float);
}

extern "C" int wft_gemm_nt_stream_q8(const wft_gemm_args* a, const float* b_scale, void* stream) {
  const char* why = stream_q8_why_not(a);
  if (why) {
    wft_set_error("wft_gemm_nt_stream_q8: not served: %s (ask wft_gemm_nt_stream_q8_ok; wft_gemm_nt_stream_bf16 takes the bf16 shadow)", why);
    return WFT_ERR_UNSUPPORTED;
  }
  if (!b_scale || ((uintptr_t)b_scale & 15) != 0) {
    wft_set_error("wft_gemm_nt_stream_q8: b_scale must be a 16-byte aligned f32 [N] vector");
    return WFT_ERR_ARG;
  }
  return stream_launch(a, b_scale, "wft_gemm_nt_stream_q8", "wft_gemm_nt_stream_q8_workspace_bytes", stream);
}
