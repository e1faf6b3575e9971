// gemm_i8.hip — W8A8 NT GEMM on the int8 matrix cores: int8 x int8 -> int32, scaled per row of both operands, bf16 out.
//
//   acc  = sum_k (int32)A[m][k] * (int32)B[n][k]          exact, order-free
//   f    = (float)acc                                      round to nearest even (matters above 2^24)
//   s    = a_scale[m] * b_scale[n]
//   v    = f * s  (+ bias[n])  (gelu)  (+ (float)residual[m][n])
//   C    = bf16(v)                                         one rounding
// every f32 operation correctly rounded and none fused (include/wft.h restates it; tests/_i8_cases.py is the numpy form).
//
// The product of decoding's weights="w8a8" mode for M > 32 (the encoder, the prefill, the cross key / value projections): A is an
// activation matrix that wft_quantize_rows_i8 has just quantised per row, B the int8 image of a weight shadow (LinearGroup.shadows_q8).
// The sum is integer arithmetic, so there is no accumulation order to pin: one launch, no split of K, no workspace, no atomics, and
// row m of C is the same bits whatever M it sat in.
//
// gemm_nt_i8_kernel, correctness first (DESIGN.md §5 "W8A8" has what it costs next to the hand-scheduled bf16 kernels):
//  * a workgroup of 4 waves owns a 128 x 128 tile of C, wave (wm, wn) its 64 x 64 quadrant: 4 x 4 tiles of v_mfma_i32_16x16x64_i8;
//  * per 64-wide k-step both operand tiles (128 rows x 64 bytes each) go global -> registers -> LDS, 16 bytes per lane, two LDS
//    buffers: the loads of step s + 1 are issued before the MFMAs of step s and stored behind them, one barrier per step;
//  * the k index inside an MFMA is a dummy: lane group g = lane >> 4 takes bytes [16g, 16g + 16) of the 64-byte line of its row for
//    BOTH operands, so the instruction's own byte-to-k map never enters (any map pairs A's byte j of group g with B's byte j of
//    group g).  The exact tests are the check of that statement;
//  * the weight rows are MFMA source A and the activation rows source B, so the accumulators hold C^T in the standard gfx950 map
//    D[row = 4g + reg][col = lane & 15]: a lane's four registers are four consecutive n of one m — one 8-byte store, 16-byte loads of
//    b_scale and bias;
//  * LDS image: row r of a tile at 64r bytes, its 16-byte chunk c at slot c ^ ((4 - (r >> 2)) & 3).  ds_read_b128 resolves banks per
//    16-lane group {0-3, 12-15, 20-27}, ... (MI355X_MICROARCH.md §LDS): with linear rows every group has two lanes on each slot; the
//    XOR puts the four row quads of a group on four different slot columns;
//  * rows >= M of the last row tile read row M - 1 (a column of C^T depends on its own activation row only) and are never stored.
#include "gemm_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

static const char* i8_why_not(const wft_gemm_args* a) {
  if (!a || !a->A || !a->B || !a->C) return "null pointer";
  if (a->M < 1 || a->M >= (1ll << 31)) return "M must lie in [1, 2^31)";
  if (a->batch != 1) return "batch must be 1";
  if (a->c_is_f32 || a->accumulate) return "C must be bf16, not accumulated into";
  if (a->alpha != 1.0f) return "alpha must be 1";
  if (a->epilogue != WFT_EPI_NONE && a->epilogue != WFT_EPI_GELU) return "only the plain and the gelu epilogue are served";
  if (a->aux) return "aux is not served";
  if (a->colsum || a->p_valid != 0 || a->valid_rows_period != 0) return "colsum / p_valid / valid_rows_period are not served";
  if (a->residual && (a->residual_first != 0 || (a->beta != 0.0f && a->beta != 1.0f))) return "the residual is added after the epilogue with beta 1";
  if (a->N < 128 || a->N % 128 != 0 || a->N / 128 > 65535) return "N must be a multiple of 128 (at most 65535 column tiles)";
  if (a->K < 64 || a->K % 64 != 0) return "K must be a multiple of 64";
  if (a->K > 65536) return "K must be at most 65536 (the int32 sum of K products of int8 must not overflow)";
  if (a->lda % 16 != 0 || a->ldb % 16 != 0) return "lda and ldb must be multiples of 16 (int8 rows are read 16 bytes at a time)";
  if (a->ldc % 4 != 0) return "ldc must be a multiple of 4";
  if ((((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C) & 15) != 0) return "base pointers must be 16-byte aligned";
  if (a->bias && ((uintptr_t)a->bias & 15) != 0) return "bias must be 16-byte aligned";
  if (a->residual && (a->ldr % 4 != 0 || ((uintptr_t)a->residual & 7) != 0)) return "residual alignment";
  return nullptr;
}

// 16-byte slot of chunk c of row r inside a [128][64 B] operand tile (see the head of the file)
__device__ __forceinline__ int i8_slot(int r, int c) { return r * 4 + (c ^ ((4 - (r >> 2)) & 3)); }

// the f32 epilogue of four consecutive n of one m: one operation per line of the definition, none fused
template <int GELU>
__device__ __forceinline__ u32x2 i8_epilogue(i32x4 acc, float sa, f32x4 sb, const float* __restrict__ bias_n, const unsigned short* res_mn) {
#pragma clang fp contract(off)
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float f = (float)acc[j];
    const float s = __fmul_rn(sa, sb[j]);
    v[j] = __fmul_rn(f, s);
  }
  if (bias_n) {
    const f32x4 b = *(const f32x4*)bias_n;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], b[j]);
  }
  if (GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = gelu_f(v[j]);
  }
  if (res_mn) {
    const u32x2 rv = *(const u32x2*)res_mn;
    v[0] = __fadd_rn(v[0], bf2f((unsigned short)(rv[0] & 0xffffu)));
    v[1] = __fadd_rn(v[1], bf2f((unsigned short)(rv[0] >> 16)));
    v[2] = __fadd_rn(v[2], bf2f((unsigned short)(rv[1] & 0xffffu)));
    v[3] = __fadd_rn(v[3], bf2f((unsigned short)(rv[1] >> 16)));
  }
  const u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
  return pk;
}

// grid (row tiles of C, column tiles of C), 256 threads.  X = A of the call (activations [M, K]), W = B of the call (weights [N, K]).
template <int GELU>
__global__ __launch_bounds__(256) void gemm_nt_i8_kernel(const signed char* __restrict__ X, long lda, const signed char* __restrict__ W, long ldb,
                                                         const float* __restrict__ a_scale, const float* __restrict__ b_scale,
                                                         const float* __restrict__ bias, const unsigned short* res, long ldr,
                                                         unsigned short* C, long ldc, int M, int nk) {
  __shared__ i32x4 lds[2][2][128 * 4];  // [buffer][0: X tile, 1: W tile][16-byte slot]: 32 KiB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const long m0 = (long)blockIdx.x * 128;
  const int n0 = blockIdx.y * 128;

  // staging: thread t moves chunk t & 3 of rows t >> 2 and 64 + (t >> 2) of both tiles
  const int sc = tid & 3, sr = tid >> 2;
  const signed char* xg[2];
  const signed char* wg[2];
  int slot[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = p * 64 + sr;
    long m = m0 + row;
    if (m > M - 1) m = M - 1;
    xg[p] = X + m * lda + sc * 16;
    wg[p] = W + (long)(n0 + row) * ldb + sc * 16;
    slot[p] = i8_slot(row, sc);
  }
  // operand reads: row 16 * tile + r of the wave's quadrant, chunk g
  int xs[4], ws[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    xs[t] = i8_slot(wm * 64 + t * 16 + r, g);
    ws[t] = i8_slot(wn * 64 + t * 16 + r, g);
  }

  i32x4 acc[4][4];  // [i: 16 n][t: 16 m]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = i32x4{0, 0, 0, 0};

  i32x4 gx[2], gw[2];
  auto load = [&](int ks) {
    const long ko = (long)ks * 64;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      gx[p] = *(const i32x4*)(xg[p] + ko);
      gw[p] = *(const i32x4*)(wg[p] + ko);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      lds[buf][0][slot[p]] = gx[p];
      lds[buf][1][slot[p]] = gw[p];
    }
  };

  load(0);
  stage(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const int cur = ks & 1;
    const bool more = ks + 1 < nk;
    if (more) load(ks + 1);
    i32x4 xf[4], wf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      xf[t] = lds[cur][0][xs[t]];
      wf[t] = lds[cur][1][ws[t]];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[i], xf[t], acc[i][t], 0, 0, 0);
    // buffer cur ^ 1 was last read in step ks - 1, and every wave has passed the barrier behind that step
    if (more) stage(cur ^ 1);
    __syncthreads();
  }

  // D[row = n within the 16-tile = 4g + reg][col = m within the 16-tile = r]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const long m = m0 + wm * 64 + t * 16 + r;
    if (m < M) {
      const float sa = a_scale[m];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + g * 4;
        const f32x4 sb = *(const f32x4*)(b_scale + n);
        *(u32x2*)(C + m * ldc + n) = i8_epilogue<GELU>(acc[i][t], sa, sb, bias ? bias + n : nullptr, res ? res + m * ldr + n : nullptr);
      }
    }
  }
}

}  // namespace

extern "C" int wft_gemm_nt_i8_ok(const wft_gemm_args* a) { return i8_why_not(a) == nullptr ? 1 : 0; }

extern "C" int wft_gemm_nt_i8(const wft_gemm_args* a, const float* a_scale, const float* b_scale, void* stream) {
  const char* why = i8_why_not(a);
  if (why) {  // (before any device call: the refusal is a pure host decision)
    wft_set_error("wft_gemm_nt_i8: not served: %s (ask wft_gemm_nt_i8_ok; wft_gemm_nt_bf16 on the bf16 operands takes the call)", why);
    return WFT_ERR_UNSUPPORTED;
  }
  if (!a_scale || !b_scale || ((((uintptr_t)a_scale) | ((uintptr_t)b_scale)) & 15) != 0) {
    wft_set_error("wft_gemm_nt_i8: a_scale (f32 [M]) and b_scale (f32 [N]) must be 16-byte aligned vectors");
    return WFT_ERR_ARG;
  }
  const int M = (int)a->M, nk = (int)(a->K / 64);
  const dim3 grid((unsigned)((a->M + 127) / 128), (unsigned)(a->N / 128));
  hipStream_t s = (hipStream_t)stream;
  if (a->epilogue == WFT_EPI_GELU)
    hipLaunchKernelGGL(gemm_nt_i8_kernel<1>, grid, dim3(256), 0, s, (const signed char*)a->A, (long)a->lda, (const signed char*)a->B, (long)a->ldb,
                       a_scale, b_scale, a->bias, (const unsigned short*)a->residual, (long)a->ldr, (unsigned short*)a->C, (long)a->ldc, M, nk);
  else
    hipLaunchKernelGGL(gemm_nt_i8_kernel<0>, grid, dim3(256), 0, s, (const signed char*)a->A, (long)a->lda, (const signed char*)a->B, (long)a->ldb,
                       a_scale, b_scale, a->bias, (const unsigned short*)a->residual, (long)a->ldr, (unsigned short*)a->C, (long)a->ldc, M, nk);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
