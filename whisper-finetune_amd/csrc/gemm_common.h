// gemm_common.h — what the GEMM translation units share: the parameter block, tile-order helpers, per-device host helpers, and
// what each kernel file offers nt_plan / tn_plan and the entry points of gemm.hip (the host file).  Kernel files: gemm_nt4w.hip /
// gemm_tn4w.hip (256x256, one wave per SIMD), gemm_pp256.hip (256x256 8-wave ping-pong), gemm_nt128.hip / gemm_tn128.hip
// (128x128), gemm_rank.hip (rank-r operands); gemm_stream.hip (small-M weight streaming) and gemm_i8.hip (int8 x int8 -> int32, the W8A8
// product of decoding) have entry points of their own.
#pragma once
#include "common.h"
#include <type_traits>

struct GemmP {
  const unsigned short* A; long lda; long sA;
  const unsigned short* B; long ldb; long sB;
  void* C; long ldc; long sC;
  const float* bias;
  const unsigned short* res; long ldr; long sR;
  unsigned short* aux; long ldaux; long sAux;
  float alpha, beta;
  int M, N, K, batch;
  int accumulate;
  int period, valid;
  int res_first;
  float* ws;  // split-K partial tiles [nsplit][P][Q] fp32 (TN, optional)
  float* cs_part;  // NT256: per-(row tile, wave row) column-sum partials [2*tiles_m][N] fp32, or NULL
  int nsplit;  // gemm_tn_rank_kernel: split-K factor (its grid is 1-D)
  int band;  // NT256: tile-order band width in column tiles (WFT_NT256_BAND, default 5)
  int diag;  // WFT_GEMM_DIAG, NT256 A/B switches: 6 skips the staged epilogue (timing only), 7 = general epilogue body everywhere, 8 = no continuous staging
};

// sid -> (row tile, column tile) in column BANDS of 5 tiles, row-major inside a band: the 32 workgroups an XCD
// runs at a time (consecutive sids) then cover a ~6 x 5 patch = 11 operand panels instead of 2 x 20 = 22 for a
// wide N.  Measured before: FETCH_SIZE of the 48000x5120x1280 GEMM was 8x its algorithmic A+B bytes (every XCD
// re-streamed all of B every round).
__device__ __forceinline__ void band_coords(int sid, int tiles_r, int tiles_c, int& tr, int& tc, int W = 5) {
  const int band = sid / (tiles_r * W);
  const int c0 = band * W;
  const int w = (tiles_c - c0) < W ? (tiles_c - c0) : W;
  const int r = sid - band * tiles_r * W;
  tr = r / w;
  tc = c0 + r - tr * w;
}

__device__ __forceinline__ int xcd_remap(int bid, int ntile) {
  const int q = ntile >> 3, r = ntile & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- device helpers of several kernel files (shared here, every kernel compiles to the machine code it had with a copy of its own)
// ds_read_b128 from inline asm with an immediate offset: gemm_nt_kernel's ring form, gemm_nt_rank_kernel
template <int IMM>
__device__ __forceinline__ bf16x8 lds_b128_asm(unsigned lds_byte_addr) {
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(IMM));
  return r;
}
// ds_read_b64_tr_b16 from inline asm with an immediate offset (contract as lds_read_tr16_asm in common.h)
template <int IMM>
__device__ __forceinline__ s16x4 tn_tr_asm(unsigned lds_byte_addr) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_byte_addr), "n"(IMM));
  return r;
}
// the TN kernels' row swizzle of 16-byte chunk pairs (gemm_tn_kernel, gemm_tn_rank_kernel, gemm_tn256_kernel)
__device__ __forceinline__ int tn_f(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }

// ---- host side
#define WFT_MAX_DEVICES 64
static inline int wft_cur_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= WFT_MAX_DEVICES) dev = 0;
  return dev;
}
// CU count of the CURRENT device (cached per device id: a process may drive several GPUs)
static inline int wft_num_cus() {
  static int n[WFT_MAX_DEVICES] = {0};
  const int dev = wft_cur_device();
  if (n[dev] == 0) {
    hipDeviceProp_t prop;
    int v = 0;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) v = prop.multiProcessorCount;
    n[dev] = v > 0 ? v : 256;
  }
  return n[dev];
}
// hipFuncSetAttribute is per device: remember, per kernel call site, which devices have it
struct DynLdsOnce {
  bool done[WFT_MAX_DEVICES] = {false};
  template <class K>
  bool set(K kfn, int bytes) {  // false (and wft_last_error says why): the caller returns WFT_ERR_LAUNCH instead of launching
    const int dev = wft_cur_device();
    if (!done[dev]) {
      const hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess) {
        wft_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d) failed on device %d: %s", bytes, dev, hipGetErrorString(e));
        return false;
      }
      done[dev] = true;
    }
    return true;
  }
};
// launch of a kernel whose dynamic LDS exceeds the 64 KiB default: one DynLdsOnce per kernel, however many call sites launch it
template <auto KFN, class... Args>
static inline int wft_launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args&... args) {
  static DynLdsOnce once;
  if (!once.set(KFN, lds_bytes)) return WFT_ERR_LAUNCH;
  hipLaunchKernelGGL(KFN, grid, block, lds_bytes, s, args...);
  return WFT_OK;
}

// f(epilogue, C is fp32) with both as compile-time constants, for the (epilogue, C type) pairs the 128-tile and the ping-pong
// kernels are instantiated with: GELU_GRAD and MUL_AUX write a bf16 C only
template <int E>
using EpiC = std::integral_constant<int, E>;
template <class F>
static int nt_with_epilogue(const wft_gemm_args* a, F&& f) {
  const auto either = [&](auto e) { return a->c_is_f32 ? f(e, std::true_type{}) : f(e, std::false_type{}); };
  switch (a->epilogue) {
    case WFT_EPI_NONE: return either(EpiC<WFT_EPI_NONE>{});
    case WFT_EPI_GELU: return either(EpiC<WFT_EPI_GELU>{});
    case WFT_EPI_DGELU: return either(EpiC<WFT_EPI_DGELU>{});
    case WFT_EPI_GELU_GRAD: return f(EpiC<WFT_EPI_GELU_GRAD>{}, std::false_type{});
    case WFT_EPI_MUL_AUX: return f(EpiC<WFT_EPI_MUL_AUX>{}, std::false_type{});
    default: wft_set_error("wft_gemm_nt_bf16: unknown epilogue %d", a->epilogue); return WFT_ERR_ARG;
  }
}

// ---- what each kernel file offers nt_plan / tn_plan and the entry points (gemm.hip): its eligibility rule, its share of the plan
// and the launch on the plan's grid (the file knows its kernels' LDS bytes and instantiations; int: WFT_OK or an error code).
// `diag` is WFT_GEMM_DIAG, read once in gemm.hip; the launches see it as GemmP.diag.
enum NtKind { NT_4W, NT_256, NT_RANK, NT_128_SPLITK, NT_128_RING, NT_128_2BUF };
enum TnKind { TN_4W, TN_256, TN_RANK, TN_128_PB, TN_128_RING, TN_128_2BUF, TN_128_BF16C };
bool wft_nt4w_eligible(const wft_gemm_args* a);                                             // gemm_nt4w.hip
int wft_nt4w_launch(const wft_gemm_args* a, const GemmP& p, unsigned grid, void* stream);
bool wft_tn4w_eligible(const wft_gemm_args* a);                                             // gemm_tn4w.hip
void wft_tn4w_plan(const wft_gemm_args* a, int* nsplit_out, int* per_out);
int wft_tn4w_launch(const GemmP& p, unsigned grid, void* stream);
int wft_nt256_launch(const wft_gemm_args* a, const GemmP& p, unsigned grid, hipStream_t s);  // gemm_pp256.hip
void wft_nt_colsum_reduce_launch(const wft_gemm_args* a, hipStream_t s);
int wft_tn256_nsplit(const wft_gemm_args* a);
int wft_tn256_launch(const GemmP& p, unsigned grid, hipStream_t s);
bool wft_nt128_ring(const wft_gemm_args* a, int diag);                                      // gemm_nt128.hip
int wft_nt128_splitk_plan(const wft_gemm_args* a, int diag, int* per_out);
int wft_nt128_launch(const wft_gemm_args* a, const GemmP& p, NtKind kind, int nsplit, int per, dim3 grid, hipStream_t s);
bool wft_tn128_ring(const wft_gemm_args* a, int diag);                                      // gemm_tn128.hip
int wft_tn128_nsplit(const wft_gemm_args* a, bool ring);
int wft_tn128_pb(const wft_gemm_args* a);
int wft_tn128_launch(const GemmP& p, TnKind kind, int pb, dim3 grid, hipStream_t s);
int wft_nt_rank_pb(const wft_gemm_args* a);                                                 // gemm_rank.hip
int wft_nt_rank_launch(int pb, const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s);
int wft_tn_rank_launch(int pb, const GemmP& p0, const GemmP& p1, int n0, int n1, hipStream_t s);
